"""bench.py --dump-outputs: the arrays written for the last timed step must hold exactly the records of the sampled reads and a
CRC-32 per block of reads over the whole response.  CPU suite: the response is the oracle's, handed to dump_outputs through a
stand-in for the two library calls it makes."""
import ctypes
import os
import sys
import zlib

import numpy as np

import bwalib as B

sys.path.insert(0, B.ROOT)
import bench  # noqa: E402


class _FakeLib:
    """bwamem_hip_batch_result_bytes / bwamem_hip_batch_download over a response held in host memory"""
    def __init__(self, resp):
        self.resp = resp

    def bwamem_hip_batch_result_bytes(self, batch):
        return len(self.resp)

    def bwamem_hip_batch_download(self, batch, dst):
        ctypes.memmove(dst, self.resp, len(self.resp))
        return 0


def test_dump_outputs_holds_the_sampled_records(oracle, rota_img, tmp_path, monkeypatch):
    seqs = []
    name, cur = None, []
    for line in open(os.path.join(B.GOLDEN, "rotavirus", "ref.fa")):
        if line.startswith(">"):
            if name:
                seqs.append((name, "".join(cur).encode()))
            name, cur = line[1:].split()[0], []
        else:
            cur.append(line.strip())
    seqs.append((name, "".join(cur).encode()))
    n = 300
    reads = B.simulate_reads(seqs, n, length=100, seed=5)
    h = oracle.open_index(rota_img)
    resp = oracle.align_raw(h, oracle.default_options(), B.pack_request(reads))
    oracle.destroy_index(h)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 37)
    monkeypatch.setattr(bench, "DUMP_BLOCK", 64)
    out = tmp_path / "dump"
    bench.dump_outputs(_FakeLib(resp), None, n, str(out))
    a = {k: np.load(out / (k + ".npy")) for k in ("read_index", "record_offsets", "record_words", "block_crc32", "response_info")}
    assert all(v.dtype == np.float64 for v in a.values())
    assert list(a["response_info"]) == [n, len(resp)]
    idx = a["read_index"].astype(np.int64)
    assert len(idx) == 37 and len(set(idx)) == 37 and list(idx) == sorted(idx) and idx.max() < n
    per_read = B.split_response(resp, n)
    off = a["record_offsets"].astype(np.int64)
    words = a["record_words"].astype(np.int64).astype(np.int32)
    assert len(off) == len(idx) + 1 and off[-1] == len(words)
    for k, r in enumerate(idx):
        assert words[off[k]:off[k + 1]].tobytes() == per_read[r]
    assert list(a["block_crc32"]) == [zlib.crc32(b"".join(per_read[b:b + 64])) for b in range(0, n, 64)]
    # the same arguments pick the same reads
    out2 = tmp_path / "dump2"
    bench.dump_outputs(_FakeLib(resp), None, n, str(out2))
    assert all(np.array_equal(np.load(out / f), np.load(out2 / f)) for f in os.listdir(out))
