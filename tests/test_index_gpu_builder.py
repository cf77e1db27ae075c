"""The torch index builder (bench-scale path) must produce the same image, byte for byte, as the host
builder -- also when its chunked code paths (needed beyond 2^31 elements) are exercised."""
import ctypes
import os
import sys

import numpy as np
import torch

import bwalib as B

sys.path.insert(0, B.PKG)


def test_torch_builder_matches_host_builder(hip_lib, workdir, monkeypatch):
    import index_build_gpu as G
    monkeypatch.setattr(G, "CHUNK", 100003)                    # force many chunks
    seqs = B.synth_genome(260000, n_contigs=3, seed=5, repeat_frac=0.2)
    seqs[-1] = (seqs[-1][0], seqs[-1][1] + b"A" * 70 + b"T" * 40)      # low-complexity tail: stresses end-of-text ties
    fa = os.path.join(workdir, "tb.fa")
    B.write_fasta(fa, seqs)
    build = hip_lib.dll.jnibwa_createReferenceIndex
    build.argtypes = [ctypes.c_char_p] * 3
    assert build(fa.encode(), fa.encode(), b"auto") == 0
    assert hip_lib.create_index_file(fa, fa + ".img") == 0
    lut = torch.zeros(256, dtype=torch.uint8)
    for k, v in {65: 0, 67: 1, 71: 2, 84: 3}.items():
        lut[k] = v
    fwd = lut[torch.from_numpy(np.frombuffer(b"".join(s for _, s in seqs), dtype=np.uint8).copy()).long()]
    pieces = G.build_pieces(fwd)
    G.write_image(fa + ".torch.img", pieces, [(n, len(s)) for n, s in seqs])
    assert open(fa + ".torch.img", "rb").read() == open(fa + ".img", "rb").read()


import pytest


@pytest.mark.gpu
def test_torch_builder_on_the_gpu_matches_host_builder(hip_lib, workdir, monkeypatch):
    """the same comparison with the builder running where the bench runs it (cuda:0), chunked paths forced"""
    import index_build_gpu as G
    monkeypatch.setattr(G, "CHUNK", 250007)
    seqs = B.synth_genome(900000, n_contigs=5, seed=6, repeat_frac=0.2)
    seqs[-1] = (seqs[-1][0], seqs[-1][1] + b"C" * 90 + b"G" * 30)
    fa = os.path.join(workdir, "tbg.fa")
    B.write_fasta(fa, seqs)
    build = hip_lib.dll.jnibwa_createReferenceIndex
    build.argtypes = [ctypes.c_char_p] * 3
    assert build(fa.encode(), fa.encode(), b"auto") == 0
    assert hip_lib.create_index_file(fa, fa + ".img") == 0
    lut = torch.zeros(256, dtype=torch.uint8)
    for k, v in {65: 0, 67: 1, 71: 2, 84: 3}.items():
        lut[k] = v
    fwd = lut[torch.from_numpy(np.frombuffer(b"".join(s for _, s in seqs), dtype=np.uint8).copy()).long()].to("cuda:0")
    pieces = G.build_pieces(fwd)
    G.write_image(fa + ".torch.img", pieces, [(n, len(s)) for n, s in seqs])
    assert open(fa + ".torch.img", "rb").read() == open(fa + ".img", "rb").read()


BUILD_IMAGE_CODE = r"""
import ctypes, os, sys
import torch                                     # (first: the process then has one HIP runtime, torch's, as in bench.py)
sys.path[:0] = [%(tests)r, %(root)r, %(pkg)r]
import bench
import index_build_gpu as G
dev = torch.device("cuda", 0)
codes, contigs = bench.synth_genome(torch, dev, 20_000_003, 5, 0x5EED)
lib = bench.load_lib()
lib.bwamem_hip_set_device(0)
h = codes.cpu().numpy()
names = (ctypes.c_char_p * len(contigs))(*[n.encode() for n, _ in contigs])
lens = (ctypes.c_int64 * len(contigs))(*[l for _, l in contigs])
a, b = os.path.join(%(workdir)r, "bi_lib.img"), os.path.join(%(workdir)r, "bi_torch.img")
assert lib.bwamem_hip_build_image(h.ctypes.data, int(h.size), len(contigs), names, lens, a.encode()) == 0
G.write_image(b, G.build_pieces(codes), contigs)
assert open(a, "rb").read() == open(b, "rb").read(), "images differ"
print("build-image-ok")
"""


@pytest.mark.gpu
def test_library_image_builder_matches_torch_builder(workdir):
    """bwamem_hip_build_image (bench.py's index builder: threaded packing and counting on the host, image streamed to the file)
    against the torch builder, byte for byte, on a 20 Mbp genome of odd length (past the threads' threshold, partial last pac
    byte).  Own process: torch has to initialise HIP before the library does."""
    import subprocess
    code = BUILD_IMAGE_CODE % dict(tests=os.path.join(B.ROOT, "tests"), root=B.ROOT, pkg=B.PKG, workdir=workdir)
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "build-image-ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
