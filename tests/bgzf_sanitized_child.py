"""Child process of tests/test_bgzf_device.py::test_bgzf_device_sanitizers: loads the AddressSanitizer + UBSan flavour of the emulation
build and runs the device-BGZF calls of the CPU suite on it (every input of the round-trip test, the batch path, bwamem_hip_align_to_bam_device,
the error paths).  Any sanitizer report aborts the process.  usage: bgzf_sanitized_child.py <small-genome.img> <small-genome.fa>"""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bwalib as B  # noqa: E402
import test_bgzf_device as T  # noqa: E402

emu = B.Lib(os.path.join(B.ROOT, "tests", "emu", "_build", "libbwamem_emu_asan.so"), "jnibwa_")
img, fa = sys.argv[1:3]
seqs = []
for blk in open(fa).read().split(">")[1:]:
    name, _, body = blk.partition("\n")
    seqs.append((name.strip(), body.replace("\n", "").encode()))
h = emu.open_index(img)
T.check_all_inputs(emu, h)
T.check_batch_path(emu, h, seqs)
with tempfile.TemporaryDirectory() as tmp:
    T.check_align_to_bam_device(emu, h, seqs, tmp)
T.check_errors_device(emu, h, seqs)
emu.destroy_index(h)
print("sanitized-ok")
