"""Child process of tests/test_bam_writer.py::test_bam_sanitizers: loads the AddressSanitizer + UBSan flavour of the emulation build
and runs the BAM calls of the CPU suite on it (records single-end and paired-end with default and caller's names, header, BGZF,
bwamem_hip_align_to_bam, the error paths).  Any sanitizer report aborts the process.  usage: bam_sanitized_child.py <small-genome.img> <small-genome.fa>"""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bwalib as B  # noqa: E402
import test_bam_writer as T  # noqa: E402

emu = B.Lib(os.path.join(B.ROOT, "tests", "emu", "_build", "libbwamem_emu_asan.so"), "jnibwa_")
img, fa = sys.argv[1:3]
seqs = []
for blk in open(fa).read().split(">")[1:]:
    name, _, body = blk.partition("\n")
    seqs.append((name.strip(), body.replace("\n", "").encode()))
h = emu.open_index(img)
T.run_small_cases(emu, h, seqs)
T.check_header(emu, h, seqs)
T.check_bgzf(emu)
with tempfile.TemporaryDirectory() as tmp:
    T.check_align_to_bam(emu, h, seqs, tmp)
T.check_errors(emu, h, seqs)
T.check_cigar_limit(emu)
emu.destroy_index(h)
print("sanitized-ok")
