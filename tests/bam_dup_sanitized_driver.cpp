// TEST INFRASTRUCTURE ONLY: a stand-alone driver of the duplicate-marking calls, compiled with AddressSanitizer + UBSan and linked
// against the sanitized emulation build by tests/test_bam_dup.py::test_dup_sanitizers.
//   driver <index image> <directory>
// The directory holds manifest.txt, one case per line, and the files it names:
//   rec   <tag> <paired> <six counts>    <tag>.bam (records grouped by read), <tag>.off (int64 offsets): bwamem_hip_mark_duplicates_device
//                                        must hand back <tag>.want and these counts, and again when called on its own output
//   fastq <text> <paired> 0 0 0 0 0 0    upload_fastq, align, encode, mark, sort, compress, index; then the marked file call
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "bwamem_hip.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "driver: %s failed (line %d, case '%s')\n", #c, __LINE__, g_case.c_str()); exit(1); } } while (0)
static std::string g_case;

static std::string slurp(const std::string& path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) { fprintf(stderr, "driver: cannot read %s\n", path.c_str()); exit(1); }
    std::ostringstream o; o << f.rdbuf();
    return o.str();
}

// exact-size heap copies, so that an access past either end is seen
static char* exact(const std::string& s) { char* p = (char*)malloc(s.size() ? s.size() : 1); memcpy(p, s.data(), s.size()); return p; }

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s <image> <directory>\n", argv[0]); return 2; }
    const std::string dir = std::string(argv[2]) + "/";
    const int fd = open(argv[1], O_RDONLY);
    CHECK(fd >= 0);
    bwaidx_t* idx = jnibwa_openIndex(fd);
    CHECK(idx);
    mem_opt_t* opt = jnibwa_createDefaultOptions();
    mem_opt_t* opt_pe = jnibwa_createDefaultOptions();
    { int32_t flag; memcpy(&flag, (char*)opt_pe + 60, 4); flag |= 0x2; memcpy((char*)opt_pe + 60, &flag, 4); }
    std::ifstream mf(dir + "manifest.txt");
    CHECK((bool)mf);
    std::string kind, tag; int paired; unsigned long long want[6];
    int n_cases = 0;
    while (mf >> kind >> tag >> paired >> want[0] >> want[1] >> want[2] >> want[3] >> want[4] >> want[5]) {
        g_case = kind + " " + tag;
        ++n_cases;
        if (kind == "rec") {
            const std::string bam = slurp(dir + tag + ".bam"), off = slurp(dir + tag + ".off"), marked = slurp(dir + tag + ".want");
            CHECK(off.size() >= 8 && off.size() % 8 == 0 && marked.size() == bam.size());
            char* rp = exact(bam); char* op = exact(off);
            const size_t n_reads = off.size() / 8 - 1;
            for (int round = 0; round < 2; ++round) {
                bwamem_dup_counts_t c; memset(&c, 0x55, sizeof c);
                CHECK(bwamem_hip_mark_duplicates_device(idx, rp, bam.size(), (const int64_t*)op, n_reads, paired, &c) == 0);
                CHECK(memcmp(rp, marked.data(), bam.size()) == 0);
                CHECK(c.unpaired_reads_examined == want[0] && c.read_pairs_examined == want[1] && c.secondary_or_supplementary == want[2] && c.unmapped_reads == want[3]
                      && c.unpaired_read_duplicates == want[4] && c.read_pair_duplicates == want[5]);
            }
            CHECK(bwamem_hip_mark_duplicates_device(idx, rp, bam.size(), (const int64_t*)op, n_reads, paired, nullptr) == 0);
            if (bam.size() > 40 && n_reads > 0) {                      // a cut stream does not chain: refused, and nothing written
                int64_t* cut = (int64_t*)exact(off);
                cut[n_reads] = (int64_t)bam.size() - 7;
                for (size_t i = 0; i < n_reads; ++i) if (cut[i] > cut[n_reads]) cut[i] = cut[n_reads];
                char* sp = exact(bam.substr(0, bam.size() - 7));
                CHECK(bwamem_hip_mark_duplicates_device(idx, sp, bam.size() - 7, cut, n_reads, paired, nullptr) != 0);
                CHECK(memcmp(sp, bam.data(), bam.size() - 7) == 0);
                free(sp); free(cut);
            }
            free(rp); free(op);
            continue;
        }
        CHECK(kind == "fastq");
        const std::string text = slurp(dir + tag);
        char* tp = exact(text);
        int64_t bad = -7;
        bwamem_batch_t* b = bwamem_hip_batch_upload_fastq(idx, tp, text.size(), nullptr, 0, &bad);
        CHECK(b && bad == -1);
        bwamem_dup_counts_t c, c2;
        CHECK(bwamem_hip_batch_mark_duplicates(b, paired, &c) != 0);   // before encode
        CHECK(bwamem_hip_batch_keep_offsets(b, 1) == 0 && bwamem_hip_batch_align(idx, paired ? opt_pe : opt, nullptr, b, 0) == 0);
        CHECK(bwamem_hip_batch_encode_bam(b, paired, nullptr, nullptr) == 0);
        CHECK(bwamem_hip_batch_mark_duplicates(b, paired, &c) == 0);
        CHECK(c.read_pairs_examined + c.unpaired_reads_examined > 0 && c.read_pair_duplicates + c.unpaired_read_duplicates > 0);
        const size_t n = bwamem_hip_batch_bam_bytes(b);
        std::vector<char> m1(n), m2(n);
        CHECK(n > 0 && bwamem_hip_batch_bam_download(b, m1.data()) == 0);
        CHECK(bwamem_hip_batch_mark_duplicates(b, paired, &c2) == 0 && bwamem_hip_batch_bam_download(b, m2.data()) == 0);
        CHECK(m1 == m2 && memcmp(&c, &c2, sizeof c) == 0);
        CHECK(bwamem_hip_batch_sort_bam(b) == 0 && bwamem_hip_batch_mark_duplicates(b, paired, &c2) != 0);
        CHECK(bwamem_hip_batch_compress_bam(b, 1) == 0);
        size_t nb = 0;
        void* bai = bwamem_hip_batch_index_bam(b, 0, &nb);
        CHECK(bai && nb > 8);
        jnibwa_free(bai);
        bwamem_hip_batch_free(b);
        const std::string out = dir + "driver.bam", out_bai = dir + "driver.bai";
        const int fo = open(out.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644), fb = open(out_bai.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        CHECK(fo >= 0 && fb >= 0);
        CHECK(bwamem_hip_align_fastq_to_marked_bam(idx, paired ? opt_pe : opt, nullptr, tp, text.size(), nullptr, 0, "@RG\tID:san\tSM:s", 1, fo, fb, 1, &c2) == 0);
        CHECK(memcmp(&c, &c2, sizeof c) == 0 && lseek(fo, 0, SEEK_END) > 28 && lseek(fb, 0, SEEK_END) > 8);
        close(fo); close(fb);
        free(tp);
    }
    CHECK(n_cases >= 3);
    jnibwa_free(opt); jnibwa_free(opt_pe);
    jnibwa_destroyIndex(idx);
    printf("sanitized-ok %d cases\n", n_cases);
    return 0;
}
