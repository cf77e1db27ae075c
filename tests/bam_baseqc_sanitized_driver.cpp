// TEST INFRASTRUCTURE ONLY: a stand-alone driver of the base-level QC calls, compiled with AddressSanitizer + UBSan and linked against
// the sanitized emulation build by tests/test_bam_baseqc.py::test_baseqc_sanitizers.
//   driver <index image> <directory>
// The directory holds manifest.txt, one case per line, and the files it names:
//   rec <tag>    <tag>.bam (a stream of BAM records): bwamem_hip_baseqc_add_records_device into a new accumulator must give <tag>.want
//                -- 64-bit words: bwamem_baseqc_counts_t, then the tables in the order of BWAMEM_HIP_BASEQC_* -- whole and in two
//                parts, and the serialized form added to another accumulator must double every word
//   bad <tag>    <tag>.bam must be refused and leave an accumulator that holds the first case byte for byte as it was
// and windows.want, the 101 words bwamem_hip_index_gc_windows must give.
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

static std::vector<uint64_t> words_of(const bwamem_baseqc_t* q)
{
    bwamem_baseqc_counts_t c;
    CHECK(bwamem_hip_baseqc_counts(q, &c) == 0);
    std::vector<uint64_t> w(sizeof c / 8);
    memcpy(w.data(), &c, sizeof c);
    for (int which = BWAMEM_HIP_BASEQC_BASE; which <= BWAMEM_HIP_BASEQC_GCB_QUAL_N; ++which) {
        const int64_t n = bwamem_hip_baseqc_array(q, which, nullptr, 0);
        CHECK(n > 0);
        uint64_t* a = (uint64_t*)malloc((size_t)n * 8);                 // exactly n words
        CHECK(bwamem_hip_baseqc_array(q, which, a, (size_t)n) == n);
        w.insert(w.end(), a, a + n);
        free(a);
    }
    CHECK(bwamem_hip_baseqc_array(q, BWAMEM_HIP_BASEQC_GCB_QUAL_N + 1, nullptr, 0) < 0);
    return w;
}

static std::string blob_of(const bwamem_baseqc_t* q)
{
    size_t n = 0;
    void* p = bwamem_hip_baseqc_serialize(q, &n);
    CHECK(p && n > 32);
    std::string s((const char*)p, n);
    jnibwa_free(p);
    return s;
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s <image> <directory>\n", argv[0]); return 2; }
    const std::string dir = std::string(argv[2]) + "/";
    const int fd = open(argv[1], O_RDONLY);
    CHECK(fd >= 0);
    bwaidx_t* idx = jnibwa_openIndex(fd);
    CHECK(idx);
    {
        g_case = "windows";
        const std::string want = slurp(dir + "windows.want");
        uint64_t* win = (uint64_t*)malloc(101 * 8);                     // exactly 101 words
        CHECK(bwamem_hip_index_gc_windows(idx, win) == 0 && want.size() == 101 * 8 && memcmp(win, want.data(), want.size()) == 0);
        free(win);
    }
    std::ifstream mf(dir + "manifest.txt");
    CHECK((bool)mf);
    bwamem_baseqc_t* kept = bwamem_hip_baseqc_create(idx);             // holds the first case; the refused streams must not touch it
    CHECK(kept);
    std::string kept_blob;
    std::string kind, tag;
    int n_cases = 0, n_bad = 0;
    while (mf >> kind >> tag) {
        g_case = kind + " " + tag;
        ++n_cases;
        const std::string bam = slurp(dir + tag + ".bam");
        char* rp = exact(bam);
        if (kind == "rec") {
            const std::string want = slurp(dir + tag + ".want");
            bwamem_baseqc_t* q = bwamem_hip_baseqc_create(idx);
            bwamem_baseqc_t* parts = bwamem_hip_baseqc_create(idx);
            CHECK(q && parts);
            CHECK(bwamem_hip_baseqc_add_records_device(q, rp, bam.size()) == 0);
            const std::vector<uint64_t> w = words_of(q);
            CHECK(w.size() * 8 == want.size() && memcmp(w.data(), want.data(), want.size()) == 0);
            size_t cut = 0;                                             // the first record boundary at or beyond the middle
            while (cut < bam.size() / 2) { int32_t bs; memcpy(&bs, bam.data() + cut, 4); cut += 4 + (size_t)bs; }
            char* p0 = exact(bam.substr(0, cut)); char* p1 = exact(bam.substr(cut));
            CHECK(bwamem_hip_baseqc_add_records_device(parts, p0, cut) == 0 && bwamem_hip_baseqc_add_records_device(parts, p1, bam.size() - cut) == 0);
            free(p0); free(p1);
            const std::string blob = blob_of(q);
            CHECK(blob == blob_of(parts));
            char* bp = exact(blob);
            CHECK(bwamem_hip_baseqc_add_serialized(parts, bp, blob.size()) == 0);
            CHECK(bwamem_hip_baseqc_add_serialized(parts, bp, blob.size() - 1) != 0 && bwamem_hip_baseqc_add_serialized(parts, bp, 16) != 0);
            free(bp);
            const std::vector<uint64_t> w2 = words_of(parts);
            for (size_t k = 0; k < w.size(); ++k) CHECK(w2[k] == 2 * w[k]);
            for (int kd = BWAMEM_HIP_BASEQC_CYCLES; kd <= BWAMEM_HIP_BASEQC_GC; ++kd) {
                size_t n = 0;
                char* t = bwamem_hip_baseqc_report(parts, kd, &n);
                CHECK(t && strlen(t) == n && (n > 0 || kd == BWAMEM_HIP_BASEQC_CYCLES));      // (no end with records: no cycle table)
                jnibwa_free(t);
            }
            if (kept_blob.empty()) { CHECK(bwamem_hip_baseqc_add_records_device(kept, rp, bam.size()) == 0); kept_blob = blob_of(kept); }
            bwamem_hip_baseqc_free(q); bwamem_hip_baseqc_free(parts);
        } else {
            CHECK(kind == "bad" && !kept_blob.empty());
            CHECK(bwamem_hip_baseqc_add_records_device(kept, rp, bam.size()) != 0);
            CHECK(blob_of(kept) == kept_blob);
            ++n_bad;
        }
        free(rp);
    }
    CHECK(n_cases >= 5 && n_bad >= 10);
    bwamem_hip_baseqc_free(kept);
    jnibwa_destroyIndex(idx);
    printf("sanitized-ok %d cases\n", n_cases);
    return 0;
}
