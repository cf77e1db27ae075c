// TEST INFRASTRUCTURE ONLY: a stand-alone driver of the compressed-FASTQ calls, compiled with AddressSanitizer + UBSan and linked
// against the sanitized emulation build by tests/test_fastq_gz.py::test_fastq_gz_sanitizers.
//   driver <index image> <directory>
// The directory holds manifest.txt, one case per line, and the files it names:
//   inflate <stream> <expected bytes> 0        bgzf_inflate_device must give exactly these bytes, twice (inflate1: once)
//   refuse  <stream> - <bad_member>            bgzf_inflate_device must return NULL with that member
//   fq      <stream> <plain text> <paired>     upload_fastq_gz, align, encode == upload_fastq of the text, align, encode
//   fq2     <stream 1> <stream 2> <paired>     the same for two BGZF streams; the texts come from bgzf_inflate_device
//   badrec  <stream> - <bad_record>            upload_fastq_gz must return NULL with that record and no member
//   badmem2 <stream 1> <stream 2> <bad_member> upload_fastq_gz must return NULL with that member and no record
// Every input is an exact-size heap copy, so that a read past either end is seen.
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
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

static char* exact(const std::string& s) { char* p = (char*)malloc(s.size() ? s.size() : 1); memcpy(p, s.data(), s.size()); return p; }

// align and encode a batch -> the records; frees the batch
static std::string records(bwaidx_t* idx, mem_opt_t* opt, bwamem_batch_t* b, int paired)
{
    CHECK(bwamem_hip_batch_keep_offsets(b, 1) == 0 && bwamem_hip_batch_align(idx, opt, nullptr, b, 0) == 0);
    CHECK(bwamem_hip_batch_encode_bam(b, paired, nullptr, nullptr) == 0);
    std::string bam(bwamem_hip_batch_bam_bytes(b), '\0');
    CHECK(bwamem_hip_batch_bam_download(b, bam.empty() ? nullptr : &bam[0]) == 0);
    bwamem_hip_batch_free(b);
    return bam;
}

static std::string inflated(bwaidx_t* idx, const std::string& z)
{
    char* p = exact(z);
    size_t n = 0; int64_t bad = -7;
    void* r = bwamem_hip_bgzf_inflate_device(idx, p, z.size(), &n, &bad);
    CHECK(r && bad == -1);
    std::string out((const char*)r, n);
    jnibwa_free(r); free(p);
    return out;
}

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
    std::string kind, f1, f2; long long val;
    int n_cases = 0;
    while (mf >> kind >> f1 >> f2 >> val) {
        g_case = kind + " " + f1 + " " + f2;
        ++n_cases;
        const std::string a = slurp(dir + f1), b2 = f2 == "-" ? std::string() : slurp(dir + f2);
        if (kind == "inflate") { CHECK(inflated(idx, a) == b2 && inflated(idx, a) == b2); continue; }
        if (kind == "inflate1") { CHECK(inflated(idx, a) == b2); continue; }
        char* pa = exact(a);
        if (kind == "refuse") {
            size_t n = 7; int64_t bad = -7;
            CHECK(!bwamem_hip_bgzf_inflate_device(idx, pa, a.size(), &n, &bad) && n == 0 && bad == val);
        } else if (kind == "fq" || kind == "fq2") {
            const int paired = (int)val;
            const bool two = kind == "fq2";
            char* pb = two ? exact(b2) : nullptr;
            int64_t bad = -7, bm = -7;
            bwamem_batch_t* g = bwamem_hip_batch_upload_fastq_gz(idx, pa, a.size(), pb, two ? b2.size() : 0, &bad, &bm);
            CHECK(g && bad == -1 && bm == -1);
            const std::string got = records(idx, paired ? opt_pe : opt, g, paired);
            const std::string t1 = two ? inflated(idx, a) : b2, t2 = two ? inflated(idx, b2) : std::string();
            char* q1 = exact(t1); char* q2 = two ? exact(t2) : nullptr;
            bwamem_batch_t* w = bwamem_hip_batch_upload_fastq(idx, q1, t1.size(), q2, t2.size(), &bad);
            CHECK(w && bad == -1);
            CHECK(records(idx, paired ? opt_pe : opt, w, paired) == got && !got.empty());
            free(pb); free(q1); free(q2);
        } else if (kind == "badrec") {
            int64_t bad = -7, bm = -7;
            CHECK(!bwamem_hip_batch_upload_fastq_gz(idx, pa, a.size(), nullptr, 0, &bad, &bm) && bad == val && bm == -1);
        } else if (kind == "badmem2") {
            char* pb = exact(b2);
            int64_t bad = -7, bm = -7;
            CHECK(!bwamem_hip_batch_upload_fastq_gz(idx, pa, a.size(), pb, b2.size(), &bad, &bm) && bad == -1 && bm == val);
            free(pb);
        } else CHECK(!"a known kind");
        free(pa);
    }
    CHECK(n_cases >= 10);
    jnibwa_free(opt); jnibwa_free(opt_pe);
    jnibwa_destroyIndex(idx);
    printf("sanitized-ok %d cases\n", n_cases);
    return 0;
}
