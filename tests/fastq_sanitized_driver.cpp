// TEST INFRASTRUCTURE ONLY: a stand-alone driver of the FASTQ, qualities and read-group calls, compiled with AddressSanitizer + UBSan
// and linked against the sanitized emulation build by tests/test_fastq_device.py::test_fastq_sanitizers.
//   driver <index image> <directory>
// The directory holds manifest.txt, one case per line, and the files it names:
//   ok  <text1> <text2 or -> <paired>        upload_fastq, align, read group, encode, sort, compress, index
//   bad <text1> <text2 or -> <bad_record>    upload_fastq must return NULL with that record
//   req <request> <qualities> 0              batch_upload, set_qualities (and a refused blob), read group, align, encode, SAM text
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

// exact-size heap copies, so that a read past either end is seen
static char* exact(const std::string& s) { char* p = (char*)malloc(s.size() ? s.size() : 1); memcpy(p, s.data(), s.size()); return p; }

static void encode_all(bwaidx_t* idx, bwamem_batch_t* b, int paired)
{
    CHECK(bwamem_hip_batch_encode_bam(b, paired, nullptr, nullptr) == 0);
    const size_t n = bwamem_hip_batch_bam_bytes(b);
    std::vector<char> bam(n ? n : 1);
    CHECK(bwamem_hip_batch_bam_download(b, bam.data()) == 0);
    CHECK(bwamem_hip_batch_sort_bam(b) == 0);
    if (n) {
        CHECK(bwamem_hip_batch_compress_bam(b, 1) == 0);
        std::vector<char> z(bwamem_hip_batch_bgzf_bytes(b));
        CHECK(bwamem_hip_batch_bgzf_download(b, z.data()) == 0);
        size_t nb = 0;
        void* bai = bwamem_hip_batch_index_bam(b, 0, &nb);
        CHECK(bai && nb > 8);
        jnibwa_free(bai);
    }
    (void)idx;
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
    const char* rg = "@RG\tID:san\tSM:s";
    std::ifstream mf(dir + "manifest.txt");
    CHECK((bool)mf);
    std::string kind, f1, f2; long long val;
    int n_cases = 0;
    while (mf >> kind >> f1 >> f2 >> val) {
        g_case = kind + " " + f1 + " " + f2;
        ++n_cases;
        if (kind == "req") {
            const std::string req = slurp(dir + f1), q = slurp(dir + f2);
            char* rp = exact(req); char* qp = exact(q);
            bwamem_batch_t* b = bwamem_hip_batch_upload(idx, rp, req.size());
            CHECK(b);
            CHECK(bwamem_hip_batch_set_qualities(b, qp, q.size()) == 0);
            std::string bad = q; bad[bad.size() / 2] = bad[bad.size() / 2] ? 0 : 'I';
            char* bp = exact(bad);
            CHECK(bwamem_hip_batch_set_qualities(b, bp, bad.size()) != 0);
            CHECK(bwamem_hip_batch_set_qualities(b, qp, q.size() - 1) != 0);
            CHECK(bwamem_hip_batch_set_read_group(b, "@RG\tSM:s") != 0);
            CHECK(bwamem_hip_batch_set_read_group(b, rg) == 0);
            CHECK(bwamem_hip_batch_keep_offsets(b, 1) == 0 && bwamem_hip_batch_align(idx, opt, nullptr, b, 0) == 0);
            const size_t nr = bwamem_hip_batch_result_bytes(b);
            std::vector<char> resp(nr ? nr : 1);
            CHECK(bwamem_hip_batch_download(b, resp.data()) == 0);
            size_t ns = 0;
            char* sam = bwamem_hip_response_to_sam_q(idx, rp, resp.data(), nr, nullptr, 0, qp, "san", &ns);
            CHECK(sam && ns > 0 && strstr(sam, "RG:Z:san"));
            jnibwa_free(sam);
            encode_all(idx, b, 0);
            bwamem_hip_batch_free(b);
            free(rp); free(qp); free(bp);
            continue;
        }
        const std::string t1 = slurp(dir + f1), t2 = f2 == "-" ? std::string() : slurp(dir + f2);
        char* p1 = exact(t1); char* p2 = f2 == "-" ? nullptr : exact(t2);
        int64_t bad = -7;
        bwamem_batch_t* b = bwamem_hip_batch_upload_fastq(idx, p1, t1.size(), p2, t2.size(), &bad);
        if (kind == "bad") { CHECK(!b && bad == val); }
        else {
            CHECK(b && bad == -1);
            const int paired = (int)val;
            CHECK(bwamem_hip_batch_set_read_group(b, rg) == 0);
            CHECK(bwamem_hip_batch_keep_offsets(b, 1) == 0 && bwamem_hip_batch_align(idx, paired ? opt_pe : opt, nullptr, b, 0) == 0);
            encode_all(idx, b, paired);
            bwamem_hip_batch_free(b);
        }
        free(p1); free(p2);
    }
    CHECK(n_cases >= 3);
    size_t nh = 0;
    void* hdr = bwamem_hip_bam_header_rg(idx, 1, rg, &nh);
    CHECK(hdr && nh > 0);
    jnibwa_free(hdr);
    CHECK(!bwamem_hip_bam_header_rg(idx, 0, "@RG\tID:", &nh) && !bwamem_hip_sam_header_rg(idx, "@RG", &nh));
    jnibwa_free(opt); jnibwa_free(opt_pe);
    jnibwa_destroyIndex(idx);
    printf("sanitized-ok %d cases\n", n_cases);
    return 0;
}
