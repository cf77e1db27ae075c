// tests/gpu_units/drive_ab.cpp -- the torch-free driver as a switch sweep: for each setting ("NAME=V,NAME=V", "-" = none) set
// the variables, open the image afresh (the seeding stream and its priority are made per index handle), align the request
// warm-up + steps times and print the wall time per step and the isolated-kernel sums of the stats block.
// usage: drive_ab <image> <request-file> <steps> <warmup> <setting> [setting ...]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fcntl.h>
#include <unistd.h>
#include <chrono>
#include <string>
#include <vector>
#include "../../include/bwamem_hip.h"

int main(int argc, char** argv)
{
    if (argc < 6) { fprintf(stderr, "usage: drive_ab <image> <request-file> <steps> <warmup> <setting> [setting ...]\n"); return 2; }
    const int steps = atoi(argv[3]), warmup = atoi(argv[4]);
    FILE* fp = fopen(argv[2], "rb");
    if (!fp) { perror(argv[2]); return 1; }
    fseek(fp, 0, SEEK_END); long n = ftell(fp); fseek(fp, 0, SEEK_SET);
    std::vector<char> req((size_t)n);
    if (fread(req.data(), 1, (size_t)n, fp) != (size_t)n) return 1;
    fclose(fp);
    bwamem_hip_set_device(0);
    for (int a = 5; a < argc; ++a) {
        std::vector<std::string> names;
        if (strcmp(argv[a], "-") != 0) {
            std::string s(argv[a]);
            for (size_t at = 0; at < s.size();) {
                size_t e = s.find(',', at); if (e == std::string::npos) e = s.size();
                const std::string kv = s.substr(at, e - at); const size_t q = kv.find('=');
                if (q != std::string::npos) { setenv(kv.substr(0, q).c_str(), kv.substr(q + 1).c_str(), 1); names.push_back(kv.substr(0, q)); }
                at = e + 1;
            }
        }
        int fd = open(argv[1], O_RDONLY);
        if (fd < 0) { perror(argv[1]); return 1; }
        bwaidx_t* idx = jnibwa_openIndex(fd);                        // takes the descriptor
        if (!idx) { fprintf(stderr, "openIndex failed\n"); return 1; }
        bwamem_batch_t* b = bwamem_hip_batch_upload(idx, req.data(), (size_t)n);
        if (!b) return 1;
        mem_opt_t* opt = jnibwa_createDefaultOptions();
        for (int i = 0; i < warmup; ++i)
            if (bwamem_hip_batch_align(idx, opt, 0, b, 0) != 0) { fprintf(stderr, "align failed\n"); return 1; }
        bwamem_hip_stats_enable(1); bwamem_hip_stats_reset();
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < steps; ++i)
            if (bwamem_hip_batch_align(idx, opt, 0, b, 0) != 0) { fprintf(stderr, "align failed\n"); return 1; }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / (steps > 0 ? steps : 1);
        bwamem_stats_t st; bwamem_hip_stats_get(&st);
        bwamem_hip_stats_enable(0);
        const double k = 1.0 / (steps > 0 ? steps : 1);              // HIP-event sums per step: isolated times only with BWAMEM_HIP_STREAMS=1,BWAMEM_HIP_SEED_AHEAD=0
        printf("{\"setting\": \"%s\", \"ms_per_step\": %.2f, \"steps\": %d, \"warmup\": %d, \"n_ext\": %llu, \"result_bytes\": %zu, \"retries\": %llu, "
               "\"event_ms\": {\"seed\": %.1f, \"sa\": %.1f, \"chain\": %.1f, \"extend\": %.1f, \"post\": %.1f, \"final\": %.1f}}\n", argv[a], ms, steps, warmup,
               (unsigned long long)st.n_ext, bwamem_hip_batch_result_bytes(b), (unsigned long long)st.n_retries,
               st.ms_seed * k, st.ms_sa * k, st.ms_chain * k, st.ms_extend * k, st.ms_post * k, st.ms_final * k);
        fflush(stdout);
        bwamem_hip_batch_free(b);
        jnibwa_free(opt);
        jnibwa_destroyIndex(idx);
        for (auto& nm : names) unsetenv(nm.c_str());
    }
    return 0;
}
