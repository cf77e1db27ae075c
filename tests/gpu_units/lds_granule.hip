// tests/gpu_units/lds_granule.hip -- how many one-wave workgroups asking for a given amount of dynamic LDS the device keeps
// resident at once.  Every workgroup notes the wall clock, idles for a fixed time and notes the clock again; the host takes the
// largest number of intervals that overlap.  With more workgroups than fit, that number is n_cu x (workgroups per CU), and the
// sizes at which it steps down give the LDS allocation granule (the plan of launch_seed in k_seed.hip rounds up to it).
// usage: lds_granule [bytes ...]      prints one line per size
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

__global__ void k_hold(unsigned long long* t, long long ticks)
{
    extern __shared__ int lds[];
    if (threadIdx.x == 0) lds[0] = (int)blockIdx.x;                  // the allocation is used: it cannot be dropped
    __syncthreads();
    const unsigned long long t0 = wall_clock64();
    while ((long long)(wall_clock64() - t0) < ticks) __builtin_amdgcn_s_sleep(32);
    if (threadIdx.x == 0) { t[2 * blockIdx.x] = t0; t[2 * blockIdx.x + 1] = wall_clock64() + (unsigned long long)(lds[0] < 0); }
}

int main(int argc, char** argv)
{
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, 0) != hipSuccess) { fprintf(stderr, "no device\n"); return 1; }
    int lds_cu = 0;
    (void)hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, 0);
    printf("n_cu=%d lds_per_cu=%d lds_per_block=%zu\n", p.multiProcessorCount, lds_cu, p.sharedMemPerBlock);
    const int grid = p.multiProcessorCount * 40;                     // more than any size below lets in at once (32 waves per CU)
    unsigned long long* d = nullptr;
    if (hipMalloc(&d, (size_t)grid * 16) != hipSuccess) return 1;
    std::vector<unsigned long long> h((size_t)grid * 2);
    std::vector<int> sizes;
    for (int i = 1; i < argc; ++i) sizes.push_back(atoi(argv[i]));
    if (sizes.empty()) sizes = {8193, 8705, 9217, 16144, 16385};
    for (int bytes : sizes) {
        if (bytes < 4 || (size_t)bytes > p.sharedMemPerBlock) continue;
        hipLaunchKernelGGL(k_hold, dim3(grid), dim3(64), (size_t)bytes, 0, d, 20000ll);   // 200 us at the 100 MHz wall clock
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h.data(), d, (size_t)grid * 16, hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "run failed\n"); return 1; }
        std::vector<std::pair<unsigned long long, int>> ev;
        for (int i = 0; i < grid; ++i) { ev.push_back({h[2 * i], 1}); ev.push_back({h[2 * i + 1], -1}); }
        std::sort(ev.begin(), ev.end());
        int cur = 0, best = 0;
        for (auto& e : ev) { cur += e.second; best = std::max(best, cur); }
        printf("lds=%d resident=%d per_cu=%.2f\n", bytes, best, (double)best / p.multiProcessorCount);
    }
    (void)hipFree(d);
    return 0;
}
