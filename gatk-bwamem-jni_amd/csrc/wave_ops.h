// wave_ops.h -- 64-lane wavefront collectives used by the DP kernels (CDNA wave64).
#pragma once
#include <hip/hip_runtime.h>

#define WAVE 64
#define NEG_INF_I32 (-0x40000000)

// inclusive prefix maximum across the wave (Hillis-Steele over lane shuffles)
static __device__ inline int wave_prefix_max(int v, int lane)
{
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        int u = __shfl_up(v, o);
        if (lane >= o) v = v > u ? v : u;
    }
    return v;
}

static __device__ inline int wave_max(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { int u = __shfl_xor(v, o); v = v > u ? v : u; }
    return v;
}

static __device__ inline int wave_bcast(int v, int src) { return __shfl(v, src); }

static __device__ inline unsigned long long wave_ballot(int pred) { return __ballot(pred); }

static __device__ inline bool wave_any(int pred) { return __ballot(pred) != 0ull; }
// ballot of a condition: the compare's own lane mask.  (__ballot takes an int: where the compiler does not see through the
// conversion it costs a select and a second compare per call)
#if defined(__HIP__)
static __device__ inline unsigned long long wave_ballot_b(bool pred) { return __builtin_amdgcn_ballot_w64(pred); }
#else
static __device__ inline unsigned long long wave_ballot_b(bool pred) { return __ballot(pred); }
#endif

// ---- DPP (data-parallel primitives) forms: cross-lane moves folded into VALU instructions, no LDS round trip.
// gfx9 controls: row_shr:n = 0x110+n (within a 16-lane row), wave_shr:1 = 0x138, row_bcast:15 = 0x142, row_bcast:31 = 0x143.
#define DPP_ROW_SHR(n) (0x110 + (n))
#define DPP_WAVE_SHR1 0x138
#define DPP_WAVE_SHL1 0x130
#define DPP_ROW_BCAST15 0x142
#define DPP_ROW_BCAST31 0x143

// inclusive prefix maximum over the 64 lanes.  Lanes without a source keep their own value: the DPP "old" operand is
// INT_MIN, the identity of v_max_i32, which lets the compiler fold each move into the max (one v_max_i32_dpp per step).
static __device__ inline int dpp_prefix_max(int v, int /*neg*/)
{
    const int id = (int)0x80000000;
    int t;
    t = __builtin_amdgcn_update_dpp(id, v, DPP_ROW_SHR(1), 0xf, 0xf, false); v = v > t ? v : t;
    t = __builtin_amdgcn_update_dpp(id, v, DPP_ROW_SHR(2), 0xf, 0xf, false); v = v > t ? v : t;
    t = __builtin_amdgcn_update_dpp(id, v, DPP_ROW_SHR(4), 0xf, 0xf, false); v = v > t ? v : t;
    t = __builtin_amdgcn_update_dpp(id, v, DPP_ROW_SHR(8), 0xf, 0xf, false); v = v > t ? v : t;
    t = __builtin_amdgcn_update_dpp(id, v, DPP_ROW_BCAST15, 0xa, 0xf, false); v = v > t ? v : t;
    t = __builtin_amdgcn_update_dpp(id, v, DPP_ROW_BCAST31, 0xc, 0xf, false); v = v > t ? v : t;
    return v;
}
// lane l <- lane l-1; lane 0 <- fill
static __device__ inline int dpp_shr1(int v, int fill) { return __builtin_amdgcn_update_dpp(fill, v, DPP_WAVE_SHR1, 0xf, 0xf, false); }
// lane l <- lane l+1; lane 63 <- fill
static __device__ inline int dpp_shl1(int v, int fill) { return __builtin_amdgcn_update_dpp(fill, v, DPP_WAVE_SHL1, 0xf, 0xf, false); }
// value of a (wave-uniform) lane as a scalar
static __device__ inline int wave_readlane(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

// ---- wave-uniform values.  The kernels that run one wavefront per item take every decision for the whole wave, but the
// compiler only sees that for values it can trace to scalar sources: anything that went through a shuffle, a vector load or a
// float division looks per-lane to it, is kept in a VGPR, and every `if` on it becomes an exec-mask region.  These helpers hand
// a value that the code knows to be equal in all 64 lanes back as a scalar (one v_readlane; free when the compiler knew
// already).  Only to be called with all 64 lanes active and in wave-uniform control flow: on the device the value is read from
// lane 0, and in the CPU emulation the call is a rendezvous of the 64 fibres.
static __device__ inline int wave_uni(int v) { return __builtin_amdgcn_readlane(v, 0); }
static __device__ inline unsigned wave_uni(unsigned v) { return (unsigned)__builtin_amdgcn_readlane((int)v, 0); }
static __device__ inline bool wave_uni(bool v) { return __builtin_amdgcn_readlane((int)v, 0) != 0; }
static __device__ inline long long wave_uni64(long long v)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v & 0xffffffffull), 0);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), 0);
    return (long long)((unsigned long long)hi << 32 | lo);
}
static __device__ inline float wave_uni(float v) { int b; __builtin_memcpy(&b, &v, 4); b = __builtin_amdgcn_readlane(b, 0); float r; __builtin_memcpy(&r, &b, 4); return r; }

// inclusive prefix sum over the 64 lanes (the DPP pattern of dpp_prefix_max with 0 as the identity)
static __device__ inline int dpp_prefix_sum(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_SHR(1), 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_SHR(2), 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_SHR(4), 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_SHR(8), 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_BCAST15, 0xa, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_BCAST31, 0xc, 0xf, false);
    return v;
}
// reductions and broadcasts whose result every lane uses as a scalar: a DPP scan and the last lane's value, or the value of a
// uniform source lane, instead of a tree of shuffles (LDS permutes, and per-lane results as far as the compiler can tell)
static __device__ inline int wave_max_u(int v) { return __builtin_amdgcn_readlane(dpp_prefix_max(v, 0), WAVE - 1); }
static __device__ inline int wave_sum_u(int v) { return __builtin_amdgcn_readlane(dpp_prefix_sum(v), WAVE - 1); }
static __device__ inline int wave_bcast_u(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
static __device__ inline unsigned long long wave_bcast_u64(unsigned long long v, int src)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v & 0xffffffffull), src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src);
    return (unsigned long long)hi << 32 | lo;
}
