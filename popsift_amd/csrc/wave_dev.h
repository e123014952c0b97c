/*
 * wave_dev.h -- device primitives of one wave (64 lanes) and of one workgroup of whole waves, each written once for every
 * kernel file: wave-uniform values, the inclusive prefix sum and the sum over a wave, the exclusive prefix sum over a
 * workgroup, one operation per distinct key among a wave's lanes; and clampi, which the blur and the DoG readers share.
 * Every function here is called by ALL lanes of its wave (the scan and the sum of a workgroup: by all its waves).
 */
#pragma once
#include <hip/hip_runtime.h>

namespace popsift_hip {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* a value every lane of the wave holds identically, moved to scalar registers */
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float uniformf(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ long long uniform64(long long v)
{
    const unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int)(v & 0xffffffffll));
    const unsigned int hi = __builtin_amdgcn_readfirstlane((unsigned int)(v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

/* Inclusive prefix sum over the 64 lanes in six DPP adds (row_shr 1, 2, 4, 8 inside the rows of 16, then row_bcast:15
 * and row_bcast:31 carry the row totals across), register to register -- no LDS round trips as with six shuffles. */
__device__ __forceinline__ int wave_incl_scan(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true); /* row_shr:1, out-of-row lanes read 0 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false); /* row_bcast:15 into rows 1 and 3 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false); /* row_bcast:31 into rows 2 and 3 */
    return v;
}

/* the last lane's inclusive prefix: the sum over the wave, in scalar registers */
__device__ __forceinline__ int wave_scan_total(int incl) { return __builtin_amdgcn_readlane(incl, 63); }

/* the sum over the 64 lanes, in every lane */
__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

/* Prefix sum over a workgroup of NW waves: `excl` = the sum of `v` over the lanes before this one, `total` = over all.
 * s_wsum[NW] is the workgroup's; the barrier between its writes and its reads is inside, a caller that comes back (a
 * loop) puts a barrier of its own before the next call. */
struct WgScan {
    int excl, total;
};
template <int NW>
__device__ __forceinline__ WgScan wg_scan(int v, int* s_wsum)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_incl_scan(v);
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    int woff = 0, total = 0;
    for (int w = 0; w < wave; w++) woff += s_wsum[w];
#pragma unroll
    for (int w = 0; w < NW; w++) total += s_wsum[w];
    return WgScan{woff + incl - v, total};
}

/* One call of op(key, mask, leader) per distinct `key` among the wave's lanes with `active` set, in the order of each
 * key's first lane: `mask` = the lanes that hold the key, `leader` = the first of them; all three are wave-uniform.
 * op runs with the whole wave converged, so it may ballot or read lanes itself.  max_rounds > 0 stops after that many
 * keys; returned: the active lanes whose key had no call (0 without a bound). */
template <typename Op>
__device__ __forceinline__ unsigned long long wave_each_key(int key, bool active, Op op, int max_rounds = 0)
{
    unsigned long long todo = __ballot(active);
    for (int round = 0; todo && (max_rounds <= 0 || round < max_rounds); round++) {
        const int                leader = __ffsll((long long)todo) - 1;
        const int                k = __builtin_amdgcn_readlane(key, leader);
        const unsigned long long mask = __ballot(active && key == k) & todo;
        op(k, mask, leader);
        todo &= ~mask;
    }
    return todo;
}

}  // namespace popsift_hip
