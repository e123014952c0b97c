/*
 * ext_list.h -- the rules of the keypoint lists, each written once.  The object every stage between refinement and the
 * descriptors works on is the per-octave extrema lists of one image (iext / iext2: octave o's records start at
 * o * max_extrema, their number is in Counters::ext_ct[o]), read as ONE flattened list, octave after octave:
 *   ext_count    how many records octave o's list holds
 *   ext_prefix   the exclusive prefix of those counts in LDS: s_ps[o] = flat index of octave o's first record
 *   ext_octave   flat index -> octave (its position there: g - s_ps[o])
 *   ExtChunk     "this workgroup is chunk c of octave o" for the kernels launched with one workgroup per chunk of a list
 * The wave and workgroup primitives the same kernels are built from are in wave_dev.h.
 */
#pragma once
#include <hip/hip_runtime.h>

#include "sift_types.h"
#include "wave_dev.h"

namespace popsift_hip {

/* The number of records of octave o's list.  ext_ct[o] counts every extremum refinement found, the list holds the first
 * max_extrema of them (k_refine's guarded store), and the counter is clamped by whoever reads it (the reference clamps
 * with atomicMin in the extrema kernel, s_extrema.cu:558).  The lower clamp changes no result: a count is a sum of
 * non-negative atomicAdds or a value a commit kernel wrote.  It stays because record indices are formed from this value,
 * and none must ever be formed from a negative count, whatever a counter holds. */
__host__ __device__ __forceinline__ int ext_count(const Counters* ct, int max_extrema, int o)
{
    return min(max(ct->ext_ct[o], 0), max_extrema);
}

/* s_ps[0 .. PS_MAX_OCT] = exclusive prefix of the counts; ends with a barrier; returns the total.  EVERY entry is filled:
 * those from n_oct upward hold the total (k_scan_apply and k_strongest_select hand them out).  Lane o of the workgroup's
 * first wave takes octave o (PS_MAX_OCT < 64) and the wave scans: one load, six DPP adds and one LDS write, where a loop
 * in lane 0 is some hundred scalar instructions ahead of every workgroup's first barrier.  Called by the whole workgroup. */
__device__ __forceinline__ int ext_prefix(int* s_ps, const Counters* ct, int max_extrema, int n_oct)
{
    static_assert(PS_MAX_OCT < 64, "one lane per prefix entry");
    if (threadIdx.x < 64) {
        const int o = threadIdx.x;
        const int n = (o < n_oct) ? ext_count(ct, max_extrema, o) : 0;
        const int incl = wave_incl_scan(n);
        if (o <= PS_MAX_OCT) s_ps[o] = incl - n;
    }
    __syncthreads();
    return s_ps[PS_MAX_OCT];
}

/* the octave of flat index g (0 <= g < total; anything else gives the first or the last octave) */
__device__ __forceinline__ int ext_octave(const int* s_ps, int n_oct, int g)
{
    int o = 0;
    while (o + 1 < n_oct && g >= s_ps[o + 1]) o++;
    return o;
}

/* Workgroup blockIdx.x of a launch of n_oct * chunks_per_oct workgroups: chunk `chunk` of octave `o`, whose records are
 * i0 .. i0 + chunk_len - 1 of that octave's list.  The launch is sized by the capacity, so most chunks lie beyond the
 * list: within(n) takes the list's length and says whether the workgroup has any record at all. */
struct ExtChunk {
    int o, chunk, i0, n;
    __device__ __forceinline__ ExtChunk(int chunks_per_oct, int chunk_len)
        : o(blockIdx.x / chunks_per_oct), chunk(blockIdx.x % chunks_per_oct), i0(chunk * chunk_len), n(0) {}
    __device__ __forceinline__ bool within(int count)
    {
        n = count;
        return i0 < n;
    }
};

}  // namespace popsift_hip
