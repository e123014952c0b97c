/*
 * top2.h -- what the matchers share on the device (match.hip, match_mfma.hip, match_u8.hip, match_guided.hip): the two
 * nearest candidates of a row under lexicographic (distance, index), the reference's 32-lane distance, the row a top-2
 * becomes, and the kernel that merges the per-split candidates of a sweep into rows.
 *
 * "The two smallest with ties to the lower index" is order-independent, which is what allows lanes, and several workgroups
 * per row block, to keep private candidates that are merged at the end.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "sift_types.h"

namespace popsift_hip {

/* D = float: squared distances, "none" is +INFINITY.  D = int: exact integer distances, "none" is U_NONE.  16 bytes. */
template <class D>
struct Top2 {
    D   v1, v2; /* the two smallest distances */
    int i1, i2; /* their indices              */
};

constexpr int U_NONE = INT_MAX; /* Top2<int>: "no candidate yet"; becomes +INFINITY in the row */

template <class D>
__device__ __forceinline__ bool lex_less(D d, int i, D e, int j)
{
    return d < e || (d == e && i < j);
}

template <class D>
__device__ __forceinline__ void top2_insert(Top2<D>& t, D d, int i)
{
    if (lex_less(d, i, t.v1, t.i1)) {
        t.v2 = t.v1;
        t.i2 = t.i1;
        t.v1 = d;
        t.i1 = i;
    } else if (lex_less(d, i, t.v2, t.i2)) {
        t.v2 = d;
        t.i2 = i;
    }
}

template <class D>
__device__ __forceinline__ void top2_merge(Top2<D>& t, const Top2<D>& o)
{
    top2_insert(t, o.v1, o.i1);
    top2_insert(t, o.v2, o.i2);
}

typedef float top2_v4f __attribute__((ext_vector_type(4)));

/* The reference's distance of one pair, 32 lanes per pair and one float4 chunk of each descriptor per lane (l2_in_t0,
 * features.cu:157-176): the per-lane sum of squares as an FMA chain (nvcc contracts it so), then the shuffle_down
 * (16, 8, 4, 2, 1) tree.  Valid in lane 0 of each 32-lane group. */
__device__ __forceinline__ float l2_in_t0(top2_v4f a, top2_v4f b)
{
    const float x = a.x - b.x, y = a.y - b.y, z = a.z - b.z, w = a.w - b.w;
    float       res = fmaf(w, w, fmaf(z, z, fmaf(y, y, x * x)));
    res += __shfl_down(res, 16, 32);
    res += __shfl_down(res, 8, 32);
    res += __shfl_down(res, 4, 32);
    res += __shfl_down(res, 2, 32);
    res += __shfl_down(res, 1, 32);
    return res;
}

__device__ __forceinline__ float as_dist(float d) { return d; }
__device__ __forceinline__ float as_dist(int d) { return d == U_NONE ? INFINITY : (float)d; }

/* the row of a top-2; accept as in features.cu:217-218, formed from the float distances */
template <class D>
__device__ __forceinline__ popsift_hip_match top2_row(const Top2<D>& t)
{
    popsift_hip_match m;
    m.best = t.i1;
    m.second = t.i2;
    m.dist_best = as_dist(t.v1);
    m.dist_second = as_dist(t.v2);
    m.accept = (__fdiv_rn(m.dist_best, m.dist_second) < 0.8f) ? 1 : 0;
    return m;
}

/*
 * Merge the n_split candidates of every row and write the rows.  rows != null: only the list positions
 * [first_row, min(*n_rows, row_end)) -- the rows the screening pass could not decide; positions index `partial`, the
 * list's entries index `out`.
 * A candidate is merged whatever it holds.  For the exact float sweep that is the rule: a real index can carry an INFINITY
 * distance, and k_match's (INFINITY, 0) placeholders take part like any candidate.  For the guided sweep, whose "none" is
 * (INFINITY, -1), it is a no-op: its drain admits only d < INFINITY, so in every partial and in every merged t an INFINITY
 * distance comes with index -1, and lex_less(INFINITY, -1, e, j) is false both for a finite e and for (INFINITY, -1).
 */
template <class D>
__global__ __launch_bounds__(256) void k_top2_finish(const Top2<D>* __restrict__ partial, int l_len, int n_split,
                                                     popsift_hip_match* __restrict__ out, const int* __restrict__ rows,
                                                     const int* __restrict__ n_rows, int first_row, int row_end)
{
    const int l = first_row + blockIdx.x * 256 + threadIdx.x;
    if (rows) l_len = min(min(*n_rows, row_end), l_len);
    if (l >= l_len) return;
    Top2<D> t = partial[(size_t)l * n_split];
    for (int k = 1; k < n_split; k++) {
        const Top2<D> o = partial[(size_t)l * n_split + k]; /* a copy: one 16-byte load, not four under the inserts' branches */
        top2_merge(t, o);
    }
    out[rows ? rows[l] : l] = top2_row(t);
}

/* rows [first_row, row_end) of a list, or with rows == null all of [0, l_len): pass first_row = 0, row_end = l_len */
template <class D>
void launch_top2_finish(const Top2<D>* partial, int l_len, int n_split, popsift_hip_match* out, const int* rows,
                        const int* n_rows, int first_row, int row_end, hipStream_t s)
{
    hipLaunchKernelGGL(k_top2_finish<D>, dim3((row_end - first_row + 255) / 256), dim3(256), 0, s, partial, l_len, n_split, out,
                       rows, n_rows, first_row, row_end);
}

/* Workgroups over the searched side for a sweep of l_len rows against r_len: enough to reach target_groups workgroups,
 * at most one per tile.  A workgroup owns rows_per_group rows and walks tiles of cols_per_tile. */
inline int splits(int l_len, int r_len, int rows_per_group, int cols_per_tile, int target_groups)
{
    const int groups = std::max((l_len + rows_per_group - 1) / rows_per_group, 1);
    const int tiles = std::max((r_len + cols_per_tile - 1) / cols_per_tile, 1);
    return std::max(std::min((target_groups + groups - 1) / groups, tiles), 1);
}

/* bytes of a sweep's per-split candidates */
inline size_t partial_bytes(int l_len, int n_split, size_t record) { return (size_t)std::max(l_len, 1) * n_split * record; }

}  // namespace popsift_hip
