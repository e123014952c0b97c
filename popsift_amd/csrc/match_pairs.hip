/*
 * match_pairs.hip -- from the 2-NN rows of a sweep (match.hip / match_mfma.hip / match_u8.hip / match_guided.hip) to a list
 * of pairs: ratio test, distance cap and mutual-nearest-neighbour check (popsift_hip_match_pairs, include/popsift_hip.h).
 *
 * The sweeps are the expensive part and are not touched.  Everything here is one pass over 20-byte rows:
 *   k_pair_mark     with the cross-check: flag the nearest right descriptor of every row that passes the ratio test
 *                   and the cap -- the only right descriptors whose nearest LEFT neighbour can matter
 *   k_count /       order-preserving compaction of the indices a predicate keeps, in two launches: per-workgroup
 *   k_compact       counts, then every workgroup adds up the counts before it (a few hundred values), ranks its own
 *                   elements with a ballot scan and writes.  No atomic: the position of an element is a function of
 *                   the predicate alone, so the output is the same bytes on every run.  Used twice: flagged right
 *                   indices -> the ascending list J (and every member's rank), surviving rows -> the pair records.
 *   k_gather_rows   the descriptors of J into a contiguous buffer: the left operand of the reverse sweep
 */
#include "devfeatures.h"
#include "kernels.h"

namespace popsift_hip {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int C_BLOCK = 256; /* elements (= lanes) per workgroup of the compaction kernels */

/* conditions 2 and 3 of the rule; __fdiv_rn and '<' as top2_row (top2.h) forms `accept`: a NaN quotient
 * (0 / 0, inf / inf) fails */
__device__ __forceinline__ bool row_passes(const popsift_hip_match& m, float ratio, float max_dist2)
{
    return (ratio == 0.0f || __fdiv_rn(m.dist_best, m.dist_second) < ratio) && m.dist_best <= max_dist2;
}

/* a right descriptor some passing row points to (several rows may store the same 1) */
struct Flagged {
    const int* flags;
    __device__ bool operator()(int j) const { return flags[j] != 0; }
};

/* row i yields a pair: it has a candidate (the guided matcher's rows may have none: best = -1; the other sweeps' always
 * do), it passes, and with the cross-check it is the nearest left descriptor of its best right one.  With a rank,
 * back[rank[j]] is the reverse sweep's row of right descriptor j: rank is defined for every flagged j, and a passing
 * row's best is flagged.  Without one, `back` holds a row for every right descriptor. */
struct PairKept {
    const popsift_hip_match* fwd;
    const popsift_hip_match* back; /* null: no cross-check */
    const int*               rank; /* null: back[j] is the row of j */
    float                    ratio, max_dist2;
    __device__ bool operator()(int i) const
    {
        const popsift_hip_match m = fwd[i];
        if (m.best < 0 || !row_passes(m, ratio, max_dist2)) return false;
        return !back || back[rank ? rank[m.best] : m.best].best == i;
    }
};

struct WriteIndex {
    int* list;
    int* rank;
    __device__ void operator()(int pos, int j) const
    {
        list[pos] = j;
        rank[j] = pos;
    }
};

struct WritePair {
    const popsift_hip_match* fwd;
    popsift_hip_pair*        pairs; /* room for every row */
    __device__ void operator()(int pos, int i) const
    {
        const popsift_hip_match m = fwd[i];
        pairs[pos] = popsift_hip_pair{i, m.best, m.dist_best, m.dist_second};
    }
};

/* number of kept elements in front of this lane's within the workgroup, and the workgroup's count */
__device__ __forceinline__ int block_rank(bool keep, int* total)
{
    __shared__ int           s_wave[C_BLOCK / 64];
    const unsigned long long b = __ballot(keep);
    const int                lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_wave[wave] = __popcll(b);
    __syncthreads();
    int before = __popcll(b & ((1ull << lane) - 1ull)), all = 0;
#pragma unroll
    for (int w = 0; w < C_BLOCK / 64; w++) {
        if (w < wave) before += s_wave[w];
        all += s_wave[w];
    }
    *total = all;
    return before;
}

template <class Keep>
__global__ __launch_bounds__(C_BLOCK) void k_count(Keep keep, int n, int* __restrict__ counts)
{
    const int e = blockIdx.x * C_BLOCK + threadIdx.x;
    int       total;
    (void)block_rank(e < n && keep(e), &total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

/* *n_kept: the number of kept elements, written by the last workgroup */
template <class Keep, class Write>
__global__ __launch_bounds__(C_BLOCK) void k_compact(Keep keep, Write write, int n, const int* __restrict__ counts,
                                                     int* __restrict__ n_kept)
{
    __shared__ int s_part[C_BLOCK / 64];
    int            part = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += C_BLOCK) part += counts[b];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) part += __shfl_down(part, d);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = part;
    __syncthreads();
    int first = 0;
#pragma unroll
    for (int w = 0; w < C_BLOCK / 64; w++) first += s_part[w];

    const int  e = blockIdx.x * C_BLOCK + threadIdx.x;
    const bool k = e < n && keep(e);
    int        total;
    const int  before = block_rank(k, &total);
    if (k) write(first + before, e);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *n_kept = first + total;
}

__global__ __launch_bounds__(256) void k_pair_mark(const popsift_hip_match* __restrict__ fwd, int l_len, float ratio,
                                                   float max_dist2, int* __restrict__ flags)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= l_len) return;
    const popsift_hip_match m = fwd[i];
    if (row_passes(m, ratio, max_dist2)) flags[m.best] = 1;
}

/* one 16-byte chunk per lane */
template <int ROW_BYTES>
__global__ __launch_bounds__(256) void k_gather_rows(const char* __restrict__ desc, const int* __restrict__ list, int n,
                                                     char* __restrict__ out)
{
    constexpr int CHUNKS = ROW_BYTES / 16;
    const int     c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n * CHUNKS) return;
    const int row = c / CHUNKS, ch = c % CHUNKS;
    *(v4f*)(out + (size_t)row * ROW_BYTES + 16 * ch) = *(const v4f*)(desc + (size_t)list[row] * ROW_BYTES + 16 * ch);
}

int blocks_of(int n) { return (n + C_BLOCK - 1) / C_BLOCK; }

}  // namespace

int pair_count_blocks(int n) { return std::max(blocks_of(n), 1); }

hipError_t launch_pair_targets(const popsift_hip_match* fwd, int l_len, int r_len, float ratio, float max_dist2, int* flags,
                               int* counts, int* list, int* rank, int* n_list, hipStream_t s)
{
    hipError_t err = hipMemsetAsync(flags, 0, sizeof(int) * (size_t)r_len, s);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(k_pair_mark, dim3((l_len + 255) / 256), dim3(256), 0, s, fwd, l_len, ratio, max_dist2, flags);
    const Flagged keep{flags};
    hipLaunchKernelGGL(k_count<Flagged>, dim3(blocks_of(r_len)), dim3(C_BLOCK), 0, s, keep, r_len, counts);
    hipLaunchKernelGGL((k_compact<Flagged, WriteIndex>), dim3(blocks_of(r_len)), dim3(C_BLOCK), 0, s, keep,
                       WriteIndex{list, rank}, r_len, counts, n_list);
    return hipGetLastError();
}

template <class T>
hipError_t launch_gather_rows(const T* desc, const int* list, int n, T* out, hipStream_t s)
{
    constexpr int ROW_BYTES = 128 * sizeof(T);
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_gather_rows<ROW_BYTES>, dim3((n * (ROW_BYTES / 16) + 255) / 256), dim3(256), 0, s, (const char*)desc, list,
                       n, (char*)out);
    return hipGetLastError();
}
template hipError_t launch_gather_rows<float>(const float*, const int*, int, float*, hipStream_t);
template hipError_t launch_gather_rows<uint8_t>(const uint8_t*, const int*, int, uint8_t*, hipStream_t);

hipError_t launch_pair_emit(const popsift_hip_match* fwd, int l_len, float ratio, float max_dist2,
                            const popsift_hip_match* back, const int* rank, int* counts, popsift_hip_pair* pairs, int* n_pairs,
                            hipStream_t s)
{
    const PairKept keep{fwd, back, rank, ratio, max_dist2};
    hipLaunchKernelGGL(k_count<PairKept>, dim3(blocks_of(l_len)), dim3(C_BLOCK), 0, s, keep, l_len, counts);
    hipLaunchKernelGGL((k_compact<PairKept, WritePair>), dim3(blocks_of(l_len)), dim3(C_BLOCK), 0, s, keep,
                       WritePair{fwd, pairs}, l_len, counts, n_pairs);
    return hipGetLastError();
}

}  // namespace popsift_hip
