/*
 * match_guided.hip -- nearest neighbours under a known homography or fundamental matrix (popsift_hip_match_guided,
 * popsift_hip_match_pairs_guided; the rule is stated in include/popsift_hip.h).
 *
 * For two 1080p images there are 9 x 10^9 (left, right) pairs, and only the few whose positions agree with the model
 * need a 128-D distance.  So the sweep is over POSITIONS: 8 bytes per descriptor, gathered once per call through the
 * sets' maps (k_guided_pos), not over descriptors.
 *
 *   k_guided         One wave per workgroup owns 64 rows (lane k keeps the two best candidates of row k in registers)
 *                    and walks the other side's positions 256 at a time, four per lane.  What the candidate test needs of
 *                    a point alone is formed once per point -- for a homography u, v, w and lim of the left point, for
 *                    the epipolar test a, b, c of the left point and fmaf(d, d, e * e) of the right one -- and what joins
 *                    the two points is left for the pair: 4 operations (homography) or 6 (epipolar), the operations of
 *                    the verifier's test in the verifier's order, so the bits are the verifier's.  The row's terms come
 *                    from LDS by a broadcast read; the loop over the rows is wave-uniform and the test is branch-free.
 *                    Pairs that pass are ranked by ballot and bit count into the wave's LDS queue (no atomic).  When the
 *                    next 64 might not fit, and at the end, the wave drains the queue: two pairs at a time, 32 lanes per
 *                    pair, one float4 chunk each, the 16 / 8 / 4 / 2 / 1 shuffle tree -- the exact matcher's arithmetic
 *                    in the reference's own shape -- and the lane that keeps the pair's row inserts under (d, j).  "The
 *                    two smallest under lexicographic (d, j)" does not depend on the order of insertion, which is what
 *                    lets waves that share rows (the candidate side split over gridDim.y for small row counts) keep
 *                    private candidates; k_top2_finish (top2.h) merges them and writes the rows.
 *                    One wave per workgroup: no barrier couples waves whose queues fill at different times.
 *   SWAP             The cross-check's search the other way round is the same kernel with the right descriptors as rows
 *                    and the left ones as candidates; the test itself stays left -> right.  It runs over all of r: on
 *                    positions that is as cheap as the forward sweep, and it needs no read-back between the sweeps.
 *   pairs            match_pairs.hip's order-preserving compaction over the forward rows (launch_pair_emit without a rank).
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "devfeatures.h"
#include "kernels.h"
#include "top2.h"

namespace popsift_hip {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));

constexpr int G_ROWS = POPSIFT_HIP_GUIDED_ROWS;   /* rows per wave: lane k keeps row k */
constexpr int G_PER = 4;                          /* candidate positions per lane and step */
constexpr int G_STEP = POPSIFT_HIP_GUIDED_STEP;   /* candidate positions per step */
constexpr int G_QUEUE = POPSIFT_HIP_GUIDED_QUEUE; /* pairs waiting for their distance */
static_assert(G_ROWS == 64, "one row per lane of a wave");
static_assert(G_STEP == 64 * G_PER, "a step is G_PER positions per lane");
static_assert(G_QUEUE >= 64 && G_QUEUE % 2 == 0, "a ballot's worth of pairs always fits an empty queue");

struct Model {
    float m[9];
    float max_err2; /* max_err * max_err */
};

/* what the test needs of the left point alone.  Homography (step 4 of popsift_hip_ransac): u, v, w, lim.  Epipolar (step 6
 * of popsift_hip_epipolar): a, b, c. */
template <int MODEL>
__device__ __forceinline__ v4f left_terms(const Model& M, v2f p)
{
    const float a = fmaf(M.m[0], p.x, fmaf(M.m[1], p.y, M.m[2]));
    const float b = fmaf(M.m[3], p.x, fmaf(M.m[4], p.y, M.m[5]));
    const float c = fmaf(M.m[6], p.x, fmaf(M.m[7], p.y, M.m[8]));
    if (MODEL == POPSIFT_HIP_GUIDE_HOMOGRAPHY) return v4f{a, b, c, M.max_err2 * (c * c)};
    return v4f{a, b, c, 0.0f};
}

/* of the right point alone: x', y' and, epipolar, fmaf(d, d, e * e): the inner half of g */
template <int MODEL>
__device__ __forceinline__ v4f right_terms(const Model& M, v2f p)
{
    if (MODEL == POPSIFT_HIP_GUIDE_HOMOGRAPHY) return v4f{p.x, p.y, 0.0f, 0.0f};
    const float d = fmaf(M.m[0], p.x, fmaf(M.m[3], p.y, M.m[6]));
    const float e = fmaf(M.m[1], p.x, fmaf(M.m[4], p.y, M.m[7]));
    return v4f{p.x, p.y, fmaf(d, d, e * e), 0.0f};
}

/* the rest of the test: what joins the two points.  A NaN fails every comparison. */
template <int MODEL>
__device__ __forceinline__ bool pair_ok(v4f L, v4f R, float max_err2)
{
    if (MODEL == POPSIFT_HIP_GUIDE_HOMOGRAPHY) {
        const float dx = fmaf(-L.z, R.x, L.x);
        const float dy = fmaf(-L.z, R.y, L.y);
        const float e = fmaf(dx, dx, dy * dy);
        return L.z > 0.0f && e <= L.w;
    }
    const float r = fmaf(L.x, R.x, fmaf(L.y, R.y, L.z));
    const float g = fmaf(L.x, L.x, fmaf(L.y, L.y, R.z));
    const float lim = max_err2 * g;
    return g > 0.0f && g < INFINITY && r * r <= lim;
}

/* descriptor -> position through the set's map; an entry that names no feature raises *bad and becomes NaN, which is
 * nobody's candidate, so the sweeps stay in bounds whatever the map holds */
__global__ __launch_bounds__(256) void k_guided_pos(const DevFeature* __restrict__ feat, const int* __restrict__ rev, int n_desc,
                                                    int n_feat, v2f* __restrict__ pos, int* __restrict__ bad)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_desc) return;
    const int f = rev[i];
    if (f < 0 || f >= n_feat) {
        *bad = 1;
        pos[i] = v2f{NAN, NAN};
        return;
    }
    pos[i] = v2f{feat[f].xpos, feat[f].ypos};
}

/* the queued pairs' distances, two at a time: lanes 0 .. 31 take s_q[q], lanes 32 .. 63 s_q[q + 1], one float4 chunk a
 * lane.  p(c) and the shuffle tree are l2_in_t0's (top2.h); (l - r)^2 and (r - l)^2 are the same bits, so
 * rows minus candidates serves both directions.  Lane i of the wave keeps row r0 + i. */
__device__ __forceinline__ void drain(const int2* s_q, int qn, const float* __restrict__ row_desc, int r0,
                                      const float* __restrict__ col_desc, Top2<float>& top)
{
    __syncthreads(); /* the queue's entries are written (a one-wave workgroup: this orders LDS, nothing waits) */
    const int lane = threadIdx.x, half = lane >> 5, ch = lane & 31;
    for (int q = 0; q < qn; q += 2) {
        const int2 e0 = s_q[q], e1 = s_q[min(q + 1, qn - 1)]; /* an odd tail: computed twice, inserted once */
        const int2 e = half ? e1 : e0;
        const v4f  a = *(const v4f*)(row_desc + (size_t)(r0 + e.x) * 128 + 4 * ch);
        const v4f  b = *(const v4f*)(col_desc + (size_t)e.y * 128 + 4 * ch);
        const float p = l2_in_t0(a, b);
        const float d0 = __shfl(p, 0), d1 = __shfl(p, 32);
        /* d < +inf: a NaN or an overflowed distance is no candidate */
        if (lane == e0.x && d0 < INFINITY) top2_insert(top, d0, e0.y);
        if (q + 1 < qn && lane == e1.x && d1 < INFINITY) top2_insert(top, d1, e1.y);
    }
    __syncthreads(); /* read, before the next entries overwrite it */
}

/*
 * grid (ceil(n_rows / 64), n_split), 64 lanes.  Rows: the searching side -- the left descriptors, or with SWAP the right
 * ones; cols: the side searched.  Workgroup (bx, by) takes rows 64 * bx .. and the steps by, by + n_split, .. of the cols;
 * partial[row * n_split + by] receives its two best.
 */
template <int MODEL, bool SWAP>
__global__ __launch_bounds__(64) void k_guided(Model M, const v2f* __restrict__ row_pos, int n_rows,
                                               const float* __restrict__ row_desc, const v2f* __restrict__ col_pos, int n_cols,
                                               const float* __restrict__ col_desc, int n_split, Top2<float>* __restrict__ partial)
{
    __shared__ v4f  s_row[G_ROWS];
    __shared__ int2 s_q[G_QUEUE];
    const int       lane = threadIdx.x;
    const int       r0 = blockIdx.x * G_ROWS;
    {
        v2f p = {NAN, NAN}; /* a row past the end fails every test */
        if (r0 + lane < n_rows) p = row_pos[r0 + lane];
        s_row[lane] = SWAP ? right_terms<MODEL>(M, p) : left_terms<MODEL>(M, p);
    }
    __syncthreads();

    Top2<float>              top = {INFINITY, INFINITY, -1, -1};
    int                      qn = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int                n_steps = (n_cols + G_STEP - 1) / G_STEP;
    for (int step = blockIdx.y; step < n_steps; step += n_split) {
        v4f col[G_PER];
#pragma unroll
        for (int k = 0; k < G_PER; k++) {
            const int j = step * G_STEP + 64 * k + lane;
            v2f       p = col_pos[min(j, n_cols - 1)];
            if (j >= n_cols) p = v2f{NAN, NAN};
            col[k] = SWAP ? left_terms<MODEL>(M, p) : right_terms<MODEL>(M, p);
        }
        for (int i = 0; i < G_ROWS; i++) {
            const v4f row = s_row[i];
            bool      hit[G_PER], any = false;
#pragma unroll
            for (int k = 0; k < G_PER; k++) {
                hit[k] = SWAP ? pair_ok<MODEL>(col[k], row, M.max_err2) : pair_ok<MODEL>(row, col[k], M.max_err2);
                any = any || hit[k];
            }
            if (__ballot(any) == 0) continue;
#pragma unroll
            for (int k = 0; k < G_PER; k++) {
                const unsigned long long b = __ballot(hit[k]);
                const int                n = __popcll(b);
                if (n == 0) continue;
                if (qn + n > G_QUEUE) {
                    drain(s_q, qn, row_desc, r0, col_desc, top);
                    qn = 0;
                }
                if (hit[k]) s_q[qn + __popcll(b & below)] = make_int2(i, step * G_STEP + 64 * k + lane);
                qn += n;
            }
        }
    }
    drain(s_q, qn, row_desc, r0, col_desc, top);
    if (r0 + lane < n_rows) partial[(size_t)(r0 + lane) * n_split + blockIdx.y] = top;
}

template <int MODEL, bool SWAP>
hipError_t launch_sweep(const Model& M, const v2f* row_pos, int n_rows, const float* row_desc, const v2f* col_pos, int n_cols,
                        const float* col_desc, int n_split, Top2<float>* partial, popsift_hip_match* out, hipStream_t s)
{
    hipLaunchKernelGGL((k_guided<MODEL, SWAP>), dim3((n_rows + G_ROWS - 1) / G_ROWS, n_split), dim3(64), 0, s, M, row_pos, n_rows,
                       row_desc, col_pos, n_cols, col_desc, n_split, partial);
    launch_top2_finish(partial, n_rows, n_split, out, nullptr, nullptr, 0, n_rows, s);
    return hipGetLastError();
}

bool opts_valid(const popsift_hip_guided_opts* o)
{
    if (!o || (o->model != POPSIFT_HIP_GUIDE_HOMOGRAPHY && o->model != POPSIFT_HIP_GUIDE_EPIPOLAR)) return false;
    if (!std::isfinite(o->max_err) || !(o->max_err > 0.0f)) return false;
    for (float m : o->M)
        if (!std::isfinite(m)) return false;
    if (!(o->ratio >= 0.0f) || std::isinf(o->ratio) || std::isnan(o->max_dist2)) return false;
    return (o->cross_check == 0 || o->cross_check == 1) && o->reserved[0] == 0 && o->reserved[1] == 0;
}

const popsift_hip_match EMPTY_ROW = {-1, -1, 0, INFINITY, INFINITY};

/* Both entry points.  rows != null: the forward rows to `rows`; else the pairs.  Arguments are checked; l and r hold
 * descriptors. */
int run(popsift_hip_devfeatures* l, const popsift_hip_devfeatures* r, const popsift_hip_guided_opts* o, popsift_hip_match* rows,
        popsift_hip_pair* pairs, size_t cap, int* n_pairs)
{
    if (hipSetDevice(l->device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    const int  nl = l->n_desc, nr = r->n_desc;
    const bool cross = !rows && o->cross_check;
    Status     ok;
    hipStream_t const s = stream_of(ok, *l);

    /* l's block: header, forward rows | positions of l, of r | reverse rows | the compaction's counts */
    const size_t b_head = 16, b_rows = round16(sizeof(popsift_hip_match) * (size_t)nl);
    const size_t b_lpos = round16(sizeof(v2f) * (size_t)nl), b_rpos = round16(sizeof(v2f) * (size_t)nr);
    const size_t b_back = cross ? round16(sizeof(popsift_hip_match) * (size_t)nr) : 0;
    const size_t b_counts = round16(sizeof(int) * (size_t)pair_count_blocks(nl));
    const size_t need = b_head + b_rows + b_lpos + b_rpos + b_back + b_counts;
    grow(ok, l->g_buf, l->g_cap, need, 1);
    if (ok.good() && !l->g_host) ok(hipHostMalloc(&l->g_host, b_head + b_rows, hipHostMallocDefault));
    /* at least 4096 waves where the candidate side has the steps for it */
    const int split_f = splits(nl, nr, G_ROWS, G_STEP, 4096), split_b = cross ? splits(nr, nl, G_ROWS, G_STEP, 4096) : 1;
    grow(ok, l->m_partial, l->m_partial_cap,
         std::max(partial_bytes(nl, split_f, sizeof(Top2<float>)), cross ? partial_bytes(nr, split_b, sizeof(Top2<float>)) : 0), 1);
    /* the pairs' block is popsift_hip_match_pairs'; its header int [2] is the map flag */
    if (!rows) pair_block(ok, *l, nl);
    /* a right set on another GPU: its feature records, its map and its descriptors come over for the call */
    const DevFeature* rf = r->d_feat;
    const int*        rrev = r->d_rev;
    const float*      rdesc = r->d_desc;
    PeerCopy          peer;
    if (peer.fetch(ok, l->device, r->device,
                   {{r->d_feat, sizeof(DevFeature) * (size_t)std::max(r->n_feat, 1)},
                    {r->d_rev, sizeof(int) * (size_t)nr},
                    {r->d_desc, sizeof(float) * 128 * (size_t)nr}})) {
        rf = (const DevFeature*)peer.at[0];
        rrev = (const int*)peer.at[1];
        rdesc = (const float*)peer.at[2];
    }
    if (ok.good()) {
        char* const d = (char*)l->g_buf;
        auto* const d_fwd = (popsift_hip_match*)(d + b_head);
        v2f* const  lpos = (v2f*)(d + b_head + b_rows);
        v2f* const  rpos = (v2f*)(d + b_head + b_rows + b_lpos);
        auto* const d_back = (popsift_hip_match*)(d + b_head + b_rows + b_lpos + b_rpos);
        int* const  counts = (int*)(d + b_head + b_rows + b_lpos + b_rpos + b_back);
        int* const  head = rows ? (int*)d : (int*)l->p_pairs;
        int* const  bad = rows ? head : head + 2;
        auto* const partial = (Top2<float>*)l->m_partial;
        Model       M;
        memcpy(M.m, o->M, sizeof M.m);
        M.max_err2 = o->max_err * o->max_err;
        const bool hom = o->model == POPSIFT_HIP_GUIDE_HOMOGRAPHY;
        ok(hipMemsetAsync(head, 0, 16, s));
        if (ok.good()) {
            hipLaunchKernelGGL(k_guided_pos, dim3((nl + 255) / 256), dim3(256), 0, s, l->d_feat, l->d_rev, nl, l->n_feat, lpos, bad);
            hipLaunchKernelGGL(k_guided_pos, dim3((nr + 255) / 256), dim3(256), 0, s, rf, rrev, nr, r->n_feat, rpos, bad);
            ok(hipGetLastError());
        }
        if (ok.good())
            ok(hom ? launch_sweep<POPSIFT_HIP_GUIDE_HOMOGRAPHY, false>(M, lpos, nl, l->d_desc, rpos, nr, rdesc, split_f, partial,
                                                                       d_fwd, s)
                   : launch_sweep<POPSIFT_HIP_GUIDE_EPIPOLAR, false>(M, lpos, nl, l->d_desc, rpos, nr, rdesc, split_f, partial,
                                                                     d_fwd, s));
        if (ok.good() && cross)
            ok(hom ? launch_sweep<POPSIFT_HIP_GUIDE_HOMOGRAPHY, true>(M, rpos, nr, rdesc, lpos, nl, l->d_desc, split_b, partial,
                                                                      d_back, s)
                   : launch_sweep<POPSIFT_HIP_GUIDE_EPIPOLAR, true>(M, rpos, nr, rdesc, lpos, nl, l->d_desc, split_b, partial,
                                                                    d_back, s));
        if (rows) {
            if (ok.good() && ok(hipMemcpyAsync(l->g_host, d, b_head + sizeof(popsift_hip_match) * (size_t)nl, hipMemcpyDeviceToHost, s)) &&
                ok(hipStreamSynchronize(s))) {
                if (*(const int*)l->g_host != 0) ok.rc = POPSIFT_HIP_ERR_INVALID;
                else memcpy(rows, (const char*)l->g_host + b_head, sizeof(popsift_hip_match) * (size_t)nl);
            }
        } else {
            /* no rank: d_back holds a row for every right descriptor */
            if (ok.good() && ok(launch_pair_emit(d_fwd, nl, o->ratio, o->max_dist2, cross ? d_back : nullptr, nullptr, counts,
                                                 (popsift_hip_pair*)l->p_pairs + 1, head, s)))
                download_pairs(ok, *l, std::min(cap, (size_t)nl), 2, pairs, cap, n_pairs, s);
        }
    }
    return ok.rc;
}

}  // namespace
}  // namespace popsift_hip

using namespace popsift_hip;

extern "C" {

void popsift_hip_default_guided_opts(popsift_hip_guided_opts* o)
{
    if (!o) return;
    o->model = POPSIFT_HIP_GUIDE_HOMOGRAPHY;
    for (int i = 0; i < 9; i++) o->M[i] = (i % 4 == 0) ? 1.0f : 0.0f;
    o->max_err = 2.0f;
    o->ratio = 0.8f;
    o->max_dist2 = INFINITY;
    o->cross_check = 0;
    o->reserved[0] = o->reserved[1] = 0;
}

int popsift_hip_match_guided(const popsift_hip_devfeatures* l, const popsift_hip_devfeatures* r, const popsift_hip_guided_opts* o,
                             popsift_hip_match* out)
{
    if (!l || !r || !out || !opts_valid(o)) return POPSIFT_HIP_ERR_INVALID;
    if (l->n_desc == 0) return POPSIFT_HIP_OK;
    if (r->n_desc == 0) {
        for (int i = 0; i < l->n_desc; i++) out[i] = EMPTY_ROW;
        return POPSIFT_HIP_OK;
    }
    return run(const_cast<popsift_hip_devfeatures*>(l), r, o, out, nullptr, 0, nullptr);
}

int popsift_hip_match_pairs_guided(const popsift_hip_devfeatures* l, const popsift_hip_devfeatures* r,
                                   const popsift_hip_guided_opts* o, popsift_hip_pair* pairs, size_t cap, int* n_pairs)
{
    if (!l || !r || !n_pairs || (cap > 0 && !pairs) || !opts_valid(o)) return POPSIFT_HIP_ERR_INVALID;
    if (l->n_desc == 0 || r->n_desc == 0) {
        *n_pairs = 0;
        return POPSIFT_HIP_OK;
    }
    return run(const_cast<popsift_hip_devfeatures*>(l), r, o, nullptr, pairs, cap, n_pairs);
}

} /* extern "C" */
