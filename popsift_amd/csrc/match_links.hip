/*
 * match_links.hip -- any list of member pairs ("links") of one gallery in one pass (popsift_hip_match_links,
 * popsift_hip_match_pairs_links, popsift_hip_gallery_link_points).  A link (a, b) is the per-pair call with member a on the
 * left and member b on the right (include/popsift_hip.h); what is new against match_gallery.hip is that the LEFT side is a
 * member too, so its rows, its norms and its length vary from work item to work item:
 *
 *   k_match_links    k_match_gallery with a left side per item.  A workgroup takes one item = (link of the group, block
 *                    of U_LB left rows, split of the link's right tiles) and sees both sides through the link's record:
 *                    left rows and norms at lbase + l_first, right rows and norms at the gallery's + r_first.  Operand
 *                    loads, sign flip, the four 32x32x32 i8 steps, the epilogue and the half merge are restated from
 *                    k_match_gallery (and so from k_match_u8) operation for operation.  The left base is a parameter: the
 *                    forward sweep passes the gallery's rows and norms, the reverse sweep of the cross-check the gathered
 *                    rows of J and theirs.  A link with an empty side has no item.
 *   k_links_finish   per flat row of the group: find its link in the row0 table (binary search), merge the link's splits
 *                    under (d, j), write the row; a link with an empty right side gets {0, 0, 0, inf, inf} from here.
 *   pairs            k_links_mark flags (link, right row): the same member is the right side of many links, so a flag
 *                    belongs to the link's own columns, col0 + best.  One compaction turns the flags into J, link-major
 *                    -- link e's flagged rows are the segment [jstart[e], jstart[e + 1]) -- with their ranks.  One
 *                    read-back of jstart sizes the reverse sweep: the same kernel with segment e of the gathered rows on
 *                    the left and member a_e on the right.  A second compaction over the group's flat rows emits the
 *                    pairs behind those of the earlier groups and writes offsets[e] with the first row of link e.
 *
 * A link whose left member is empty has no row, so nothing on the device writes its offset (nor, for a link without
 * columns, its jstart).  The host fills these in after the download, from the back: such an entry equals the next one.
 *
 * The host walks the links in groups of consecutive links holding at most group_rows left rows, always at least one link.
 * Per group: one table upload, the sweep, the finish, and for pairs 2 (with the cross-check 5, one read-back, one more
 * upload, the gather, the norms, the reverse sweep and its finish) more launches, however many links the group has.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "devfeatures.h"
#include "kernels.h"
#include "top2.h"

namespace popsift_hip {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int     U_ROW = 144;              /* as match_u8.hip: bytes per LDS row */
constexpr int     U_FAR = INT_MAX / 2;      /* as match_u8.hip: norm of a row past the member's end */
constexpr int     C_BLOCK = 256;            /* elements per workgroup of the compactions */
constexpr int     MAX_LINKS = 1 << 20;      /* popsift_hip_ransac_many's limit on lists */
constexpr int64_t GROUP_COLS = (int64_t)1 << 28; /* flag columns of a group: keeps col0 and 3 * cols in an int */

/* a link of the group in flight: its left rows [l_first, l_first + l_count) of the left base, its right rows of the
 * gallery, over how many items its right tiles are split, its first flat row and its first flag column in the group */
struct LLink {
    int l_first, l_count, r_first, r_count, n_split, row0, col0, pad;
};
/* a workgroup's share of the sweep */
struct LItem {
    int link, lblock, split, pad;
};
static_assert(sizeof(LLink) == 32 && sizeof(LItem) == 16, "uploaded as 32- and 16-byte records");

__device__ __forceinline__ v4i to_signed(v4i v)
{
    const int f = (int)0x80808080u;
    return v4i{v.x ^ f, v.y ^ f, v.z ^ f, v.w ^ f};
}

__device__ __forceinline__ int k_off(int s, int h) { return 32 * s + 16 * h; }

/* partial: [flat row of the group][stride] */
__global__ __launch_bounds__(256, 2) void k_match_links(const uint8_t* __restrict__ lbase, const int* __restrict__ lnbase,
                                                        const uint8_t* __restrict__ gdesc, const int* __restrict__ gnorm,
                                                        const LLink* __restrict__ links, const LItem* __restrict__ items,
                                                        int stride, Top2<int>* __restrict__ partial)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_r[U_RB * U_ROW];
    __shared__ __attribute__((aligned(16))) int     s_rn[U_RB];
    const LItem          it = items[blockIdx.x];
    const LLink          lk = links[it.link];
    const uint8_t* const ldesc = lbase + (size_t)lk.l_first * 128;
    const int* const     lnorm = lnbase + lk.l_first;
    const uint8_t* const rdesc = gdesc + (size_t)lk.r_first * 128;
    const int* const     rnorm = gnorm + lk.r_first;
    const int            l_len = lk.l_count, r_len = lk.r_count, n_split = lk.n_split; /* both >= 1: else no item */

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int l = it.lblock * U_LB + wave * 32 + col;
    const int lc = min(l, l_len - 1); /* lanes past the end work on the link's last left row and write nothing */

    v4i bl[4];
#pragma unroll
    for (int s = 0; s < 4; s++) bl[s] = to_signed(*(const v4i*)(ldesc + (size_t)lc * 128 + k_off(s, half)));

    int e1 = U_NONE, e2 = U_NONE, j1 = 0, j2 = 0;

    const int n_tiles = (r_len + U_RB - 1) / U_RB;
    v4i       stage[4];
    int       stage_n = U_FAR;
    auto      fetch = [&](int tile) {
        const int r0 = tile * U_RB;
        /* clamped within the member: never another member's rows, never past the gallery's end */
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int c = tid + 256 * k, row = c >> 3, ch = c & 7;
            stage[k] = *(const v4i*)(rdesc + (size_t)min(r0 + row, r_len - 1) * 128 + 16 * ch);
        }
        const int rn = rnorm[min(r0 + (tid & (U_RB - 1)), r_len - 1)];
        stage_n = (r0 + (tid & (U_RB - 1)) < r_len) ? rn : U_FAR;
    };
    int tile = it.split;
    if (tile < n_tiles) fetch(tile);
    for (; tile < n_tiles; tile += n_split) {
        const int r0 = tile * U_RB;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int c = tid + 256 * k, row = c >> 3, ch = c & 7;
            *(v4i*)(s_r + row * U_ROW + 16 * ch) = to_signed(stage[k]);
        }
        if (tid < U_RB) s_rn[tid] = stage_n;
        __syncthreads();
        if (tile + n_split < n_tiles) fetch(tile + n_split);

        v16i acc[4];
#pragma unroll
        for (int m = 0; m < 4; m++)
#pragma unroll
            for (int v = 0; v < 16; v++) acc[m][v] = 0;
        const uint8_t* arow = s_r + col * U_ROW;
#pragma unroll
        for (int s = 0; s < 4; s++) {
            v4i a[4];
#pragma unroll
            for (int m = 0; m < 4; m++) a[m] = *(const v4i*)(arow + m * 32 * U_ROW + k_off(s, half));
#pragma unroll
            for (int m = 0; m < 4; m++) acc[m] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[m], bl[s], acc[m], 0, 0, 0);
        }
#pragma unroll
        for (int m = 0; m < 4; m++) {
            int e[16];
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const v4i rn = *(const v4i*)(s_rn + 32 * m + 8 * g + 4 * half);
                e[4 * g + 0] = rn.x - 2 * acc[m][4 * g + 0];
                e[4 * g + 1] = rn.y - 2 * acc[m][4 * g + 1];
                e[4 * g + 2] = rn.z - 2 * acc[m][4 * g + 2];
                e[4 * g + 3] = rn.w - 2 * acc[m][4 * g + 3];
            }
            int lo = e[0];
#pragma unroll
            for (int v = 1; v < 16; v++) lo = min(lo, e[v]);
            if (lo < e2) {
#pragma unroll
                for (int v = 0; v < 16; v++) { /* ascending member-local index */
                    const int j = r0 + 32 * m + (v & 3) + 8 * (v >> 2) + 4 * half;
                    if (e[v] < e2 && j < r_len) {
                        if (e[v] < e1) {
                            e2 = e1;
                            j2 = j1;
                            e1 = e[v];
                            j1 = j;
                        } else {
                            e2 = e[v];
                            j2 = j;
                        }
                    }
                }
            }
        }
    }
    const int ln = lnorm[lc];
    Top2<int> best{e1 == U_NONE ? U_NONE : e1 + ln, e2 == U_NONE ? U_NONE : e2 + ln, j1, j2};
    const int od1 = __shfl_xor(best.v1, 32), od2 = __shfl_xor(best.v2, 32);
    const int oj1 = __shfl_xor(best.i1, 32), oj2 = __shfl_xor(best.i2, 32);
    top2_insert(best, od1, oj1);
    top2_insert(best, od2, oj2);
    if (half == 0 && l < l_len) partial[((size_t)lk.row0 + l) * stride + it.split] = best;
}

/* The link of flat row e < n: the last link whose row0 is <= e.  Links without rows share their row0 with the link after
 * them, so the last one of a run of equal row0 is the one that has the row; rows past the last link do not exist. */
__device__ __forceinline__ int link_of_row(const LLink* __restrict__ links, int n_links, int e)
{
    int lo = 0, hi = n_links - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (links[mid].row0 <= e) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

/* the same over the flag columns */
__device__ __forceinline__ int link_of_col(const LLink* __restrict__ links, int n_links, int j)
{
    int lo = 0, hi = n_links - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (links[mid].col0 <= j) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

/* n flat rows of the group */
__global__ __launch_bounds__(256) void k_links_finish(const Top2<int>* __restrict__ partial, const LLink* __restrict__ links,
                                                      int n_links, int n, int stride, popsift_hip_match* __restrict__ out)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const LLink lk = links[link_of_row(links, n_links, e)];
    Top2<int>   t{U_NONE, U_NONE, 0, 0};
    if (lk.r_count > 0) {
        t = partial[(size_t)e * stride];
        for (int k = 1; k < lk.n_split; k++) {
            const Top2<int> o = partial[(size_t)e * stride + k];
            top2_merge(t, o);
        }
    }
    out[e] = top2_row(t);
}

/* conditions 2 and 3, as match_pairs.hip states them */
__device__ __forceinline__ bool row_passes(const popsift_hip_match& m, float ratio, float max_dist2)
{
    return (ratio == 0.0f || __fdiv_rn(m.dist_best, m.dist_second) < ratio) && m.dist_best <= max_dist2;
}

/* flags: one int per (link, right row) of the group, link e's at col0 */
__global__ __launch_bounds__(256) void k_links_mark(const popsift_hip_match* __restrict__ fwd, const LLink* __restrict__ links,
                                                    int n_links, int n, float ratio, float max_dist2, int* __restrict__ flags)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const LLink lk = links[link_of_row(links, n_links, e)];
    if (lk.r_count == 0) return; /* condition 1 */
    const popsift_hip_match m = fwd[e];
    if (row_passes(m, ratio, max_dist2)) flags[lk.col0 + m.best] = 1;
}

/* Flag column j is kept when set: J holds global gallery rows, link-major; the rank is found by the column; the first
 * column of a link has as many flagged columns in front of it as the links before have: jstart[link]. */
struct FlagOp {
    const int*   flags;
    const LLink* links;
    int          n_links;
    int*         list;
    int*         rank;
    int*         jstart;
    __device__ bool keep(int j) const { return flags[j] != 0; }
    __device__ int  locate(int j) const { return link_of_col(links, n_links, j); }
    __device__ bool keep_at(int j, int) const { return flags[j] != 0; }
    __device__ void put(int pos, int j, int k, bool kept) const
    {
        const LLink lk = links[k];
        if (j == lk.col0) jstart[k] = pos;
        if (kept) {
            list[pos] = lk.r_first + (j - lk.col0);
            rank[j] = pos;
        }
    }
};

/* Flat row e yields a pair: its link's right side is not empty, the row passes, and with the cross-check the row is the
 * nearest left descriptor of its best right row.  none: the group's J is empty and `back` was never formed.  pos counts
 * from the first pair of the call; every pair is counted, those the buffer has room for are written.  The first row of a
 * link has as many pairs in front of it as the links before have: offsets[link]. */
struct PairOp {
    const popsift_hip_match* fwd;
    const LLink*             links;
    const popsift_hip_match* back; /* null: no cross-check */
    const int*               rank;
    popsift_hip_pair*        pairs;
    int*                     offsets; /* of the group's first link */
    int                      n_links, none, room;
    float                    ratio, max_dist2;
    __device__ int  locate(int e) const { return link_of_row(links, n_links, e); }
    __device__ bool keep(int e) const { return keep_at(e, locate(e)); }
    __device__ bool keep_at(int e, int k) const
    {
        if (none) return false;
        const LLink lk = links[k];
        if (lk.r_count == 0) return false;
        const popsift_hip_match m = fwd[e];
        if (!row_passes(m, ratio, max_dist2)) return false;
        return !back || back[rank[lk.col0 + m.best]].best == e - lk.row0;
    }
    __device__ void put(int pos, int e, int k, bool kept) const
    {
        const int row0 = links[k].row0;
        if (e == row0) offsets[k] = pos;
        if (kept && pos < room) {
            const popsift_hip_match m = fwd[e];
            pairs[pos] = popsift_hip_pair{e - row0, m.best, m.dist_best, m.dist_second};
        }
    }
};

/* number of kept elements in front of this lane's within the workgroup, and the workgroup's count (as match_pairs.hip) */
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

template <class Op>
__global__ __launch_bounds__(C_BLOCK) void k_lcount(Op op, int n, int* __restrict__ counts)
{
    const int e = blockIdx.x * C_BLOCK + threadIdx.x;
    int       total;
    (void)block_rank(e < n && op.keep(e), &total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

/* Order-preserving compaction in front of which *start elements already lie (null: none).  The last workgroup writes
 * the new total to *end (never the word *start is read from). */
template <class Op>
__global__ __launch_bounds__(C_BLOCK) void k_lcompact(Op op, int n, const int* __restrict__ counts, const int* __restrict__ start,
                                                      int* __restrict__ end)
{
    __shared__ int s_part[C_BLOCK / 64];
    int            part = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += C_BLOCK) part += counts[b];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) part += __shfl_down(part, d);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = part;
    __syncthreads();
    int first = start ? *start : 0;
#pragma unroll
    for (int w = 0; w < C_BLOCK / 64; w++) first += s_part[w];

    const int  e = blockIdx.x * C_BLOCK + threadIdx.x;
    const int  k = e < n ? op.locate(e) : 0;
    const bool kept = e < n && op.keep_at(e, k);
    int        total;
    const int  before = block_rank(kept, &total);
    if (e < n) op.put(first + before, e, k, kept);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *end = first + total;
}

/* item = (gallery row of the left descriptor, gallery row of the right one): both positions from the gallery's array */
__global__ __launch_bounds__(256) void k_link_points(const int2* __restrict__ items, int n, const float2* __restrict__ xy,
                                                     float4* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int2   it = items[i];
    const float2 a = xy[it.x], b = xy[it.y];
    out[i] = make_float4(a.x, a.y, b.x, b.y);
}

int blocks_of(int n) { return (n + C_BLOCK - 1) / C_BLOCK; }

/* ---- the host side */

bool grow_pinned(Status& ok, void*& p, size_t& cap, size_t need)
{
    if (!ok.good() || need <= cap) return ok.good();
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    if (ok(hipHostMalloc(&p, need, hipHostMallocDefault))) cap = need;
    return ok.good();
}

struct Group {
    int     e0, n;   /* links [e0, e0 + n) */
    int     rows;    /* their left rows: the flat rows of the group */
    int     cols;    /* their flag columns: the right rows of the links that have left rows */
    int     n_items, stride;
};

/* the flag columns of a link: none without a left row to point at them */
int width_of(const popsift_hip_gallery* g, const popsift_hip_link& k) { return g->count[k.a] > 0 ? g->count[k.b] : 0; }

/* sum over the links of their left rows, or -1 for a link out of range */
int64_t total_rows(const popsift_hip_gallery* g, const popsift_hip_link* links, int n_links)
{
    int64_t total = 0;
    for (int e = 0; e < n_links; e++) {
        if (links[e].a < 0 || links[e].a >= g->n_members || links[e].b < 0 || links[e].b >= g->n_members) return -1;
        total += g->count[links[e].a];
    }
    return total;
}

/* what every entry point checks first; *total: R[n_links] */
bool links_valid(const popsift_hip_gallery* g, const popsift_hip_link* links, int n_links, int64_t* total)
{
    if (!g || n_links < 0 || n_links > MAX_LINKS || (n_links > 0 && !links)) return false;
    *total = total_rows(g, links, n_links);
    return *total >= 0 && *total <= INT32_MAX;
}

/* consecutive links from e0 on holding at most `budget` left rows (and GROUP_COLS flag columns), at least one link */
Group group_at(const popsift_hip_gallery* g, const popsift_hip_link* links, int n_links, int e0, int budget)
{
    Group   gr{};
    int64_t rows = g->count[links[e0].a], cols = width_of(g, links[e0]);
    int     e = e0 + 1;
    for (; e < n_links; e++) {
        const int64_t r = g->count[links[e].a], c = width_of(g, links[e]);
        if (rows + r > budget || cols + c > GROUP_COLS) break;
        rows += r;
        cols += c;
    }
    gr.e0 = e0;
    gr.n = e - e0;
    gr.rows = (int)rows;
    gr.cols = (int)cols; /* one link alone may pass GROUP_COLS: the gallery's 2^30 rows bound it */
    return gr;
}

/* One side table of a sweep: link records and work items, written by `fill` into a pinned block and uploaded.  side[k] =
 * (l_first, l_count, r_first, r_count) of link k; a link with an empty side has no item.  Members are split only when the
 * launch would otherwise have fewer than U_GROUPS workgroups; items are in the order link, split, row block, so that
 * workgroups next to each other walk the same right tiles. */
struct Side {
    int l_first, l_count, r_first, r_count, width; /* width: the link's flag columns */
    int lblocks() const { return l_count > 0 && r_count > 0 ? (l_count + U_LB - 1) / U_LB : 0; }
    int splits(int want) const { return lblocks() > 0 ? std::min(want, (r_count + U_RB - 1) / U_RB) : 0; }
};

/* the splits to aim at per link, the items that makes and the most splits of a link */
template <class SideOf>
int plan(int n, SideOf side, int* n_items, int* stride)
{
    int64_t unsplit = 0, items = 0;
    for (int k = 0; k < n; k++) unsplit += side(k).lblocks();
    const int want = unsplit > 0 && unsplit < U_GROUPS ? (int)((U_GROUPS + unsplit - 1) / unsplit) : 1;
    *stride = 1;
    for (int k = 0; k < n; k++) {
        const Side sd = side(k);
        items += (int64_t)sd.splits(want) * sd.lblocks();
        *stride = std::max(*stride, sd.splits(want));
    }
    *n_items = (int)items;
    return want;
}

template <class SideOf>
void fill(int n, SideOf side, int want, void* host)
{
    LLink* const lk = (LLink*)host;
    LItem*       it = (LItem*)(lk + n);
    int          row0 = 0, col0 = 0;
    for (int k = 0; k < n; k++) {
        const Side sd = side(k);
        const int  ns = sd.splits(want), lblocks = sd.lblocks();
        lk[k] = LLink{sd.l_first, sd.l_count, sd.r_first, sd.r_count, ns, row0, col0, 0};
        row0 += sd.l_count;
        col0 += sd.width;
        for (int sp = 0; sp < ns; sp++)
            for (int lb = 0; lb < lblocks; lb++) *it++ = LItem{k, lb, sp, 0};
    }
}

size_t table_bytes(int n, int n_items) { return sizeof(LLink) * (size_t)n + sizeof(LItem) * (size_t)n_items; }

/* the sweep and its finish over an uploaded table: n flat rows into `out` */
void sweep(Status& ok, popsift_hip_gallery* g, const uint8_t* lbase, const int* lnbase, const void* table, int n_links,
           int n_items, int stride, int n, popsift_hip_match* out, hipStream_t s)
{
    if (!grow(ok, g->partial, g->partial_cap, (size_t)n * stride * sizeof(Top2<int>), 1)) return;
    const LLink* const lk = (const LLink*)table;
    if (n_items > 0)
        hipLaunchKernelGGL(k_match_links, dim3(n_items), dim3(256), 0, s, lbase, lnbase, (const uint8_t*)g->d_desc,
                           (const int*)g->d_norm, lk, (const LItem*)(lk + n_links), stride, (Top2<int>*)g->partial);
    hipLaunchKernelGGL(k_links_finish, dim3((n + 255) / 256), dim3(256), 0, s, (const Top2<int>*)g->partial, lk, n_links, n,
                       stride, out);
    ok(hipGetLastError());
}

/* What both calls share: the rows of one group of links in g->rows, its table in g->w_dev.  The table is built in the
 * gallery's pinned block: a call's first group finds the block free (the call before ended with a wait for the stream); a
 * later group rewrites it only after the upload before it has been read (w_event, recorded when another group follows). */
struct Forward {
    popsift_hip_gallery*    g;
    const popsift_hip_link* links;
    int                     n_links, budget;
    hipStream_t             s;
    bool                    uploaded = false; /* an upload of this call has recorded w_event */

    void begin(popsift_hip_gallery* gal, const popsift_hip_link* l, int n)
    {
        g = gal;
        links = l;
        n_links = n;
        s = (hipStream_t)g->stream;
        budget = g->group_rows > 0 ? g->group_rows : POPSIFT_HIP_GALLERY_GROUP_ROWS;
    }

    /* false: the group has no rows and nothing was launched, or a call failed (see ok) */
    bool run(Status& ok, Group& gr)
    {
        if (gr.rows == 0 || !ok.good()) return false;
        const popsift_hip_link* const l = links + gr.e0;
        auto                          side = [&](int k) {
            return Side{(int)g->first[l[k].a], g->count[l[k].a], (int)g->first[l[k].b], g->count[l[k].b], width_of(g, l[k])};
        };
        const int    want = plan(gr.n, side, &gr.n_items, &gr.stride);
        const size_t bytes = table_bytes(gr.n, gr.n_items);
        if (bytes > g->w_cap) {
            if (!ok(hipStreamSynchronize(s))) return false; /* nothing reads the old block any more */
            grow_twin(ok, g->w_dev, g->w_host, g->w_cap, std::max(bytes, 2 * g->w_cap));
        } else if (uploaded) {
            ok(hipEventSynchronize((hipEvent_t)g->w_event));
        }
        if (!ok.good()) return false;
        fill(gr.n, side, want, g->w_host);
        if (ok(hipMemcpyAsync(g->w_dev, g->w_host, bytes, hipMemcpyHostToDevice, s)) && gr.e0 + gr.n < n_links)
            uploaded = ok(hipEventRecord((hipEvent_t)g->w_event, s));
        if (!grow(ok, g->rows, g->rows_cap, (size_t)gr.rows, sizeof(popsift_hip_match))) return false;
        sweep(ok, g, g->d_desc, g->d_norm, g->w_dev, gr.n, gr.n_items, gr.stride, gr.rows, (popsift_hip_match*)g->rows, s);
        return ok.good();
    }
};

}  // namespace
}  // namespace popsift_hip

using namespace popsift_hip;

extern "C" {

int popsift_hip_match_links(popsift_hip_gallery* g, const popsift_hip_link* links, int n_links, popsift_hip_match* out,
                            size_t cap_rows)
{
    int64_t total = 0;
    if (!links_valid(g, links, n_links, &total) || (total > 0 && !out)) return POPSIFT_HIP_ERR_INVALID;
    if (cap_rows < (size_t)total) return POPSIFT_HIP_ERR_TOO_SMALL; /* all or nothing */
    if (total == 0) return POPSIFT_HIP_OK;
    if (hipSetDevice(g->device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    Status  ok;
    Forward fw;
    fw.begin(g, links, n_links);
    if ((size_t)total > g->rows_host_cap) { /* in rows, as popsift_hip_match_gallery keeps it */
        if (g->rows_host) (void)hipHostFree(g->rows_host);
        g->rows_host = nullptr;
        g->rows_host_cap = 0;
        if (ok(hipHostMalloc(&g->rows_host, sizeof(popsift_hip_match) * (size_t)total, hipHostMallocDefault)))
            g->rows_host_cap = (size_t)total;
    }
    size_t done = 0;
    for (int e0 = 0; ok.good() && e0 < n_links;) {
        Group gr = group_at(g, links, n_links, e0, fw.budget);
        if (fw.run(ok, gr))
            ok(hipMemcpyAsync((popsift_hip_match*)g->rows_host + done, g->rows, sizeof(popsift_hip_match) * (size_t)gr.rows,
                              hipMemcpyDeviceToHost, fw.s));
        done += (size_t)gr.rows;
        e0 += gr.n;
    }
    if (ok.good() && ok(hipStreamSynchronize(fw.s))) memcpy(out, g->rows_host, sizeof(popsift_hip_match) * (size_t)total);
    else (void)hipStreamSynchronize(fw.s);
    return ok.rc;
}

int popsift_hip_match_pairs_links(popsift_hip_gallery* g, const popsift_hip_link* links, int n_links,
                                  const popsift_hip_match_opts* opts, popsift_hip_pair* pairs, size_t cap, int32_t* offsets,
                                  int* n_pairs)
{
    int64_t total = 0;
    if (!opts || !offsets || !n_pairs || !links_valid(g, links, n_links, &total) || (cap > 0 && !pairs))
        return POPSIFT_HIP_ERR_INVALID;
    if (!(opts->ratio >= 0.0f) || std::isinf(opts->ratio) || std::isnan(opts->max_dist2) || opts->reserved != 0 ||
        (opts->cross_check != 0 && opts->cross_check != 1))
        return POPSIFT_HIP_ERR_INVALID;
    *n_pairs = 0;
    memset(offsets, 0, sizeof(int32_t) * ((size_t)n_links + 1));
    if (total == 0) return POPSIFT_HIP_OK;
    if (hipSetDevice(g->device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    const bool   cross = opts->cross_check != 0;
    const float  ratio = opts->ratio, max_dist2 = opts->max_dist2;
    const size_t room = std::min(cap, (size_t)total); /* the device pair buffer */
    Status       ok;
    Forward      fw;
    fw.begin(g, links, n_links);
    hipStream_t const s = fw.s;

    /* result block: the running pair count (two words, written and read in turn; the first compaction reads none),
     * offsets[n_links]; the pairs.  Its pinned twin holds the head, and the pairs found once their number is known. */
    const size_t head = round16(sizeof(int) * ((size_t)n_links + 5));
    grow(ok, g->lk_res, g->lk_res_cap, head + sizeof(popsift_hip_pair) * room, 1);
    grow_pinned(ok, g->lk_host, g->lk_host_cap, head);
    int* const              d_run = (int*)g->lk_res;
    int* const              d_off = d_run + 4;
    popsift_hip_pair* const d_pairs = (popsift_hip_pair*)((char*)g->lk_res + head);

    int  turn = 0;
    bool any = false; /* a compaction has run: d_run[turn] holds the pairs so far */
    for (int e0 = 0; ok.good() && e0 < n_links;) {
        Group gr = group_at(g, links, n_links, e0, fw.budget);
        e0 += gr.n;
        if (!fw.run(ok, gr)) continue;
        const int          n = gr.rows, n_cols = gr.cols;
        const LLink* const lk = (const LLink*)g->w_dev;
        const auto* const  fwd = (const popsift_hip_match*)g->rows;
        const size_t       n_counts = (size_t)std::max(blocks_of(std::max(n, n_cols)), 1);
        if (!grow(ok, g->idx, g->idx_cap, n_counts + (cross ? 3 * (size_t)n_cols + (size_t)gr.n + 1 : 0), sizeof(int))) break;
        int* const               counts = g->idx;
        int* const               flags = counts + n_counts;
        int* const               rank = flags + n_cols;
        int* const               list = rank + n_cols;
        int* const               jstart = list + n_cols;
        const popsift_hip_match* back = nullptr;
        int                      n_list = 0;
        if (cross && n_cols > 0) {
            /* J: the (link, right row) a passing row points to, link-major.  One read-back per group, of the segments'
             * starts, sizes the reverse sweep. */
            ok(hipMemsetAsync(flags, 0, sizeof(int) * (size_t)n_cols, s));
            hipLaunchKernelGGL(k_links_mark, dim3((n + 255) / 256), dim3(256), 0, s, fwd, lk, gr.n, n, ratio, max_dist2, flags);
            const FlagOp op{flags, lk, gr.n, list, rank, jstart};
            hipLaunchKernelGGL(k_lcount<FlagOp>, dim3(blocks_of(n_cols)), dim3(C_BLOCK), 0, s, op, n_cols, counts);
            hipLaunchKernelGGL(k_lcompact<FlagOp>, dim3(blocks_of(n_cols)), dim3(C_BLOCK), 0, s, op, n_cols, counts,
                               (const int*)nullptr, jstart + gr.n);
            int* const js = (int*)g->lk_host; /* gr.n + 1 <= n_links + 1 ints: within the head */
            if (!(ok(hipGetLastError()) && ok(hipMemcpyAsync(js, jstart, sizeof(int) * ((size_t)gr.n + 1), hipMemcpyDeviceToHost, s)) &&
                  ok(hipStreamSynchronize(s))))
                break;
            n_list = js[gr.n];
            if (n_list > 0) {
                /* a link without columns has no first column to write its start: it equals the next link's */
                const popsift_hip_link* const l = links + gr.e0;
                for (int k = gr.n - 1; k >= 0; k--)
                    if (width_of(g, l[k]) == 0) js[k] = js[k + 1];
                /* the reverse sweep: segment k of J's gathered rows on the left, member a_k on the right */
                auto side = [&](int k) {
                    return Side{js[k], js[k + 1] - js[k], (int)g->first[l[k].a], g->count[l[k].a], 0};
                };
                int          r_items = 0, r_stride = 1;
                const int    want = plan(gr.n, side, &r_items, &r_stride);
                const size_t bytes = table_bytes(gr.n, r_items);
                /* the stream is idle: the block is free, and may be replaced */
                if (!grow_twin(ok, g->lk_rev, g->lk_rev_host, g->lk_rev_cap, bytes)) break;
                fill(gr.n, side, want, g->lk_rev_host);
                const size_t per = 128 + sizeof(popsift_hip_match) + sizeof(int);
                if (!grow(ok, g->back, g->back_cap, (size_t)n_list, per)) break;
                uint8_t* const gdesc = (uint8_t*)g->back;
                auto* const    brow = (popsift_hip_match*)(gdesc + 128 * (size_t)n_list);
                int* const     gnorm = (int*)(brow + n_list);
                if (ok(hipMemcpyAsync(g->lk_rev, g->lk_rev_host, bytes, hipMemcpyHostToDevice, s)) &&
                    ok(launch_gather_rows(g->d_desc, list, n_list, gdesc, s)) && ok(launch_norms_u8(gdesc, n_list, gnorm, s)))
                    sweep(ok, g, gdesc, gnorm, g->lk_rev, gr.n, r_items, r_stride, n_list, brow, s);
                back = brow;
            }
        }
        if (!ok.good()) break;
        const PairOp op{fwd, lk, back, rank, d_pairs, d_off + gr.e0, gr.n, cross && n_list == 0 ? 1 : 0, (int)std::min<size_t>(room, INT_MAX),
                        ratio, max_dist2};
        hipLaunchKernelGGL(k_lcount<PairOp>, dim3(blocks_of(n)), dim3(C_BLOCK), 0, s, op, n, counts);
        hipLaunchKernelGGL(k_lcompact<PairOp>, dim3(blocks_of(n)), dim3(C_BLOCK), 0, s, op, n, counts,
                           any ? (const int*)(d_run + turn) : (const int*)nullptr, d_run + (turn ^ 1));
        ok(hipGetLastError());
        turn ^= 1;
        any = true;
    }
    /* two downloads: the head, and the pairs found */
    if (ok.good() && any && ok(hipMemcpyAsync(g->lk_host, g->lk_res, head, hipMemcpyDeviceToHost, s)) && ok(hipStreamSynchronize(s))) {
        const int* const h = (const int*)g->lk_host;
        const int        found = h[turn];
        memcpy(offsets, h + 4, sizeof(int32_t) * (size_t)n_links);
        offsets[n_links] = found;
        /* a link without left rows has no first row to write its offset: it equals the next link's */
        for (int e = n_links - 1; e >= 0; e--)
            if (g->count[links[e].a] == 0) offsets[e] = offsets[e + 1];
        *n_pairs = found;
        const size_t n = std::min((size_t)found, cap);
        if (n > 0 && grow_pinned(ok, g->lk_host, g->lk_host_cap, std::max(head, sizeof(popsift_hip_pair) * n)) &&
            ok(hipMemcpyAsync(g->lk_host, d_pairs, sizeof(popsift_hip_pair) * n, hipMemcpyDeviceToHost, s)) &&
            ok(hipStreamSynchronize(s)))
            memcpy(pairs, g->lk_host, sizeof(popsift_hip_pair) * n);
        if (ok.good() && (size_t)found > cap) ok.rc = POPSIFT_HIP_ERR_TOO_SMALL;
    } else {
        (void)hipStreamSynchronize(s);
    }
    return ok.rc;
}

int popsift_hip_gallery_link_points(popsift_hip_gallery* g, const popsift_hip_link* links, int n_links,
                                    const popsift_hip_pair* pairs, const int32_t* offsets, float* pts)
{
    int64_t total = 0;
    if (!offsets || !links_valid(g, links, n_links, &total) || offsets[0] != 0) return POPSIFT_HIP_ERR_INVALID;
    for (int e = 0; e < n_links; e++)
        if (offsets[e + 1] < offsets[e]) return POPSIFT_HIP_ERR_INVALID;
    const int n = offsets[n_links];
    if (n > 0 && (!pairs || !pts)) return POPSIFT_HIP_ERR_INVALID;
    for (int e = 0; e < n_links; e++) {
        const int a = links[e].a, b = links[e].b;
        if (offsets[e + 1] > offsets[e] && !(g->has_xy[a] && g->has_xy[b])) return POPSIFT_HIP_ERR_INVALID;
        for (int i = offsets[e]; i < offsets[e + 1]; i++)
            if (pairs[i].l < 0 || pairs[i].l >= g->count[a] || pairs[i].r < 0 || pairs[i].r >= g->count[b]) return POPSIFT_HIP_ERR_INVALID;
    }
    if (n == 0) return POPSIFT_HIP_OK;
    if (hipSetDevice(g->device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    Status            ok;
    hipStream_t const s = (hipStream_t)g->stream;
    /* device block and its pinned twin: the items, the points */
    const size_t b_items = round16(sizeof(int2) * (size_t)n), b_pts = sizeof(float) * 4 * (size_t)n;
    grow_twin(ok, g->xy_dev, g->xy_host, g->xy_cap, b_items + b_pts);
    if (ok.good()) {
        char* const d = (char*)g->xy_dev;
        char* const h = (char*)g->xy_host;
        int2* const items = (int2*)h;
        for (int e = 0; e < n_links; e++)
            for (int i = offsets[e]; i < offsets[e + 1]; i++)
                items[i] = make_int2((int)(g->first[links[e].a] + pairs[i].l), (int)(g->first[links[e].b] + pairs[i].r));
        if (ok(hipMemcpyAsync(d, h, b_items, hipMemcpyHostToDevice, s))) {
            hipLaunchKernelGGL(k_link_points, dim3((n + 255) / 256), dim3(256), 0, s, (const int2*)d, n, (const float2*)g->d_xy,
                               (float4*)(d + b_items));
            ok(hipGetLastError());
        }
        if (ok.good() && ok(hipMemcpyAsync(h + b_items, d + b_items, b_pts, hipMemcpyDeviceToHost, s)) && ok(hipStreamSynchronize(s)))
            memcpy(pts, h + b_items, b_pts);
    }
    return ok.rc;
}

} /* extern "C" */
