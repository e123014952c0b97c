/*
 * match_gallery.hip -- one byte set against a gallery of byte sets (popsift_hip_match_gallery,
 * popsift_hip_match_pairs_gallery; the gallery object itself is sets.hip).  The rule is the per-pair calls', member by
 * member (include/popsift_hip.h); what is new is that the members of a group share their launches:
 *
 *   k_match_gallery   k_match_u8 (match_u8.hip) over a work list.  A workgroup takes one item = (member of the group,
 *                     block of U_LB query rows, split of that member's right tiles).  Tiles are member-local: the
 *                     workgroup sees the member's rows and norms through pointers offset by first[m] and its count as
 *                     r_len, so the clamp of rows past the end and the index test are k_match_u8's and no load leaves
 *                     the member.  Operand loads, sign flip, the four 32x32x32 i8 steps, the epilogue and the half merge
 *                     are restated from k_match_u8 operation for operation (sharing a header would have to be shown to
 *                     leave that kernel's ISA alone).  An empty member has no item.
 *   k_gallery_finish  per (member, query row): merge the member's splits under (d, j) and write the member-local row; an
 *                     empty member's rows are {0, 0, 0, inf, inf} from here.
 *   pairs             k_gallery_mark flags the gallery row first[m] + best of every row that passes conditions 2 and 3;
 *                     one compaction turns the flags into the ascending list J of GLOBAL gallery rows and its ranks; the
 *                     reverse sweep is the per-pair one (launch_gather_rows, launch_norms_u8, launch_match_u8 with J on
 *                     the left and the query on the right); a second compaction over the group's (member, row) elements
 *                     emits the pairs in flat order behind those of the earlier groups.  The exclusive rank of a member's
 *                     first element IS offsets[m], so the same scan that places the pairs writes the offsets.
 *                     Every pair is counted, those below the device buffer's size are written.
 *
 * The host walks the members in groups of max(1, group_rows / l_len): the scratch follows the group, not the gallery.
 * Per group: one work-list upload, the sweep, the finish, and for pairs 2 (5 + the reverse sweep with the cross-check)
 * more launches, however many members the group has.
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

constexpr int U_ROW = 144;         /* as match_u8.hip: bytes per LDS row */
constexpr int U_FAR = INT_MAX / 2; /* as match_u8.hip: norm of a row past the member's end */
constexpr int C_BLOCK = 256;       /* elements per workgroup of the compactions */

/* a member of the group in flight: its rows of the gallery, and over how many items its right tiles are split */
struct GMember {
    int first, count, n_split, pad;
};
/* a workgroup's share of the sweep */
struct GItem {
    int member, lblock, split, pad;
};
static_assert(sizeof(GMember) == 16 && sizeof(GItem) == 16, "uploaded as 16-byte records");

__device__ __forceinline__ v4i to_signed(v4i v)
{
    const int f = (int)0x80808080u;
    return v4i{v.x ^ f, v.y ^ f, v.z ^ f, v.w ^ f};
}

__device__ __forceinline__ int k_off(int s, int h) { return 32 * s + 16 * h; }

/* partial: [member of the group][query row][stride] */
__global__ __launch_bounds__(256, 2) void k_match_gallery(const uint8_t* __restrict__ ldesc, int l_len,
                                                          const int* __restrict__ lnorm, const uint8_t* __restrict__ gdesc,
                                                          const int* __restrict__ gnorm, const GMember* __restrict__ members,
                                                          const GItem* __restrict__ items, int stride,
                                                          Top2<int>* __restrict__ partial)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_r[U_RB * U_ROW];
    __shared__ __attribute__((aligned(16))) int     s_rn[U_RB];
    const GItem          it = items[blockIdx.x];
    const GMember        mem = members[it.member];
    const uint8_t* const rdesc = gdesc + (size_t)mem.first * 128;
    const int* const     rnorm = gnorm + mem.first;
    const int            r_len = mem.count, n_split = mem.n_split; /* r_len >= 1: an empty member has no item */

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int l = it.lblock * U_LB + wave * 32 + col;
    const int lc = min(l, l_len - 1); /* lanes past the end work on the last row and write nothing */

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
    if (half == 0 && l < l_len) partial[((size_t)it.member * l_len + l) * stride + it.split] = best;
}

/* element e = member * l_len + row of the group; n = members * l_len */
__global__ __launch_bounds__(256) void k_gallery_finish(const Top2<int>* __restrict__ partial, const GMember* __restrict__ members,
                                                        int l_len, int n, int stride, popsift_hip_match* __restrict__ out)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const GMember mem = members[e / l_len];
    Top2<int>     t{U_NONE, U_NONE, 0, 0};
    if (mem.count > 0) {
        t = partial[(size_t)e * stride];
        for (int k = 1; k < mem.n_split; k++) {
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

/* flags: one int per gallery row of the group, row 0 = gallery row `base` */
__global__ __launch_bounds__(256) void k_gallery_mark(const popsift_hip_match* __restrict__ fwd, const GMember* __restrict__ members,
                                                      int l_len, int n, float ratio, float max_dist2, int base,
                                                      int* __restrict__ flags)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const GMember mem = members[e / l_len];
    if (mem.count == 0) return; /* condition 1 */
    const popsift_hip_match m = fwd[e];
    if (row_passes(m, ratio, max_dist2)) flags[mem.first - base + m.best] = 1;
}

struct Flagged {
    const int* flags;
    __device__ bool operator()(int j) const { return flags[j] != 0; }
};

/* J holds global gallery rows, the rank is found by the row's place in the group */
struct WriteIndex {
    int* list;
    int* rank;
    int  base;
    __device__ void kept(int pos, int j) const
    {
        list[pos] = base + j;
        rank[j] = pos;
    }
    __device__ void every(int, int) const {}
};

/* element e yields a pair: its member is not empty, its row passes, and with the cross-check the row is the nearest query
 * descriptor of its best gallery row.  none: the group's J is empty and `back` was never formed. */
struct PairKept {
    const popsift_hip_match* fwd;
    const GMember*           members;
    const popsift_hip_match* back; /* null: no cross-check */
    const int*               rank;
    int                      l_len, base, none;
    float                    ratio, max_dist2;
    __device__ bool operator()(int e) const
    {
        if (none) return false;
        const GMember mem = members[e / l_len];
        if (mem.count == 0) return false;
        const popsift_hip_match m = fwd[e];
        if (!row_passes(m, ratio, max_dist2)) return false;
        return !back || back[rank[mem.first - base + m.best]].best == e % l_len;
    }
};

/* pos counts from the first pair of the call.  Every pair is counted; those the buffer has room for are written.  The
 * first element of a member has as many pairs in front of it as the members before have: offsets[m]. */
struct WritePair {
    const popsift_hip_match* fwd;
    popsift_hip_pair*        pairs;
    int*                     offsets; /* of the group's first member */
    int                      l_len, room;
    __device__ void kept(int pos, int e) const
    {
        if (pos >= room) return;
        const popsift_hip_match m = fwd[e];
        pairs[pos] = popsift_hip_pair{e % l_len, m.best, m.dist_best, m.dist_second};
    }
    __device__ void every(int pos, int e) const
    {
        if (e % l_len == 0) offsets[e / l_len] = pos;
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

template <class Keep>
__global__ __launch_bounds__(C_BLOCK) void k_gcount(Keep keep, int n, int* __restrict__ counts)
{
    const int e = blockIdx.x * C_BLOCK + threadIdx.x;
    int       total;
    (void)block_rank(e < n && keep(e), &total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

/* Order-preserving compaction in front of which *start elements already lie (null: none).  The last workgroup writes
 * the new total to *end (never the word *start is read from) and, when given, to *end2. */
template <class Keep, class Write>
__global__ __launch_bounds__(C_BLOCK) void k_gcompact(Keep keep, Write write, int n, const int* __restrict__ counts,
                                                      const int* __restrict__ start, int* __restrict__ end,
                                                      int* __restrict__ end2)
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
    const bool k = e < n && keep(e);
    int        total;
    const int  before = block_rank(k, &total);
    if (e < n) write.every(first + before, e);
    if (k) write.kept(first + before, e);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        *end = first + total;
        if (end2) *end2 = first + total;
    }
}

int blocks_of(int n) { return (n + C_BLOCK - 1) / C_BLOCK; }

/* ---- the host side */

struct Group {
    int     m0, n;      /* members [m0, m0 + n) */
    int     n_items, stride;
    int64_t base, rows; /* their gallery rows [base, base + rows) */
};

/* The member table and the work list of a group, built in the gallery's pinned block and uploaded.  A call's first group
 * finds the block free (the call before ended with a wait for the stream); a later group rewrites it only after the
 * upload before it has been read (w_event, recorded when another group follows). */
void upload_group(Status& ok, popsift_hip_gallery* g, int l_len, Group& gr, bool first, bool more, hipStream_t s)
{
    const int lblocks = (l_len + U_LB - 1) / U_LB;
    int64_t   unsplit = 0;
    for (int m = gr.m0; m < gr.m0 + gr.n; m++)
        if (g->count[m] > 0) unsplit += lblocks;
    /* members are split only when the launch would otherwise have fewer than U_GROUPS workgroups */
    const int want = unsplit > 0 && unsplit < U_GROUPS ? (int)((U_GROUPS + unsplit - 1) / unsplit) : 1;
    int64_t   n_items = 0;
    gr.stride = 1;
    for (int m = gr.m0; m < gr.m0 + gr.n; m++) {
        if (g->count[m] == 0) continue;
        const int ns = std::min(want, (g->count[m] + U_RB - 1) / U_RB);
        n_items += (int64_t)ns * lblocks;
        gr.stride = std::max(gr.stride, ns);
    }
    gr.n_items = (int)n_items;
    const size_t bytes = sizeof(GMember) * (size_t)gr.n + sizeof(GItem) * (size_t)n_items;
    if (!ok.good()) return;
    if (bytes > g->w_cap) {
        if (!ok(hipStreamSynchronize(s))) return; /* nothing reads the old block any more */
        grow_twin(ok, g->w_dev, g->w_host, g->w_cap, std::max(bytes, 2 * g->w_cap));
    } else if (!first) {
        ok(hipEventSynchronize((hipEvent_t)g->w_event));
    }
    if (!ok.good()) return;
    GMember* const mem = (GMember*)g->w_host;
    GItem*         it = (GItem*)(mem + gr.n);
    for (int k = 0; k < gr.n; k++) {
        const int m = gr.m0 + k, count = g->count[m];
        const int ns = count > 0 ? std::min(want, (count + U_RB - 1) / U_RB) : 0;
        mem[k] = GMember{(int)g->first[m], count, ns, 0};
        /* workgroups next to each other walk the same right tiles */
        for (int sp = 0; sp < ns; sp++)
            for (int lb = 0; lb < lblocks; lb++) *it++ = GItem{k, lb, sp, 0};
    }
    if (ok(hipMemcpyAsync(g->w_dev, g->w_host, bytes, hipMemcpyHostToDevice, s)) && more)
        ok(hipEventRecord((hipEvent_t)g->w_event, s));
}

/* What both calls share.  begin(): the gallery's GPU is current, the query's bytes are on it and its norms formed;
 * forward(): the rows of one group in g->rows. */
struct Sweep {
    popsift_hip_gallery* g;
    const uint8_t*       ldesc = nullptr;
    int                  l_len, per_group;
    hipStream_t          s;
    PeerCopy             peer;

    void begin(Status& ok, const popsift_hip_bytefeatures* l, popsift_hip_gallery* gal)
    {
        g = gal;
        l_len = l->n_desc;
        s = (hipStream_t)g->stream;
        const int rows = g->group_rows > 0 ? g->group_rows : POPSIFT_HIP_GALLERY_GROUP_ROWS;
        per_group = std::max(rows / l_len, 1);
        ldesc = l->d_desc;
        if (peer.fetch(ok, g->device, l->device, {{l->d_desc, 128 * (size_t)l_len}})) ldesc = (const uint8_t*)peer.at[0];
        if (grow(ok, g->lnorm, g->lnorm_cap, (size_t)l_len, sizeof(int))) ok(launch_norms_u8(ldesc, l_len, g->lnorm, s));
        grow(ok, g->rows, g->rows_cap, (size_t)std::min(per_group, g->n_members) * (size_t)l_len, sizeof(popsift_hip_match));
    }

    Group group_at(int m0) const
    {
        Group gr{};
        gr.m0 = m0;
        gr.n = std::min(per_group, g->n_members - m0);
        gr.base = g->first[m0];
        gr.rows = g->first[m0 + gr.n - 1] + g->count[m0 + gr.n - 1] - gr.base;
        return gr;
    }

    void forward(Status& ok, Group& gr)
    {
        upload_group(ok, g, l_len, gr, gr.m0 == 0, gr.m0 + gr.n < g->n_members, s);
        const int n = gr.n * l_len;
        if (!grow(ok, g->partial, g->partial_cap, (size_t)n * gr.stride * sizeof(Top2<int>), 1)) return;
        const GMember* const mem = (const GMember*)g->w_dev;
        if (gr.n_items > 0)
            hipLaunchKernelGGL(k_match_gallery, dim3(gr.n_items), dim3(256), 0, s, ldesc, l_len, g->lnorm, g->d_desc, g->d_norm,
                               mem, (const GItem*)(mem + gr.n), gr.stride, (Top2<int>*)g->partial);
        hipLaunchKernelGGL(k_gallery_finish, dim3((n + 255) / 256), dim3(256), 0, s, (const Top2<int>*)g->partial, mem, l_len, n,
                           gr.stride, (popsift_hip_match*)g->rows);
        ok(hipGetLastError());
    }
};

int64_t total_rows(const popsift_hip_bytefeatures* l, const popsift_hip_gallery* g) { return (int64_t)g->n_members * l->n_desc; }

}  // namespace
}  // namespace popsift_hip

using namespace popsift_hip;

extern "C" {

int popsift_hip_match_gallery(const popsift_hip_bytefeatures* l, popsift_hip_gallery* g, popsift_hip_match* out, size_t cap_rows)
{
    if (!l || !g) return POPSIFT_HIP_ERR_INVALID;
    const int64_t total = total_rows(l, g);
    if (total > INT32_MAX || (total > 0 && !out)) return POPSIFT_HIP_ERR_INVALID;
    if (cap_rows < (size_t)total) return POPSIFT_HIP_ERR_TOO_SMALL; /* all or nothing */
    if (total == 0) return POPSIFT_HIP_OK;
    if (hipSetDevice(g->device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    Status ok;
    Sweep  sw;
    sw.begin(ok, l, g);
    if (ok.good() && (size_t)total > g->rows_host_cap) {
        if (g->rows_host) (void)hipHostFree(g->rows_host);
        g->rows_host = nullptr;
        g->rows_host_cap = 0;
        if (ok(hipHostMalloc(&g->rows_host, sizeof(popsift_hip_match) * (size_t)total, hipHostMallocDefault)))
            g->rows_host_cap = (size_t)total;
    }
    for (int m0 = 0; ok.good() && m0 < g->n_members; m0 += sw.per_group) {
        Group gr = sw.group_at(m0);
        sw.forward(ok, gr);
        if (ok.good())
            ok(hipMemcpyAsync((popsift_hip_match*)g->rows_host + (size_t)m0 * sw.l_len, g->rows,
                              sizeof(popsift_hip_match) * (size_t)gr.n * sw.l_len, hipMemcpyDeviceToHost, sw.s));
    }
    if (ok.good() && ok(hipStreamSynchronize(sw.s))) memcpy(out, g->rows_host, sizeof(popsift_hip_match) * (size_t)total);
    else (void)hipStreamSynchronize(sw.s); /* nothing of this call is in flight when its peer copy goes */
    return ok.rc;
}

int popsift_hip_match_pairs_gallery(const popsift_hip_bytefeatures* l, popsift_hip_gallery* g, const popsift_hip_match_opts* opts,
                                    popsift_hip_pair* pairs, size_t cap, int32_t* offsets, int* n_pairs)
{
    if (!l || !g || !opts || !offsets || !n_pairs || (cap > 0 && !pairs)) return POPSIFT_HIP_ERR_INVALID;
    if (!(opts->ratio >= 0.0f) || std::isinf(opts->ratio) || std::isnan(opts->max_dist2) || opts->reserved != 0 ||
        (opts->cross_check != 0 && opts->cross_check != 1))
        return POPSIFT_HIP_ERR_INVALID;
    const int64_t total = total_rows(l, g);
    if (total > INT32_MAX) return POPSIFT_HIP_ERR_INVALID;
    *n_pairs = 0;
    memset(offsets, 0, sizeof(int32_t) * ((size_t)g->n_members + 1));
    if (total == 0 || g->n_desc == 0) return POPSIFT_HIP_OK;
    if (hipSetDevice(g->device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    const int    n_mem = g->n_members, l_len = l->n_desc;
    const bool   cross = opts->cross_check != 0;
    const float  ratio = opts->ratio, max_dist2 = opts->max_dist2;
    const size_t room = std::min(cap, (size_t)total); /* the device pair buffer */
    Status       ok;
    Sweep        sw;
    sw.begin(ok, l, g);
    hipStream_t const s = sw.s;

    /* result block: offsets[n_mem + 1], the running pair count (two words, written and read in turn; the first group
     * reads none), |J|; the pairs */
    const size_t head = round16(sizeof(int) * ((size_t)n_mem + 4));
    grow_twin(ok, g->res, g->res_host, g->res_cap, head + sizeof(popsift_hip_pair) * room);
    int* const              d_off = (int*)g->res;
    int* const              d_run = d_off + n_mem + 1;
    int* const              d_nlist = d_run + 2;
    popsift_hip_pair* const d_pairs = (popsift_hip_pair*)((char*)g->res + head);

    size_t most = cross ? 0 : room; /* pairs the download has to cover */
    int    turn = 0;
    for (int m0 = 0; ok.good() && m0 < n_mem; m0 += sw.per_group, turn ^= 1) {
        Group gr = sw.group_at(m0);
        sw.forward(ok, gr);
        const int            n = gr.n * l_len, r_len = (int)gr.rows;
        const GMember* const mem = (const GMember*)g->w_dev;
        const auto* const    fwd = (const popsift_hip_match*)g->rows;
        const size_t         n_counts = (size_t)std::max(blocks_of(std::max(n, r_len)), 1);
        if (!grow(ok, g->idx, g->idx_cap, n_counts + (cross ? 3 * (size_t)r_len : 0), sizeof(int))) break;
        int* const               counts = g->idx;
        int* const               flags = counts + n_counts;
        int* const               rank = flags + r_len;
        int* const               list = rank + r_len;
        const popsift_hip_match* back = nullptr;
        int                      n_list = 0;
        if (cross && r_len > 0) {
            /* J: the gallery rows a passing row points to.  |J| sizes the reverse sweep: one 4-byte read-back per group */
            ok(hipMemsetAsync(flags, 0, sizeof(int) * (size_t)r_len, s));
            hipLaunchKernelGGL(k_gallery_mark, dim3((n + 255) / 256), dim3(256), 0, s, fwd, mem, l_len, n, ratio, max_dist2,
                               (int)gr.base, flags);
            const Flagged keep{flags};
            hipLaunchKernelGGL(k_gcount<Flagged>, dim3(blocks_of(r_len)), dim3(C_BLOCK), 0, s, keep, r_len, counts);
            hipLaunchKernelGGL((k_gcompact<Flagged, WriteIndex>), dim3(blocks_of(r_len)), dim3(C_BLOCK), 0, s, keep,
                               WriteIndex{list, rank, (int)gr.base}, r_len, counts, (const int*)nullptr, d_nlist, (int*)nullptr);
            if (ok(hipGetLastError()) && ok(hipMemcpyAsync(g->res_host, d_nlist, sizeof(int), hipMemcpyDeviceToHost, s)) &&
                ok(hipStreamSynchronize(s)))
                n_list = *(const int*)g->res_host;
            if (ok.good() && n_list > 0) {
                /* the per-pair reverse sweep: J's rows on the left, the query on the right, no segments */
                const size_t per = 128 + sizeof(popsift_hip_match) + sizeof(int);
                if (!grow(ok, g->back, g->back_cap, (size_t)n_list, per)) break;
                uint8_t* const gdesc = (uint8_t*)g->back;
                auto* const    brow = (popsift_hip_match*)(gdesc + 128 * (size_t)n_list);
                int* const     gnorm = (int*)(brow + n_list);
                const int      n_split = splits(n_list, l_len, U_LB, U_RB, U_GROUPS);
                if (!grow(ok, g->partial, g->partial_cap, partial_bytes(n_list, n_split, sizeof(Top2<int>)), 1)) break;
                ok(launch_gather_rows(g->d_desc, list, n_list, gdesc, s)) && ok(launch_norms_u8(gdesc, n_list, gnorm, s)) &&
                    ok(launch_match_u8(gdesc, n_list, gnorm, sw.ldesc, l_len, g->lnorm, n_split, g->partial, brow, s));
                back = brow;
                most = std::min(room, most + (size_t)n_list); /* every member of J has one nearest query descriptor */
            }
        }
        if (!ok.good()) break;
        const bool     last = m0 + gr.n >= n_mem;
        const PairKept keep{fwd, mem, back, rank, l_len, (int)gr.base, cross && n_list == 0 ? 1 : 0, ratio, max_dist2};
        hipLaunchKernelGGL(k_gcount<PairKept>, dim3(blocks_of(n)), dim3(C_BLOCK), 0, s, keep, n, counts);
        hipLaunchKernelGGL((k_gcompact<PairKept, WritePair>), dim3(blocks_of(n)), dim3(C_BLOCK), 0, s, keep,
                           WritePair{fwd, d_pairs, d_off + m0, l_len, (int)room}, n, counts, m0 == 0 ? (const int*)nullptr : (const int*)(d_run + turn),
                           d_run + (turn ^ 1), last ? d_off + n_mem : (int*)nullptr);
        ok(hipGetLastError());
    }
    /* one download: offsets and pairs */
    if (ok.good() && ok(hipMemcpyAsync(g->res_host, g->res, head + sizeof(popsift_hip_pair) * most, hipMemcpyDeviceToHost, s)) &&
        ok(hipStreamSynchronize(s))) {
        const int* const h = (const int*)g->res_host;
        memcpy(offsets, h, sizeof(int32_t) * ((size_t)n_mem + 1));
        const int found = h[n_mem];
        *n_pairs = found;
        const size_t n = std::min((size_t)found, cap);
        if (n > 0) memcpy(pairs, (const char*)g->res_host + head, sizeof(popsift_hip_pair) * n);
        if ((size_t)found > cap) ok.rc = POPSIFT_HIP_ERR_TOO_SMALL;
    } else {
        (void)hipStreamSynchronize(s);
    }
    return ok.rc;
}

} /* extern "C" */
