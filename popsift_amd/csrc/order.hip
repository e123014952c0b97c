/*
 * order.hip -- POPSIFT_HIP_ORDER_RASTER: put the per-octave extrema lists into the order include/popsift_hip.h defines,
 * so that everything derived from list order (features, descriptor slabs, byte descriptors, cloned sets, the reverse map,
 * the grid filter's tie-break) is a function of (image, params) alone.
 *
 * The lists arrive in the order in which k_refine's / k_filter_compact's workgroups won their returning atomics.  Per
 * (image, octave) list of n = ext_count() records (ext_list.h), ascending in the tuple
 *     ( iy, ix, lpos, bits(ypos), bits(xpos), bits(sigma) )
 * by a bucket pass and a ranking pass:
 *   k_order_clear    zero the row counters of every octave
 *   k_order_count    rows[iy >> b]++ for every record (plain atomics, no return value used)
 *   k_order_scan     one workgroup per octave: counts -> exclusive start of every row's run
 *   k_order_scatter  record -> scratch list at rows[row]++: the runs are now contiguous, row after row, in ANY order
 *                    inside a run; rows[r] has become the END of run r (= the start of run r + 1)
 *   k_order_place    every record counts the records of its run with a smaller tuple, or an equal tuple at a lower
 *                    scratch position, and goes to run start + that count in the list it came from
 * The scatter's returning atomic only decides where in the scratch run a record waits; its final place is its rank under
 * the whole tuple, and records whose tuples are equal are byte-identical (cell is a function of the position), so no
 * output byte depends on who won.  That is what lets the bucket pass be one unordered scatter instead of the three
 * stable digit passes (histogram per block, scan over digit x block, ballot-ranked scatter: nine launches and a
 * digit x block table per octave) an LSD radix sort on the 34-bit pixel key would take: a run is the extrema of one
 * pixel row of the octave, some tens of records on a full image, and the ranking loop over it is short.  It is written
 * as loops over the run, so a run as long as the whole list (ORDER_COARSE = 15, or every extremum in one row) is only
 * slower, n^2 / 2 comparisons.
 *
 * The row counters sit on thousands of addresses; the one-hot-counter limit of Counters (sift_types.h) does not bite.
 * All launches are sized by capacities (max_extrema), the counts are read on the device, nothing synchronises with the
 * host (the count and the chunk of an octave: ext_list.h; the row scan: wave_dev.h).  Scratch (one InitExt list and the
 * row counters per slot) exists only in a context created with feature_order = POPSIFT_HIP_ORDER_RASTER.
 */
#include <hip/hip_runtime.h>

#include "ext_list.h"
#include "kernels.h"
#include "sift_types.h"
#include "wave_dev.h"

namespace popsift_hip {
namespace {

constexpr int ORDER_CHUNK = POPSIFT_HIP_ORDER_CHUNK; /* records per workgroup of the three per-record kernels */
constexpr int ORDER_ITEMS = ORDER_CHUNK / 256;
static_assert(ORDER_CHUNK % 256 == 0, "whole records per lane");

/* the header's pix(): NaN and everything <= 0 give 0, everything >= 32767 (+inf included) gives 32767 */
__device__ __forceinline__ int order_pix(float v) { return !(v > 0.0f) ? 0 : (v >= 32767.0f ? 32767 : (int)v); }

/* a < b under the header's tuple */
__device__ __forceinline__ bool order_less(const InitExt& a, const InitExt& b, bool& equal)
{
    equal = false;
    const int ay = order_pix(a.ypos), by = order_pix(b.ypos);
    if (ay != by) return ay < by;
    const int ax = order_pix(a.xpos), bx = order_pix(b.xpos);
    if (ax != bx) return ax < bx;
    if (a.lpos != b.lpos) return a.lpos < b.lpos;
    const unsigned int ayb = __float_as_uint(a.ypos), byb = __float_as_uint(b.ypos);
    if (ayb != byb) return ayb < byb;
    const unsigned int axb = __float_as_uint(a.xpos), bxb = __float_as_uint(b.xpos);
    if (axb != bxb) return axb < bxb;
    const unsigned int asb = __float_as_uint(a.sigma), bsb = __float_as_uint(b.sigma);
    if (asb != bsb) return asb < bsb;
    equal = true;
    return false;
}

/* the run of a record: its pixel row without the low `coarse` bits, as an index into the slot's row counters.  The
 * clamp to the octave's last row keeps the index inside the octave's counters whatever the position holds, and leaves
 * the run a non-decreasing function of iy */
__device__ __forceinline__ int order_row(const OrderArgs& a, int o, const InitExt& e)
{
    return a.row_base[o] + min(order_pix(e.ypos) >> a.coarse, a.rows[o] - 1);
}

__global__ __launch_bounds__(256) void k_order_clear(OrderArgs a, OrderBatch ob)
{
    int* __restrict__ rows = ob.s[blockIdx.y].rows;
    for (int r = blockIdx.x * 256 + threadIdx.x; r < a.rows_total; r += gridDim.x * 256) rows[r] = 0;
}

/* SCATTER = false: count the records of every run; true: move every record to the scratch list, run by run */
template <bool SCATTER>
__global__ __launch_bounds__(256) void k_order_bucket(OrderArgs a, OrderBatch ob)
{
    const Counters* __restrict__ ct = ob.s[blockIdx.y].ct;
    const InitExt* __restrict__  list = ob.s[blockIdx.y].list;
    InitExt* __restrict__        tmp = ob.s[blockIdx.y].tmp;
    int* __restrict__            rows = ob.s[blockIdx.y].rows;
    ExtChunk c(a.chunks, ORDER_CHUNK);
    if (!c.within(ext_count(ct, a.max_extrema, c.o))) return;
    const int o = c.o, i0 = c.i0, n = c.n;
    const size_t base = (size_t)o * a.max_extrema;
#pragma unroll
    for (int k = 0; k < ORDER_ITEMS; k++) {
        const int i = i0 + k * 256 + threadIdx.x;
        if (i >= n) continue;
        const InitExt e = list[base + i];
        const int     r = order_row(a, o, e);
        if (SCATTER) {
            const int pos = atomicAdd(&rows[r], 1);
            if (pos >= 0 && pos < n) tmp[base + pos] = e;
        } else {
            atomicAdd(&rows[r], 1);
        }
    }
}

/* one workgroup per (octave, image): counts -> exclusive prefix sums, in place, 256 rows a step */
__global__ __launch_bounds__(256) void k_order_scan(OrderArgs a, OrderBatch ob)
{
    int* __restrict__ rows = ob.s[blockIdx.y].rows + a.row_base[blockIdx.x];
    const int         nr = a.rows[blockIdx.x];
    __shared__ int    s_wsum[4];
    const int         tid = threadIdx.x;
    int               carry = 0;
    for (int r0 = 0; r0 < nr; r0 += 256) { /* workgroup-uniform trip count */
        const int r = r0 + tid;
        const int mine = r < nr ? rows[r] : 0;
        const WgScan scan = wg_scan<4>(mine, s_wsum);
        if (r < nr) rows[r] = carry + scan.excl;
        carry += scan.total;
        __syncthreads(); /* s_wsum is rewritten by the next step */
    }
}

/* rank inside the run, then home: tmp -> list */
__global__ __launch_bounds__(256) void k_order_place(OrderArgs a, OrderBatch ob)
{
    const Counters* __restrict__ ct = ob.s[blockIdx.y].ct;
    InitExt* __restrict__        list = ob.s[blockIdx.y].list;
    const InitExt* __restrict__  tmp = ob.s[blockIdx.y].tmp;
    const int* __restrict__      rows = ob.s[blockIdx.y].rows;
    ExtChunk c(a.chunks, ORDER_CHUNK);
    if (!c.within(ext_count(ct, a.max_extrema, c.o))) return;
    const int o = c.o, i0 = c.i0, n = c.n;
    const size_t base = (size_t)o * a.max_extrema;
#pragma unroll 1
    for (int k = 0; k < ORDER_ITEMS; k++) {
        const int i = i0 + k * 256 + threadIdx.x;
        if (i >= n) continue;
        const InitExt e = tmp[base + i];
        const int     r = order_row(a, o, e);
        /* after the scatter rows[r] is the end of run r, and the end of the run before is its start */
        const int rb = min(max(r > a.row_base[o] ? rows[r - 1] : 0, 0), n);
        const int re = min(max(rows[r], rb), n);
        int       rank = 0;
        for (int j = rb; j < re; j++) {
            const InitExt f = tmp[base + j];
            bool          eq;
            const bool    lt = order_less(f, e, eq);
            rank += (lt || (eq && j < i)) ? 1 : 0;
        }
        if (rb + rank < n) list[base + rb + rank] = e;
    }
}

}  // namespace

size_t order_rows(const PyrDesc& pd)
{
    size_t n = 0;
    for (int o = 0; o < pd.n_oct; o++) n += (size_t)std::max(pd.o[o].h, 1);
    return n;
}

hipError_t launch_order(const PyrDesc& pd, const SiftConsts& sc, int coarse, const OrderBatch& ob, int nb, hipStream_t s)
{
    if (pd.n_oct <= 0) return hipSuccess;
    OrderArgs a{};
    a.n_oct = pd.n_oct;
    a.coarse = coarse;
    a.max_extrema = sc.max_extrema;
    a.chunks = (sc.max_extrema + ORDER_CHUNK - 1) / ORDER_CHUNK;
    int acc = 0;
    for (int o = 0; o < pd.n_oct; o++) {
        a.row_base[o] = acc;
        a.rows[o] = ((std::max(pd.o[o].h, 1) - 1) >> coarse) + 1; /* <= h: inside the order_rows(pd) counters */
        acc += a.rows[o];
    }
    a.rows_total = acc;
    const dim3 block(256), per_rec(pd.n_oct * a.chunks, nb);
    hipLaunchKernelGGL(k_order_clear, dim3(std::min((acc + 255) / 256, 256), nb), block, 0, s, a, ob);
    hipLaunchKernelGGL(k_order_bucket<false>, per_rec, block, 0, s, a, ob);
    hipLaunchKernelGGL(k_order_scan, dim3(pd.n_oct, nb), block, 0, s, a, ob);
    hipLaunchKernelGGL(k_order_bucket<true>, per_rec, block, 0, s, a, ob);
    hipLaunchKernelGGL(k_order_place, per_rec, block, 0, s, a, ob);
    return hipGetLastError();
}

}  // namespace popsift_hip
