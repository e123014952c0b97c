/*
 * strongest.hip -- popsift_hip_set_keep_strongest: keep the n refined extrema of an image with the largest DoG response
 * (OpenCV's nfeatures / KeyPointsFilter::retainBest), all octaves together, and hand every survivor's response out.
 * The rule is stated in include/popsift_hip.h; tests/strongest_rule.py states it in numpy.
 *
 * The pass runs between refinement (and the ordering pass) and orientation, where the grid filter runs, and like the
 * grid filter it leaves its survivors in the slot's second list (iext2): everything after it sees the shorter lists.
 *   k_strongest_response  one lane per record: |D| at the sample nearest to the refined position, read through the
 *                         DogView k_refine reads through; responses in flattened list order (octave after octave)
 *   k_strongest_select    ONE workgroup per image: four 8-bit MSD radix passes over the image's keys with a histogram in
 *                         LDS -> t, the key of the n-th largest; then the survivor count of every chunk of
 *                         POPSIFT_HIP_STRONGEST_CHUNK records and its exclusive prefix within its octave.  A few hundred
 *                         thousand keys at most: hundreds of steps of 1024 lanes, no global atomic, no launch per digit
 *   k_strongest_compact   one workgroup per chunk: stable prefix scatter of the records whose key >= t, and of their
 *                         responses, to chunk offset + rank; the new per-octave counts replace the old ones
 * The compaction is STABLE: survivors keep their octave and their relative order, so a raster-ordered list stays one and
 * needs no second ordering pass (k_filter_compact appends by arrival and does).  Every record that ties with the n-th
 * stays, so the surviving set depends on the records alone, not on their order.
 *
 * All launches are sized by capacities (max_extrema); the counts are read on the device, nothing synchronises with the
 * host.  The buffers exist only in a context on which the setting was ever on.  The list rules (count, prefix, chunk of an
 * octave) come from ext_list.h, the scans and the per-digit histogram add from wave_dev.h.
 */
#include <hip/hip_runtime.h>

#include "dog_view.h"
#include "ext_list.h"
#include "kernels.h"
#include "sift_types.h"
#include "wave_dev.h"

namespace popsift_hip {
namespace {

constexpr int STRONG_CHUNK = POPSIFT_HIP_STRONGEST_CHUNK; /* records per workgroup of the per-record kernels */
constexpr int STRONG_ITEMS = STRONG_CHUNK / 256;
constexpr int SELECT_LANES = 1024;
constexpr int SELECT_ITEMS = 16; /* keys per lane and step of a radix pass */
static_assert(STRONG_CHUNK % 256 == 0, "whole records per lane");
static_assert(STRONG_CHUNK == SELECT_LANES, "k_strongest_select counts one chunk per step");

/* the header's key: responses are >= 0 or NaN, so the bit pattern orders them */
__device__ __forceinline__ unsigned int strong_key(float r) { return r != r ? 0u : __float_as_uint(r); }

template <bool FLY>
__global__ __launch_bounds__(256) void k_strongest_response(const PyrDesc* __restrict__ pdp, StrongArgs a, StrongBatch sb)
{
    const Counters* __restrict__ ct = sb.s[blockIdx.y].ct;
    const InitExt* __restrict__  in = sb.s[blockIdx.y].in;
    float* __restrict__          resp = sb.s[blockIdx.y].resp_in;
    __shared__ int s_ps[PS_MAX_OCT + 1];
    ext_prefix(s_ps, ct, a.max_extrema, a.n_oct);
    ExtChunk c(a.chunks, STRONG_CHUNK);
    if (!c.within(s_ps[c.o + 1] - s_ps[c.o])) return;
    const int o = c.o, i0 = c.i0, n = c.n;
    const OctDesc* od = &pdp->o[o];
    DogView<FLY>   dog;
    dog.arena = (const char*)sb.s[blockIdx.y].arena;
    dog.off = (unsigned int)(FLY ? od->data_off : od->dog_off);
    dog.ps = (unsigned int)od->plane_stride;
    dog.w = od->w;
    dog.h = od->h;
    dog.pitch = od->pitch;
    dog.nl = a.levels + 2;
#pragma unroll
    for (int k = 0; k < STRONG_ITEMS; k++) {
        const int i = i0 + k * 256 + threadIdx.x;
        if (i >= n) continue;
        const InitExt e = in[(size_t)o * a.max_extrema + i];
        float         r = __uint_as_float(0x7fc00000u);
        const bool    finite = (__float_as_uint(e.xpos) & 0x7f800000u) != 0x7f800000u &&
                            (__float_as_uint(e.ypos) & 0x7f800000u) != 0x7f800000u;
        if (finite) {
            /* clamped as floats: the same integers as clamp((int)floorf(v + 0.5f), 0, size - 1) wherever the conversion
             * is defined */
            const int xi = (int)fminf(fmaxf(floorf(e.xpos + 0.5f), 0.0f), (float)(dog.w - 1));
            const int yi = (int)fminf(fmaxf(floorf(e.ypos + 0.5f), 0.0f), (float)(dog.h - 1));
            const int di = clampi(e.lpos, 1, a.levels);
            r = fabsf(dog.raw(xi, yi, di));
        }
        resp[s_ps[o] + i] = r;
    }
}

/* one LDS add per distinct digit among a wave's first candidates, then one per lane that is left: in the first passes
 * almost every key of an image shares its digit (responses of one order of magnitude share their exponent) */
__device__ __forceinline__ void select_count(int* hist, int digit, bool act)
{
    const int                lane = threadIdx.x & 63;
    const unsigned long long left = wave_each_key(
        digit, act,
        [&](int d, unsigned long long same, int leader) {
            if (lane == leader) atomicAdd(&hist[d], __popcll(same));
        },
        2);
    if ((left >> lane) & 1ull) atomicAdd(&hist[digit], 1);
}

__global__ __launch_bounds__(SELECT_LANES) void k_strongest_select(StrongArgs a, StrongBatch sb)
{
    const Counters* __restrict__ ct = sb.s[blockIdx.y].ct;
    const float* __restrict__    resp = sb.s[blockIdx.y].resp_in;
    StrongState* __restrict__    st = sb.s[blockIdx.y].state;
    int* __restrict__            chunk_off = sb.s[blockIdx.y].chunk_off;
    __shared__ int s_ps[PS_MAX_OCT + 1];
    __shared__ int s_hist[256];
    __shared__ int s_new_ct[PS_MAX_OCT];
    __shared__ int s_digit, s_above;
    const int      tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int total = ext_prefix(s_ps, ct, a.max_extrema, a.n_oct);

    /* t = the keep-th largest key: digit by digit from the top, among the keys that share the digits chosen so far.
     * Everything below is workgroup-uniform but the lanes' own keys, so every barrier is reached by all waves */
    unsigned int t = 0u;
    if (total > a.keep) {
        int rem = a.keep; /* rank of t among the remaining candidates, 1 .. their number */
        for (int pass = 0; pass < 4; pass++) {
            const int shift = 24 - 8 * pass;
            if (tid < 256) s_hist[tid] = 0;
            __syncthreads();
            /* SELECT_ITEMS independent loads per lane and step: one workgroup has to hide the memory latency itself.
             * The index is clamped, not guarded: a load under a lane's own condition is not moved ahead of the work on
             * the load before it, and the step then pays the latency SELECT_ITEMS times over */
            for (int g0 = 0; g0 < total; g0 += SELECT_LANES * SELECT_ITEMS) {
                unsigned int key[SELECT_ITEMS];
#pragma unroll
                for (int k = 0; k < SELECT_ITEMS; k++) {
                    const int g = g0 + k * SELECT_LANES + tid;
                    key[k] = strong_key(resp[min(g, total - 1)]);
                }
#pragma unroll
                for (int k = 0; k < SELECT_ITEMS; k++) {
                    const bool act = g0 + k * SELECT_LANES + tid < total && (pass == 0 || (key[k] >> (shift + 8)) == t);
                    select_count(s_hist, (int)((key[k] >> shift) & 255u), act);
                }
            }
            __syncthreads();
            if (wave == 0) {
                /* lane l holds digits 4l .. 4l+3; candidates with a larger digit: the lanes above, then inside the lane */
                int c[4], sum = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) sum += c[b] = s_hist[4 * lane + b];
                const int incl = wave_incl_scan(sum);
                int       above = wave_scan_total(incl) - incl; /* the lanes above = all - those up to this one */
#pragma unroll
                for (int b = 3; b >= 0; b--) {
                    if (above < rem && rem <= above + c[b]) { /* exactly one digit satisfies this */
                        s_digit = 4 * lane + b;
                        s_above = above;
                    }
                    above += c[b];
                }
            }
            __syncthreads();
            t = (t << 8) | (unsigned int)s_digit;
            rem -= s_above;
        }
    }

    if (tid == 0) {
        st->t = t;
        st->total = total;
    }
    if (tid < PS_MAX_OCT) {
        st->old_ct[tid] = s_ps[tid + 1] - s_ps[tid]; /* from n_oct upward every entry is the total: counts of 0 */
        st->old_ps[tid] = s_ps[tid];
    }
    /* survivors per chunk, a chunk per wave (no barrier inside: the trip counts are wave-uniform) ... */
    for (int o = 0; o < a.n_oct; o++) {
        const int n = s_ps[o + 1] - s_ps[o];
        const int n_chunks = (n + STRONG_CHUNK - 1) / STRONG_CHUNK; /* <= a.chunks */
        for (int c = wave; c < n_chunks; c += SELECT_LANES / 64) {
            int cnt = 0;
#pragma unroll
            for (int k = 0; k < STRONG_CHUNK / 64; k++) {
                const int  i = c * STRONG_CHUNK + k * 64 + lane;
                const bool keep = strong_key(resp[s_ps[o] + min(i, n - 1)]) >= t && i < n; /* clamped: see above */
                cnt += __popcll(__ballot(keep));
            }
            if (lane == 0) chunk_off[o * a.chunks + c] = cnt;
        }
    }
    __syncthreads(); /* the counts are this workgroup's own global writes */
    /* ... -> exclusive prefix within the octave, an octave per wave, 64 chunks a step ... */
    for (int o = wave; o < a.n_oct; o += SELECT_LANES / 64) {
        const int n = s_ps[o + 1] - s_ps[o];
        const int n_chunks = (n + STRONG_CHUNK - 1) / STRONG_CHUNK;
        int       run = 0;
        for (int c0 = 0; c0 < n_chunks; c0 += 64) {
            const int c = c0 + lane;
            const int mine = c < n_chunks ? chunk_off[o * a.chunks + c] : 0;
            const int incl = wave_incl_scan(mine);
            if (c < n_chunks) chunk_off[o * a.chunks + c] = run + incl - mine;
            run += wave_scan_total(incl);
        }
        if (lane == 0) s_new_ct[o] = run;
    }
    __syncthreads();
    /* ... and per octave -> exclusive prefix within the image */
    if (tid == 0) {
        int new_ps = 0;
        for (int o = 0; o < PS_MAX_OCT; o++) {
            const int n = o < a.n_oct ? s_new_ct[o] : 0;
            st->new_ct[o] = n;
            st->new_ps[o] = new_ps;
            new_ps += n;
        }
    }
}

__global__ __launch_bounds__(256) void k_strongest_compact(StrongArgs a, StrongBatch sb)
{
    Counters* __restrict__          ct = sb.s[blockIdx.y].ct;
    const InitExt* __restrict__     in = sb.s[blockIdx.y].in;
    InitExt* __restrict__           out = sb.s[blockIdx.y].out;
    const float* __restrict__       resp_in = sb.s[blockIdx.y].resp_in;
    float* __restrict__             resp_out = sb.s[blockIdx.y].resp_out;
    const StrongState* __restrict__ st = sb.s[blockIdx.y].state;
    const int* __restrict__         chunk_off = sb.s[blockIdx.y].chunk_off;
    __shared__ int s_wsum[4];
    ExtChunk       c(a.chunks, STRONG_CHUNK);
    const int      o = c.o, i0 = c.i0, tid = threadIdx.x;
    /* the counts of before the pass come from the state: ext_ct[o] is rewritten here, by the octave's first chunk, which
     * exists for every octave whatever its count */
    if (c.chunk == 0 && tid == 0) ct->ext_ct[o] = st->new_ct[o];
    if (!c.within(st->old_ct[o])) return; /* whole workgroup */
    const int n = c.n;
    const unsigned int t = st->t;
    const int          src = st->old_ps[o], dst = st->new_ps[o], new_n = st->new_ct[o];

    /* STRONG_ITEMS consecutive records per lane: rank = survivors before the lane + survivors before it in the lane;
     * the responses decide, only the survivors' records are read */
    float   r[STRONG_ITEMS];
    bool    keep[STRONG_ITEMS];
    int     self = 0;
#pragma unroll
    for (int k = 0; k < STRONG_ITEMS; k++) {
        const int i = i0 + tid * STRONG_ITEMS + k;
        keep[k] = false;
        if (i < n) {
            r[k] = resp_in[src + i];
            keep[k] = strong_key(r[k]) >= t;
        }
        self += keep[k] ? 1 : 0;
    }
    int pos = chunk_off[o * a.chunks + c.chunk] + wg_scan<4>(self, s_wsum).excl;
#pragma unroll
    for (int k = 0; k < STRONG_ITEMS; k++)
        if (keep[k]) {
            if (pos >= 0 && pos < new_n) { /* new_n <= n <= max_extrema */
                out[(size_t)o * a.max_extrema + pos] = in[(size_t)o * a.max_extrema + i0 + tid * STRONG_ITEMS + k];
                resp_out[dst + pos] = r[k];
            }
            pos++;
        }
}

}  // namespace

int strongest_chunks(int max_extrema) { return (std::max(max_extrema, 1) + STRONG_CHUNK - 1) / STRONG_CHUNK; }

hipError_t launch_strongest(const PyrDesc& pd, const PyrDesc* d_pd, const SiftConsts& sc, int keep, const StrongBatch& sb, int nb,
                            hipStream_t s)
{
    if (pd.n_oct <= 0) return hipSuccess;
    StrongArgs a{};
    a.n_oct = pd.n_oct;
    a.max_extrema = sc.max_extrema;
    a.keep = keep;
    a.chunks = strongest_chunks(sc.max_extrema);
    a.levels = pd.levels;
    const dim3 per_rec(pd.n_oct * a.chunks, nb);
    if (pd.dog_fly)
        hipLaunchKernelGGL(k_strongest_response<true>, per_rec, dim3(256), 0, s, d_pd, a, sb);
    else
        hipLaunchKernelGGL(k_strongest_response<false>, per_rec, dim3(256), 0, s, d_pd, a, sb);
    hipLaunchKernelGGL(k_strongest_select, dim3(1, nb), dim3(SELECT_LANES), 0, s, a, sb);
    hipLaunchKernelGGL(k_strongest_compact, per_rec, dim3(256), 0, s, a, sb);
    return hipGetLastError();
}

}  // namespace popsift_hip
