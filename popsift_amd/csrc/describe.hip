/*
 * describe.hip -- caller-supplied keypoints (popsift_hip_describe_batch): the frames take the place of detection and
 * refinement, the orientation / scan / descriptor kernels of keypoint.hip run on them unchanged.
 *
 *   k_frame_count  resolves every frame to (octave, level) and counts the valid ones per (octave, chunk of FRAME_CHUNK)
 *   k_frame_place  stable partition by octave: the InitExt lists in caller order within an octave, ext_ct, the list
 *                  position <-> frame maps; with given orientations also the Ext records and k_orientation's partial sums,
 *                  so that k_scan_apply alone finishes the scan
 *   k_frame_out    after the descriptor kernel: k_scan_apply's feature records moved to caller order (invalid frames get
 *                  their own record), the descriptor -> feature map rewritten to caller indices
 *
 * The rank of a frame among its wave's frames of the same octave and the wave sums come from wave_dev.h.
 * No atomics decide a position: the lists, the descriptor order and every output byte are the same from run to run.
 * The counterpart of vl_sift(I, 'frames', F[, 'orientations']) and of OpenCV's SIFT::compute; the reference has none.
 */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "sift_types.h"
#include "wave_dev.h"

namespace popsift_hip {
namespace {

/* The frame in octave units and the octave it goes to; -1: invalid (the rules of include/popsift_hip.h).  One function
 * for both launches, so that the count and the placement agree. */
__device__ __forceinline__ int resolve(const popsift_hip_frame& f, const PyrDesc* __restrict__ pdp, const SiftConsts& sc,
                                       int given, InitExt& ie)
{
    const int n_oct = pdp->n_oct, L = pdp->L, levels = pdp->levels;
    if (!isfinite(f.xpos) || !isfinite(f.ypos) || !isfinite(f.sigma) || !(f.sigma > 0.0f)) return -1;
    if (given && !isfinite(f.orientation)) return -1;
    if (f.octave < -1 || f.octave >= n_oct || f.level < -1 || f.level >= L) return -1;
    int o = f.octave;
    if (o < 0) {
        /* refinement's sigma = sigma0 * 2^(sn / levels) in octave o is sigma0 * 2^(o - up + sn / levels) in the input
         * image; sn in [0.5, levels + 0.5) is the band extraction produces */
        const float t = log2f(f.sigma / sc.sigma0) + (float)sc.up_fac_int;
        o = (int)fminf(fmaxf(floorf(t - 0.5f / (float)levels), 0.0f), (float)(n_oct - 1));
    }
    const int      sh = sc.up_fac_int - o;
    const float    x = ldexpf(f.xpos, sh), y = ldexpf(f.ypos, sh), s = ldexpf(f.sigma, sh);
    const OctDesc& od = pdp->o[o];
    /* the oracle's acceptance rules (oracle_keypoint_stages_from) */
    if (!(x >= 0.0f && x <= (float)(od.w - 1) && y >= 0.0f && y <= (float)(od.h - 1))) return -1;
    if (!(s > 0.0f && s <= POPSIFT_HIP_FRAME_SIGMA_MAX)) return -1;
    int l = f.level;
    if (l < 0) l = (int)fminf(fmaxf(roundf((float)levels * log2f(s / sc.sigma0)), 0.0f), (float)(L - 1)); /* roundf(sn) */
    ie.xpos = x;
    ie.ypos = y;
    ie.lpos = l;
    ie.sigma = s;
    ie.cell = 0;
    return o;
}

constexpr int FW = FRAME_CHUNK / 64; /* waves per workgroup */

__global__ __launch_bounds__(FRAME_CHUNK) void k_frame_count(const PyrDesc* __restrict__ pdp, FrameBatch fb, SiftConsts sc, int given)
{
    const popsift_hip_frame* __restrict__ frames = fb.s[blockIdx.y].frames;
    int* __restrict__                     counts = fb.s[blockIdx.y].counts;
    const int                             n = fb.s[blockIdx.y].n;
    const int                             chunk = blockIdx.x;
    if (chunk * FRAME_CHUNK >= n) return; /* the launch is sized for the image of the batch with the most frames */
    __shared__ int s_ct[PS_MAX_OCT];
    if (threadIdx.x < PS_MAX_OCT) s_ct[threadIdx.x] = 0;
    __syncthreads();
    const int i = chunk * FRAME_CHUNK + threadIdx.x;
    if (i < n) {
        InitExt   ie;
        const int o = resolve(frames[i], pdp, sc, given, ie);
        if (o >= 0) atomicAdd(&s_ct[o], 1); /* a count: the order of the adds does not matter */
    }
    __syncthreads();
    const int nc = (n + FRAME_CHUNK - 1) / FRAME_CHUNK;
    if ((int)threadIdx.x < pdp->n_oct) counts[threadIdx.x * nc + chunk] = s_ct[threadIdx.x];
}

/*
 * Position of a valid frame in its octave's list = valid frames of that octave in the preceding chunks (summed here,
 * redundantly per workgroup, as k_scan_apply sums its partials) + in the preceding waves of this chunk + in the preceding
 * lanes of this wave (ballot per distinct octave of the wave).  List position g = start of the octave + that.
 */
__global__ __launch_bounds__(FRAME_CHUNK) void k_frame_place(const PyrDesc* __restrict__ pdp, BatchDesc bd, FrameBatch fb,
                                                            SiftConsts sc, int given, int lchunk)
{
    const popsift_hip_frame* __restrict__ frames = fb.s[blockIdx.y].frames;
    const int* __restrict__               counts = fb.s[blockIdx.y].counts;
    int* __restrict__                     perm = fb.s[blockIdx.y].perm;
    int* __restrict__                     inv = fb.s[blockIdx.y].inv;
    const int                             n = fb.s[blockIdx.y].n;
    Counters* __restrict__                ct = bd.s[blockIdx.y].ct;
    InitExt* __restrict__                 iext = bd.s[blockIdx.y].iext;
    Ext* __restrict__                     ext = bd.s[blockIdx.y].ext;
    int* __restrict__                     partial = bd.s[blockIdx.y].partial;
    const int                             chunk = blockIdx.x;
    /* workgroup 0 writes the counts also when there is no frame at all */
    if (chunk > 0 && chunk * FRAME_CHUNK >= n) return;
    const int      n_oct = pdp->n_oct;
    const int      nc = (n + FRAME_CHUNK - 1) / FRAME_CHUNK;
    const int      lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ int s_before[PS_MAX_OCT], s_total[PS_MAX_OCT], s_ps[PS_MAX_OCT + 1];
    __shared__ int s_wc[FW][PS_MAX_OCT];
    for (int o = wave; o < n_oct; o += FW) {
        int before = 0, total = 0;
        for (int c = lane; c < nc; c += 64) {
            const int v = counts[o * nc + c];
            total += v;
            before += c < chunk ? v : 0;
        }
        before = wave_sum(before);
        total = wave_sum(total);
        if (lane == 0) {
            s_before[o] = before;
            s_total[o] = total;
        }
    }
    for (int k = threadIdx.x; k < FW * PS_MAX_OCT; k += FRAME_CHUNK) (&s_wc[0][0])[k] = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int o = 0; o < n_oct; o++) {
            s_ps[o] = acc;
            acc += s_total[o];
        }
        s_ps[n_oct] = acc;
    }
    const int i = chunk * FRAME_CHUNK + threadIdx.x;
    InitExt   ie;
    const int o = i < n ? resolve(frames[i], pdp, sc, given, ie) : -1;
    int       rank = 0;
    wave_each_key(o, o >= 0, [&](int oo, unsigned long long m, int first) {
        if (o == oo) rank = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == first) s_wc[wave][oo] = __popcll(m);
    });
    __syncthreads();
    if (chunk == 0 && (int)threadIdx.x < PS_MAX_OCT) ct->ext_ct[threadIdx.x] = (int)threadIdx.x < n_oct ? s_total[threadIdx.x] : 0;
    if (o >= 0) {
        int r = s_before[o] + rank;
        for (int w = 0; w < wave; w++) r += s_wc[w][o];
        ie.cell = i;
        iext[(size_t)o * sc.max_extrema + r] = ie;
        const int g = s_ps[o] + r;
        perm[g] = i;
        inv[i] = g;
        if (given) {
            /* what k_orientation would leave for an extremum with this one orientation: idx_ori local to its group of
             * lchunk list entries, one partial sum per such chunk (every entry has one descriptor) */
            Ext e;
            e.xpos = ie.xpos;
            e.ypos = ie.ypos;
            e.lpos = ie.lpos;
            e.sigma = ie.sigma;
            e.octave = o;
            e.num_ori = 1;
            e.idx_ori = g % lchunk;
            e.orientation[0] = frames[i].orientation;
            for (int q = 1; q < POPSIFT_HIP_ORI_MAX; q++) e.orientation[q] = 0.0f;
            ext[g] = e;
            if (g % lchunk == 0) partial[g / lchunk] = min(lchunk, s_ps[n_oct] - g);
        }
    } else if (i < n) {
        inv[i] = -1;
    }
}

__global__ __launch_bounds__(256) void k_frame_out(BatchDesc bd, FrameBatch fb, int desc_cap)
{
    const popsift_hip_frame* __restrict__   frames = fb.s[blockIdx.y].frames;
    const int* __restrict__                 perm = fb.s[blockIdx.y].perm;
    const int* __restrict__                 inv = fb.s[blockIdx.y].inv;
    const popsift_hip_feature* __restrict__ lfeats = fb.s[blockIdx.y].lfeats;
    const int                               n = fb.s[blockIdx.y].n;
    popsift_hip_feature* __restrict__       feats = bd.s[blockIdx.y].feats;
    int* __restrict__                       map = bd.s[blockIdx.y].map;
    const int                               nd = min(bd.s[blockIdx.y].ct->ori_total, desc_cap);
    const int                               end = max(n, nd);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < end; i += gridDim.x * 256) {
        if (i < n) {
            const int           g = inv[i];
            popsift_hip_feature f;
            if (g >= 0) {
                f = lfeats[g];
            } else {
                const popsift_hip_frame fr = frames[i];
                f.debug_octave = -1;
                f.xpos = fr.xpos;
                f.ypos = fr.ypos;
                f.sigma = fr.sigma;
                f.num_ori = 0;
                for (int q = 0; q < POPSIFT_HIP_ORI_MAX; q++) {
                    f.orientation[q] = 0.0f;
                    f.desc_idx[q] = -1;
                }
            }
            feats[i] = f;
        }
        if (i < nd) map[i] = perm[map[i]];
    }
}

}  // namespace

int frame_chunks(int n_max) { return (std::max(n_max, 0) + FRAME_CHUNK - 1) / FRAME_CHUNK; }

hipError_t launch_frame_count(const PyrDesc* d_pd, const FrameBatch& fb, int nb, const SiftConsts& sc, int given, int n_max,
                              hipStream_t s)
{
    if (n_max > 0) hipLaunchKernelGGL(k_frame_count, dim3(frame_chunks(n_max), nb), dim3(FRAME_CHUNK), 0, s, d_pd, fb, sc, given);
    return hipGetLastError();
}

hipError_t launch_frame_place(const PyrDesc* d_pd, const BatchDesc& bd, const FrameBatch& fb, int nb, const SiftConsts& sc,
                              int given, int n_max, hipStream_t s)
{
    hipLaunchKernelGGL(k_frame_place, dim3(std::max(frame_chunks(n_max), 1), nb), dim3(FRAME_CHUNK), 0, s, d_pd, bd, fb, sc,
                       given, scan_chunk() / scan_partials_per_chunk());
    return hipGetLastError();
}

hipError_t launch_frame_out(const BatchDesc& bd, const FrameBatch& fb, int nb, int desc_cap, int n_max, hipStream_t s)
{
    /* up to four descriptors per frame */
    const int blocks = std::min(std::max((4 * n_max + 255) / 256, 1), 1024);
    hipLaunchKernelGGL(k_frame_out, dim3(blocks, nb), dim3(256), 0, s, bd, fb, desc_cap);
    return hipGetLastError();
}

}  // namespace popsift_hip
