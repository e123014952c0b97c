/*
 * desc_modes.hip -- the descriptors of the reference's other DescModes, kept for parity with it (the loop descriptor,
 * k_descriptor, is the one that is tuned and benchmarked: keypoint.hip).  One wave per (extremum, orientation); every
 * step the three bodies share is written once: the per-descriptor frame, the rotated interpolated gradient, the
 * angle-to-bin split, normalise-and-store.
 *
 * Replaces:
 *   ext_desc_grid         s_desc_grid.cu:19-147     -> k_descriptor_grid
 *   ext_desc_notile/igrid s_desc_notile.cu:28-166, s_desc_igrid.cu:20-109 -> k_descriptor_notile<false>
 *   ext_desc_iloop        s_desc_iloop.cu:18-154    -> k_descriptor_notile<true>
 *   normalize_histogram   s_desc_normalize.h:14-33, s_desc_norm_rs.h, s_desc_norm_l2.h
 *                                                   -> normalize_store
 */
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "keypoint_dev.h"
#include "sift_types.h"

namespace popsift_hip {
namespace {

/* Everything about descriptor d that does not depend on the lane: the extremum it belongs to (ext + map[d]), its plane
 * and that plane's geometry, the orientation and its rotation (rot[d], worked out in double by k_scan_apply). */
struct DescFrame {
    float        x, y, sigma, SBP;
    float        cos_t, sin_t, ang;
    int          width, height, pitch;
    const float* layer;
};
__device__ __forceinline__ DescFrame desc_frame(const PyrDesc* __restrict__ pdp, const Slot& s, int d)
{
    DescFrame      f;
    const Ext*     e = s.ext + s.map[d];
    const OctDesc* od = &pdp->o[e->octave];
    f.x = uniformf(e->xpos);
    f.y = uniformf(e->ypos);
    f.sigma = uniformf(e->sigma);
    f.ang = e->orientation[min(max(d - e->idx_ori, 0), POPSIFT_HIP_ORI_MAX - 1)];
    f.width = uniform(od->w);
    f.height = uniform(od->h);
    f.pitch = uniform(od->pitch);
    f.layer = s.arena + uniform64(od->data_off + min(max(e->lpos, 0), pdp->L - 1) * od->plane_stride);
    f.SBP = fabsf(DESC_MAGNIFY * f.sigma);
    f.cos_t = uniformf(s.rot[d].x);
    f.sin_t = uniformf(s.rot[d].y);
    return f;
}

/* linear-filter read at pixel-centre coordinates, clamp addressing, 1.8 fixed-point weights
 * (what tex2DLayered on the reference's linear texture returns, common/assist.h:66-81) */
__device__ __forceinline__ float tex_linear(const float* pl, int w, int h, int pitch, float x, float y)
{
    const float fx = floorf(x), fy = floorf(y);
    float       a = x - fx, b = y - fy;
    a = floorf(a * 256.0f + 0.5f) * (1.0f / 256.0f);
    b = floorf(b * 256.0f + 0.5f) * (1.0f / 256.0f);
    const int    i = (int)fx, j = (int)fy;
    const int    x0 = min(max(i, 0), w - 1), x1 = min(max(i + 1, 0), w - 1);
    const int    r0 = __mul24(min(max(j, 0), h - 1), pitch);
    const int    r1 = __mul24(min(max(j + 1, 0), h - 1), pitch);
    const float  top = (1.0f - a) * plane_at(pl, r0 + x0) + a * plane_at(pl, r0 + x1);
    const float  bot = (1.0f - a) * plane_at(pl, r1 + x0) + a * plane_at(pl, r1 + x1);
    return (1.0f - b) * top + b * bot;
}

/* The gradient at (px, py) along the keypoint's rotated axes from four bilinearly interpolated reads one pixel away
 * (s_gradiant.h:71-87): its magnitude and its angle in [-pi, pi], relative to the keypoint orientation. */
__device__ __forceinline__ void rot_gradient(const DescFrame& f, float px, float py, float& mod, float& th)
{
    const float dxv = tex_linear(f.layer, f.width, f.height, f.pitch, px + f.cos_t, py + f.sin_t) -
                      tex_linear(f.layer, f.width, f.height, f.pitch, px - f.cos_t, py - f.sin_t);
    const float dyv = tex_linear(f.layer, f.width, f.height, f.pitch, px - f.sin_t, py + f.cos_t) -
                      tex_linear(f.layer, f.width, f.height, f.pitch, px + f.sin_t, py - f.cos_t);
    mod = __builtin_amdgcn_sqrtf(dxv * dxv + dyv * dyv);
    th = atan2_acc(dyv, dxv);
}

/* Angle th (radians, in (-2 pi, 2 pi)) -> the lower of the two orientation bins it lies between (pi / 4 each) and the
 * fraction of the way to the upper one: wrap into [0, 2 pi), x 4 / pi, floor, fraction, & 7.
 * Grid and ILoop wrap both ways in the reference, NoTile only below zero (s_desc_notile.cu:96-97).  The upper wrap is
 * bit-identical for NoTile: its th comes from atan2_acc, in [-pi, pi], so after the lower wrap the only value the
 * upper one can catch is th == F_PI2, which a tiny negative angle rounds up to.  In float32 F_PI2 * (4.0f / F_PI) is
 * exactly 8.0f: without the wrap that is floor 8, fraction 0 and bin 8 & 7 = 0; with it th = 0, floor 0, fraction 0,
 * bin 0 -- the same bin and the same fraction. */
__device__ __forceinline__ void bin_split(float th, int& b0, float& do0)
{
    th += (th < 0.0f ? F_PI2 : 0.0f);
    th -= (th >= F_PI2 ? F_PI2 : 0.0f);
    const float tth = th * (4.0f / F_PI);
    const float ffo = floorf(tth);
    do0 = tth - ffo;
    b0 = (int)ffo & 7;
}

/* Normalisation (s_desc_norm_rs.h:44-79, s_desc_norm_l2.h:87-134) of the 128 bins a wave holds as (v0, v1) = elements
 * (lane, lane + 64), and the store as two coalesced 256 B rows.  sqrtf and "/" as the library rounds them; k_descriptor
 * (keypoint.hip) has the one other version, on the hardware reciprocal and roots. */
__device__ __forceinline__ void normalize_store(float v0, float v1, const SiftConsts& sc, float* __restrict__ desc, int d,
                                                int lane)
{
    if (sc.norm_mode == POPSIFT_HIP_NORM_ROOTSIFT) {
        float sum = v0 + v1;
        sum = wave_allsum(sum);
        v0 = scalbnf(sqrtf(v0 / sum), sc.norm_multi);
        v1 = scalbnf(sqrtf(v1 / sum), sc.norm_multi);
    } else {
        float sq = v0 * v0 + v1 * v1;
        sq = wave_allsum(sq);
        const float norm = sqrtf(sq);
        v0 = fminf(v0, 0.2f * norm);
        v1 = fminf(v1, 0.2f * norm);
        sq = v0 * v0 + v1 * v1;
        sq = wave_allsum(sq);
        float rn = 1.0f / sqrtf(sq);
        rn = scalbnf(rn, sc.norm_multi);
        v0 = v0 * rn;
        v1 = v1 * rn;
    }
    desc[(size_t)d * 128 + lane] = v0;
    desc[(size_t)d * 128 + 64 + lane] = v1;
}

/* --------------------------------------------------------- descriptor: grid */

/*
 * DescMode Grid (s_desc_grid.cu:19-147): every cell samples a FIXED 16 x 16 grid of points of its
 * own rotated unit square, each snapped to the nearest pixel, and bins only into its own 8
 * orientation bins.  The reference runs a (16,4,4) block per descriptor: 16 lanes per cell, each
 * looping over 16 rows.  Here one wave owns a descriptor and visits the cells one after the other
 * with all 64 lanes (4 grid rows x 16 columns per step); bins are accumulated in registers with
 * predicated adds and summed over the wave by a butterfly -- no atomics, fixed summation order.
 * The position arithmetic follows the reference operation by operation (the float -> int
 * truncation of "pt + (round(pt + pix) - pt)" included), so the sampled pixels are the oracle's.
 */
__global__ __launch_bounds__(256) void k_descriptor_grid(const PyrDesc* __restrict__ pdp, BatchDesc bd, SiftConsts sc,
                                                         int desc_cap)
{
    __shared__ float s_feat[4][128];
    const int        lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float*           feat = s_feat[wave];
    const int        total = min(bd.s[blockIdx.y].ct->ori_total, desc_cap);
    const int        xd = lane & 15, ysub = lane >> 4;

    for (XcdSlice sl = xcd_slice<4>(); sl.more(total); sl.s += sl.step) {
        const int d = sl.index();
        if (d >= total) continue;
        const DescFrame f = desc_frame(pdp, bd.s[blockIdx.y], d);
        const float     SBP = f.SBP, cos_t = f.cos_t, sin_t = f.sin_t;

        feat[lane] = 0.0f;
        feat[lane + 64] = 0.0f;
        if (SBP != 0.0f) {
            const float csbp = cos_t * SBP, ssbp = sin_t * SBP;
            const float ldx = -cos_t + sin_t, ldy = -cos_t - sin_t; /* lft_dn  */
            const float rsx = cos_t / 8.0f, rsy = sin_t / 8.0f;     /* rgt_stp */
            const float usx = -sin_t / 8.0f, usy = cos_t / 8.0f;    /* up__stp */
            for (int cell = 0; cell < 16; cell++) {
                const int   ix = cell & 3, iy = cell >> 2;
                const float offx = ix - 1.5f, offy = iy - 1.5f;
                const float ptx = fmaf(csbp, offx, fmaf(-ssbp, offy, f.x));
                const float pty = fmaf(csbp, offy, fmaf(ssbp, offx, f.y));
                float       acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int step = 0; step < 4; step++) {
                    const int yd = step * 4 + ysub;
                    float     pixox = ldx + (xd + 0.5f) * rsx + (yd + 0.5f) * usx;
                    float     pixoy = ldy + (xd + 0.5f) * rsy + (yd + 0.5f) * usy;
                    float     pixx = pixox * SBP, pixy = pixoy * SBP;
                    pixx = roundf(ptx + pixx) - ptx;
                    pixy = roundf(pty + pixy) - pty;
                    pixox = pixx / SBP;
                    pixoy = pixy / SBP;
                    const int    gx = (int)(ptx + pixx), gy = (int)(pty + pixy);
                    /* point texture, clamp addressing */
                    const int    xc = min(max(gx, 0), f.width - 1), yc = min(max(gy, 0), f.height - 1);
                    const int    xl = min(max(gx - 1, 0), f.width - 1), xr = min(max(gx + 1, 0), f.width - 1);
                    const int    yu = min(max(gy - 1, 0), f.height - 1), yl = min(max(gy + 1, 0), f.height - 1);
                    const int    rowc = __mul24(yc, f.pitch);
                    const float  dxv = plane_at(f.layer, rowc + xr) - plane_at(f.layer, rowc + xl);
                    const float  dyv = plane_at(f.layer, __mul24(yl, f.pitch) + xc) - plane_at(f.layer, __mul24(yu, f.pitch) + xc);
                    const float  mod = __builtin_amdgcn_sqrtf(dxv * dxv + dyv * dyv);
                    const float  th = atan2_acc(dyv, dxv);
                    const float  npx = fmaf(cos_t, pixox, sin_t * pixoy);
                    const float  npy = fmaf(cos_t, pixoy, -sin_t * pixox);
                    const float  dnx = npx + offx, dny = npy + offy;
                    const float  ww = __expf(-0.125f * (dnx * dnx + dny * dny));
                    const float  wx_ = 1.0f - fabsf(npx), wy_ = 1.0f - fabsf(npy);
                    const float  wgt = (wx_ < 0.0f || wy_ < 0.0f) ? 0.0f : ww * wx_ * wy_ * mod;
                    int          b0;
                    float        do0;
                    bin_split(th - f.ang, b0, do0);
                    const int    b1 = (b0 + 1) & 7;
                    const float  w1 = do0 * wgt, w0 = wgt - w1;
#pragma unroll
                    for (int b = 0; b < 8; b++) acc[b] += (b == b0 ? w0 : 0.0f) + (b == b1 ? w1 : 0.0f);
                }
#pragma unroll
                for (int b = 0; b < 8; b++) {
                    const float v = wave_allsum(acc[b]);
                    if (lane == 0) feat[(cell << 3) + b] = v;
                }
            }
        }
        wave_lds_sync();

        normalize_store(feat[lane], feat[lane + 64], sc, bd.s[blockIdx.y].desc, d, lane);
        wave_lds_sync();
    }
}

/* ------------------------------------------------ descriptor: notile, iloop */

/*
 * DescMode NoTile (s_desc_notile.cu:28-128): a 40 x 40 grid of sample points at 1/8-cell pitch in
 * the keypoint's rotated frame; at each point the gradient is taken along the rotated axes from
 * four bilinearly interpolated reads (rot_gradient), weighted by a Gaussian table
 * (desc_gauss, sift_constants.cu:33-41) and by tent weights over the 16 x 16 points of every cell
 * that covers it (desc_tile, :43-46).  The reference evaluates each point once per covering
 * cell (up to four times); here one wave owns the descriptor, evaluates each of the 1600 points
 * once and spreads it to its <= 2 x 2 cells with the packed fixed-point LDS atomics of the loop
 * kernel: a word holds two 32-bit sums, low = the share of bin b, high = the share of bin b + 1 from the samples whose
 * lower bin is b.
 */
template <bool ILOOP>
__global__ __launch_bounds__(256) void k_descriptor_notile(const PyrDesc* __restrict__ pdp, BatchDesc bd, SiftConsts sc,
                                                           int desc_cap)
{
    constexpr int    DCOPY = 2;
    /* notile: 256 points per cell, iloop: up to 1024, each <= 361 * 1: low halves stay below 2^32 */
    constexpr int    FBITS = ILOOP ? 13 : 14;
    __shared__ fix64 s_hist[4][DCOPY][128];
    const int        lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    fix64*           hist = s_hist[wave][lane & (DCOPY - 1)];
    fix64*           hall = s_hist[wave][0];
    const int        total = min(bd.s[blockIdx.y].ct->ori_total, desc_cap);
    const float      stepbase = -2.5f + 1.0f / 16.0f;
    const float      fscale = (float)(1 << FBITS);

    for (XcdSlice sl = xcd_slice<4>(); sl.more(total); sl.s += sl.step) {
        const int d = sl.index();
        if (d >= total) continue;
        const DescFrame f = desc_frame(pdp, bd.s[blockIdx.y], d);
        const float     SBP = f.SBP, cos_t = f.cos_t, sin_t = f.sin_t;

#pragma unroll
        for (int k = 0; k < 2 * DCOPY; k++) hall[lane + 64 * k] = 0ull;
        wave_lds_sync();

        if (f.sigma != 0.0f) {
            if (ILOOP) {
                /* DescMode ILoop (s_desc_iloop.cu:18-133): every cell samples a FIXED 32 x 32 lattice over the
                 * bounding box of its rotated two-cell square and keeps the points inside the square; the
                 * gradient is the interpolated, rotated one of notile, the weights are the loop descriptor's.
                 * The reference gives a cell 32 lanes x 32 steps; a wave here takes two lattice rows a step. */
                const float csbp = cos_t * SBP, ssbp = sin_t * SBP;
                const float bsz = fabsf(cos_t) + fabsf(sin_t);
                const int   j = lane & 31;
                for (int cell = 0; cell < 16; cell++) {
                    const float offx = (float)(cell & 3) - 1.5f, offy = (float)(cell >> 2) - 1.5f;
                    const float ptx = fmaf(csbp, offx, -ssbp * offy);
                    const float pty = fmaf(csbp, offy, ssbp * offx);
                    for (int it = 0; it < 16; it++) {
                        const int   i = 2 * it + (lane >> 5);
                        const float dx = -bsz + (float)j * bsz / 16.0f;
                        const float dy = -bsz + (float)i * bsz / 16.0f;
                        const float nx = fmaf(cos_t, dx, sin_t * dy);
                        const float ny = fmaf(cos_t, dy, -sin_t * dx);
                        const float nnx = fabsf(nx), nny = fabsf(ny);
                        if (nnx < 1.0f && nny < 1.0f) {
                            float mod, th, do0;
                            int   b0;
                            rot_gradient(f, f.x + ptx + dx * SBP, f.y + pty + dy * SBP, mod, th);
                            bin_split(th, b0, do0);
                            const float dnx = nx + offx, dny = ny + offy;
                            const float ww = __expf(-0.125f * (dnx * dnx + dny * dny));
                            const float wgt = ww * (1.0f - nnx) * (1.0f - nny) * mod * fscale;
                            const float a1 = do0 * wgt, a0 = wgt - a1;
                            atomicAdd(&hist[(cell << 3) + b0],
                                      ((fix64)(unsigned int)(a1 + 0.5f) << 32) | (unsigned int)(a0 + 0.5f));
                        }
                    }
                }
            } else
            for (int p = lane; p < 1600; p += 64) {
                const int   newy = p / 40, newx = p - newy * 40;
                const float stepx = stepbase + 0.125f * (float)newx;
                const float stepy = stepbase + 0.125f * (float)newy;
                const float ptx = cos_t * stepx + -sin_t * stepy;
                const float pty = cos_t * stepy + sin_t * stepx;
                float       mod, th, do0;
                int         b0;
                rot_gradient(f, f.x + ptx * SBP, f.y + pty * SBP, mod, th);
                bin_split(th, b0, do0);
                /* desc_gauss[newy][newx]: exp(-(dnx^2 + dny^2) / 8), dn = step position */
                const float ww = __expf(-0.125f * (stepx * stepx + stepy * stepy)) * mod * fscale;
                const float a1 = do0 * ww, a0 = ww - a1;
                /* cells cx with 8cx <= newx <= 8cx+15, tent weight desc_tile[newx - 8cx] */
#pragma unroll
                for (int jy = 0; jy < 2; jy++) {
                    const int cy = (newy >> 3) - jy;
                    if (cy < 0 || cy > 3) continue;
                    const float wy = 1.0f - fabsf(-1.0f + 1.0f / 16.0f + 0.125f * (float)(newy - 8 * cy));
#pragma unroll
                    for (int jx = 0; jx < 2; jx++) {
                        const int cx = (newx >> 3) - jx;
                        if (cx < 0 || cx > 3) continue;
                        const float wx = 1.0f - fabsf(-1.0f + 1.0f / 16.0f + 0.125f * (float)(newx - 8 * cx));
                        const float wgt = wx * wy;
                        const unsigned int lo = (unsigned int)fmaf(a0, wgt, 0.5f);
                        const unsigned int hi = (unsigned int)fmaf(a1, wgt, 0.5f);
                        atomicAdd(&hist[((((cy << 2) + cx) << 3)) + b0], ((fix64)hi << 32) | lo);
                    }
                }
            }
        }
        wave_lds_sync();

        /* bin b of a cell = low half of word b + high half of word b-1 (mod 8), over the copies */
        fix64     a0 = 0ull, a1 = 0ull;
        const int prevw = (lane & ~7) | ((lane + 7) & 7);
#pragma unroll
        for (int k = 0; k < DCOPY; k++) {
            a0 += (hall[k * 128 + lane] & 0xffffffffull) + (hall[k * 128 + prevw] >> 32);
            a1 += (hall[k * 128 + lane + 64] & 0xffffffffull) + (hall[k * 128 + prevw + 64] >> 32);
        }
        normalize_store((float)a0 * (1.0f / (float)(1 << FBITS)), (float)a1 * (1.0f / (float)(1 << FBITS)), sc,
                        bd.s[blockIdx.y].desc, d, lane);
        wave_lds_sync();
    }
}

}  // namespace

hipError_t launch_desc_modes(const PyrDesc* pd, const BatchDesc& bd, int nb, const SiftConsts& sc, int desc_cap, int blocks,
                             hipStream_t s)
{
    /* IGrid (s_desc_igrid.cu:20-83) evaluates the same 40 x 40 point lattice with the same weights as NoTile,
     * cell by cell (each point up to four times); the two differ only in summation order (6e-7 relative in the
     * oracle), so both run the one-evaluation-per-point kernel */
    if (sc.desc_mode == POPSIFT_HIP_DESC_NOTILE || sc.desc_mode == POPSIFT_HIP_DESC_IGRID)
        hipLaunchKernelGGL(k_descriptor_notile<false>, dim3(blocks / 4, nb), dim3(256), 0, s, pd, bd, sc, desc_cap);
    else if (sc.desc_mode == POPSIFT_HIP_DESC_ILOOP)
        hipLaunchKernelGGL(k_descriptor_notile<true>, dim3(blocks / 4, nb), dim3(256), 0, s, pd, bd, sc, desc_cap);
    else
        hipLaunchKernelGGL(k_descriptor_grid, dim3(blocks / 4, nb), dim3(256), 0, s, pd, bd, sc, desc_cap);
    return hipGetLastError();
}

}  // namespace popsift_hip
