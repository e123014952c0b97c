/*
 * pyr_direct.hip -- octave 0 of the 'vlfeat-direct' Gauss mode (Config::VLFeat_Relative_All) for gfx950.
 *
 * In this mode every octave-0 level l is a fresh blur of the upscaled input image with the abs_o0[l] taps
 * (Pyramid::build_pyramid, s_pyramid_build.cu:545-548):
 *   horizontal pass  gauss::normalizedSource::horiz_all  (s_pyramid_build_ra.cu:94-130)
 *   vertical pass    gauss::absoluteSource::vert_all_abs0 (s_pyramid_build_aa.cu:134-176)
 * The default mode needs L dependent launches for octave 0, each reading the plane the one before wrote.  Here ONE
 * launch reads the input once per tile and writes all L planes:
 *   phase 1  the bilinearly upscaled tile U plus the largest halo of the L levels is staged in LDS, once;
 *   per level l:
 *   phase 2  horizontal pass from U (it is not overwritten) into a second LDS buffer T of TW columns;
 *   phase 3  vertical pass from T, 4 columns x 4 rows per lane from a register window of ds_read_b128 rows; the lane
 *            keeps its block of level l-1 in registers, so the DoG plane l-1 = G(l) - G(l-1) costs no reads.
 * Octave 1's level 0 (every second pixel of level L-3) and the clearing of the image's Counters ride along, as they
 * do with the default mode's launches.
 *
 * Arithmetic is that of the level-0 kernel (pyramid.hip, MODE 1/2) in the reference's order with explicit fmaf and
 * -ffp-contract=off: the planes are bit-identical to the CPU restatement (tests/gauss_direct_ref.c).  A level with a
 * shorter filter than its instance runs with zero-padded taps, fmaf(v, 0, out) == out for finite v.
 *
 * The taps of all levels (L x 32 floats, up to 1.5 KiB) live in a device buffer of the context, not in the kernel
 * arguments (which already carry the 2 KiB slot table): the addresses are uniform, so they come through the scalar
 * cache with s_load.
 */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sift_types.h"
#include "kernels.h"
#include "blur_common.h"

namespace popsift_hip {

namespace {

constexpr int TW = BLUR_TW; /* tile width (outputs) */
constexpr int TH = 64;      /* tile height: a taller tile amortises the halo rows of the H pass (1.3x at 20 taps, not 1.6x) */
constexpr int NT = 512;     /* one 4x4 output block per lane */

template <int HALO>
struct Geo {
    static constexpr int HP = (HALO + 3) & ~3; /* left/right halo of U, padded to 16 B */
    static constexpr int SW = TW + 2 * HP;     /* U row pitch                          */
    static constexpr int SR = TH + 2 * HALO;   /* rows of U and T                      */
    static constexpr int U_FLOATS = SR * SW;
    static constexpr int T_FLOATS = SR * TW;
};

/*
 * One level from the staged tile: H pass U -> T for the rows the level needs, V pass T -> planes.
 * HALO: the staging geometry (largest halo of the launch), HL: this level's halo class (<= HALO).
 */
template <int HALO, int HL>
__device__ __forceinline__ void direct_level(const DirectArgs& a, int l, int tx0, int ty0, const float* __restrict__ s_u,
                                             float* __restrict__ s_t, float* const arena, v4f (&prev)[4])
{
    using G = Geo<HALO>;
    constexpr int HPL = (HL + 3) & ~3; /* window halo, 16 B aligned          */
    constexpr int NW = 1 + HPL / 2;    /* H-pass window in 16 B chunks       */
    constexpr int VW = 4 + 2 * HL;     /* V-pass window rows                 */
    /* the constant address space: uniform loads of it are s_load, so the taps sit in SGPRs, not in VGPRs */
    const __attribute__((address_space(4))) float* g = (const __attribute__((address_space(4))) float*)(a.taps + l * PS_GA);
    const int tid = threadIdx.x;
    const int lx = (tid & 31) * 4;

    /* ---- phase 2: horizontal pass (normalizedSource::horiz_all): outermost tap first, centre last, x 255 ---- */
    for (int r = HALO - HL + (tid >> 5); r < HALO + TH + HL; r += NT / 32) {
        v4f        win[NW];
        const v4f* p = reinterpret_cast<const v4f*>(&s_u[r * G::SW + G::HP - HPL + lx]);
#pragma unroll
        for (int j = 0; j < NW; j++) win[j] = p[j];
#define PS_W(i) win[(i) >> 2][(i) & 3]
        v4f out;
#pragma unroll
        for (int o = 0; o < 4; o++) {
            const int cpos = HPL + o;
            float     acc = 0.0f;
#pragma unroll
            for (int k = HL; k > 0; k--) acc = fmaf(PS_W(cpos - k) + PS_W(cpos + k), g[k], acc);
            acc = fmaf(PS_W(cpos), g[0], acc);
            out[o] = acc * 255.0f;
        }
#undef PS_W
        *reinterpret_cast<v4f*>(&s_t[r * TW + lx]) = out;
    }
    __syncthreads();

    /* ---- phase 3: vertical pass (absoluteSource::vert_all_abs0): outermost tap first, upper then lower, centre last ---- */
    {
        const int r0 = (tid >> 5) * 4; /* first output row of this lane's block (tile-relative) */
        const int gx = tx0 + lx;
        float* const dst = arena + a.dst_off + (int64_t)l * a.plane_stride;
        float* const dog = (a.dog_off >= 0 && l > 0) ? arena + a.dog_off + (int64_t)(l - 1) * a.plane_stride : nullptr;
        float* const next0 = (a.next0_off >= 0 && l == a.L - 3) ? arena + a.next0_off : nullptr;
        v4f          res[4];
        if (HL <= 16) {
            v4f win[VW];
#pragma unroll
            for (int j = 0; j < VW; j++) win[j] = *reinterpret_cast<const v4f*>(&s_t[(HALO - HL + r0 + j) * TW + lx]);
#pragma unroll
            for (int oo = 0; oo < 4; oo++) {
                const int cpos = HL + oo;
                /* explicit 2-vectors: every FMA of the chain is a v_pk_fma_f32 */
                v2f alo = {0.0f, 0.0f}, ahi = {0.0f, 0.0f};
#pragma unroll
                for (int k = HL; k > 0; k--) {
                    const v2f gk = {g[k], g[k]};
                    alo = __builtin_elementwise_fma(win[cpos - k].lo, gk, alo);
                    ahi = __builtin_elementwise_fma(win[cpos - k].hi, gk, ahi);
                    alo = __builtin_elementwise_fma(win[cpos + k].lo, gk, alo);
                    ahi = __builtin_elementwise_fma(win[cpos + k].hi, gk, ahi);
                }
                const v2f g0 = {g[0], g[0]};
                alo = __builtin_elementwise_fma(win[cpos].lo, g0, alo);
                ahi = __builtin_elementwise_fma(win[cpos].hi, g0, ahi);
                res[oo] = __builtin_shufflevector(alo, ahi, 0, 1, 2, 3);
            }
        } else {
            /* a window of 4 + 2 HL rows x 4 columns does not fit 256 VGPRs (512 lanes): two halves of 2 columns, the
             * scheduler barrier keeps the second half's window from being loaded while the first one is live */
#pragma unroll
            for (int half = 0; half < 2; half++) {
                v2f win[VW];
#pragma unroll
                for (int j = 0; j < VW; j++) win[j] = *reinterpret_cast<const v2f*>(&s_t[(HALO - HL + r0 + j) * TW + lx + 2 * half]);
#pragma unroll
                for (int oo = 0; oo < 4; oo++) {
                    const int cpos = HL + oo;
                    v2f       acc = {0.0f, 0.0f};
#pragma unroll
                    for (int k = HL; k > 0; k--) {
                        const v2f gk = {g[k], g[k]};
                        acc = __builtin_elementwise_fma(win[cpos - k], gk, acc);
                        acc = __builtin_elementwise_fma(win[cpos + k], gk, acc);
                    }
                    const v2f g0 = {g[0], g[0]};
                    acc = __builtin_elementwise_fma(win[cpos], g0, acc);
                    if (half == 0)
                        res[oo].lo = acc;
                    else
                        res[oo].hi = acc;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int oo = 0; oo < 4; oo++) {
            const v4f acc = res[oo];
            const int gy = ty0 + r0 + oo;
            if (gx < a.w && gy < a.h) {
                /* rows are padded to 64 floats, so a 16 B store at gx < w stays inside the row */
                *reinterpret_cast<v4f*>(&dst[(size_t)gy * a.pitch + gx]) = acc;
                if (dog) __builtin_nontemporal_store(acc - prev[oo], reinterpret_cast<v4f*>(&dog[(size_t)gy * a.pitch + gx]));
                /* octave 1's level 0 takes pixel (2x, 2y); its width is ceil(w / 2), so 2x <= w - 1 always */
                if (next0 && (gy & 1) == 0) {
                    float* q = next0 + (size_t)(gy >> 1) * a.next_pitch + (gx >> 1);
                    q[0] = acc.x;
                    if (gx + 2 < a.w) q[1] = acc.z;
                }
            }
            prev[oo] = acc;
        }
    }
    __syncthreads(); /* T is rewritten by the next level's H pass */
}

template <int HALO, int MODE>
__global__ __launch_bounds__(NT) void k_pyr_direct(DirectArgs a, BatchDesc bd)
{
    using G = Geo<HALO>;
    static_assert((G::U_FLOATS + G::T_FLOATS) * 4 + (G::SW + G::SR) * 8 + 1024 <= 160 * 1024, "LDS of one workgroup");
    __shared__ __attribute__((aligned(16))) float s_u[G::U_FLOATS];
    __shared__ __attribute__((aligned(16))) float s_t[G::T_FLOATS];
    __shared__ int   s_ix[G::SW];
    __shared__ float s_fa[G::SW];
    __shared__ int   s_iy[G::SR];
    __shared__ float s_fb[G::SR];
    __shared__ float s_lut[256]; /* cudaReadModeNormalizedFloat: v / 255 */

    const int tid = threadIdx.x;
    if (a.zero_words > 0 && blockIdx.x == gridDim.x - 1) {
        int* zero = (int*)bd.s[blockIdx.y].ct;
        for (int i = tid; i < a.zero_words; i += NT) zero[i] = 0;
    }
    float* const      arena = bd.s[blockIdx.y].arena;
    const void* const in = bd.s[blockIdx.y].input;
    const int         tile = xcd_remap(blockIdx.x, a.tiles_x * a.tiles_y);
    const int         tx0 = (tile % a.tiles_x) * TW;
    const int         ty0 = (tile / a.tiles_x) * TH;
    const int         w = a.w, h = a.h;

    /* ---- phase 1: U = the upscaled input over the tile + halo (s_pyramid_build_ra.cu:38-39, read_x = (x + shift) / w) ---- */
    if (MODE == 1) s_lut[tid & 255] = (float)(tid & 255) / 255.0f;
    for (int c = tid; c < G::SW; c += NT) {
        const int X = tx0 + c - G::HP;
        lin_coord(((float)X + a.shift) / (float)w, a.in_w, s_ix[c], s_fa[c]);
    }
    for (int r = tid; r < G::SR; r += NT) {
        const int Y = clampi(ty0 + r - HALO, 0, h - 1);
        lin_coord(((float)Y + a.shift) / (float)h, a.in_h, s_iy[r], s_fb[r]);
    }
    __syncthreads();
    /* the source texels the tile touches (sample coordinates are monotone): staged in T, which is free until the first
     * H pass, when they fit (always for up-scaling); otherwise the bilinear taps read global memory */
    const int  xs0 = clampi(s_ix[0], 0, a.in_w - 1), xs1 = clampi(s_ix[G::SW - 1] + 1, 0, a.in_w - 1);
    const int  ys0 = clampi(s_iy[0], 0, a.in_h - 1), ys1 = clampi(s_iy[G::SR - 1] + 1, 0, a.in_h - 1);
    const int  RW = xs1 - xs0 + 1, RH = ys1 - ys0 + 1;
    const bool staged = RW * RH <= G::T_FLOATS;
    auto texel = [&](int x, int y) -> float { /* x, y clamped */
        if (MODE == 1) return s_lut[((const uint8_t*)in)[(size_t)y * a.in_pitch + x]];
        return ((const float*)in)[(size_t)y * a.in_pitch + x];
    };
    if (staged) {
        constexpr int LD = 4;
        for (int i0 = tid; i0 < RW * RH; i0 += LD * NT) {
            float v[LD];
#pragma unroll
            for (int k = 0; k < LD; k++) {
                const int i = i0 + k * NT;
                if (i < RW * RH) {
                    const int r = i / RW, c = i - r * RW;
                    v[k] = texel(xs0 + c, ys0 + r);
                }
            }
#pragma unroll
            for (int k = 0; k < LD; k++)
                if (i0 + k * NT < RW * RH) s_t[i0 + k * NT] = v[k];
        }
        __syncthreads();
    }
    for (int idx = tid; idx < G::U_FLOATS; idx += NT) {
        const int   r = idx / G::SW, c = idx - r * G::SW;
        const int   ix = s_ix[c], iy = s_iy[r];
        const float fa = s_fa[c], fb = s_fb[r];
        const int   x0 = clampi(ix, 0, a.in_w - 1), x1 = clampi(ix + 1, 0, a.in_w - 1);
        const int   y0 = clampi(iy, 0, a.in_h - 1), y1 = clampi(iy + 1, 0, a.in_h - 1);
        float       t00, t10, t01, t11;
        if (staged) {
            const int j0 = (y0 - ys0) * RW, j1 = (y1 - ys0) * RW;
            t00 = s_t[j0 + x0 - xs0];
            t10 = s_t[j0 + x1 - xs0];
            t01 = s_t[j1 + x0 - xs0];
            t11 = s_t[j1 + x1 - xs0];
        } else {
            t00 = texel(x0, y0);
            t10 = texel(x1, y0);
            t01 = texel(x0, y1);
            t11 = texel(x1, y1);
        }
        const float top = (1.0f - fa) * t00 + fa * t10;
        const float bot = (1.0f - fa) * t01 + fa * t11;
        s_u[idx] = (1.0f - fb) * top + fb * bot;
    }
    __syncthreads();

    /* ---- phases 2 + 3, level by level; each level takes the smallest instantiated halo class that covers it ---- */
    v4f prev[4];
    for (int l = 0; l < a.L; l++) {
        const int hl = a.halo[l];
#define PS_LEVEL(H)                                                                                          \
    if (hl <= (H)) {                                                                                         \
        direct_level<HALO, ((H) < HALO ? (H) : HALO)>(a, l, tx0, ty0, s_u, s_t, arena, prev);                \
        continue;                                                                                            \
    }
        PS_LEVEL(4)
        PS_LEVEL(6)
        PS_LEVEL(8)
        PS_LEVEL(10)
        PS_LEVEL(13)
        PS_LEVEL(16)
        PS_LEVEL(22)
        PS_LEVEL(30)
#undef PS_LEVEL
    }
}

template <int MODE>
hipError_t launch_direct_mode(const DirectArgs& a, const BatchDesc& bd, int nb, int halo, hipStream_t s)
{
    const dim3 grid(a.tiles_x * a.tiles_y, nb), block(NT);
#define PS_CASE(H)                                                                      \
    if (halo <= H) {                                                                    \
        hipLaunchKernelGGL((k_pyr_direct<H, MODE>), grid, block, 0, s, a, bd);          \
        return hipGetLastError();                                                       \
    }
    PS_CASE(4)
    PS_CASE(6)
    PS_CASE(8)
    PS_CASE(10)
    PS_CASE(13)
    PS_CASE(16)
    PS_CASE(22)
    PS_CASE(30)
#undef PS_CASE
    return hipErrorInvalidValue;
}

/* get_by_2_pick_every_second (s_pyramid_build.cu:50-71) of one plane, for every image of the batch */
__global__ void k_pick_every_second(int64_t src_off, int w, int h, int pitch, int64_t dst_off, int nw, int nh, int npitch, BatchDesc bd)
{
    float* const arena = bd.s[blockIdx.y].arena;
    const int    n = nw * nh;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int y = i / nw, x = i - y * nw;
        arena[dst_off + (size_t)y * npitch + x] = arena[src_off + (size_t)min(2 * y, h - 1) * pitch + min(2 * x, w - 1)];
    }
}

/* make_dog (s_pyramid_build.cu:74-92) of one level, for every image of the batch (the whole pitched plane) */
__global__ void k_dog_batch(int64_t lower_off, int64_t upper_off, int64_t dog_off, int64_t n, BatchDesc bd)
{
    float* const arena = bd.s[blockIdx.y].arena;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        arena[dog_off + i] = arena[upper_off + i] - arena[lower_off + i];
}

}  // namespace

int pyr_direct_tile_h() { return TH; }

hipError_t launch_pyr_direct(const DirectArgs& a, const BatchDesc& bd, int nb, int is_f32, hipStream_t s)
{
    if (a.L < 1 || a.L > PS_MAX_PLANES || !a.taps) return hipErrorInvalidValue;
    int halo = 0;
    for (int l = 0; l < a.L; l++) {
        if (a.halo[l] < 0 || a.halo[l] > 30) return hipErrorInvalidValue;
        halo = std::max(halo, a.halo[l]);
    }
    return is_f32 ? launch_direct_mode<2>(a, bd, nb, halo, s) : launch_direct_mode<1>(a, bd, nb, halo, s);
}

hipError_t launch_pick_every_second(int64_t src_off, int w, int h, int pitch, int64_t dst_off, int nw, int nh, int npitch,
                                    const BatchDesc& bd, int nb, hipStream_t s)
{
    const int blocks = std::max(1, std::min(2048, (nw * nh + 255) / 256));
    hipLaunchKernelGGL(k_pick_every_second, dim3(blocks, nb), dim3(256), 0, s, src_off, w, h, pitch, dst_off, nw, nh, npitch, bd);
    return hipGetLastError();
}

hipError_t launch_dog_batch(int64_t lower_off, int64_t upper_off, int64_t dog_off, int64_t n, const BatchDesc& bd, int nb,
                            hipStream_t s)
{
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n + 255) / 256));
    hipLaunchKernelGGL(k_dog_batch, dim3(blocks, nb), dim3(256), 0, s, lower_off, upper_off, dog_off, n, bd);
    return hipGetLastError();
}

}  // namespace popsift_hip
