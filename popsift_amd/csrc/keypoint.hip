/*
 * keypoint.hip -- orientation assignment, orientation prefix sum, the 128-D loop descriptor + normalisation, Feature
 * assembly: the kernels of every benchmark step.  The descriptors of the other DescModes (grid, notile / igrid,
 * iloop) are in desc_modes.hip, the device helpers both files use (the float wave sum, the work distribution KP_CHUNK,
 * atan2_acc) in keypoint_dev.h, the rules of the lists the kernels walk in ext_list.h, the wave and workgroup scans in
 * wave_dev.h.  All kernels size themselves
 * from the device-resident counters (grid-stride), so the host never has to
 * read a count back between stages (the reference blocks on the counters twice
 * per image: s_orientation.cu:351, sift_desc.cu:60-61).
 *
 * Replaces:
 *   ori_par               s_orientation.cu:60-242   -> k_orientation (1 wave / group of 16 extrema)
 *   ori_prefix_sum        s_orientation.cu:303-345  -> the epilogue of k_orientation (16 extrema / wave) + k_scan_apply (256 / workgroup)
 *   ext_desc_loop(+_sub)  s_desc_loop.cu:19-161     -> k_descriptor (1 wave / descriptor)
 *   normalize_histogram   s_desc_normalize.h:14-33, s_desc_norm_rs.h, s_desc_norm_l2.h
 *                                                   -> fused into k_descriptor
 *   prep_features         sift_pyramid.cu:249-279   -> fused into k_scan_apply
 */
#include <hip/hip_runtime.h>

#include "ext_list.h"
#include "kernels.h"
#include "keypoint_dev.h"
#include "sift_types.h"

namespace popsift_hip {
namespace {

constexpr float ORI_WINFACTOR = 1.5f; /* sift_constants.h:22-29 */

/* The four gradient taps around plane element `off` (>= pitch + 1, so every tap is in the plane).  `layer` and
 * `pitch` are wave-uniform: with an UNSIGNED 32-bit byte offset the loads take the scalar-base + vector-offset
 * form (three scalar bases: the row, the row below, the row above) instead of 64-bit vector address arithmetic
 * per tap.  A plane is far below 4 GiB (the arena's largest is 7680 x 4320 floats). */
/* ISA: taps */
struct Taps {
    const char* row;
    const char* dn;
    const char* up;
    __device__ __forceinline__ Taps(const float* layer, int pitch)
        : row((const char*)layer), dn((const char*)(layer + pitch)), up((const char*)(layer - pitch)) {}
    /* b: the BYTE offset of the element */
    __device__ __forceinline__ void load_b(unsigned int b, float& xp, float& xm, float& yp, float& ym) const
    {
        xp = *(const float*)(row + (size_t)b + 4);
        xm = *(const float*)(row + (size_t)b - 4);
        yp = *(const float*)(dn + (size_t)b);
        ym = *(const float*)(up + (size_t)b);
    }
};

/* ISA: end */

/* ------------------------------------------------------------ orientation */

/*
 * cos / sin of the keypoint orientation, evaluated in double and rounded once: the same two floats as the oracle's
 * sincos_cr (correctly rounded up to a ~1e-8 chance of double rounding).  |ang| <= pi (s_orientation.cu:222), so a
 * quadrant reduction with pi/2 split in two doubles and Taylor polynomials on [-pi/4, pi/4] (truncation < 1e-19,
 * rounding ~3e-16 relative) do it in ~35 double operations -- the library's double sincos with its large-argument
 * path is far bigger.  Done once per descriptor in k_scan_apply and stored next to the descriptor -> extremum map: inside the descriptor kernels
 * (64-register budget) any double arithmetic spilled and cost 5-9 %, inside k_orientation it raised the register
 * count from 62 to 86.
 */
__device__ __forceinline__ void sincos_cr(float ang, float& s, float& c)
{
    const double x = (double)ang;
    const double q = rint(x * 0.63661977236758134308);             /* 2/pi */
    double       r = fma(-q, 1.57079632679489655800e+00, x);       /* pi/2, high part */
    r = fma(-q, 6.12323399573676603587e-17, r);                     /* pi/2, low part  */
    const double z = r * r;
    double       ps = 2.81145725434552075980e-15;                    /* 1/17! */
    ps = fma(ps, z, -7.64716373181981647590e-13);                    /* 1/15! */
    ps = fma(ps, z, 1.60590438368216145994e-10);                     /* 1/13! */
    ps = fma(ps, z, -2.50521083854417187751e-08);                    /* 1/11! */
    ps = fma(ps, z, 2.75573192239858906526e-06);                     /* 1/9!  */
    ps = fma(ps, z, -1.98412698412698412698e-04);                    /* 1/7!  */
    ps = fma(ps, z, 8.33333333333333333333e-03);                     /* 1/5!  */
    ps = fma(ps, z, -1.66666666666666666667e-01);                    /* 1/3!  */
    const double sr = fma(ps * z, r, r);
    double       pc = -1.56192069685862264622e-16;                   /* 1/18! */
    pc = fma(pc, z, 4.77947733238738529744e-14);                     /* 1/16! */
    pc = fma(pc, z, -1.14707455977297247139e-11);                    /* 1/14! */
    pc = fma(pc, z, 2.08767569878680989792e-09);                     /* 1/12! */
    pc = fma(pc, z, -2.75573192239858906526e-07);                    /* 1/10! */
    pc = fma(pc, z, 2.48015873015873015873e-05);                     /* 1/8!  */
    pc = fma(pc, z, -1.38888888888888888889e-03);                    /* 1/6!  */
    pc = fma(pc, z, 4.16666666666666666667e-02);                     /* 1/4!  */
    pc = fma(pc, z, -0.5);
    const double cr = fma(pc, z, 1.0);
    const int    n = (int)q & 3; /* quadrant: sin/cos of r + n pi/2 */
    const double sd = (n & 1) ? cr : sr, cd = (n & 1) ? sr : cr;
    s = (float)((n & 2) ? -sd : sd);
    c = (float)(((n + 1) & 2) ? -cd : cd);
}

/* ISA: magnitude + angle */
/* The angle of the gradient (x, y) from the tangent of HALF the angle, which needs no octant reduction: with
 * theta' = the angle of (|x|, y), in [-pi/2, pi/2],
 *   tan(theta' / 2) = y / (|x| + |g|),   |g| = mod = sqrt(x^2 + y^2), which both callers have for their weight,
 * lies in [-1, 1], where the odd degree-11 minimax polynomial of atan(t) * 8/pi (the one of atan(r) * 4/pi on [0, 1],
 * max error 2.2e-6 there, fitted offline, every coefficient doubled) gives theta' in units of pi / 4 ("bins"): no min,
 * no max, no swap, no quadrant signs -- compares, selects and min / max are half rate on gfx950
 * (tools/ubench/valu_rate.hip).  x < 0 mirrors: theta = 4 - theta' bins, one v_bfi for the sign and the caller's scale
 * and offset in the same two FMAs:
 *   returns  scale * theta + k0 - 2 * scale   for x >= 0,  that plus 8 * scale where x < 0 and y < 0,
 * i.e. the angle in [-2, 6] bins where atan2 gives (-4, 4]: equal mod 8.  `scale` and `k0` are wave-uniform.
 * 1e-18 in the denominator keeps |t| <= 1 for EVERY gradient: a zero one gives t = 0, not 0 * inf, and one below
 * 1.1e-19, whose squares underflow so that mod comes out as 0 although y is not, gives |y| / (|x| + 1e-18) < 1 -- with
 * 1e-30 there it gave t = 1e4, the polynomial overflowed and the NaN fraction went into the histogram words of a sample
 * whose weight is zero (planes with a black background have such tails: a bright edge blurred level after level).  Such
 * a sample's angle is then wrong and harmless, its weight being 0 in fixed point below |g| = 1e-6; above that 1e-18 is
 * less than 1e-12 of the denominator.  Error against the float64 atan2 with v_sqrt and v_rcp one ulp off either way:
 * 4.9e-6 bins for |g| >= 1e-6 (tests/test_half_angle.py).  v_rcp instead of a division, as before. */
__device__ __forceinline__ float half_angle_bins(float y, float x, float mod, float scale, float k0)
{
    const float d = (fabsf(x) + 1e-18f) + mod;
    const float t = y * __builtin_amdgcn_rcpf(d);
    const float s = t * t;
    float       p = fmaf(-0.02984253503382206f, s, 0.13406537473201752f);
    p = fmaf(p, s, -0.2964776158332825f);
    p = fmaf(p, s, 0.4928465187549591f);
    p = fmaf(p, s, -0.8470170497894287f);
    p = fmaf(p, s, 2.5464210510253906f);
    const float th = t * p;
    const float sg = copysignf(scale, x);
    return fmaf(th, sg, fmaf(-2.0f, sg, k0));
}

typedef __attribute__((address_space(3))) fix64 lds_fix64;
typedef __attribute__((address_space(3))) unsigned int lds_u32;
typedef __attribute__((address_space(3))) float lds_f32;
typedef __attribute__((address_space(3))) short lds_i16;
typedef __attribute__((address_space(3))) unsigned long long lds_u64;

/* ISA: end */
#ifndef KP_NW
#define KP_NW 1 /* waves per workgroup of k_orientation / k_descriptor: the waves are independent (a group / one descriptor each) */
#endif
constexpr int ORI_COPIES = 4; /* private histogram copies by lane: neighbouring pixels often share a bin */

/* ISA: peaks */
/*
 * x / 3.0f, correctly rounded for normal x (Markstein: q = x * RN(1/3), one FMA residual, one FMA correction; checked
 * against IEEE division for every float of six binades, tools/check_div3.py) instead of the ten-instruction division
 */
__device__ __forceinline__ float div3(float x)
{
    const float r = 0.333333343267440796f; /* RN(1/3) */
    const float q = x * r;
    return fmaf(fmaf(-3.0f, q, x), r, q);
}

/*
 * ori_par, second half (s_orientation.cu:142-240), FOUR lanes per extremum, nine of the 36 bins each: six circular
 * box-filter passes, parabolic peak interpolation, the (at most four) best peaks within 80 % of the best.  The lanes of
 * a quad exchange their edge bins and their candidates with DPP quad permutes (register-to-register, no LDS);
 * BitonicSort::Warp32::sort64 (common/warp_bitonic_sort.h:35-78) becomes four selection rounds, ties to the lower
 * bin.  Everything is indexed statically, so the bins live in registers.  (One LANE per extremum -- 36 bins in
 * registers, no exchange at all -- needs only 1200 waves for a 1080p image: 24 us at barely one wave per SIMD.)
 * All four lanes of a quad must be active; all return the same result.  hsrc: the raw histogram, in LDS.
 */
__device__ __forceinline__ float quad_from_prev(float v) /* lane j of a quad reads lane (j + 3) & 3 */
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x93, 0xf, 0xf, false));
}
__device__ __forceinline__ float quad_from_next(float v) /* lane j reads lane (j + 1) & 3 */
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x39, 0xf, 0xf, false));
}
template <int CTRL> /* 0xB1: lane ^ 1, 0x4E: lane ^ 2 */
__device__ __forceinline__ int quad_xchg(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}

__device__ __forceinline__ int ori_peaks_quad(const lds_f32* __restrict__ hsrc, int j, bool have, float* angle_out)
{
    constexpr int N = PS_ORI_NBINS, M = N / 4; /* 9 bins per lane: 9j .. 9j+8 */
    float         h[M], t[M];
#pragma unroll
    for (int b = 0; b < M; b++) h[b] = have ? hsrc[M * j + b] : 0.0f;
#pragma unroll
    for (int pass = 0; pass < 3; pass++) {
        {
            const float lft = quad_from_prev(h[M - 1]), rgt = quad_from_next(h[0]);
#pragma unroll
            for (int b = 0; b < M; b++) t[b] = div3(((b == 0 ? lft : h[b - 1]) + h[b]) + (b == M - 1 ? rgt : h[b + 1]));
        }
        {
            const float lft = quad_from_prev(t[M - 1]), rgt = quad_from_next(t[0]);
#pragma unroll
            for (int b = 0; b < M; b++) h[b] = div3(((b == 0 ? lft : t[b - 1]) + t[b]) + (b == M - 1 ? rgt : t[b + 1]));
        }
    }
    float refined[M], yval[M];
    {
        const float lft = quad_from_prev(h[M - 1]), rgt = quad_from_next(h[0]);
#pragma unroll
        for (int b = 0; b < M; b++) {
            const int   bin = M * j + b;
            const int   prev = (bin == 0) ? N - 1 : bin - 1;
            const float hp = (b == 0) ? lft : h[b - 1], hv = h[b], hn = (b == M - 1) ? rgt : h[b + 1];
            bool        predicate = hv > fmaxf(hp, hn);
            const float num = predicate ? 3.0f * hp - 4.0f * hv + 1.0f * hn : 0.0f;
            const float denB = predicate ? 2.0f * (hp - 2.0f * hv + hn) : 1.0f;
            const float newbin = num / denB;
            predicate = (predicate && newbin >= 0.0f && newbin <= 2.0f);
            refined[b] = predicate ? prev + newbin : -1.0f;
            yval[b] = predicate ? -(num * num) / (4.0f * denB) + hp : -INFINITY;
        }
    }
    unsigned int used = 0u; /* of this lane's nine bins */
    float        best0 = 0.0f;
    int          angles = 0;
#pragma unroll
    for (int k = 0; k < POPSIFT_HIP_ORI_MAX; k++) {
        /* best unused bin of this lane: largest value, lowest bin on ties (every lane has unused bins: 9 > 4) */
        float bv = 0.0f, br = -1.0f;
        int   bi = -1;
#pragma unroll
        for (int b = 0; b < M; b++) {
            const bool take = !((used >> b) & 1u) && (bi < 0 || yval[b] > bv);
            bv = take ? yval[b] : bv;
            br = take ? refined[b] : br;
            bi = take ? M * j + b : bi;
        }
        /* ... of the quad */
        {
            const float ov = __int_as_float(quad_xchg<0xB1>(__float_as_int(bv))), orf = __int_as_float(quad_xchg<0xB1>(__float_as_int(br)));
            const int   oi = quad_xchg<0xB1>(bi);
            const bool  take = ov > bv || (ov == bv && oi < bi);
            bv = take ? ov : bv;
            br = take ? orf : br;
            bi = take ? oi : bi;
        }
        {
            const float ov = __int_as_float(quad_xchg<0x4E>(__float_as_int(bv))), orf = __int_as_float(quad_xchg<0x4E>(__float_as_int(br)));
            const int   oi = quad_xchg<0x4E>(bi);
            const bool  take = ov > bv || (ov == bv && oi < bi);
            bv = take ? ov : bv;
            br = take ? orf : br;
            bi = take ? oi : bi;
        }
        const int mine = bi - M * j;
        if (mine >= 0 && mine < M) used |= 1u << mine;
        if (k == 0) best0 = bv;
        /* the candidates come in descending order, so the accepted ones are a prefix */
        if (bv >= 0.8f * best0) {
            float chosen_bin = br;
            if (chosen_bin >= N) chosen_bin -= N;
            angle_out[k] = fmaf(F_PI2 * chosen_bin, 1.0f / N, -F_PI);
            angles = k + 1;
        } else {
            angle_out[k] = 0.0f;
        }
    }
    return angles;
}
/* ISA: end */

/* The scan's granularity: k_orientation leaves idx_ori local to its group of SCAN_LCHUNK list entries and one partial sum
 * per group; k_scan_apply (SCAN_CHUNK entries per workgroup, SCAN_SUB groups) adds what precedes. */
constexpr int SCAN_LCHUNK = KP_GROUP;

/*
 * ori_par (s_orientation.cu:60-242), a wave per group of KP_GROUP = 16 consecutive list entries.  First half, the whole
 * wave on one extremum after the other: its weighted 36-bin gradient-orientation histogram, whose 36 floats stay in the
 * wave's LDS (s_stage).  Second half -- smoothing, peak interpolation, the four best peaks -- is serial per extremum and
 * runs once per group, FOUR lanes per extremum (ori_peaks_quad): as a wave-wide epilogue per extremum it was ~350 of the
 * kernel's ~1250 vector instructions per extremum, as a launch of its own (k_scan_local, until the groups) it read the
 * histograms back from device memory, 144 bytes per extremum written and read for nothing.  The quad's first lane then
 * writes the extremum's Ext record with idx_ori local to the group, and the group's number of orientations goes to
 * partial[group] for k_scan_apply.
 * Every extremum of the list gets its record; those from hist_cap on (the host's capacity for this pass: it raises it and
 * runs the stages again, ctx.hip finish) get no histogram and no orientation.
 */
__global__ __launch_bounds__(64 * KP_NW, 8) void k_orientation(const PyrDesc* __restrict__ pdp, BatchDesc bd, SiftConsts sc,
                                                        int filtered, int hist_cap)
{
    /* this image's planes and lists (the slot of blockIdx.y) */
    const float* __restrict__   arena = bd.s[blockIdx.y].arena;
    Counters* __restrict__      ct = bd.s[blockIdx.y].ct;
    const InitExt* __restrict__ iext = filtered ? bd.s[blockIdx.y].iext2 : bd.s[blockIdx.y].iext;
    Ext* __restrict__           ext = bd.s[blockIdx.y].ext;
    int* __restrict__           partial = bd.s[blockIdx.y].partial;
    const int n_oct = pdp->n_oct, L = pdp->L;
    /* The histogram is circular and the loop's bin coordinate runs from 9 to 45 (half_angle_bins: the angle in [-pi/2,
     * 3pi/2]; next to a bin edge from 0 to 36, atan2_acc): bin b + 36 is bin b.  A sample is added where it falls and
     * the bins 36 .. 45 join the bins 0 .. 9 at the read-out, so the loop needs no wrap-around select. */
    constexpr int    NB = PS_ORI_NBINS + 10;
    __shared__ fix64 s_hist[KP_NW][ORI_COPIES][NB];
    const int        wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    fix64*           hall = &s_hist[wave][0][0];
    fix64*           hist = s_hist[wave][lane & (ORI_COPIES - 1)];

    /* the group's raw histograms, for the peak search after the group's last extremum */
    __shared__ float s_stage[KP_NW][KP_GROUP][PS_ORI_NBINS];
    static_assert(KP_GROUP * 4 == 64, "four lanes per extremum of a group");
    static_assert(sizeof(s_hist) / KP_NW + sizeof(s_stage) / KP_NW + 64 <= 5120, "32 waves per CU share 160 KiB");

    __shared__ int ps[PS_MAX_OCT + 1];
    const int total = ext_prefix(ps, ct, sc.max_extrema, n_oct);

    for (XcdSliceOf<KP_GROUP> sl = xcd_slice<KP_NW, KP_GROUP>(); sl.more(total); sl.s += sl.step) {
        const int g0 = uniform(sl.index());
        if (g0 >= total) continue;
        /* the histograms of the group's extrema below the list's end and below the capacity of this pass */
        const int g_end = min(min(g0 + KP_GROUP, total), hist_cap);
        for (int g = g0; g < g_end; g++) {
        /* ISA: record */
        const int o = uniform(ext_octave(ps, n_oct, g)); /* the octave record and the list entry are then fetched through the scalar cache */
        const InitExt  ie = iext[(size_t)o * sc.max_extrema + (g - uniform(ps[o]))];
        const OctDesc* od = &pdp->o[o];
        const int      w = uniform(od->w), h = uniform(od->h), pitch = uniform(od->pitch);
        const int      lvl = uniform(min(max(ie.lpos, 0), L - 1));
        const float*   layer = arena + uniform64(od->data_off + lvl * od->plane_stride);

        /* ISA: clear */
        for (int k = lane; k < ORI_COPIES * NB; k += 64) hall[k] = 0ull;
        wave_lds_sync();
        /* ISA: set-up */

        const float x = uniformf(ie.xpos), y = uniformf(ie.ypos), sig = uniformf(ie.sigma);
        const float sigw = ORI_WINFACTOR * sig;
        const int   rad = (int)roundf(3.0f * sigw);
        const float factor2 = (-0.5f / (sigw * sigw)) * 1.4426950408889634f; /* in powers of two */
        const int   sq_thres = rad * rad;
        const int   xmin = max(1, (int)roundf(x) - rad);
        const int   xmax = min(w - 2, (int)roundf(x) + rad);
        const int   ymin = max(1, (int)roundf(y) - rad);
        const int   ymax = min(h - 2, (int)roundf(y) + rad);
        const int   wx = xmax - xmin + 1;
        const int   hy = ymax - ymin + 1;
#ifdef ORI_PROBE_NOLOOP
        const int   loops = 0;
#else
        const int   loops = (wx > 0 && hy > 0) ? wx * hy : 0;
#endif
        /* row of flat index i = floor((i + 0.5) / wx): the half keeps the quotient at least 0.5 / wx away from an integer,
         * far more than the ulp by which v_rcp may miss 1 / wx, so the approximate reciprocal gives the exact row */
        const float inv_wx = __builtin_amdgcn_rcpf((float)max(wx, 1));
        const float wxf = (float)wx, xminf = (float)xmin, yminf = (float)ymin, pitch4f = (float)(4 * pitch);
        const float* corner = layer + (size_t)(ymin * pitch + xmin);

        /* software pipeline as in k_descriptor: request the taps of sample i+64 while binning sample i.  Row, column
         * and the byte offset of the taps are formed in floats (exact small integers): one conversion, one floor and FMAs
         * instead of two conversions, two 24-bit multiplies and a shift-add -- half-rate instructions on gfx950
         * (tools/ubench/valu_rate.hip).  (fx, fy) = the pixel, as the floats the reference converts its ints to. */
        auto coord = [&](int i, float& fx, float& fy, unsigned int& off) { /* ISA: coordinates */
            const float fi = (float)i;
            const float frow = floorf((fi + 0.5f) * inv_wx);
            const float fcol = fmaf(-frow, wxf, fi);
            fx = fcol + xminf;
            fy = frow + yminf;
            off = (unsigned int)fmaf(frow, pitch4f, fcol * 4.0f);
        };
        /* one sample: pixel (fx, fy) with gradient (gdx, gdy) -> at most one fixed-point LDS atomic */
        auto bin = [&](float fx, float fy, float gdx, float gdy, bool live) { /* ISA: bin */
            const float dx = fx - x;
            const float dy = fy - y;
            /* int truncation, s_orientation.cu:123 -- as a float (the values are far below 2^24, so truncf, the
             * comparison with rad^2 and the product with `factor` give what the int round trip gives) */
            const float sq_dist = truncf(dx * dx + dy * dy);
            if (live && sq_dist <= (float)sq_thres) {
                /* hypotf * expf(sq_dist * factor) * 2^20 (the fixed-point scale of from_fix): the scale and log2(e) go into
                 * the exponent, so the window weight is one FMA and one v_exp */
                const float mod = __builtin_amdgcn_sqrtf(fmaf(gdx, gdx, gdy * gdy));
                const float wfix = mod * __builtin_amdgcn_exp2f(fmaf(sq_dist, factor2, 20.0f));
                /* The bin is a HARD decision, so the angle needs libm-grade accuracy -- but only when it lies next to a
                 * bin edge: the cheap arctangent (the descriptor's: one reciprocal, a degree-11 polynomial in units of
                 * pi / 4, error < 4.9e-6 of those = 2.2e-5 of these bins) decides every sample farther than 1e-4 bins
                 * from an edge identically to the accurate one, which the others (1 in 5000) then take.  Scale and
                 * offset ride in its last FMA: theta * 36 / 8 + 18, up to a multiple of 36 (NB above). */
                float fb = half_angle_bins(gdy, gdx, mod, (float)PS_ORI_NBINS / 8.0f, 0.75f * (float)PS_ORI_NBINS);
                /* next to an edge the value is formed exactly as the oracle forms it (product, then IEEE quotient): gradients
                 * of exactly 45 degrees -- frequent in level 0 of the up-scaled octave -- sit ON the edge 22.5, 31.5, ...,
                 * where the two formulas round to different sides */
                if (fabsf((fb - floorf(fb)) - 0.5f) < 1e-4f) fb = (float)PS_ORI_NBINS * (atan2_acc(gdy, gdx) + F_PI) / F_PI2;
                /* roundf(fb) for fb in [0, 45]: floor(fb + 0.5), one instruction; 36 .. 45 are bins 0 .. 9 (NB above) */
                int bidx;
                asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(bidx) : "v"(fb));
                atomicAdd(&hist[bidx], (fix64)(unsigned int)wfix);
            }
        };
        /* ISA: control */
        /* two register sets take turns as "being binned" and "in flight", as in k_descriptor (unrolled by two, so no
         * value is copied from one role to the other) */
        float        xa = 0.0f, ya = 0.0f, xb = 0.0f, yb = 0.0f;
        unsigned int oa = 0, ob = 0;
        float        a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f, b0 = 0.0f, b1 = 0.0f, b2 = 0.0f, b3 = 0.0f;
        const Taps   taps(corner, pitch);
        /* steps of 64 window positions, exactly (wave-uniform): the last one may be partial, none is empty */
        const int steps = (loops + 63) >> 6;
        if (steps > 0) {
            coord(min(lane, loops - 1), xa, ya, oa);
            taps.load_b(oa, a0, a1, a2, a3);
        }
        /* double steps while a further step follows them, as in k_descriptor: only then is the set requested at the end
         * ever binned.  Neither step of the pair is the window's last, so both are full (no lane beyond the window);
         * the step after them may be the last one, so its index is held inside the window. */
        int t = steps, i = lane;
        for (; t > 2; t -= 2, i += 128) {
            coord(i + 64, xb, yb, ob);
            taps.load_b(ob, b0, b1, b2, b3);
            bin(xa, ya, a0 - a1, a2 - a3, true);
            coord(min(i + 128, loops - 1), xa, ya, oa);
            taps.load_b(oa, a0, a1, a2, a3);
            bin(xb, yb, b0 - b1, b2 - b3, true);
        }
        /* the last one or two steps (wave-uniform branches): nothing is requested beyond the window's last step.  With
         * a double step to the end, every window with an odd number of steps (half of them, at about nine steps per
         * keypoint) walked a whole dead half-step: coordinates, four tap loads, the distance test. */
        if (t == 2) {
            coord(min(i + 64, loops - 1), xb, yb, ob);
            taps.load_b(ob, b0, b1, b2, b3);
        }
        if (t > 0) bin(xa, ya, a0 - a1, a2 - a3, i < loops);
        if (t == 2) bin(xb, yb, b0 - b1, b2 - b3, i + 64 < loops);
        wave_lds_sync();

        /* ISA: read-out */
        if (lane < PS_ORI_NBINS) {
            fix64 acc = 0ull;
#pragma unroll
            for (int k = 0; k < ORI_COPIES; k++)
                acc += hall[k * NB + lane] + (lane < NB - PS_ORI_NBINS ? hall[k * NB + PS_ORI_NBINS + lane] : 0ull);
            s_stage[wave][g - g0][lane] = from_fix(acc);
        }
        wave_lds_sync(); /* ISA: end */
        } /* the group's extrema */

        /* ISA: peaks */
        /* The second half for the whole group: lane 4k + j is lane j of the quad of extremum g0 + k.  Quads beyond the
         * list's end compute along on its last entry (the quad exchanges need every lane) and write nothing. */
        {
            const int  j = lane & 3;
            const int  g = g0 + (lane >> 2);
            const bool valid = g < total;
            const int  gc = min(g, total - 1);
            /* the extremum's record (sift_extremum.h:40-51) */
            const int     o = ext_octave(ps, n_oct, gc);
            const InitExt ie = iext[(size_t)o * sc.max_extrema + (gc - ps[o])];
            Ext           e;
            e.xpos = ie.xpos;
            e.ypos = ie.ypos;
            e.lpos = ie.lpos;
            e.sigma = ie.sigma;
            e.octave = o;
            /* beyond the capacity of this pass (the host raises it and re-runs the stages): no orientation */
            const bool have = gc < hist_cap;
            const int  n = ori_peaks_quad((const lds_f32*)&s_stage[wave][gc - g0][0], j, have, e.orientation);
            e.num_ori = have ? n : 0;
            if (!have)
                for (int q = 0; q < POPSIFT_HIP_ORI_MAX; q++) e.orientation[q] = 0.0f;
            const int self = (valid && j == 0) ? e.num_ori : 0;
            const int incl = wave_incl_scan(self);
            if (valid && j == 0) {
                e.idx_ori = incl - self; /* local to the group for now */
                ext[g] = e;
            }
            if (lane == 63) partial[g0 / SCAN_LCHUNK] = incl;
        }
        wave_lds_sync(); /* the next group's histograms go where these were read */ /* ISA: end */
    }
}

/* The per-descriptor constants of the loop descriptor (k_descriptor), computed where one lane serves one extremum.
 * fbits: each cell word packs two 32-bit fixed-point sums (low = share of orientation bin b, high = share of bin b+1
 * from samples whose lower bin is b), so ONE 64-bit LDS atomic per cell serves both bins of a sample; the scale 2^fbits
 * keeps the worst-case low sum below 2^32 (no carry into the high half): a sample weighs <= 361 (|gradient| of a
 * 0..255 plane, unit window weights) and a cell sees at most (2.83*SBP+1)^2 pixels. */
__device__ __forceinline__ DescRec make_desc_rec(const PyrDesc* __restrict__ pdp, const Ext& e, float angle, float cos_t, float sin_t)
{
    DescRec        r;
    const OctDesc* od = &pdp->o[e.octave];
    const int      lvl = min(max(e.lpos, 0), pdp->L - 1);
    const long long off = od->data_off + lvl * od->plane_stride;
    const float    x = e.xpos, y = e.ypos;
    const float    SBP = fabsf(DESC_MAGNIFY * e.sigma);
    const float    cell_px = (2.83f * SBP + 1.0f) * (2.83f * SBP + 1.0f);
    /* ... and below 2^23 per sample (361 * 2^14 < 2^23): k_descriptor reads a word as the bits of a product scaled by
     * 2^-149, which are the integer below 2^24 (PS_CELL) */
    const int      fbits = min(max(31 - (int)ceilf(log2f(361.0f * cell_px)), 2), 14);
    const float    csbp = cos_t * SBP, ssbp = sin_t * SBP;
    const float    bsz = fabsf(csbp) + fabsf(ssbp);
    /* union of the 16 cell boxes: cell centres reach 1.5 * bsz, each box adds bsz */
    const float    ext_r = 2.5f * bsz;
    const int      xmin = max(1, (int)floorf(x - ext_r));
    const int      ymin = max(1, (int)floorf(y - ext_r));
    const int      xmax = min(od->w - 2, (int)floorf(x + ext_r) + 1);
    const int      ymax = min(od->h - 2, (int)floorf(y + ext_r) + 1);
    r.x = x;
    r.y = y;
    r.crsbp = cos_t / SBP;
    r.srsbp = sin_t / SBP;
    r.ang_bins = angle * (4.0f / F_PI);
    /* Extraction's orientations lie within a bin of [-pi, pi], |ang_bins| <= 4.2, and stay the float they were.  The
     * describe path accepts every finite angle: beyond two turns the bin count is brought back into [-4, 4] (any multiple
     * of 8 bins may be missing), so that k_descriptor's slot sum has ONE bound for all of them (DESC_SLOT_BIAS). */
    if (!(fabsf(r.ang_bins) <= 16.0f)) r.ang_bins = (float)remainder((double)angle * (4.0 / 3.14159265358979323846), 8.0);
    /* the hardware reciprocal, formed here once per descriptor instead of in all 64 lanes of its wave: the same
     * instruction on the same float, so the row spans of k_descriptor are what they were */
    r.inv_c = (fabsf(r.crsbp) > 1e-20f) ? __builtin_amdgcn_rcpf(r.crsbp) : 0.0f;
    r.inv_s = (fabsf(r.srsbp) > 1e-20f) ? __builtin_amdgcn_rcpf(r.srsbp) : 0.0f;
    r.xymin = ((unsigned int)xmin & 0xffffu) | ((unsigned int)ymin << 16);
    r.xymax = ((unsigned int)xmax & 0xffffu) | ((unsigned int)ymax << 16);
    r.off_lo = (unsigned int)((unsigned long long)off & 0xffffffffull);
    r.off_hi = (unsigned int)((unsigned long long)off >> 32);
    r.misc = (unsigned int)od->pitch | ((unsigned int)fbits << 16) | ((SBP != 0.0f) ? (1u << 24) : 0u);
    return r;
}

/* ------------------------------------------------------------------- scan */

/*
 * Exclusive prefix sum of num_ori over all extrema -> idx_ori, the reverse map
 * descriptor -> extremum, and the totals (replaces ori_prefix_sum's single
 * 32x32 block looping over everything, s_orientation.cu:303-345).  k_orientation
 * scans each group of 16 extrema and leaves one partial per group (on the describe
 * path with given angles: k_frame_place); k_scan_apply (256 extrema per workgroup)
 * adds the sum of the preceding partials (<= 56 300 values for the default 9 x 100000
 * capacity, ~4 800 for a 1080p image, summed redundantly per workgroup) and writes
 * the map and the counters.
 */
/* extrema per lane: 1 -- the per-extremum work of k_scan_apply (feature record, double-precision cos / sin)
 * is serial per lane, so wide beats deep (8 per lane: 22.8 us, 2: 10.2 us, 1: 7.5 us) */
constexpr int SCAN_ITEMS = 1;
constexpr int SCAN_CHUNK = 256 * SCAN_ITEMS;
constexpr int SCAN_SUB = SCAN_CHUNK / SCAN_LCHUNK;
static_assert(SCAN_CHUNK % SCAN_LCHUNK == 0 && SCAN_SUB <= 64, "whole groups per chunk, one lane of a wave per group");

__global__ __launch_bounds__(256) void k_scan_apply(const PyrDesc* __restrict__ pdp, SiftConsts sc, BatchDesc bd,
                                                    int with_drec, int desc_cap)
{
    Counters* __restrict__            ct = bd.s[blockIdx.y].ct;
    Ext* __restrict__                 ext = bd.s[blockIdx.y].ext;
    const int* __restrict__           partial = bd.s[blockIdx.y].partial;
    int* __restrict__                 map = bd.s[blockIdx.y].map;
    float2* __restrict__              rot = bd.s[blockIdx.y].rot;
    DescRec* __restrict__             drec = with_drec ? bd.s[blockIdx.y].drec : nullptr;
    popsift_hip_feature* __restrict__ feats = bd.s[blockIdx.y].feats;
    __shared__ int s_red[4];
    __shared__ int s_sub[SCAN_SUB];
    __shared__ int s_ps[PS_MAX_OCT + 1];
    const int      n_oct = pdp->n_oct;
    const int      tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int total = ext_prefix(s_ps, ct, sc.max_extrema, n_oct);
    const int nb = (total + SCAN_CHUNK - 1) / SCAN_CHUNK;
    if (nb == 0 && blockIdx.x == 0 && tid == 0) { /* no extrema at all: the counters still have to be written */
        ct->ori_total = 0;
        ct->ext_total = 0;
        for (int o = 0; o < PS_MAX_OCT; o++) {
            ct->ext_ct[o] = 0;
            ct->ext_ps[o] = 0;
        }
    }
    /* the launch is sized for the device, not for the capacity of the lists: workgroups stride over the chunks */
    for (int chunk = blockIdx.x; chunk < nb; chunk += gridDim.x) {
    const int base = chunk * SCAN_CHUNK;

    /* offset of this chunk = sum of the partials of all preceding chunks (SCAN_SUB groups per chunk here) */
    /* four partials per load (whole chunks: a multiple of four of them): the loop is a chain of dependent round trips, and
     * with a partial per 16 extrema instead of per 64 it would be four times as long */
    static_assert(SCAN_SUB % 4 == 0, "16-byte loads of the partials");
    int acc = 0;
    for (int b = tid; b < chunk * (SCAN_SUB / 4); b += 256) {
        const int4 v = reinterpret_cast<const int4*>(partial)[b];
        acc += (v.x + v.y) + (v.z + v.w);
    }
    acc = wave_sum(acc);
    if (lane == 0) s_red[wave] = acc;
    /* ... plus the groups of this chunk that precede the lane's own: their exclusive prefix, one lane of the first wave per
     * group (a group beyond the list's end has no partial; what is read there reaches only groups beyond it) */
    if (wave == 0) {
        const int v = (lane < SCAN_SUB) ? partial[chunk * SCAN_SUB + lane] : 0;
        const int incl = wave_incl_scan(v);
        if (lane < SCAN_SUB) s_sub[lane] = incl - v;
    }
    __syncthreads();
    const int chunk_offset = s_red[0] + s_red[1] + s_red[2] + s_red[3];
    const int offset = chunk_offset + s_sub[(tid * SCAN_ITEMS) / SCAN_LCHUNK];

    const int g0 = base + tid * SCAN_ITEMS;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        const int g = g0 + k;
        if (g < total) {
            Ext       e = ext[g];
            const int idx = e.idx_ori + offset;
            const int n = e.num_ori;
            ext[g].idx_ori = idx;
            /* prep_features (sift_pyramid.cu:249-279): positions and scale in input-image coordinates,
             * descriptor indices instead of pointers */
            popsift_hip_feature f;
            const float         scl = powf(2.0f, (float)(e.octave - sc.up_fac_int));
            f.debug_octave = e.octave;
            f.xpos = e.xpos * scl;
            f.ypos = e.ypos * scl;
            f.sigma = e.sigma * scl;
            f.num_ori = n;
#pragma unroll
            for (int q = 0; q < POPSIFT_HIP_ORI_MAX; q++) {
                const bool on = q < n && idx + q < desc_cap;
                f.desc_idx[q] = on ? idx + q : -1;
                f.orientation[q] = (q < n) ? e.orientation[q] : 0.0f;
                if (on) {
                    map[idx + q] = g;
                    /* the rotation of the descriptor frame, in double, here where registers are plentiful */
                    float sn, cs;
                    sincos_cr(e.orientation[q], sn, cs);
                    rot[idx + q] = make_float2(cs, sn);
                    if (drec) drec[idx + q] = make_desc_rec(pdp, e, e.orientation[q], cs, sn);
                }
            }
            feats[g] = f;
            /* first extremum of an octave: start of that octave's descriptors (dct.ori_ps) */
            for (int o = 0; o < n_oct; o++)
                if (g == s_ps[o] && s_ps[o + 1] > s_ps[o]) ct->ori_ps[o] = idx;
        }
    }
    if (tid == 0 && chunk == nb - 1) {
        int last = chunk_offset;
        for (int k = 0; k < SCAN_SUB && (chunk * SCAN_SUB + k) * SCAN_LCHUNK < total; k++) last += partial[chunk * SCAN_SUB + k];
        ct->ori_total = last;
        ct->ext_total = total;
        for (int o = 0; o < PS_MAX_OCT; o++) {
            /* the reference clamps with atomicMin in the extrema kernel, s_extrema.cu:558 */
            ct->ext_ct[o] = (o < n_oct) ? ext_count(ct, sc.max_extrema, o) : 0;
            ct->ext_ps[o] = s_ps[o];
        }
    }
    __syncthreads(); /* s_red and s_sub are reused by the next chunk */
    }
}

/* ------------------------------------------------------------- descriptor */

/*
 * One wave per (extremum, orientation), no workgroup barrier.  The reference gives every one of the 16 cells
 * its own warp, which re-computes the gradient of each patch pixel for up to four overlapping cells
 * (s_desc_loop.cu:78-122).  Here each patch pixel is visited once: its gradient is computed once and its
 * contribution is spread to the (at most) 2x2 cells whose unit square contains it -- the same sample set and
 * weights, a different summation order.  The 128-bin histogram lives in LDS (per wave, fixed point: exact and
 * order-independent sums), is normalised in registers and leaves as two coalesced 256 B rows.
 *
 * LDS atomics set the pace of the first version (rocprofv3, round 2: the LDS was busy 73 % of the kernel's cycles,
 * 63 % of that bank-conflict cycles): 64 lanes on 64 consecutive pixels of a patch row mostly fall into the same
 * cell row, a few cells and -- gradients being smooth -- one or two orientation bins, i.e. up to 16 lanes on one
 * address, and the two private copies sat exactly 1 KiB apart, on the same banks.  Now
 *   - the wave works as four groups of 16 lanes, each on its own quarter of the sample list (different cell rows),
 *   - four private copies by lane (neighbouring lanes never share a word),
 *   - the word of (copy c, cell iy ix, bin b) is c*140 + iy*36 + ix*8 + ((b + c + 4*(ix & 1)) & 7) (DESC_CS, DESC_RS
 *     below): for lanes that agree in the bin, the copies, the two cell columns a group straddles and the four groups'
 *     cell rows land on different bank pairs, and the four words of a sample are one address + immediate offsets.
 */
#ifndef DESC_NCOPY
#define DESC_NCOPY 4
#endif
constexpr int DESC_COPIES = DESC_NCOPY;
/* LINEAR histogram layout: the word (8 bytes) of (copy c, cell row iy, cell column ix, slot s) is
 * c * DESC_CS + iy * DESC_RS + ix * 8 + s with a cell-row stride of 36 words instead of 32.  The four words of a sample
 * are then ONE address plus the immediate offsets 0 / 64 / 288 / 352 bytes (no per-cell index arithmetic, cells -1 and
 * 4 fall out naturally), and the four extra words per row shift consecutive cell rows by four bank pairs, which does
 * what the (ix + iy) rotation of the 32-word layout did for the four lane groups working on different rows. */
constexpr int DESC_RS = 36;                /* words per cell row */
constexpr int DESC_CS = 3 * DESC_RS + 32;  /* words per copy (the last row needs no padding): 140 */
/* A pass of the span path: at most DESC_MAXROWS patch rows (the default configuration's largest patches have 93) and at
 * most DESC_LISTCAP list positions.  In front of a wave's histograms lie, per pass, one 16-bit record per row and one bit
 * per list position (k_descriptor); the table has one 64-bit word more than the positions need, because the sample loop
 * reads the word of the step AFTER the one it works on.  Records and table are sized together: with the histograms they
 * fill the 5120 bytes that 32 waves per CU leave each wave. */
constexpr int DESC_MAXROWS = 96;
constexpr int DESC_REC_WORDS = (((DESC_MAXROWS + 1) * 2 + 7) / 8) * 2; /* 50 words: the rows' records and the sentinel */
constexpr int DESC_TAB64 = 55;                                          /* 64-bit words of the row-end bits */
constexpr int DESC_LISTCAP = (DESC_TAB64 - 1) * 64;                     /* 3456 list positions per pass */
/* k_descriptor reads the slot of a sample's lower bin from the BITS of the float (32 cx0 + 8 bin + 8 copy + BIAS) * 2^-149,
 * which are that integer only while the sum is positive (a negative float is sign and magnitude).  cx0 >= -1 (the
 * in-square test: u > -2.5); copy >= 0; the bin is floor(half_angle_bins(.., 1, 2 - ang_bins)), whose value lies in
 * [-2, 6] + (2 - ang_bins) - 2 up to the polynomial's 5e-6, with |ang_bins| <= 16 (make_desc_rec): bin >= -19.  So the sum
 * is at least -32 - 152 = -184 without the bias.  A multiple of 64: invisible to the `& 56` and the `^ 32` that use it. */
constexpr int DESC_SLOT_BIAS = 512;
static_assert(DESC_SLOT_BIAS % 64 == 0 && DESC_SLOT_BIAS > 32 + 8 * 19, "the slot sum stays positive and the bias drops out");
/* The 64 lanes walk 64 CONSECUTIVE samples of the list, i.e. one and a half to two neighbouring patch rows, whose up /
 * down taps are each other's centre rows.  Round 2 ran four lane groups (16 lanes each, on four distant parts of the
 * patch: 61 % fewer LDS bank conflicts) while the kernel was bound by vector issue and LDS; once round 3 had slimmed the
 * loop, the L1 -> L2 request stream of the taps bound it (four streams touch four times the cache lines per wave step),
 * and one group made the timed loop 4.8 % faster (1 / 2 / 4 / 8 groups: 3.36 / 3.36 / 3.20 / 2.74 Gpix/s). */

__global__ __launch_bounds__(64 * KP_NW, 8) void k_descriptor(BatchDesc bd, SiftConsts sc, int desc_cap)
{
    const float* __restrict__   arena = bd.s[blockIdx.y].arena;
    const Counters* __restrict__ ct = bd.s[blockIdx.y].ct;
    const DescRec* __restrict__ drec = bd.s[blockIdx.y].drec;
    float* __restrict__         desc = bd.s[blockIdx.y].desc;
    /* LDS of a wave: the row records, the row-end bits, then the histogram copies.  The rows' column intervals of the
     * current pass are laid end to end as one flat list.  Record k (16 bits, signed) belongs to the k-th row from the first
     * one that holds a sample: the first column of the row's interval relative to xmin minus the flat index of its first
     * sample, so that column = flat index + record.  Bit p of the table is set where list position p is the LAST of its
     * row.  The row of position p is then the number of bits below p: the bits of the earlier 64-bit words are a
     * running count, those of p's own word below p are one v_mbcnt pair -- no search.  Every row between the first and
     * the last of a pass holds at least one position, so that count IS the index of the row's record.  All this lies IN
     * FRONT of the histograms so that the address of cell (-1, -1) of copy 0, which the cell arithmetic forms although
     * no weight ever goes there (352 bytes before the copy), is still a non-negative LDS address. */
    constexpr int ROW_WORDS = DESC_REC_WORDS + 2 * DESC_TAB64; /* 160 */
    static_assert(ROW_WORDS % 4 == 0 && DESC_REC_WORDS % 2 == 0, "the histograms start on a 16-byte boundary, the table on an 8-byte one");
    static_assert(ROW_WORDS * 4 >= 352, "cell (-1, -1) of copy 0 stays inside the wave's LDS");
    static_assert((ROW_WORDS + 2 * DESC_COPIES * DESC_CS) * 4 <= 5120, "32 waves per CU share 160 KiB");
    static_assert(DESC_TAB64 <= 64, "one lane clears one word of the table");
    __shared__ __attribute__((aligned(16))) unsigned int s_lds[KP_NW][ROW_WORDS + 2 * DESC_COPIES * DESC_CS];
    const int     lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int     cpy = lane & (DESC_COPIES - 1);
    short*        rec = (short*)s_lds[wave];
    unsigned int* tab = s_lds[wave] + DESC_REC_WORDS;
    fix64*        hall = (fix64*)(s_lds[wave] + ROW_WORDS);
    /* 32-bit LDS addresses: the row records, the bit table, this lane's histogram copy -- as the float whose BITS are the
     * address, n * 2^-149 (the cell addresses are formed by FMAs on that grid: "ISA: weights" below); the lane's copy
     * number for the slot likewise, with the bias that keeps the slot sum positive */
    const unsigned int rbase32 = (unsigned int)(size_t)(lds_i16*)rec;
    const unsigned int tbase32 = (unsigned int)(size_t)(lds_u32*)tab;
    const float        hbasef = (float)(unsigned int)(size_t)(lds_fix64*)(hall + cpy * DESC_CS) * 0x1p-149f;
    const float        cpy8f = (float)((cpy << 3) + DESC_SLOT_BIAS) * 0x1p-149f;
    const int     total = min(ct->ori_total, desc_cap);
    /* rows and list positions per pass: DESC_MAXROWS and DESC_LISTCAP, or fewer when a test asks for it
     * (popsift_hip_debug_set DESC_ROWS / DESC_LIST) */
    const int     maxrows = min(max(sc.desc_rows, 4), DESC_MAXROWS);
    const int     maxlist = min(max(sc.desc_list, 64), DESC_LISTCAP);

    for (XcdSlice sl = xcd_slice<KP_NW>(); sl.more(total); sl.s += sl.step) {
        /* one descriptor per wave: its number is wave-uniform, and said to be, so that the record below is fetched
         * through the scalar cache */
        const int d = uniform(sl.index());
        if (d >= total) continue;
        /* ISA: record */
        /* everything about the descriptor is wave-uniform and was worked out by k_scan_apply (DescRec): three 16-byte
         * SCALAR loads (the taps become scalar-base + 32-bit-offset loads).  As vector loads of one address in all 64
         * lanes every word of the record cost a v_readfirstlane on its way to a scalar register, a dozen per descriptor
         * and a 64-bit vector address. */
        typedef unsigned int u4 __attribute__((ext_vector_type(4)));
        typedef __attribute__((address_space(4))) const u4 const_u4; /* written by an earlier kernel, never by this one */
        const_u4*          rp = (const_u4*)(size_t)(drec + d);
        const u4           q0 = rp[0], q1 = rp[1], q2 = rp[2];
        const float        x = __uint_as_float(q0.x), y = __uint_as_float(q0.y);
        const float        crsbp = __uint_as_float(q0.z), srsbp = __uint_as_float(q0.w);
        /* the keypoint orientation in bins enters the angle's last FMA as 2 - ang_bins (half_angle_bins) */
        const float        ang_k0 = 2.0f - __uint_as_float(q1.x);
        const float        inv_c = __uint_as_float(q1.y), inv_s = __uint_as_float(q2.w);
        const int          pmin = (int)q1.z, pmax = (int)q1.w;
        const unsigned int misc = q2.z;
        const int          pitch = (int)(misc & 0xffffu), fbits = (int)((misc >> 16) & 0xffu);
        const float*       layer = arena + (long long)(((unsigned long long)q2.y << 32) | q2.x);

        { /* ISA: clear */
            /* the zeros are made here, every time: left to itself the compiler keeps them alive across the whole sample
             * loop, which is the 65th vector register and up (a spill, and with it scratch set-up for every wave).
             * 16-byte stores (the histograms start on a 16-byte boundary, ROW_WORDS): five per lane where 8-byte stores
             * took nine */
            u4 zero;
            asm volatile("v_mov_b32 %0, 0\n\tv_mov_b32 %1, 0\n\tv_mov_b32 %2, 0\n\tv_mov_b32 %3, 0"
                         : "=v"(zero.x), "=v"(zero.y), "=v"(zero.z), "=v"(zero.w));
            constexpr int CLEAR16 = DESC_COPIES * DESC_CS / 2; /* 16-byte pieces of the histogram copies */
            static_assert(DESC_COPIES * DESC_CS % 2 == 0, "whole 16-byte pieces");
            u4*           h16 = reinterpret_cast<u4*>(hall);
#pragma unroll
            for (int k = 0; k < (CLEAR16 + 63) / 64; k++)
                if (lane + 64 * k < CLEAR16) h16[lane + 64 * k] = zero;
        }

        /* ISA: set-up */
        if (misc & (1u << 24)) { /* DESC_MAGNIFY * sigma != 0 */
            const int   xmin = (int)(short)(pmin & 0xffff), ymin0 = pmin >> 16;
            const int   xmax = (int)(short)(pmax & 0xffff), ymax = pmax >> 16;
            const int   wx = xmax - xmin + 1;
            const int   hy_all = ymax - ymin0 + 1;
            /* the Gaussian window weight comes out of v_exp already multiplied by the fixed-point scale 2^fbits */
            const float ffbits = (float)fbits;

            /* A patch is walked in passes of at most `maxrows` rows and `maxlist` list positions (the default
             * configuration's patches: up to 93 rows and 5200 positions, so the largest take two passes; the largest the
             * library accepts -- sigma0 = 2, two levels -- span 173 rows).  A pass starts at row rb, `skip` columns into
             * that row's interval: the row in which the list fills up is cut there and the next pass takes the rest of it.
             * The histogram sums are integers, so the split changes nothing. */
            for (int rb = 0, skip = 0; rb < hy_all && wx > 0;) {
            const int   ymin = ymin0 + rb;
            const int   hy = min(hy_all - rb, maxrows);
            /* ISA: clear */
            /* the row-end bits of the previous pass go (the first pass clears what the previous descriptor left) */
            if (lane < DESC_TAB64) ((unsigned long long*)tab)[lane] = 0ull;
            wave_lds_sync();

            /* ISA: spans */
            /* Row spans.  The samples that count lie in the square |u|,|v| < 2.5 (cell units, rotated
             * by ang), which fills only 1/(|cos|+|sin|)^2 = 50..100 % of its bounding box.  Per patch
             * row the square cuts out ONE column interval; the rows' intervals are laid end to end
             * (prefix sum) and the wave walks that flat list, so nearly every lane holds a sample
             * that passes the exact test below.  The intervals only have to be a superset of the
             * samples inside the square. */
            int T = 0, grow = 0, nrec = 0; /* list length; the first row that holds a sample; rows from there to the last */
            int rb_next = rb + hy, skip_next = 0; /* where the next pass starts */
            {
                int         carry = 0;
                for (int r0 = 0; r0 < hy; r0 += 64) {
                    const int r = r0 + lane;
                    int       len = 0, jlo = xmin;
                    if (r < hy) {
                        const float dy = (float)(ymin + r) - y;
                        const float a = srsbp * dy, b = crsbp * dy;
                        float       lo = -1e30f, hi = 1e30f;
                        bool        ok = true;
                        if (inv_c != 0.0f) { /* |crsbp*dx + a| < 2.5 */
                            const float t0 = (-2.5f - a) * inv_c, t1 = (2.5f - a) * inv_c;
                            lo = fminf(t0, t1);
                            hi = fmaxf(t0, t1);
                        } else {
                            ok = fabsf(a) < 2.5f;
                        }
                        if (inv_s != 0.0f) { /* |b - srsbp*dx| < 2.5 */
                            const float t0 = (b - 2.5f) * inv_s, t1 = (b + 2.5f) * inv_s;
                            lo = fmaxf(lo, fminf(t0, t1));
                            hi = fminf(hi, fmaxf(t0, t1));
                        } else {
                            ok = ok && (fabsf(b) < 2.5f);
                        }
                        /* columns j with lo < j - x < hi: floor(x + lo) + 1 .. ceil(x + hi) - 1, the ends moved out by 1e-3
                         * pixels -- a hundred times what the reciprocals and products above can be off by (a sample ON the
                         * edge |u| = 2.5 has weight zero in the cells that exist, so even a miss would be invisible).  Widening
                         * by a whole pixel on either side, as rounds 1 and 2 did, walked two samples per row for nothing:
                         * 5 % of the list (k_descriptor 370 -> 352 us, timed loop + 1.4 %). */
                        jlo = max(xmin, (int)floorf(x + lo - 1e-3f) + 1);
                        const int jhi = min(xmax, (int)ceilf(x + hi + 1e-3f) - 1);
                        len = ok ? max(jhi - jlo + 1, 0) : 0;
                        /* the pass's first row: what the previous pass took of it */
                        if (r == 0) {
                            const int s = min(skip, len);
                            jlo += s;
                            len -= s;
                        }
                        if (len == 0) jlo = xmin;
                    }
                    /* In exact geometry the rows that hold a sample are contiguous.  The bit count below is a row INDEX only
                     * if they are, so a row without a sample below the first one that has some gets one position (column
                     * xmin: inside the image, outside the square -- the exact test drops it). */
                    const unsigned long long live = __ballot(len > 0);
                    bool                     below = carry > 0;
                    if (carry == 0 && live != 0ull) {
                        const int first = __ffsll((long long)live) - 1;
                        grow = r0 + first;
                        below = lane > first;
                    }
                    if (below && r < hy && len == 0) len = 1;
                    const int incl = wave_incl_scan(len);
                    const int start = carry + incl - len;
                    /* the list is full: the first row that ends beyond `maxlist` is cut there, the rows below it wait for the
                     * next pass (the prefix sum never falls, so they are the lanes above) */
                    const unsigned long long over = __ballot(carry + incl > maxlist);
                    if (over != 0ull) {
                        const int cut = __ffsll((long long)over) - 1;
                        if (lane == cut) len = maxlist - start;
                        if (lane > cut) len = 0;
                        rb_next = rb + r0 + cut;
                        skip_next = __builtin_amdgcn_readlane(len, cut) + ((r0 + cut == 0) ? skip : 0);
                    }
                    if (len > 0) {
                        const int last = start + len - 1;
                        rec[r - grow] = (short)((jlo - xmin) - start);
                        __hip_atomic_fetch_or((lds_u32*)(size_t)(tbase32 + 4u * (unsigned int)(last >> 5)), 1u << (last & 31),
                                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                    const unsigned long long kept = __ballot(len > 0);
                    if (kept != 0ull) nrec = r0 + 64 - __builtin_clzll(kept) - grow;
                    if (over != 0ull) {
                        carry = maxlist;
                        break;
                    }
                    carry += __builtin_amdgcn_readlane(incl, 63);
                }
                T = carry;
                /* A sentinel closes the records: a flat index at or beyond T has all the pass's bits below it, so it ends up
                 * in the "row" after the last at column -32767 -- a sample far outside the patch, which the in-square test
                 * drops (its taps are read inside the plane: at the byte offset of that column where it is positive, at
                 * offset 0 of the patch where not -- the negative offset saturates in the conversion).  So no index needs
                 * clamping and no lane needs a "past the end" flag. */
                if (lane == 0) rec[nrec] = -32767;
            }
            wave_lds_sync();

            /* ISA: set-up */
            /* steps of 64 list positions, exactly: the last one may be partial (what lies beyond the list's end drops out by
             * itself, above), none is empty */
#ifdef DESC_PROBE_NOLOOP
            const int   steps = 0;
#else
            const int   steps = (T + 63) >> 6;
#endif
            /* The wave's place in the row-end bits, all wave-uniform: the word of the step whose coordinates come next
             * (read one step ahead, with the taps, so no coord() waits for it), the LDS address of the word after it, and the
             * rows that end before that step -- counted from the top of the PATCH, so that the count plus the bits below
             * the lane is the lane's patch row; the records are addressed from row 0 of the patch to match. */
            unsigned long long rmask = *(const unsigned long long*)tab;
            unsigned int       rnext = tbase32 + 8u;
            unsigned int       rows_done = (unsigned int)(rb + grow);
            const unsigned int rec0 = rbase32 - 2u * (unsigned int)(rb + grow);

            /* Sample (row r, column c), both counted from the corner (ymin0, xmin) of the PATCH (so that the arithmetic does not
             * depend on how the patch is cut into passes): cell-unit position
             *   u = crsbp * (xmin + c - x) + srsbp * (ymin0 + r - y),  v = crsbp * (ymin0 + r - y) - srsbp * (xmin + c - x)
             * (n = u - off, dn = n + off = u, s_desc_loop.cu:88-99) as two FMAs each on the small integers c and r; the
             * keypoint's offset from the patch corner is wave-uniform and goes into u0 / v0.  The taps are addressed from the
             * patch corner, so the element offset is r * pitch + c. */
            const float  ox = (float)xmin - x, oy = (float)ymin0 - y;
            const float  u0 = fmaf(crsbp, ox, srsbp * oy), v0 = fmaf(crsbp, oy, -srsbp * ox);
            const float* corner = layer + (size_t)(ymin0 * pitch + xmin);
            const float  pitch4f = (float)(4 * pitch);

            /* Two-stage software pipeline: the coordinates of the lane's next sample are computed and its four
             * gradient taps requested while the current one is being binned, so the L2 round trip of the taps
             * overlaps the arithmetic.  The loads are unconditional (in-bounds for every span position) to
             * keep the vmcnt waits counted.
             * What an instruction costs decides the form of everything below (tools/ubench/valu_rate.hip, MI355X): f32
             * add / mul / FMA, 32-bit add / and / xor / arithmetic shift issue at twice the rate of compares, selects,
             * conversions, floor, min / max, shifts-with-add and 24-bit multiplies.  So row and column enter as floats
             * (one conversion each), and the byte offset of the taps is one FMA -- exact:
             * 4 * (row * pitch + column) < 2^24 -- and one conversion, instead of a 24-bit multiply and a shift-add. */
            /* Patch row and column of the lane's position in the step that comes next (the steps are taken in order, so the
             * word and the count move on): the rows that end before the step's 64 positions plus those that end below the
             * lane inside them give the row, its record the column.  `ahead` is where the word after this step's lies from
             * rnext (which the callers move on: the double step once for both its halves). */
            auto coord = [&](int i, unsigned int ahead, unsigned int& off, float& u, float& v) { /* ISA: coordinates */
                const unsigned int lo = (unsigned int)rmask, hi = (unsigned int)(rmask >> 32);
                const unsigned int row = __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, rows_done));
                /* rows_done += popcount(word): the instruction adds as it counts (the compiler forms count, count, add) */
                asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(rows_done) : "v"(lo));
                asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(rows_done) : "v"(hi));
                rmask = *(lds_u64*)(size_t)(rnext + ahead);
                const int   rcd = *(lds_i16*)(size_t)(rec0 + 2u * row);
                const float fr = (float)row;
                const float fc = (float)(i + rcd);
                u = fmaf(crsbp, fc, fmaf(srsbp, fr, u0));
                v = fmaf(crsbp, fr, fmaf(-srsbp, fc, v0));
                /* the end-of-list sentinel (column -32767 of a row that does not exist) can make this sum negative, and the
                 * lane must then read offset 0: v_cvt_u32_f32 saturates a negative input to 0 by definition, whereas the
                 * C++ cast of an out-of-range float is undefined (fptoui poison) -- so the instruction is named, as for
                 * v_cvt_rpi_i32_f32 in k_orientation */
                asm("v_cvt_u32_f32 %0, %1" : "=v"(off) : "v"(fmaf(fr, pitch4f, fc * 4.0f)));
            };
            /* ISA: control */
            /* one sample: gradient (gx, gy) at cell-unit position (u, v) -> up to four 64-bit LDS atomics */
            unsigned int probe_acc = 0u; /* DESC_PROBE_NOATOMIC only */
            auto bin = [&](float u, float v, float gx, float gy) {
                if (fabsf(u) < 2.5f && fabsf(v) < 2.5f) { /* ISA: control */
                    /* ISA: magnitude + angle */
                    const float  mod = __builtin_amdgcn_sqrtf(fmaf(gx, gx, gy * gy));
                    /* exp(-(u^2+v^2)/8) * 2^fbits = 2^(fbits - (u^2+v^2) * log2(e)/8) */
                    const float  wm = __builtin_amdgcn_exp2f(fmaf(-0.18033688011112042f, fmaf(u, u, v * v), ffbits)) * mod;
                    /* gradient angle relative to the keypoint orientation in units of one bin; any multiple of 8 may be
                     * missing: floor / fraction / (& 7) below do not care */
                    const float tth = half_angle_bins(gy, gx, mod, 1.0f, ang_k0);
                    const float ffo = floorf(tth);
                    const float do0 = tth - ffo;

                    /* ISA: weights */
                    /* cell centres sit at integer tu, tv in 0..3; the sample feeds cells
                     * (cx0, cx0+1) x (cy0, cy0+1) with weights (1-fx, fx) x (1-fy, fy)
                     * -- the (1-|n.x|)(1-|n.y|) of s_desc_loop.cu:100-102 -- where inside 0..3 */
                    const float tu = u + 1.5f, tv = v + 1.5f;
                    const float fcx = floorf(tu), fcy = floorf(tv);
                    const float fx = tu - fcx, fy = tv - fcy;
                    /* The histogram words are read from the bits of products on the 2^-149 grid (PS_CELL): the bin shares
                     * carry 2^-100 and the column weights 2^-49, every one of them a normal float.  A power of two commutes
                     * with the rounding, so w0 is RN(1 - do0) * 2^-100 and wx0 is RN(1 - fx) * 2^-49 exactly. */
                    const float wy0 = (1.0f - fy) * wm, wy1 = fy * wm;
                    const float wx0 = fmaf(-fx, 0x1p-49f, 0x1p-49f), fxs = fx * 0x1p-49f;
                    const float w0 = fmaf(-do0, 0x1p-100f, 0x1p-100f), do0s = do0 * 0x1p-100f;
                    /* Byte addresses of the four words: one base, the slot of the even and of the odd cell column, immediate
                     * offsets for the neighbours.  Slot of the lower bin: (bin + copy + 4 * (cx0 & 1)) mod 8 -- 4 * cx0 does
                     * for 4 * (cx0 & 1) under the mask, and the bin needs no mask of its own.  Cell indices and the bin are
                     * small integers held in floats (the floors above), so both addresses are two FMAs each and NO
                     * conversion: for an integer 0 <= n < 2^24 the float n * 2^-149 has the bit pattern n (the denormals
                     * and the first normal binade are one linear grid), so with the constants scaled by 2^-149 -- 8, 32 and
                     * 64 of them are inline integer operands -- the exact sum leaves the integer in the result's bits.
                     * Three conditions: f32 denormals are preserved (the kernels' mode; never a flush-denormals build,
                     * csrc/Makefile), the sum is below 2^24 (an LDS address; a slot sum below 1024), and it is not
                     * negative (cb: ROW_WORDS * 4 >= 352 above; s0: DESC_SLOT_BIAS). */
                    const unsigned int s0 = __float_as_uint(fmaf(fcx, 0x1p-144f, fmaf(ffo, 0x1p-146f, cpy8f))) & 56u;
                    const unsigned int cb = __float_as_uint(fmaf(fcy, (float)(DESC_RS * 8) * 0x1p-149f, fmaf(fcx, 0x1p-143f, hbasef)));
                    const unsigned int e0 = cb + s0;
                    const unsigned int e1 = (s0 ^ 32u) + cb;
                    /* A cell that does not exist (column / row -1 or 4) is skipped by the exec mask of its atomic -- the four
                     * compares below ARE the existence tests; its weight is not zeroed first, and no weight is tested against
                     * zero (an add of zero is harmless): four compares per sample where there were eight and four selects. */
                    const bool x0 = tu >= 0.0f, x1 = tu < 3.0f, y0 = tv >= 0.0f, y1 = tv < 3.0f;
/* ISA: atomics */
/* round(w * wgt) for both halves of the word is ONE multiply each: w carries 2^-100 and wgt 2^-49 (above), the product's
 * exact value is p * 2^-149 with p = w * wgt unscaled, and the hardware rounds it to the float grid there, whose step
 * is 2^-149 up to 2^-125 -- to the nearest integer p, ties to even, the integer being the result's bit pattern.  The same
 * three conditions as for the addresses: denormals preserved; p < 2^24 (make_desc_rec keeps fbits <= 14: a sample weighs
 * at most 361 * 2^14 < 2^23); no negative operand (w0, do0s in [0, 2^-100], wgt a product of weights in [0, 1], the
 * window and |g|).  Where wgt itself goes denormal and loses bits, p is below 2^-126 * 2^-100 * 2^149 = 2^-77: 0 either
 * way.  Rounds as fma(w, wgt, 2^23) & 0x7fffff did (tests/test_desc_words.py), without the FMA's addend and the AND. */
/* timing probes (results invalid): DESC_PROBE_NOATOMIC folds the words into a register instead of adding them to the LDS
 * histogram, DESC_PROBE_NOLOAD takes the taps from registers instead of memory (tools/build_variants.py) */
#ifdef DESC_PROBE_NOATOMIC
#define PS_CELL_ADD(ADDR, LO, HI) probe_acc ^= (LO) ^ (HI) ^ (ADDR);
#else
#define PS_CELL_ADD(ADDR, LO, HI)                                                                             \
    __hip_atomic_fetch_add((lds_fix64*)(size_t)(ADDR), ((fix64)(HI) << 32) | (fix64)(LO), __ATOMIC_RELAXED,    \
                           __HIP_MEMORY_SCOPE_WORKGROUP);
#endif
#define PS_CELL(ADDR, WGT)                                                                                     \
    {                                                                                                          \
        const float        wgt = (WGT);                                                                        \
        const unsigned int lo = __float_as_uint(w0 * wgt);                                                     \
        const unsigned int hi = __float_as_uint(do0s * wgt);                                                   \
        PS_CELL_ADD(ADDR, lo, hi)                                                                              \
    }
                    if (y0) {
                        if (x0) PS_CELL(e0, wy0 * wx0)
                        if (x1) PS_CELL(e1 + 64u, wy0 * fxs)
                    }
                    if (y1) {
                        if (x0) PS_CELL(e0 + DESC_RS * 8u, wy1 * wx0)
                        if (x1) PS_CELL(e1 + DESC_RS * 8u + 64u, wy1 * fxs)
                    }
#undef PS_CELL
#undef PS_CELL_ADD
                }
            };
            /* ISA: control */
            /* two register sets take turns as "being binned" and "in flight" (the loop is unrolled by two so that no
             * value has to be copied from one role to the other) */
            unsigned int off_a = 0, off_b = 0;
            float u_a = 3.0f, v_a = 3.0f, a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
            float u_b = 3.0f, v_b = 3.0f, b0 = 0.0f, b1 = 0.0f, b2 = 0.0f, b3 = 0.0f;
            const Taps taps(corner, pitch);
#ifdef DESC_PROBE_NOLOAD
#define PS_TAPS(OFF, A0, A1, A2, A3) { A0 = __uint_as_float(OFF) * 1e-9f; A1 = u0; A2 = v0; A3 = __uint_as_float((OFF) ^ 0x3f800000u); }
#else
#define PS_TAPS(OFF, A0, A1, A2, A3) taps.load_b(OFF, A0, A1, A2, A3);
#endif
            if (T > 0) {
                coord(lane, 0u, off_a, u_a, v_a);
                rnext += 8u;
                PS_TAPS(off_a, a0, a1, a2, a3)
            }
            /* double steps while a further step follows them: only then is the set requested at the end ever binned */
            int t = steps, i = lane;
            for (; t > 2; t -= 2, i += 128) {
                coord(i + 64, 0u, off_b, u_b, v_b);
                PS_TAPS(off_b, b0, b1, b2, b3)
                bin(u_a, v_a, a0 - a1, a2 - a3);
                coord(i + 128, 8u, off_a, u_a, v_a);
                PS_TAPS(off_a, a0, a1, a2, a3)
                bin(u_b, v_b, b0 - b1, b2 - b3);
                rnext += 16u;
            }
            /* the last one or two steps (wave-uniform branches): nothing is requested beyond the list's last step, and a
             * step that holds no sample is not walked -- rounding the list up to whole double steps walked 64 empty
             * positions per descriptor on average, coordinates, row lookup and four tap loads each */
            if (t == 2) {
                coord(i + 64, 0u, off_b, u_b, v_b);
                PS_TAPS(off_b, b0, b1, b2, b3)
            }
            if (t > 0) bin(u_a, v_a, a0 - a1, a2 - a3);
            if (t == 2) bin(u_b, v_b, b0 - b1, b2 - b3);
            if (probe_acc == 0x12345u) desc[(size_t)d * 128 + lane] = 1.0f; /* never true: keeps the probe's arithmetic alive */
            wave_lds_sync(); /* ISA: end */
            rb = rb_next;
            skip = skip_next;
            } /* passes */
        }
        wave_lds_sync();

        /* ISA: read-out */
        /* bin b of cell (iy, ix) = low half of that cell's word for b + high half of its word for b-1 (mod 8),
         * summed over the copies; word positions as in the header comment.  The eight halves of a bin are read as 32-bit
         * words and summed in 32 bits: the samples behind the low halves (lower bin b) and behind the high halves (lower
         * bin b-1) are different samples of the same cell, each adds at most its weight plus the half unit of its
         * rounding, and all the samples of a cell together weigh at most 361 * cell_px * 2^fbits <= 2^31 (make_desc_rec,
         * the bound that keeps a low half from carrying), so a bin is below 2^31 + cell_px / 2 < 2^32.  One v_cvt_f32_u32
         * then rounds the same integer to the same float as the 64-bit sum's conversion did, which took two carry adds
         * per term and a normalise-and-round sequence of nineteen instructions per descriptor. */
        unsigned int a0 = 0u, a1 = 0u;
        {
            /* element lane: bin b of cell (iyl, ix), element lane + 64: of cell (iyl + 2, ix).  Copy k keeps the bin in slot
             * (t + k) & 7 and the bin below it in the slot before: five slot addresses in all, everything else -- the copy,
             * the two cell rows, the high half -- is an immediate offset of the read */
            const int          b = lane & 7, ix = (lane >> 3) & 3, iyl = lane >> 5;
            const int          t = b + ((ix & 1) << 2);
            const unsigned int cell = (unsigned int)(size_t)(lds_fix64*)hall + 8u * (unsigned int)(iyl * DESC_RS + ix * 8);
            unsigned int       slot[DESC_COPIES + 1];
#pragma unroll
            for (int j = 0; j <= DESC_COPIES; j++) slot[j] = cell + 8u * (unsigned int)((t + j + 7) & 7);
#pragma unroll
            for (int k = 0; k < DESC_COPIES; k++) {
                constexpr unsigned int ROW2 = 2u * DESC_RS * 8u;
                const unsigned int     cp = (unsigned int)k * DESC_CS * 8u;
                a0 += *(lds_u32*)(size_t)(slot[k + 1] + cp) + *(lds_u32*)(size_t)(slot[k] + cp + 4u);
                a1 += *(lds_u32*)(size_t)(slot[k + 1] + cp + ROW2) + *(lds_u32*)(size_t)(slot[k] + cp + ROW2 + 4u);
            }
        }
        /* ISA: u32 to f32 */
        const float inv_scale = scalbnf(1.0f, -fbits);
        float       v0 = (float)a0 * inv_scale, v1 = (float)a1 * inv_scale;

        /* ISA: normalise + store */
        /* normalisation (s_desc_norm_rs.h:44-79, s_desc_norm_l2.h:87-134), whole wave.  The reference's RootSift is
         * __fsqrt_rn(__fdividef(v, sum)) and its L2 norms are __fsqrt_rn / __frsqrt_rn: an approximate quotient under
         * correctly rounded roots.  Here the quotient is the hardware reciprocal (1 ulp, like __fdividef's 2 ulp) and the
         * roots are v_sqrt_f32 / v_rsq_f32: 1 ulp where the reference rounds correctly, and a denormal quotient (a bin
         * below 1e-38 of the sum) comes out as 0 -- a divergence of one unit in the last place of single bins, seven orders
         * below the 1e-3 bar, recorded in DESIGN 4.  It replaced 50 instructions per descriptor; the version with sqrtf
         * and "/" is normalize_store (desc_modes.hip). */
        if (sc.norm_mode == POPSIFT_HIP_NORM_ROOTSIFT) {
            float sum = v0 + v1;
            sum = wave_allsum(sum);
            const float rs = __builtin_amdgcn_rcpf(sum);
            v0 = scalbnf(__builtin_amdgcn_sqrtf(v0 * rs), sc.norm_multi);
            v1 = scalbnf(__builtin_amdgcn_sqrtf(v1 * rs), sc.norm_multi);
        } else {
            float sq = v0 * v0 + v1 * v1;
            sq = wave_allsum(sq);
            const float norm = __builtin_amdgcn_sqrtf(sq);
            v0 = fminf(v0, 0.2f * norm);
            v1 = fminf(v1, 0.2f * norm);
            sq = v0 * v0 + v1 * v1;
            sq = wave_allsum(sq);
            const float rn = scalbnf(__builtin_amdgcn_rsqf(sq), sc.norm_multi);
            v0 = v0 * rn;
            v1 = v1 * rn;
        }
        desc[(size_t)d * 128 + lane] = v0;
        desc[(size_t)d * 128 + 64 + lane] = v1;
        wave_lds_sync(); /* ISA: end */
    }
}

}  // namespace

hipError_t launch_orientation(const PyrDesc* pd, const BatchDesc& bd, int nb, const SiftConsts& sc, bool filtered, int hist_cap,
                              int blocks, hipStream_t s)
{
    /* `blocks` waves are eight per wave slot of the device, sized for kernels that take one list entry per position; a
     * position here is a group of KP_GROUP entries, so an eighth of them (one per slot, a multiple of 8 for the XCDs) */
    const int waves = std::max(blocks / 8 / (8 * KP_NW) * (8 * KP_NW), 8 * KP_NW);
    hipLaunchKernelGGL(k_orientation, dim3(waves / KP_NW, nb), dim3(64 * KP_NW), 0, s, pd, bd, sc, filtered ? 1 : 0, hist_cap);
    return hipGetLastError();
}

hipError_t launch_scan_apply(const PyrDesc* pd, const BatchDesc& bd, int nb, const SiftConsts& sc, int n_chunks, int desc_cap,
                             hipStream_t s)
{
    /* n_chunks is the capacity of the lists; a 1080p image fills ~300 chunks */
    hipLaunchKernelGGL(k_scan_apply, dim3(std::min(n_chunks, 1024), nb), dim3(256), 0, s, pd, sc, bd,
                       sc.desc_mode == POPSIFT_HIP_DESC_LOOP ? 1 : 0, desc_cap);
    return hipGetLastError();
}

int scan_chunk() { return SCAN_CHUNK; }
int scan_partials_per_chunk() { return SCAN_SUB; }

hipError_t launch_descriptors(const PyrDesc* pd, const BatchDesc& bd, int nb, const SiftConsts& sc, int desc_cap, int blocks,
                              hipStream_t s)
{
    if (sc.desc_mode == POPSIFT_HIP_DESC_NOTILE || sc.desc_mode == POPSIFT_HIP_DESC_IGRID ||
        sc.desc_mode == POPSIFT_HIP_DESC_ILOOP || sc.desc_mode == POPSIFT_HIP_DESC_GRID)
        return launch_desc_modes(pd, bd, nb, sc, desc_cap, blocks, s);
    hipLaunchKernelGGL(k_descriptor, dim3(blocks / KP_NW, nb), dim3(64 * KP_NW), 0, s, bd, sc, desc_cap);
    return hipGetLastError();
}

}  // namespace popsift_hip
