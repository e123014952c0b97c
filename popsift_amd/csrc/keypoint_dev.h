/*
 * keypoint_dev.h -- device helpers shared by the orientation / scan / loop-descriptor kernels (keypoint.hip) and the
 * other descriptor modes (desc_modes.hip): fixed-point histogram words, the float sum over a wave, the distribution of
 * keypoints over workgroups (KP_CHUNK), the accurate arctangent.  Wave-uniform values and the integer wave primitives
 * are in wave_dev.h.
 */
#pragma once
#include <hip/hip_runtime.h>

#include "wave_dev.h"

namespace popsift_hip {

/* sift_constants.h:22-29: float constants */
constexpr float F_PI = 3.14159265358979323846f;
constexpr float F_PI2 = 2.0f * 3.14159265358979323846f;
constexpr float DESC_MAGNIFY = 3.0f;

/*
 * Histogram accumulation: on gfx950 an LDS float atomic add (ds_add_f32) costs
 * ~200 cycles per wave instruction whatever the address pattern, an integer one
 * ~6 (tools/ubench/lds_atomic.hip).  Bins are therefore 64-bit fixed point
 * (2^-32 resolution, exact and order-independent sums => bit-reproducible
 * histograms, unlike the reference's float atomicAdd, s_orientation.cu:136).
 */
typedef unsigned long long fix64;
/* one sample weighs < 2^11 (|gradient| <= 255*2*sqrt2, window weights <= 1): w * 2^20 fits 32 bits */
__device__ __forceinline__ float from_fix(fix64 v) { return (float)((double)v * (1.0 / 1048576.0)); }

__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

/* The sum over the 64 lanes, in every lane: four DPP adds inside the rows of 16 (quad butterflies, then the two mirrors),
 * the four row sums through scalar registers.  Register to register -- six __shfl_xor are six dependent ds_bpermute round
 * trips through the LDS queue (~150 cycles each behind whatever the wave has queued there), three times per descriptor
 * with the L2 normalisation.  A fixed order of additions like the butterfly's, so results stay reproducible. */
__device__ __forceinline__ float wave_allsum(float v)
{
#define PS_DPP_ADD(CTRL) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false))
    PS_DPP_ADD(0xB1);  /* quad_perm [1,0,3,2] */
    PS_DPP_ADD(0x4E);  /* quad_perm [2,3,0,1] */
    PS_DPP_ADD(0x141); /* row_half_mirror     */
    PS_DPP_ADD(0x140); /* row_mirror          */
#undef PS_DPP_ADD
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return (r0 + r1) + (r2 + r3);
}

/* element `idx` >= 0 of a wave-uniform plane through an unsigned 32-bit byte offset (scalar base + vector offset) */
__device__ __forceinline__ float plane_at(const float* pl, int idx)
{
    return *(const float*)((const char*)pl + (size_t)((unsigned int)idx * 4u));
}

/*
 * Work distribution of the keypoint kernels.  Workgroups b and b + 8 share an XCD and its 4 MiB L2 (round-robin
 * dispatch -- relied on for speed only, never for correctness).  The lists come out of refinement grouped by image
 * region (extrema.hip: a detection sub-queue is a region, refinement appends one sub-queue batch at a time), so they
 * are cut into chunks of KP_CHUNK consecutive keypoints, chunk c goes to XCD c mod 8, and the workgroups of an XCD
 * walk its chunks front to back: the patches of the waves in flight on one XCD overlap, while every XCD still gets
 * the same mix of levels and octaves (the work per keypoint grows with sigma^2; handing each XCD one contiguous
 * eighth of a level-major list left the XCD with the coarse levels running 35 % longer than the others).
 * gridDim.x is a multiple of 8; NW = waves per workgroup.  Position s of XCD x is list element
 * ((s / KP_CHUNK) * 8 + x) * KP_CHUNK + s % KP_CHUNK.
 * (Tried and dropped, round 2: resident waves pulling positions from work queues in device memory -- one returning
 * atomicAdd per keypoint on 32 padded heads, next position requested ahead of time.  592 us against 505 us for the
 * descriptor kernel, 164 against 106 for orientation: the hardware dispatcher already balances 65536 single-wave
 * workgroups, and it does so without a memory round trip in the wave's in-order load queue.  Round 3 repeated it with
 * FEWER resident waves -- 8 .. 32 per CU, one counter per XCD, one descriptor / four histograms per fetch -- so that wave
 * slots, registers and LDS stay free for the other images' bandwidth-bound kernels: at 32 per CU it equals this
 * distribution (k_descriptor 421 us, 2.90 Gpix/s), at 24 / 16 / 12 / 8 it loses (2.89 / 2.77 / 2.58 / 2.47 Gpix/s), and
 * the level launches of the other images take as long in the mix as before (107 us against 108 us per octave-0 level,
 * profiles/r03_timeline_resident16.txt): what slows them beside a descriptor kernel is the shared vector issue, LDS and
 * L2, not the lack of a free slot.  DESIGN 6.4.)
 */
#ifndef KP_CHUNK
#define KP_CHUNK 256
#endif
/* k_orientation hands a wave KP_GROUP consecutive list entries at a time (it finds the peaks of their histograms together,
 * four lanes each): a position is then a GROUP of UNIT entries, a chunk holds KP_CHUNK / UNIT of them, and index() is the
 * group's first entry -- a multiple of UNIT inside the same chunk of the same XCD as with single entries, so what the
 * waves in flight on an XCD share stays what it was.  UNIT = 1: the descriptor kernels' one entry per position. */
constexpr int KP_GROUP = 16;
template <int UNIT>
struct XcdSliceOf {
    static constexpr int PER_CHUNK = KP_CHUNK / UNIT;
    static_assert(KP_CHUNK % UNIT == 0, "whole groups per chunk");
    int x, s, step;
    __device__ __forceinline__ int index() const { return ((s / PER_CHUNK) * 8 + x) * KP_CHUNK + (s % PER_CHUNK) * UNIT; }
    /* positions whose element lies beyond the list are skipped: later chunks of the same XCD may still be inside */
    __device__ __forceinline__ bool more(int total) const { return (s / PER_CHUNK) * 8 * KP_CHUNK < total; }
};
typedef XcdSliceOf<1> XcdSlice;
template <int NW, int UNIT = 1>
__device__ __forceinline__ XcdSliceOf<UNIT> xcd_slice()
{
    XcdSliceOf<UNIT> sl;
    sl.x = blockIdx.x & 7;
    /* the wave's number in its workgroup is wave-uniform, and said to be: position, list index and the loop over them
     * then stay in scalar registers (seven vector instructions per keypoint otherwise) */
    sl.s = (int)(blockIdx.x >> 3) * NW + uniform((int)(threadIdx.x >> 6));
    sl.step = (int)(gridDim.x >> 3) * NW;
    return sl;
}

/* atan2 for the HARD 36-bin orientation histogram (s_orientation.cu:129): needs libm-grade
 * accuracy, because an error of e rad moves a sample across a bin edge with probability
 * e / 0.1745.  Cephes atanf scheme (|error| ~ 1.5e-7 rad, about 1 ulp at pi/2 -- the level at
 * which device and host libm already disagree) with Newton-refined v_rcp quotients instead of
 * the ~12-instruction IEEE division sequence of the library routine.  Returns values in [-pi, pi]. */
__device__ __forceinline__ float div_nr(float a, float b)
{
    const float r = __builtin_amdgcn_rcpf(b);
    const float q = a * r;
    return fmaf(fmaf(-b, q, a), r, q);
}
__device__ __forceinline__ float atan2_acc(float y, float x)
{
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    float       a = (mx == 0.0f) ? 0.0f : div_nr(mn, mx);
    const bool  big = a > 0.4142135623730950f; /* tan(pi/8) */
    const float t = big ? div_nr(a - 1.0f, a + 1.0f) : a;
    const float z = t * t;
    const float p = fmaf(fmaf(fmaf(8.05374449538e-2f, z, -1.38776856032e-1f), z, 1.99777106478e-1f), z,
                         -3.33329491539e-1f);
    float       r = fmaf(p * z, t, t);
    r = big ? r + 0.7853981633974483f : r;
    r = (ay > ax) ? 1.5707963267948966f - r : r;
    r = (x < 0.0f) ? 3.14159265358979323846f - r : r;
    return (y < 0.0f) ? -r : r;
}

}  // namespace popsift_hip
