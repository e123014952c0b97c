/* blur_common.h -- small device helpers shared by the blur kernels (pyramid.hip, blur_march.hip, pyr_direct.hip,
 * pyr_tail.hip). Internal. */
#pragma once
#include <hip/hip_runtime.h>

#include "wave_dev.h"

namespace popsift_hip {

constexpr int BLUR_TW = 128; /* tile / strip width (outputs) */

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));

/* One axis of a CUDA linear-filter fetch at normalised coordinate r
 * (s_image.cu:140-169: normalised coords, clamp, linear, 1.8 fixed-point weight). */
__device__ __forceinline__ void lin_coord(float r, int n, int& i0, float& alpha)
{
    const float xb = r * (float)n - 0.5f;
    const float fl = floorf(xb);
    float       a = xb - fl;
    a = floorf(a * 256.0f + 0.5f) * (1.0f / 256.0f);
    i0 = (int)fl;
    alpha = a;
}

/* Workgroup barrier that waits for this wave's LDS operations only: vector-memory loads and stores stay in flight
 * (__syncthreads() drains them -- in pyr_tail.hip ~1.5 us of write latency at each of the four barriers of a level,
 * 65 instead of 25 us for the tail of a 1080p image). */
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

/* XCD-aware tile order: blocks b and b+8 share an XCD (and its 4 MiB L2), so
 * give each XCD a contiguous run of tiles -- neighbouring tiles share halos. */
__device__ __forceinline__ int xcd_remap(int b, int n)
{
    const int q = n >> 3, r = n & 7, xcd = b & 7, k = b >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
}

}  // namespace popsift_hip
