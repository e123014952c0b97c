/*
 * desc_bytes.hip -- descriptors as bytes (popsift_hip_fetch*_u8, popsift_hip_devfeatures_download_u8).
 *
 *   k_desc_bytes  one streaming pass over a descriptor slab: every float d becomes
 *                     q(d) = 0 if d is NaN or d <= 0, 255 if d >= 255, (uint8_t)roundf(d) otherwise
 *                 (write_as_uchar's roundf -- ties away from zero -- saturated to a byte, Feature::print).  One lane
 *                 reads 16 floats (four dwordx4 loads) and writes their 16 bytes with one dwordx4 store; the grid is
 *                 capped and strides over the rest.
 *
 * A separate pass on purpose: the descriptor kernels are register-bound, and the bytes are wanted only by the callers
 * who ask for them.  Memory-bound: 4 bytes in, 1 byte out per element.
 */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"

namespace popsift_hip {
namespace {

constexpr int DB_THREADS = 256;
constexpr int DB_MAX_BLOCKS = 2048; /* 8 workgroups of 256 lanes per CU of the device; larger slabs grid-stride */

/* !(d > 0) takes NaN, -0.0 and the negatives; roundf rounds ties away from zero, as write_as_uchar does */
__device__ __forceinline__ unsigned q8(float d)
{
    if (!(d > 0.0f)) return 0u;
    if (d >= 255.0f) return 255u;
    return (unsigned)roundf(d);
}

__device__ __forceinline__ unsigned pack4(float4 v)
{
    return q8(v.x) | (q8(v.y) << 8) | (q8(v.z) << 16) | (q8(v.w) << 24);
}

/* n16: groups of 16 floats (8 per descriptor) */
__global__ void __launch_bounds__(DB_THREADS) k_desc_bytes(const float4* __restrict__ in, uint4* __restrict__ out,
                                                           size_t n16)
{
    const size_t stride = (size_t)gridDim.x * DB_THREADS;
    for (size_t i = (size_t)blockIdx.x * DB_THREADS + threadIdx.x; i < n16; i += stride) {
        const float4* p = in + 4 * i;
        const float4  a = p[0], b = p[1], c = p[2], d = p[3];
        out[i] = make_uint4(pack4(a), pack4(b), pack4(c), pack4(d));
    }
}

}  // namespace

hipError_t launch_desc_bytes(const float* desc, int n_desc, uint8_t* out, hipStream_t s)
{
    if (n_desc <= 0) return hipSuccess;
    const size_t n16 = (size_t)n_desc * 128 / 16;
    const size_t want = (n16 + DB_THREADS - 1) / DB_THREADS;
    const int    blocks = (int)std::min<size_t>(want, DB_MAX_BLOCKS);
    hipLaunchKernelGGL(k_desc_bytes, dim3(blocks), dim3(DB_THREADS), 0, s, (const float4*)desc, (uint4*)out, n16);
    return hipGetLastError();
}

}  // namespace popsift_hip
