/* dog_view.h -- how a kernel reads one DoG value of an octave (device code, internal): k_refine (extrema.hip) and the
 * response kernel of the keep-strongest pass (strongest.hip) go through the same view, so that both see the same value
 * whether the DoG planes are stored or formed on the fly. */
#pragma once
#include <hip/hip_runtime.h>

#include "wave_dev.h"

namespace popsift_hip {

/* The float at byte offset `b` behind a wave-uniform `base`.  With an UNSIGNED 32-bit offset the load takes the
 * scalar-base + vector-offset form and costs no vector instruction; with a 64-bit offset every load pays a 64-bit
 * vector add of its own.  An arena is below 4 GiB (ctx.hip refuses a larger one). */
__device__ __forceinline__ float ld_b(const char* base, unsigned int b) { return *(const float*)(base + (size_t)b); }

template <bool FLY>
struct DogView {
    const char*  arena; /* wave-uniform; the lanes' candidates may be of different octaves, so everything else is per lane */
    unsigned int off;   /* first float of the octave's stored DoG planes, or (fly) of its Gaussian planes: DoG(z) =
                         * G(z+1) - G(z), the subtraction make_dog does (s_pyramid_build.cu:74-92) on the very same f32
                         * values.  Float indices into an arena below 4 GiB: 30 bits, and their byte offsets 32. */
    unsigned int ps;
    int          w, h, pitch, nl; /* nl = number of DoG planes */
    /* byte offset of float i.  The empty asm keeps it a 32-bit value defined in the block of its load: where the
     * compiler merges the loads of two branches or moves an address out of refine()'s loop, it widens the offset to
     * 64 bits away from the load and the scalar-base form is lost. */
    __device__ __forceinline__ unsigned int byte_off(unsigned int i) const
    {
        unsigned int b = 4u * i;
        asm volatile("" : "+v"(b));
        return b;
    }
    __device__ __forceinline__ float el(unsigned int i) const { return ld_b(arena, byte_off(i)); }
    __device__ __forceinline__ float raw(int x, int y, int z) const /* caller guarantees 0<=x<w, 0<=y<h, 0<=z<nl */
    {
        const unsigned int i = off + (unsigned int)z * ps + (unsigned int)y * (unsigned int)pitch + (unsigned int)x;
        return FLY ? el(i + ps) - el(i) : el(i);
    }
    __device__ __forceinline__ float at(int x, int y, int z) const
    {
        return raw(clampi(x, 0, w - 1), clampi(y, 0, h - 1), clampi(z, 0, nl - 1));
    }
};

}  // namespace popsift_hip
