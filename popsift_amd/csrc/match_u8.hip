/*
 * match_u8.hip -- exact brute-force 2-NN of byte descriptors on the i8 matrix instructions
 * (popsift_hip_match_bytes, popsift_hip_match_pairs_bytes).
 *
 * The squared L2 distance of two byte descriptors is an integer <= 128 * 255^2 = 8 323 200 < 2^24: exact in i32 and exactly
 * representable in float.  One GEMM therefore gives the final answer -- no margin, no re-rank, no redo list (contrast
 * match_mfma.hip, which only screens for the float matcher).
 *
 *   sign        v_mfma_i32_32x32x32_i8 takes SIGNED bytes.  The distance is translation invariant, so the kernels work on
 *               x' = x - 128 = x ^ 0x80 and  d = |l'|^2 + |r'|^2 - 2 l'.r'  with |x'|^2 <= 2^21 and |l'.r'| <= 2^21: no
 *               overflow.  The sets store the caller's bytes; the flip is one v_xor per dword where an operand is loaded
 *               (16 per lane per right tile next to 16 MFMAs and ~100 epilogue instructions), which keeps download, the
 *               copy between GPUs and the row gather plain copies.
 *   k_norms_u8  |x'|^2 of every descriptor (int).
 *   k_match_u8  grid (ceil(l_len / 128), n_split), 256 lanes; the layout of k_match_screen: a wave owns 32 left
 *               descriptors as the B operand (index on the lane: col = lane & 31), the right set streams through LDS in
 *               tiles of 128 rows as the A operand (4 row blocks of 32).  K = 128 is four 32x32x32 steps; the 32 x 32
 *               accumulator tile gives each lane 16 right rows of ITS left descriptor, so the top-2 epilogue needs no
 *               cross-lane traffic.
 *   operand k   Which of a step's 32 k values a lane holds in which byte is not documented for i8, and an integer dot
 *               product does not care: it needs A and B to use the same assignment and to cover every k once.  Both hold by
 *               construction: a lane takes the 16 bytes at k_off(step, lane >> 5) of a descriptor for BOTH operands, and
 *               the eight (step, half) slices tile the 128 bytes.
 *   epilogue    per pair one v_mad (e = |r'|^2 - 2 dot; |l'|^2 is the same for all candidates of a lane and is added at the
 *               end) and its share of a min over the row block's 16 values; only when that minimum beats the lane's second
 *               best -- rare after the first tiles -- the 16 values are looked at one by one.  A lane meets its right rows
 *               in ascending index, so "ties go to the lower index" is a strict '<' there.
 *   k_top2_finish<int> (top2.h) merges the right-set splits under lexicographic (d, j) and writes popsift_hip_match rows.
 */
#include "devfeatures.h"
#include "kernels.h"
#include "top2.h"

namespace popsift_hip {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

/* U_LB left descriptors per workgroup: 32 per wave (the N dimension of its MFMA tiles); U_RB right descriptors per LDS
 * tile: 4 row blocks of 32 (the M dimension); U_NONE (top2.h): "no candidate yet" */
constexpr int U_ROW = 144;         /* bytes per LDS row: +16 keeps the rows of a ds_read_b128 group on distinct banks   */
constexpr int U_FAR = INT_MAX / 2; /* norm of a row past the end: U_FAR - 2 dot cannot overflow and beats no real row  */

/* x - 128 for the sixteen bytes of v, as signed bytes */
__device__ __forceinline__ v4i to_signed(v4i v)
{
    const int f = (int)0x80808080u;
    return v4i{v.x ^ f, v.y ^ f, v.z ^ f, v.w ^ f};
}

/* byte offset of the 16 k values lane half h holds in step s, for the A and the B operand alike */
__device__ __forceinline__ int k_off(int s, int h) { return 32 * s + 16 * h; }

__device__ __forceinline__ int sq_sum(int w)
{
    int s = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int x = ((w >> (8 * k)) & 255) - 128;
        s += x * x;
    }
    return s;
}

__global__ __launch_bounds__(256) void k_norms_u8(const uint8_t* __restrict__ desc, int n, int* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const v4i* p = (const v4i*)(desc + (size_t)i * 128);
    int        s = 0;
    for (int k = 0; k < 8; k++) {
        const v4i v = p[k];
        s += sq_sum(v.x) + sq_sum(v.y) + sq_sum(v.z) + sq_sum(v.w);
    }
    out[i] = s;
}

__global__ __launch_bounds__(256, 2) void k_match_u8(const uint8_t* __restrict__ ldesc, int l_len,
                                                     const int* __restrict__ lnorm, const uint8_t* __restrict__ rdesc,
                                                     int r_len, const int* __restrict__ rnorm, int n_split,
                                                     Top2<int>* __restrict__ partial)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_r[U_RB * U_ROW];
    __shared__ __attribute__((aligned(16))) int     s_rn[U_RB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int l = blockIdx.x * U_LB + wave * 32 + col;
    const int lc = min(l, l_len - 1); /* lanes past the end work on the last row and write nothing */

    /* B operand: this lane's four slices of its left descriptor, 16 registers for the whole sweep */
    v4i bl[4];
#pragma unroll
    for (int s = 0; s < 4; s++) bl[s] = to_signed(*(const v4i*)(ldesc + (size_t)lc * 128 + k_off(s, half)));

    /* e = |r'|^2 - 2 l'.r' of the lane's two best right rows so far */
    int e1 = U_NONE, e2 = U_NONE, j1 = 0, j2 = 0;

    const int n_tiles = (r_len + U_RB - 1) / U_RB;
    v4i       stage[4]; /* this lane's share of the next right tile (128 rows x 8 chunks of 16 bytes / 256 lanes) */
    int       stage_n = U_FAR;
    auto      fetch = [&](int tile) {
        const int r0 = tile * U_RB;
        /* unconditional, clamped loads (a load under a condition is waited for one by one); the data of rows past the
         * end is the last row's, their norm U_FAR */
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int c = tid + 256 * k, row = c >> 3, ch = c & 7;
            stage[k] = *(const v4i*)(rdesc + (size_t)min(r0 + row, r_len - 1) * 128 + 16 * ch);
        }
        const int rn = rnorm[min(r0 + (tid & (U_RB - 1)), r_len - 1)];
        stage_n = (r0 + (tid & (U_RB - 1)) < r_len) ? rn : U_FAR;
    };
    int tile = blockIdx.y;
    if (tile < n_tiles) fetch(tile);
    for (; tile < n_tiles; tile += n_split) {
        const int r0 = tile * U_RB;
        __syncthreads(); /* previous tile consumed */
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int c = tid + 256 * k, row = c >> 3, ch = c & 7;
            *(v4i*)(s_r + row * U_ROW + 16 * ch) = to_signed(stage[k]);
        }
        if (tid < U_RB) s_rn[tid] = stage_n;
        __syncthreads();
        if (tile + n_split < n_tiles) fetch(tile + n_split); /* in flight during the arithmetic */

        v16i acc[4];
#pragma unroll
        for (int m = 0; m < 4; m++)
#pragma unroll
            for (int v = 0; v < 16; v++) acc[m][v] = 0;
        const uint8_t* arow = s_r + col * U_ROW; /* A operand: row 32 m + col of the tile */
#pragma unroll
        for (int s = 0; s < 4; s++) {
            v4i a[4];
#pragma unroll
            for (int m = 0; m < 4; m++) a[m] = *(const v4i*)(arow + m * 32 * U_ROW + k_off(s, half));
#pragma unroll
            for (int m = 0; m < 4; m++) acc[m] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[m], bl[s], acc[m], 0, 0, 0);
        }
        /* C/D layout: column = lane & 31 (the left descriptor), row = (v & 3) + 8 (v >> 2) + 4 (lane >> 5) */
#pragma unroll
        for (int m = 0; m < 4; m++) {
            int e[16];
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const v4i rn = *(const v4i*)(s_rn + 32 * m + 8 * g + 4 * half);
                e[4 * g + 0] = rn.x - 2 * acc[m][4 * g + 0];
                e[4 * g + 1] = rn.y - 2 * acc[m][4 * g + 1];
                e[4 * g + 2] = rn.z - 2 * acc[m][4 * g + 2];
                e[4 * g + 3] = rn.w - 2 * acc[m][4 * g + 3];
            }
            int lo = e[0];
#pragma unroll
            for (int v = 1; v < 16; v++) lo = min(lo, e[v]);
            if (lo < e2) {
#pragma unroll
                for (int v = 0; v < 16; v++) { /* ascending right index */
                    const int j = r0 + 32 * m + (v & 3) + 8 * (v >> 2) + 4 * half;
                    if (e[v] < e2 && j < r_len) {
                        if (e[v] < e1) {
                            e2 = e1;
                            j2 = j1;
                            e1 = e[v];
                            j1 = j;
                        } else {
                            e2 = e[v];
                            j2 = j;
                        }
                    }
                }
            }
        }
    }
    const int ln = lnorm[lc];
    Top2<int> best{e1 == U_NONE ? U_NONE : e1 + ln, e2 == U_NONE ? U_NONE : e2 + ln, j1, j2};
    /* the two halves hold different right rows of the same left descriptor */
    const int od1 = __shfl_xor(best.v1, 32), od2 = __shfl_xor(best.v2, 32);
    const int oj1 = __shfl_xor(best.i1, 32), oj2 = __shfl_xor(best.i2, 32);
    top2_insert(best, od1, oj1);
    top2_insert(best, od2, oj2);
    if (half == 0 && l < l_len) partial[(size_t)l * n_split + blockIdx.y] = best;
}

}  // namespace

hipError_t launch_norms_u8(const uint8_t* desc, int n, int* out, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_norms_u8, dim3((n + 255) / 256), dim3(256), 0, s, desc, n, out);
    return hipGetLastError();
}

hipError_t launch_match_u8(const uint8_t* ldesc, int l_len, const int* lnorm, const uint8_t* rdesc, int r_len,
                           const int* rnorm, int n_split, void* partial, popsift_hip_match* out, hipStream_t s)
{
    if (l_len <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_match_u8, dim3((l_len + U_LB - 1) / U_LB, n_split), dim3(256), 0, s, ldesc, l_len, lnorm, rdesc, r_len,
                       rnorm, n_split, (Top2<int>*)partial);
    launch_top2_finish((const Top2<int>*)partial, l_len, n_split, out, nullptr, nullptr, 0, l_len, s);
    return hipGetLastError();
}

}  // namespace popsift_hip
