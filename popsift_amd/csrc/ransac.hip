/*
 * ransac.hip -- geometric verification of correspondences on the GPU (popsift_hip_ransac and popsift_hip_epipolar,
 * include/popsift_hip.h): T sampled hypotheses of a homography, an affine map or a fundamental matrix, each scored against
 * all n pairs, the best one's inlier mask.  The rules in the header define every operation; tests/ransac_ref.c and
 * tests/epipolar_ref.c restate them on the CPU and the results are equal as bytes.
 *
 *   k_ransac_bounds   bounding box of the finite coordinates, per column: integer max of order-preserving keys, so the
 *                     result does not depend on the reduction order
 *   k_ransac_models   one lane per hypothesis: sample, float64 solve in registers, denormalise, round to float32;
 *                     counts[t] = 0 for a model, -1 for none
 *   k_epipolar_models the same for a fundamental matrix: 8 pairs, the null vector of the 8 x 9 system by elimination with
 *                     complete pivoting, the closest rank-2 matrix by a Jacobi eigenvector, denormalise, scale
 *   k_ransac_score    the T x n part.  A workgroup takes S_CHUNK pairs (four per lane, in registers for the whole
 *                     sweep) and S_HYP hypotheses; a hypothesis' nine coefficients are wave-uniform loads; its count
 *                     comes from ballots, crosses the waves through LDS and is added to counts[t] by one integer atomic
 *                     per (chunk, hypothesis): integer sums do not depend on the order.  The inlier rule (transfer
 *                     error or Sampson distance) is a template parameter, here and in k_ransac_mask
 *   k_ransac_select   arg-max under (count, -t) in one workgroup, writes the result record
 *   k_ransac_mask     the winner's inlier bytes, four pairs per lane
 *   k_pair_points     (x, y, x', y') of descriptor pairs through the sets' descriptor -> feature maps
 *
 * popsift_hip_ransac_many runs the same five steps over many pair lists at once, through the same device functions
 * (transfer_hypothesis, epipolar_hypothesis, the two inlier rules, select_winner), so a list's bytes are those of the
 * per-list call:
 *
 *   k_many_bounds     the eight keys of every list, one workgroup per segment of a list
 *   k_many_models     one lane per (list, hypothesis)
 *   k_many_score      one lane per hypothesis, its model and its count in registers, over a segment's pairs, each pair a
 *                     wave-uniform 16-byte load: no ballot, no LDS, and a short list costs its own pairs only
 *   k_many_select     one workgroup per list
 *   k_many_mask       one lane and one byte per pair of a segment
 *
 * popsift_hip_refit, the least-squares refit of such a model on its inliers (tests/refit_ref.c), enqueues all its rounds up
 * front; a state record on the device carries the current model and a `done` flag between them:
 *
 *   k_refit_init        the state record from the caller's model
 *   k_refit_count       the inliers of one model, by ballots and one integer atomic per wave
 *   k_refit_accumulate  the terms of the normal equations over the current model's inliers in float64, summed as a
 *                       pairwise tree over the pair index up to one block of sums per chunk of 1024 pairs
 *   k_refit_solve       the rest of the tree over the chunks, then one lane solves and writes the round's candidate
 *   k_refit_decide      accept the candidate or stop
 *
 * Each numeric step has one text, used by the sampler's model kernels and by the refit: normalise (a pair), eliminate<R, NB>
 * (partial pivoting), null_vector<ROWS> (complete pivoting), rank2, denormalise_transfer, denormalise_fundamental and
 * round_model; all of them work on register arrays with compile-time indices.  Kind<> gives per kind the inlier rule, the
 * pairs per sample, the ints per sample row and the refit's sums.  On the host the two call bodies, run and run_refit,
 * share their frame: args_valid, Frame (the offsets both lay out alike), grow, upload and download.
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstring>
#include <memory>
#include <new>

#include "devfeatures.h"
#include "kernels.h"

namespace popsift_hip {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int S_BLOCK = 256;                       /* lanes of a k_ransac_score workgroup */
constexpr int S_PER_LANE = 4;                      /* pairs a lane keeps in registers */
constexpr int S_CHUNK = POPSIFT_HIP_RANSAC_CHUNK;  /* pairs per workgroup */
constexpr int S_HYP = POPSIFT_HIP_RANSAC_HYP_BLOCK; /* hypotheses per workgroup */
static_assert(S_CHUNK == S_BLOCK * S_PER_LANE, "chunk = lanes x pairs per lane");
static_assert(S_HYP <= S_BLOCK, "one lane per hypothesis merges the waves' counts");

/* what a call fits: the run-time value, equal to the model of popsift_hip_ransac_opts and of popsift_hip_refit_opts */
enum { FIT_HOMOGRAPHY = 0, FIT_AFFINE = 1, FIT_EPIPOLAR = 2 };
static_assert(FIT_HOMOGRAPHY == POPSIFT_HIP_MODEL_HOMOGRAPHY && FIT_AFFINE == POPSIFT_HIP_MODEL_AFFINE &&
                  FIT_HOMOGRAPHY == POPSIFT_HIP_REFIT_HOMOGRAPHY && FIT_AFFINE == POPSIFT_HIP_REFIT_AFFINE &&
                  FIT_EPIPOLAR == POPSIFT_HIP_REFIT_EPIPOLAR,
              "one numbering of the kinds");

/* per kind: the inlier rule (rule 4 below), m pairs per sample, `row` ints per row of the samples, `slots` sums of the
 * refit's normal equations held in registers */
struct Transfer;
struct Sampson;
template <int KIND> struct Kind;
template <> struct Kind<FIT_HOMOGRAPHY> { typedef Transfer Rule; static constexpr int m = 4, row = 4, slots = 29; };
template <> struct Kind<FIT_AFFINE> { typedef Transfer Rule; static constexpr int m = 3, row = 4, slots = 12; };
template <> struct Kind<FIT_EPIPOLAR> { typedef Sampson Rule; static constexpr int m = 8, row = 8, slots = 45; };
static_assert(Kind<FIT_EPIPOLAR>::m == POPSIFT_HIP_EPIPOLAR_SAMPLE && Kind<FIT_EPIPOLAR>::slots == POPSIFT_HIP_REFIT_SLOTS,
              "the header's sample size and trace slots");

/* ---- rule 1: sample */

__device__ __forceinline__ uint32_t mix(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352dU;
    x ^= x >> 15;
    x *= 0x846ca68bU;
    x ^= x >> 16;
    return x;
}

/* M distinct indices below n; false when a slot found no new index in its 9 draws (that slot and the later ones stay -1) */
template <int M, int SLOTS>
__device__ __forceinline__ bool sample(uint32_t seed, int t, int n, int (&idx)[SLOTS])
{
    const uint32_t base = mix(mix(seed + 0x9e3779b9U) ^ (uint32_t)t);
    uint32_t       c = 0;
    bool           alive = true;
#pragma unroll
    for (int k = 0; k < SLOTS; k++) idx[k] = -1;
#pragma unroll
    for (int k = 0; k < M; k++) {
        bool got = false;
        for (int draw = 0; draw < 9 && alive && !got; draw++) {
            c++;
            const int i = (int)__umulhi(mix(base + 0x9e3779b9U * c), (uint32_t)n);
            bool      seen = false;
#pragma unroll
            for (int j = 0; j < k; j++) seen |= idx[j] == i;
            if (!seen) {
                idx[k] = i;
                got = true;
            }
        }
        alive = alive && got;
    }
    return alive;
}

/* ---- rule 2: normalise */

struct Norm {
    double cx, cy, s, k;
};

/* float bits as an unsigned key that orders like the value, -0 below +0; no finite value has key 0 or ~0 */
__device__ __forceinline__ uint32_t order_key(float f)
{
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000U) ? ~b : (b | 0x80000000U);
}
__device__ __forceinline__ float key_value(uint32_t k)
{
    return __uint_as_float((k & 0x80000000U) ? (k & 0x7fffffffU) : ~k);
}

/* bounds: [col] = max key, [4 + col] = max of ~key (the minimum); 0 = no finite value in the column */
__device__ __forceinline__ void centre_half(const uint32_t* __restrict__ bounds, int col, double* centre, double* half)
{
    const uint32_t hi = bounds[col], nlo = bounds[4 + col];
    if (hi == 0) {
        *centre = 0.0;
        *half = 0.0;
        return;
    }
    const double a = (double)key_value(~nlo), b = (double)key_value(hi);
    *centre = (a + b) * 0.5;
    *half = (b - a) * 0.5;
}

__device__ __forceinline__ Norm normaliser(const uint32_t* __restrict__ bounds, int col)
{
    Norm   q;
    double hx, hy;
    centre_half(bounds, col, &q.cx, &hx);
    centre_half(bounds, col + 1, &q.cy, &hy);
    const double e = hx > hy ? hx : hy;
    q.s = e > 0.0 ? e : 1.0;
    q.k = 1.0 / q.s;
    return q;
}

/* a pair in the normalised coordinates of its two sides */
struct Pair {
    double x, y, u, v;
};
__device__ __forceinline__ Pair normalise(v4f p, const Norm& L, const Norm& Rn)
{
    Pair q;
    q.x = ((double)p[0] - L.cx) * L.k;
    q.y = ((double)p[1] - L.cy) * L.k;
    q.u = ((double)p[2] - Rn.cx) * Rn.k;
    q.v = ((double)p[3] - Rn.cy) * Rn.k;
    return q;
}

__global__ __launch_bounds__(256) void k_ransac_bounds(const v4f* __restrict__ pts, int n, uint32_t* __restrict__ bounds)
{
    uint32_t m[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const v4f p = pts[i];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const float f = p[c];
            if (isfinite(f)) {
                const uint32_t k = order_key(f);
                m[c] = max(m[c], k);
                m[4 + c] = max(m[4 + c], ~k);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 8; c++) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m[c] = max(m[c], (uint32_t)__shfl_xor((int)m[c], d));
        if ((threadIdx.x & 63) == 0 && m[c] != 0) atomicMax(&bounds[c], m[c]);
    }
}

/* ---- rule 3: solve.  Every index below is a compile-time constant after unrolling: the system stays in registers. */

template <int R, int NB>
__device__ __forceinline__ bool eliminate(double (&a)[R][R + NB])
{
    constexpr int C = R + NB;
    bool          ok = true;
#pragma unroll
    for (int c = 0; c < R; c++) {
        int    p = c;
        double best = fabs(a[c][c]);
#pragma unroll
        for (int r = c + 1; r < R; r++) {
            const double v = fabs(a[r][c]);
            const bool   g = v > best;
            best = g ? v : best;
            p = g ? r : p;
        }
#pragma unroll
        for (int r = c + 1; r < R; r++) {
            const bool sw = p == r;
#pragma unroll
            for (int j = c; j < C; j++) { /* the columns before c are not read again */
                const double lo = a[c][j], hi = a[r][j];
                a[c][j] = sw ? hi : lo;
                a[r][j] = sw ? lo : hi;
            }
        }
        ok = ok && !(a[c][c] == 0.0);
#pragma unroll
        for (int r = c + 1; r < R; r++) {
            const double f = a[r][c] / a[c][c];
#pragma unroll
            for (int j = c + 1; j < C; j++) a[r][j] = fma(-f, a[c][j], a[r][j]);
        }
    }
#pragma unroll
    for (int b = 0; b < NB; b++) {
#pragma unroll
        for (int i = R - 1; i >= 0; i--) {
            double s = a[i][R + b];
#pragma unroll
            for (int j = i + 1; j < R; j++) s = fma(-a[i][j], a[j][R + b], s);
            a[i][R + b] = s / a[i][i];
        }
    }
    return ok;
}

/* a transfer model out of the normalised coordinates: M = G * Tl, then H = Tr^-1 * M */
__device__ __forceinline__ void denormalise_transfer(const double (&g)[9], const Norm& L, const Norm& Rn, double (&h)[9])
{
    double mm[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        mm[3 * i] = g[3 * i] * L.k;
        mm[3 * i + 1] = g[3 * i + 1] * L.k;
        mm[3 * i + 2] = fma(-mm[3 * i], L.cx, fma(-mm[3 * i + 1], L.cy, g[3 * i + 2]));
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        h[j] = fma(Rn.s, mm[j], Rn.cx * mm[6 + j]);
        h[3 + j] = fma(Rn.s, mm[3 + j], Rn.cy * mm[6 + j]);
        h[6 + j] = mm[6 + j];
    }
}

/* a model's nine float64 values rounded to float32; true when all nine are finite.  A caller without a valid model
 * writes zeros and -1 instead */
__device__ __forceinline__ bool round_model(const double (&h)[9], float (&M)[9])
{
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        M[i] = (float)h[i];
        ok = ok && isfinite(M[i]);
    }
    return ok;
}

/* hypothesis t of n >= m pairs under a list's bounds: its sample, its model and its count (0, or -1 for none) into row
 * `rec` of the three arrays.  One text for a homography and an affine map, used by the per-list and the grouped kernel */
template <int MODEL>
__device__ __forceinline__ void transfer_hypothesis(const v4f* __restrict__ pts, int n, int t, uint32_t seed,
                                                    const uint32_t* __restrict__ bounds, size_t rec, float* __restrict__ models,
                                                    int* __restrict__ samples, int* __restrict__ counts)
{
    constexpr int M = Kind<MODEL>::m, ROW = Kind<MODEL>::row;
    const Norm    L = normaliser(bounds, 0), Rn = normaliser(bounds, 2);
    int        idx[ROW];
    bool       ok = sample<M>(seed, t, n, idx);
    Pair       q[M];
#pragma unroll
    for (int i = 0; i < M; i++) q[i] = normalise(pts[ok ? idx[i] : 0], L, Rn);
    double g[9];
    if (MODEL == FIT_AFFINE) {
        double a[3][5];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            a[i][0] = q[i].x;
            a[i][1] = q[i].y;
            a[i][2] = 1.0;
            a[i][3] = q[i].u;
            a[i][4] = q[i].v;
        }
        ok = eliminate<3, 2>(a) && ok;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            g[i] = a[i][3];
            g[3 + i] = a[i][4];
        }
        g[6] = 0.0;
        g[7] = 0.0;
    } else {
        double a[8][9];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const double x = q[i].x, y = q[i].y, u = q[i].u, v = q[i].v;
            double(&r0)[9] = a[2 * i];
            double(&r1)[9] = a[2 * i + 1];
            r0[0] = x; r0[1] = y; r0[2] = 1.0; r0[3] = 0.0; r0[4] = 0.0; r0[5] = 0.0;
            r0[6] = -u * x; r0[7] = -u * y; r0[8] = u;
            r1[0] = 0.0; r1[1] = 0.0; r1[2] = 0.0; r1[3] = x; r1[4] = y; r1[5] = 1.0;
            r1[6] = -v * x; r1[7] = -v * y; r1[8] = v;
        }
        ok = eliminate<8, 1>(a) && ok;
#pragma unroll
        for (int i = 0; i < 8; i++) g[i] = a[i][8];
    }
    g[8] = 1.0;
    double h[9];
    float  H[9];
    denormalise_transfer(g, L, Rn, h);
    ok = round_model(h, H) && ok;
#pragma unroll
    for (int i = 0; i < 9; i++) models[9 * rec + i] = ok ? H[i] : 0.0f;
#pragma unroll
    for (int i = 0; i < ROW; i++) samples[ROW * rec + i] = idx[i];
    counts[rec] = ok ? 0 : -1;
}

template <int MODEL>
__global__ __launch_bounds__(64) void k_ransac_models(const v4f* __restrict__ pts, int n, int T, uint32_t seed,
                                                      const uint32_t* __restrict__ bounds, float* __restrict__ models,
                                                      int* __restrict__ samples, int* __restrict__ counts)
{
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= T) return;
    transfer_hypothesis<MODEL>(pts, n, t, seed, bounds, (size_t)t, models, samples, counts);
}

/* ---- popsift_hip_epipolar, rules 3 to 5: one fundamental matrix per lane.  As above every index is a compile-time
 * constant after unrolling; row and column swaps are selects. */

/* rule 3: the null vector by eight steps of complete pivoting; false when a pivot is exactly 0.  ROWS 8: the sampler's
 * 8 x 9 system.  ROWS 9: the refit's 9 x 9 normal matrix, whose row 8 takes part in the pivoting and is then dropped */
template <int ROWS>
__device__ __forceinline__ bool null_vector(double (&a)[ROWS][9], double (&f)[9])
{
    bool ok = true;
    int  perm[9];
#pragma unroll
    for (int j = 0; j < 9; j++) perm[j] = j;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        int    pr = k, pc = k;
        double best = fabs(a[k][k]);
#pragma unroll
        for (int c = k; c < 9; c++) { /* column-major: the lowest column, then the lowest row, wins a tie */
#pragma unroll
            for (int r = (c == k ? k + 1 : k); r < ROWS; r++) {
                const double v = fabs(a[r][c]);
                const bool   g = v > best;
                best = g ? v : best;
                pr = g ? r : pr;
                pc = g ? c : pc;
            }
        }
#pragma unroll
        for (int r = k + 1; r < ROWS; r++) {
            const bool sw = pr == r;
#pragma unroll
            for (int j = k; j < 9; j++) { /* the columns before k of these rows are not read again */
                const double lo = a[k][j], hi = a[r][j];
                a[k][j] = sw ? hi : lo;
                a[r][j] = sw ? lo : hi;
            }
        }
#pragma unroll
        for (int c = k + 1; c < 9; c++) {
            const bool sw = pc == c;
#pragma unroll
            for (int r = 0; r < ROWS; r++) { /* the rows above k too: back substitution reads them */
                const double lo = a[r][k], hi = a[r][c];
                a[r][k] = sw ? hi : lo;
                a[r][c] = sw ? lo : hi;
            }
            const int lo = perm[k], hi = perm[c];
            perm[k] = sw ? hi : lo;
            perm[c] = sw ? lo : hi;
        }
        ok = ok && !(a[k][k] == 0.0);
#pragma unroll
        for (int r = k + 1; r < ROWS; r++) {
            const double q = a[r][k] / a[k][k];
#pragma unroll
            for (int j = k + 1; j < 9; j++) a[r][j] = fma(-q, a[k][j], a[r][j]);
        }
    }
    double z[9];
    z[8] = 1.0; /* the free column's unknown */
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        double s = -a[i][8];
#pragma unroll
        for (int j = i + 1; j < 8; j++) s = fma(-a[i][j], z[j], s);
        z[i] = s / a[i][i];
    }
#pragma unroll
    for (int c = 0; c < 9; c++) {
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < 9; j++) v = perm[j] == c ? z[j] : v;
        f[c] = v;
    }
    return ok;
}

/* rule 4: one Jacobi rotation of the symmetric m that zeroes m[P][Q]; O is the third index; v collects the rotations */
template <int P, int Q, int O>
__device__ __forceinline__ void rotate(double (&m)[3][3], double (&v)[3][3])
{
    if (m[P][Q] == 0.0) return;
    const double d = m[Q][Q] - m[P][P];
    const double e = 2.0 * m[P][Q];
    const double theta = d / e;
    const double root = sqrt(fma(theta, theta, 1.0));
    const double den = fabs(theta) + root;
    const double t = copysign(1.0, theta) / den;
    const double c = 1.0 / sqrt(fma(t, t, 1.0));
    const double s = t * c;
    m[P][P] = fma(-t, m[P][Q], m[P][P]);
    m[Q][Q] = fma(t, m[P][Q], m[Q][Q]);
    m[P][Q] = m[Q][P] = 0.0;
    const double mp = m[O][P], mq = m[O][Q];
    m[O][P] = m[P][O] = fma(-s, mq, c * mp);
    m[O][Q] = m[Q][O] = fma(s, mp, c * mq);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const double vp = v[r][P], vq = v[r][Q];
        v[r][P] = fma(-s, vq, c * vp);
        v[r][Q] = fma(s, vp, c * vq);
    }
}

/* f <- f - (f w) w^T, w the eigenvector of f^T f under its smallest eigenvalue: the closest matrix of rank 2 */
__device__ __forceinline__ void rank2(double (&f)[9])
{
    double m[3][3], v[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = i; j < 3; j++) m[i][j] = m[j][i] = fma(f[i], f[j], fma(f[3 + i], f[3 + j], f[6 + i] * f[6 + j]));
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) v[i][j] = i == j ? 1.0 : 0.0;
    }
    for (int sweep = 0; sweep < 6; sweep++) {
        rotate<0, 1, 2>(m, v);
        rotate<0, 2, 1>(m, v);
        rotate<1, 2, 0>(m, v);
    }
    int    b = 0;
    double mb = m[0][0];
    if (m[1][1] < mb) {
        b = 1;
        mb = m[1][1];
    }
    if (m[2][2] < mb) b = 2;
    double w[3];
#pragma unroll
    for (int j = 0; j < 3; j++) w[j] = b == 0 ? v[j][0] : b == 1 ? v[j][1] : v[j][2];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double fw = fma(f[3 * i], w[0], fma(f[3 * i + 1], w[1], f[3 * i + 2] * w[2]));
#pragma unroll
        for (int j = 0; j < 3; j++) f[3 * i + j] = fma(-fw, w[j], f[3 * i + j]);
    }
}

/* rule 5: a fundamental matrix out of the normalised coordinates, G = Fn * Tl, then H = Tr^T * G, scaled so that its
 * entry of largest magnitude is 1; false when that entry is 0 */
__device__ __forceinline__ bool denormalise_fundamental(const double (&f)[9], const Norm& L, const Norm& Rn, double (&h)[9])
{
    double g[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        g[3 * i] = f[3 * i] * L.k;
        g[3 * i + 1] = f[3 * i + 1] * L.k;
        g[3 * i + 2] = fma(-g[3 * i], L.cx, fma(-g[3 * i + 1], L.cy, f[3 * i + 2]));
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        h[j] = g[j] * Rn.k;
        h[3 + j] = g[3 + j] * Rn.k;
        h[6 + j] = fma(-h[j], Rn.cx, fma(-h[3 + j], Rn.cy, g[6 + j]));
    }
    double d = h[0], best = fabs(h[0]);
#pragma unroll
    for (int i = 1; i < 9; i++) {
        const double v = fabs(h[i]);
        const bool   gt = v > best;
        best = gt ? v : best;
        d = gt ? h[i] : d;
    }
#pragma unroll
    for (int i = 0; i < 9; i++) h[i] = h[i] / d;
    return !(d == 0.0);
}

/* the same for a fundamental matrix */
__device__ __forceinline__ void epipolar_hypothesis(const v4f* __restrict__ pts, int n, int t, uint32_t seed,
                                                    const uint32_t* __restrict__ bounds, size_t rec, float* __restrict__ models,
                                                    int* __restrict__ samples, int* __restrict__ counts)
{
    constexpr int M = Kind<FIT_EPIPOLAR>::m;
    const Norm    L = normaliser(bounds, 0), Rn = normaliser(bounds, 2);
    int        idx[M];
    bool       ok = sample<M>(seed, t, n, idx);
    double     a[M][9], f[9], h[9];
#pragma unroll
    for (int i = 0; i < M; i++) {
        const Pair q = normalise(pts[ok ? idx[i] : 0], L, Rn);
        a[i][0] = q.u * q.x; a[i][1] = q.u * q.y; a[i][2] = q.u;
        a[i][3] = q.v * q.x; a[i][4] = q.v * q.y; a[i][5] = q.v;
        a[i][6] = q.x; a[i][7] = q.y; a[i][8] = 1.0;
    }
    ok = null_vector<M>(a, f) && ok;
    rank2(f);
    ok = denormalise_fundamental(f, L, Rn, h) && ok;
    float F[9];
    ok = round_model(h, F) && ok;
#pragma unroll
    for (int i = 0; i < 9; i++) models[9 * rec + i] = ok ? F[i] : 0.0f;
#pragma unroll
    for (int i = 0; i < M; i++) samples[M * rec + i] = idx[i];
    counts[rec] = ok ? 0 : -1;
}

__global__ __launch_bounds__(64) void k_epipolar_models(const v4f* __restrict__ pts, int n, int T, uint32_t seed,
                                                        const uint32_t* __restrict__ bounds, float* __restrict__ models,
                                                        int* __restrict__ samples, int* __restrict__ counts)
{
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= T) return;
    epipolar_hypothesis(pts, n, t, seed, bounds, (size_t)t, models, samples, counts);
}

/* ---- rule 4: score */

/* transfer error in the right image, popsift_hip_ransac */
struct Transfer {
    static __device__ __forceinline__ bool inlier(const float (&H)[9], v4f p, float max_err2)
    {
        const float u = fmaf(H[0], p[0], fmaf(H[1], p[1], H[2]));
        const float v = fmaf(H[3], p[0], fmaf(H[4], p[1], H[5]));
        const float w = fmaf(H[6], p[0], fmaf(H[7], p[1], H[8]));
        const float dx = fmaf(-w, p[2], u);
        const float dy = fmaf(-w, p[3], v);
        const float e = fmaf(dx, dx, dy * dy);
        const float lim = max_err2 * (w * w);
        return w > 0.0f && e <= lim;
    }
};

/* Sampson distance to the epipolar constraint, popsift_hip_epipolar (rule 6 there) */
struct Sampson {
    static __device__ __forceinline__ bool inlier(const float (&F)[9], v4f p, float max_err2)
    {
        const float a = fmaf(F[0], p[0], fmaf(F[1], p[1], F[2]));
        const float b = fmaf(F[3], p[0], fmaf(F[4], p[1], F[5]));
        const float c = fmaf(F[6], p[0], fmaf(F[7], p[1], F[8]));
        const float d = fmaf(F[0], p[2], fmaf(F[3], p[3], F[6]));
        const float e = fmaf(F[1], p[2], fmaf(F[4], p[3], F[7]));
        const float r = fmaf(a, p[2], fmaf(b, p[3], c));
        const float g = fmaf(a, a, fmaf(b, b, fmaf(d, d, e * e)));
        const float lim = max_err2 * g;
        return g > 0.0f && g < INFINITY && r * r <= lim;
    }
};

/* grid (hypothesis blocks, pair chunks).  A hypothesis without a model is all zeros: w = 0 (g = 0), no inlier, nothing is
 * added to its -1. */
template <class Rule>
__global__ __launch_bounds__(S_BLOCK) void k_ransac_score(const v4f* __restrict__ pts, int n, const float* __restrict__ models,
                                                          int T, float max_err2, int* __restrict__ counts)
{
    __shared__ int s_cnt[S_HYP][S_BLOCK / 64];
    const int      lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int      t0 = blockIdx.x * S_HYP;
    const int      nh = min(S_HYP, T - t0);
    v4f            p[S_PER_LANE];
#pragma unroll
    for (int r = 0; r < S_PER_LANE; r++) {
        const int i = blockIdx.y * S_CHUNK + r * S_BLOCK + threadIdx.x;
        /* past the end: NaN fails both tests */
        p[r] = i < n ? pts[i] : v4f{NAN, NAN, NAN, NAN};
    }
    for (int k = 0; k < nh; k++) {
        const float* __restrict__ m = models + 9 * (size_t)(t0 + k); /* the same address in every lane */
        float H[9];
#pragma unroll
        for (int i = 0; i < 9; i++) H[i] = m[i];
        int c = 0;
#pragma unroll
        for (int r = 0; r < S_PER_LANE; r++) c += __popcll(__ballot(Rule::inlier(H, p[r], max_err2)));
        if (lane == 0) s_cnt[k][wave] = c;
    }
    __syncthreads();
    if ((int)threadIdx.x < nh) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < S_BLOCK / 64; w++) s += s_cnt[threadIdx.x][w];
        if (s != 0) atomicAdd(&counts[t0 + threadIdx.x], s);
    }
}

/* ---- rule 5: select.  One workgroup; key = (count, ~t): the largest count, then the lowest t */

__device__ __forceinline__ void select_winner(const int* __restrict__ counts, const float* __restrict__ models, int T,
                                              int min_count, popsift_hip_ransac_result* __restrict__ res)
{
    __shared__ long long s_key[4];
    __shared__ int       s_valid[4];
    long long            key = -1; /* below every (count >= 0, t) */
    int                  valid = 0;
    for (int t = threadIdx.x; t < T; t += 256) {
        const int c = counts[t];
        if (c >= 0) {
            valid++;
            key = max(key, ((long long)c << 32) | (long long)(0xffffffffU - (uint32_t)t));
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        key = max(key, __shfl_xor(key, d));
        valid += __shfl_xor(valid, d);
    }
    if ((threadIdx.x & 63) == 0) {
        s_key[threadIdx.x >> 6] = key;
        s_valid[threadIdx.x >> 6] = valid;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 4; w++) {
        key = max(key, s_key[w]);
        valid += s_valid[w];
    }
    const int  count = (int)(key >> 32);
    const int  t = (int)(0xffffffffU - (uint32_t)(key & 0xffffffffLL));
    const bool won = key >= 0 && count >= min_count;
    for (int i = 0; i < 9; i++) res->H[i] = won ? models[9 * (size_t)t + i] : 0.0f;
    res->n_inliers = won ? count : 0;
    res->hypothesis = won ? t : -1;
    res->n_valid = valid;
    res->reserved = 0;
}

__global__ __launch_bounds__(256) void k_ransac_select(const int* __restrict__ counts, const float* __restrict__ models, int T,
                                                       int min_count, popsift_hip_ransac_result* __restrict__ res)
{
    select_winner(counts, models, T, min_count, res);
}

/* four pairs and four mask bytes per lane; mask has room for n rounded up to a multiple of 4 */
template <class Rule>
__global__ __launch_bounds__(256) void k_ransac_mask(const v4f* __restrict__ pts, int n,
                                                     const popsift_hip_ransac_result* __restrict__ res, float max_err2,
                                                     uint32_t* __restrict__ mask)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (4 * q >= n) return;
    float H[9];
#pragma unroll
    for (int i = 0; i < 9; i++) H[i] = res->H[i];
    const bool won = res->hypothesis >= 0;
    uint32_t   word = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int i = 4 * q + r;
        if (won && i < n && Rule::inlier(H, pts[i], max_err2)) word |= 1u << (8 * r);
    }
    mask[q] = word;
}

/* ---- popsift_hip_ransac_many: the five kernels above over many lists.  The host cuts every list into segments of at most
 * G_SEG consecutive pairs (an empty list has none); a segment is the unit of work of the kernels that walk pairs. */

constexpr int G_SEG = POPSIFT_HIP_RANSAC_MANY_SEGMENT; /* pairs of a segment */
constexpr int G_BLOCK = 256;                           /* lanes of the grouped kernels: hypotheses of a score workgroup */
static_assert(G_SEG == G_BLOCK, "k_many_bounds and k_many_mask give a segment one lane per pair");

struct Segment {
    int list;   /* index in the call */
    int first;  /* flat index of its first pair */
    int count;  /* 1 .. G_SEG */
    int whole;  /* 1: the segment is its whole list */
};
static_assert(sizeof(Segment) == 16, "one 16-byte load");

/* grid (segments).  bounds: 8 keys per list, zeroed before */
__global__ __launch_bounds__(G_BLOCK) void k_many_bounds(const v4f* __restrict__ pts, const Segment* __restrict__ segs,
                                                         uint32_t* __restrict__ bounds)
{
    const Segment sg = segs[blockIdx.x];
    uint32_t      m[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if ((int)threadIdx.x < sg.count) {
        const v4f p = pts[(size_t)sg.first + threadIdx.x];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const float f = p[c];
            if (isfinite(f)) {
                const uint32_t k = order_key(f);
                m[c] = k;
                m[4 + c] = ~k;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 8; c++) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m[c] = max(m[c], (uint32_t)__shfl_xor((int)m[c], d));
        if ((threadIdx.x & 63) == 0 && m[c] != 0) atomicMax(&bounds[8 * (size_t)sg.list + c], m[c]);
    }
}

/* grid (lists of the group, blocks of 64 hypotheses): one lane per (list, hypothesis).  A list shorter than a sample has
 * the rows of a per-list call that never reached the GPU: -1, zeros, -1 */
template <int KIND>
__global__ __launch_bounds__(64) void k_many_models(const v4f* __restrict__ pts, const int* __restrict__ offsets, int list0, int T,
                                                    uint32_t seed, const uint32_t* __restrict__ bounds, float* __restrict__ models,
                                                    int* __restrict__ samples, int* __restrict__ counts)
{
    constexpr int M = Kind<KIND>::m, ROW = Kind<KIND>::row;
    const int     t = blockIdx.y * 64 + threadIdx.x;
    if (t >= T) return;
    const int    list = list0 + blockIdx.x;
    const int    base = offsets[list], n = offsets[list + 1] - base;
    const size_t rec = (size_t)blockIdx.x * T + t;
    if (n < M) {
#pragma unroll
        for (int i = 0; i < 9; i++) models[9 * rec + i] = 0.0f;
#pragma unroll
        for (int i = 0; i < ROW; i++) samples[ROW * rec + i] = -1;
        counts[rec] = -1;
        return;
    }
    const uint32_t* __restrict__ b = bounds + 8 * (size_t)list;
    if constexpr (KIND == FIT_EPIPOLAR) epipolar_hypothesis(pts + base, n, t, seed, b, rec, models, samples, counts);
    else transfer_hypothesis<KIND>(pts + base, n, t, seed, b, rec, models, samples, counts);
}

/* grid (segments of the group, blocks of G_BLOCK hypotheses).  A lane keeps one hypothesis' nine coefficients and its
 * count in registers and walks the segment's pairs; a pair is the same 16 bytes in every lane (a scalar load).  No
 * ballot, no LDS: a short list costs its own pairs and nothing more.  A list of one segment stores its counts; a longer
 * one adds them, one integer atomic per (segment, hypothesis).  A slot without a model is all zeros, counts nothing and
 * keeps its -1 */
template <class Rule>
__global__ __launch_bounds__(G_BLOCK) void k_many_score(const v4f* __restrict__ pts, const Segment* __restrict__ segs, int list0,
                                                        const float* __restrict__ models, int T, float max_err2,
                                                        int* __restrict__ counts)
{
    const Segment sg = segs[blockIdx.x];
    const int     t = blockIdx.y * G_BLOCK + threadIdx.x;
    if (t >= T) return;
    const size_t rec = (size_t)(sg.list - list0) * T + t;
    float        H[9];
#pragma unroll
    for (int i = 0; i < 9; i++) H[i] = models[9 * rec + i];
    const v4f* __restrict__ p = pts + sg.first;
    int                     c = 0;
#pragma unroll 4
    for (int i = 0; i < sg.count; i++) c += Rule::inlier(H, p[i], max_err2) ? 1 : 0;
    if (c == 0) return;
    if (sg.whole) counts[rec] = c;
    else atomicAdd(&counts[rec], c);
}

/* grid (lists of the group) */
__global__ __launch_bounds__(256) void k_many_select(const int* __restrict__ counts, const float* __restrict__ models, int T,
                                                     int min_count, popsift_hip_ransac_result* __restrict__ res)
{
    const size_t r0 = (size_t)blockIdx.x * T;
    select_winner(counts + r0, models + 9 * r0, T, min_count, res + blockIdx.x);
}

/* grid (segments): one lane and one byte per pair, at the pair's flat index -- a list starts at any byte of the mask */
template <class Rule>
__global__ __launch_bounds__(G_BLOCK) void k_many_mask(const v4f* __restrict__ pts, const Segment* __restrict__ segs,
                                                       const popsift_hip_ransac_result* __restrict__ res, float max_err2,
                                                       uint8_t* __restrict__ mask)
{
    const Segment sg = segs[blockIdx.x];
    if ((int)threadIdx.x >= sg.count) return;
    const popsift_hip_ransac_result* __restrict__ r = res + sg.list;
    float H[9];
#pragma unroll
    for (int i = 0; i < 9; i++) H[i] = r->H[i];
    const size_t i = (size_t)sg.first + threadIdx.x;
    mask[i] = r->hypothesis >= 0 && Rule::inlier(H, pts[i], max_err2) ? 1 : 0;
}

/* ---- popsift_hip_refit: least squares on the inliers, every round enqueued up front.  The state record starts like a
 * popsift_hip_ransac_result, so that k_ransac_mask writes the final mask from it. */

constexpr int F_SLOTS = POPSIFT_HIP_REFIT_SLOTS;
constexpr int F_ROUNDS = POPSIFT_HIP_REFIT_MAX_ROUNDS;
constexpr int F_CHUNK = POPSIFT_HIP_REFIT_CHUNK;
static_assert(F_CHUNK == 256 * 4, "a chunk is 256 lanes x 4 consecutive pairs");

struct RefitState {
    float H[9];       /* cur */
    int   n_inliers;  /* c_cur; the start count is added up here */
    int   hypothesis; /* 0: k_ransac_mask takes the record for a winner */
    int   n_start, rounds, stop;
    int   done;       /* the kernels of the rounds still enqueued return at once */
    int   pad;
};
static_assert(sizeof(RefitState) == 64 && offsetof(RefitState, n_inliers) == offsetof(popsift_hip_ransac_result, n_inliers) &&
                  offsetof(RefitState, hypothesis) == offsetof(popsift_hip_ransac_result, hypothesis),
              "the front of the state is a popsift_hip_ransac_result");

/* the trace of a call, one block on the device and in the pinned buffer */
struct RefitTrace {
    double sums[F_ROUNDS][F_SLOTS];
    float  models[F_ROUNDS][9];
    int    counts[F_ROUNDS];
    int    accepted[F_ROUNDS];
};

struct RefitStart {
    float M[9];
};

/* one lane: cur = M, the counters of the trace to "did not run" (the rest of the trace is zeroed by a memset) */
__global__ __launch_bounds__(64) void k_refit_init(RefitStart start, RefitState* __restrict__ st, RefitTrace* __restrict__ tr)
{
    if (threadIdx.x != 0) return;
    for (int i = 0; i < 9; i++) st->H[i] = start.M[i];
    st->n_inliers = 0;
    st->hypothesis = 0;
    st->n_start = 0;
    st->rounds = 0;
    st->stop = POPSIFT_HIP_REFIT_STOP_ROUNDS;
    st->done = 0;
    st->pad = 0;
    for (int r = 0; r < F_ROUNDS; r++) tr->counts[r] = -1;
}

/* the inliers of one model among all pairs, four per lane; an invalid candidate is all zeros and counts nothing */
template <class Rule>
__global__ __launch_bounds__(256) void k_refit_count(const v4f* __restrict__ pts, int n, const float* __restrict__ model,
                                                     float max_err2, int* __restrict__ counter, const int* __restrict__ done)
{
    if (*done) return;
    float H[9];
#pragma unroll
    for (int i = 0; i < 9; i++) H[i] = model[i];
    const int q = blockIdx.x * 256 + threadIdx.x;
    int       c = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int  i = 4 * q + r;
        const bool in = i < n && Rule::inlier(H, pts[i < n ? i : 0], max_err2);
        c += __popcll(__ballot(in));
    }
    if ((threadIdx.x & 63) == 0 && c != 0) atomicAdd(counter, c);
}

/* rule 3a: the terms of one pair, +0.0 for a pair that is no inlier; t + 0.0 turns a term of -0.0 into +0.0 */
template <int KIND>
__device__ __forceinline__ void refit_terms(v4f p, bool in, const Norm& L, const Norm& Rn, double (&t)[Kind<KIND>::slots])
{
    const Pair   q = normalise(p, L, Rn);
    const double x = q.x, y = q.y, u = q.u, v = q.v;
    if (KIND == POPSIFT_HIP_REFIT_EPIPOLAR) {
        const double a[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1.0};
        int          s = 0;
#pragma unroll
        for (int j = 0; j < 9; j++) {
#pragma unroll
            for (int k = j; k < 9; k++) t[s++] = a[j] * a[k];
        }
    } else {
        t[0] = x * x; t[1] = x * y; t[2] = x; t[3] = y * y; t[4] = y; t[5] = 1.0;
        constexpr int c0 = KIND == POPSIFT_HIP_REFIT_AFFINE ? 6 : 21; /* the affine map's right-hand sides follow its matrix */
        t[c0] = x * u; t[c0 + 1] = y * u; t[c0 + 2] = u; t[c0 + 3] = x * v; t[c0 + 4] = y * v; t[c0 + 5] = v;
        if (KIND == POPSIFT_HIP_REFIT_HOMOGRAPHY) {
            const double p6 = -u * x, p7 = -u * y, q6 = -v * x, q7 = -v * y;
            t[6] = x * p6; t[7] = x * p7; t[8] = y * p6; t[9] = y * p7; t[10] = p6; t[11] = p7;
            t[12] = x * q6; t[13] = x * q7; t[14] = y * q6; t[15] = y * q7; t[16] = q6; t[17] = q7;
            t[18] = fma(p6, p6, q6 * q6);
            t[19] = fma(p6, p7, q6 * q7);
            t[20] = fma(p7, p7, q7 * q7);
            t[27] = fma(p6, u, q6 * v);
            t[28] = fma(p7, u, q7 * v);
        }
    }
#pragma unroll
    for (int j = 0; j < Kind<KIND>::slots; j++) t[j] = in ? t[j] + 0.0 : 0.0;
}

/* where register j of a kind's sums lies among the 45 slots: only the affine map's right-hand sides move */
template <int KIND>
__device__ __forceinline__ constexpr int refit_slot(int j)
{
    return KIND == POPSIFT_HIP_REFIT_AFFINE && j >= 6 ? j + 15 : j;
}

/* the sum of one value per lane over the workgroup's 256 lanes in the order of the tree: xor 1, 2, .. 32 inside a wave,
 * then (w0 + w1) + (w2 + w3); valid in the first SLOTS lanes as out[lane].  s_wave: [4][SLOTS] */
template <int SLOTS>
__device__ __forceinline__ double refit_block_tree(double (&v)[SLOTS], double (*s_wave)[SLOTS])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < SLOTS; j++) {
#pragma unroll
        for (int d = 1; d <= 32; d <<= 1) v[j] = v[j] + __shfl_xor(v[j], d);
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < SLOTS; j++) s_wave[wave][j] = v[j];
    }
    __syncthreads();
    double r = 0.0;
    if ((int)threadIdx.x < SLOTS) {
        const int j = threadIdx.x;
        r = (s_wave[0][j] + s_wave[1][j]) + (s_wave[2][j] + s_wave[3][j]);
    }
    return r;
}

/* rules 3a and 3b up to a chunk: one workgroup per F_CHUNK pairs, a lane takes 4 consecutive pairs; blocks[j * chunks +
 * chunk] = tree(chunk * F_CHUNK, F_CHUNK) of the kind's register j */
template <int KIND>
__global__ __launch_bounds__(256) void k_refit_accumulate(const v4f* __restrict__ pts, int n, const uint32_t* __restrict__ bounds,
                                                          const RefitState* __restrict__ st, float max_err2,
                                                          double* __restrict__ blocks)
{
    typedef Kind<KIND> K;
    constexpr int    S = K::slots;
    __shared__ double s_wave[4][S];
    if (st->done) return; /* the same in every lane */
    const Norm L = normaliser(bounds, 0), Rn = normaliser(bounds, 2);
    float      H[9];
#pragma unroll
    for (int i = 0; i < 9; i++) H[i] = st->H[i];
    const int i0 = blockIdx.x * F_CHUNK + 4 * threadIdx.x;
    double    acc[S];
#pragma unroll
    for (int half = 0; half < 2; half++) {
        double t0[S], t1[S];
        const int  ia = i0 + 2 * half, ib = ia + 1;
        const v4f  pa = pts[ia < n ? ia : 0], pb = pts[ib < n ? ib : 0];
        refit_terms<KIND>(pa, ia < n && K::Rule::inlier(H, pa, max_err2), L, Rn, t0);
        refit_terms<KIND>(pb, ib < n && K::Rule::inlier(H, pb, max_err2), L, Rn, t1);
#pragma unroll
        for (int j = 0; j < S; j++) {
            const double s = t0[j] + t1[j];
            acc[j] = half == 0 ? s : acc[j] + s;
        }
    }
    const double r = refit_block_tree<S>(acc, s_wave);
    if ((int)threadIdx.x < S) blocks[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = r;
}

/* rule 3b above the chunks, then rule 3c on one lane: the sums go from LDS into the register system of the sampler's
 * solver.  One workgroup.  blocks: [slot][chunks] as k_refit_accumulate left them; spare: room for
 * [slot][(chunks + 1) / 2], used when there are more than 256 chunks */
template <int KIND>
__global__ __launch_bounds__(256) void k_refit_solve(double* blocks, double* spare, int chunks,
                                                     const uint32_t* __restrict__ bounds, const RefitState* __restrict__ st,
                                                     RefitTrace* __restrict__ tr, int round)
{
    typedef Kind<KIND> K;
    constexpr int    S = K::slots;
    __shared__ double s_wave[4][S];
    __shared__ double s_sum[F_SLOTS];
    if (st->done) return;
    /* level by level, pairs (2i, 2i + 1) of chunk sums, until one value per lane is left */
    double* src = blocks;
    double* dst = spare;
    int     cnt = chunks, stride = chunks;
    while (cnt > 256) {
        const int half = (cnt + 1) / 2;
        for (int e = threadIdx.x; e < S * half; e += 256) {
            const int     j = e / half, i = e - j * half;
            const double* p = src + (size_t)j * stride;
            dst[(size_t)j * half + i] = p[2 * i] + (2 * i + 1 < cnt ? p[2 * i + 1] : 0.0);
        }
        __syncthreads(); /* the next level reads what other lanes of this workgroup wrote */
        double* const tmp = src;
        src = dst;
        dst = tmp;
        cnt = stride = half;
    }
    double v[S];
#pragma unroll
    for (int j = 0; j < S; j++) v[j] = (int)threadIdx.x < cnt ? src[(size_t)j * stride + threadIdx.x] : 0.0;
    const double r = refit_block_tree<S>(v, s_wave);
    if (threadIdx.x < F_SLOTS) s_sum[threadIdx.x] = 0.0;
    __syncthreads();
    if ((int)threadIdx.x < S) s_sum[refit_slot<KIND>(threadIdx.x)] = r;
    __syncthreads();
    if (threadIdx.x < F_SLOTS) tr->sums[round][threadIdx.x] = s_sum[threadIdx.x];
    if (threadIdx.x != 0) return;

    const Norm    L = normaliser(bounds, 0), Rn = normaliser(bounds, 2);
    const double* s = s_sum;
    double        h[9];
    bool          ok;
    if (KIND == FIT_EPIPOLAR) {
        double a[9][9], f[9];
        int    k = 0;
#pragma unroll
        for (int i = 0; i < 9; i++) {
#pragma unroll
            for (int j = i; j < 9; j++) a[i][j] = a[j][i] = s[k++];
        }
        ok = null_vector<9>(a, f);
        rank2(f);
        ok = denormalise_fundamental(f, L, Rn, h) && ok;
    } else {
        double       g[9];
        const double n3[3][3] = {{s[0], s[1], s[2]}, {s[1], s[3], s[4]}, {s[2], s[4], s[5]}};
        if (KIND == FIT_AFFINE) {
            double a[3][5];
#pragma unroll
            for (int i = 0; i < 3; i++) {
#pragma unroll
                for (int j = 0; j < 3; j++) a[i][j] = n3[i][j];
                a[i][3] = s[21 + i];
                a[i][4] = s[24 + i];
            }
            ok = eliminate<3, 2>(a);
#pragma unroll
            for (int i = 0; i < 3; i++) {
                g[i] = a[i][3];
                g[3 + i] = a[i][4];
            }
            g[6] = 0.0;
            g[7] = 0.0;
        } else {
            double a[8][9];
#pragma unroll
            for (int i = 0; i < 3; i++) {
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    a[i][j] = a[3 + i][3 + j] = n3[i][j];
                    a[i][3 + j] = a[3 + i][j] = 0.0;
                }
                a[i][6] = a[6][i] = s[6 + 2 * i];
                a[i][7] = a[7][i] = s[7 + 2 * i];
                a[3 + i][6] = a[6][3 + i] = s[12 + 2 * i];
                a[3 + i][7] = a[7][3 + i] = s[13 + 2 * i];
            }
            a[6][6] = s[18];
            a[6][7] = a[7][6] = s[19];
            a[7][7] = s[20];
#pragma unroll
            for (int i = 0; i < 8; i++) a[i][8] = s[21 + i];
            ok = eliminate<8, 1>(a);
#pragma unroll
            for (int i = 0; i < 8; i++) g[i] = a[i][8];
        }
        g[8] = 1.0;
        denormalise_transfer(g, L, Rn, h);
    }
    float M[9];
    ok = round_model(h, M) && ok;
#pragma unroll
    for (int i = 0; i < 9; i++) tr->models[round][i] = ok ? M[i] : 0.0f;
    tr->counts[round] = ok ? 0 : -1;
}

/* rules 2 and 3d on the state record, one lane.  round -1: the start count has been added up in st->n_inliers */
__global__ __launch_bounds__(64) void k_refit_decide(RefitState* __restrict__ st, RefitTrace* __restrict__ tr, int round, int m)
{
    if (threadIdx.x != 0 || st->done) return;
    if (round < 0) {
        st->n_start = st->n_inliers;
        if (st->n_inliers < m) {
            st->stop = POPSIFT_HIP_REFIT_STOP_NO_SUPPORT;
            st->done = 1;
        }
        return;
    }
    const int c = tr->counts[round];
    bool      same = true;
    for (int i = 0; i < 9; i++) same = same && __float_as_uint(tr->models[round][i]) == __float_as_uint(st->H[i]);
    int stop = -1;
    if (c < 0) stop = POPSIFT_HIP_REFIT_STOP_NO_FIT;
    else if (same) stop = POPSIFT_HIP_REFIT_STOP_CONVERGED;
    else if (c < st->n_inliers) stop = POPSIFT_HIP_REFIT_STOP_NOT_BETTER;
    if (stop >= 0) {
        st->stop = stop;
        st->done = 1;
        return;
    }
    for (int i = 0; i < 9; i++) st->H[i] = tr->models[round][i];
    st->n_inliers = c;
    st->rounds = st->rounds + 1;
    tr->accepted[round] = 1;
}

/* ---- pair_points */

/* *bad = 1 when a descriptor has no feature behind it (map entry outside 0 .. n_feat - 1) */
__global__ __launch_bounds__(256) void k_pair_points(const popsift_hip_pair* __restrict__ pairs, int n,
                                                     const DevFeature* __restrict__ lf, const int* __restrict__ lrev, int l_nfeat,
                                                     const DevFeature* __restrict__ rf, const int* __restrict__ rrev, int r_nfeat,
                                                     v4f* __restrict__ out, int* __restrict__ bad)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const popsift_hip_pair p = pairs[i];
    const int              fl = lrev[p.l], fr = rrev[p.r];
    if (fl < 0 || fl >= l_nfeat || fr < 0 || fr >= r_nfeat) {
        *bad = 1;
        out[i] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
        return;
    }
    out[i] = v4f{lf[fl].xpos, lf[fl].ypos, rf[fr].xpos, rf[fr].ypos};
}

}  // namespace
}  // namespace popsift_hip

using namespace popsift_hip;

/* stream + grow-only scratch on one GPU */
struct popsift_hip_verifier {
    int         device = 0;
    hipStream_t stream = nullptr;
    char*       d_buf = nullptr; /* bounds, result record, mask, points, models, samples, counts */
    size_t      d_cap = 0;
    char*       h_buf = nullptr; /* pinned: the points going up; the result record, the mask and the trace coming down */
    size_t      h_cap = 0;
    int         many_group = 0; /* popsift_hip_verifier_debug_set_group; 0: POPSIFT_HIP_RANSAC_MANY_GROUP */
};

namespace {

constexpr int    MAX_PAIRS = 1 << 24;
constexpr int    MAX_HYP = 65536;
constexpr size_t HEAD = 64; /* bytes kept for the result record in front of the mask */
static_assert(sizeof(popsift_hip_ransac_result) <= HEAD, "the record fits its slot");

bool opts_valid(const popsift_hip_ransac_opts* o)
{
    return o && (o->model == POPSIFT_HIP_MODEL_HOMOGRAPHY || o->model == POPSIFT_HIP_MODEL_AFFINE) && o->hypotheses >= 1 &&
           o->hypotheses <= MAX_HYP && std::isfinite(o->max_err) && o->max_err > 0.0f && o->reserved[0] == 0 &&
           o->reserved[1] == 0;
}

bool epipolar_opts_valid(const popsift_hip_epipolar_opts* o)
{
    return o && o->hypotheses >= 1 && o->hypotheses <= MAX_HYP && std::isfinite(o->max_err) && o->max_err > 0.0f &&
           o->reserved[0] == 0 && o->reserved[1] == 0 && o->reserved[2] == 0;
}

/* the sampler's options, from popsift_hip_ransac_opts or popsift_hip_epipolar_opts */
struct Fit {
    int      hypotheses;
    float    max_err;
    uint32_t seed;
};

/* ---- the frame that run() and run_refit() share around their own launches */

bool args_valid(const popsift_hip_verifier* v, const float* pts, int n)
{
    return v && n >= 0 && n <= MAX_PAIRS && (n == 0 || pts);
}

/* device: [bounds 32][record 64][mask][points], then the call's own arrays from d_own; the record and the mask come down
 * together.  pinned: [points][record + mask], then the call's trace from h_own */
struct Frame {
    size_t b_pts, o_head, o_mask, o_pts, d_own, g_down, h_own;
};

Frame frame(int n)
{
    const size_t b_mask = round16((size_t)n);
    Frame        f;
    f.b_pts = sizeof(float) * 4 * (size_t)n;
    f.o_head = 32;
    f.o_mask = f.o_head + HEAD;
    f.o_pts = f.o_mask + b_mask;
    f.d_own = f.o_pts + f.b_pts;
    f.g_down = f.b_pts;
    f.h_own = f.g_down + HEAD + b_mask;
    return f;
}

bool grow(Status& ok, popsift_hip_verifier* v, size_t d_need, size_t h_need)
{
    if (ok.good() && d_need > v->d_cap) {
        if (v->d_buf) (void)hipFree(v->d_buf);
        v->d_buf = nullptr;
        v->d_cap = 0;
        if (ok(hipMalloc((void**)&v->d_buf, d_need))) v->d_cap = d_need;
    }
    if (ok.good() && h_need > v->h_cap) {
        if (v->h_buf) (void)hipHostFree(v->h_buf);
        v->h_buf = nullptr;
        v->h_cap = 0;
        if (ok(hipHostMalloc((void**)&v->h_buf, h_need, hipHostMallocDefault))) v->h_cap = h_need;
    }
    return ok.good();
}

/* the points go up through the pinned block, then k_ransac_bounds on zeroed bounds.  The launch is checked by the
 * hipGetLastError() that follows the caller's own launches */
bool upload(Status& ok, popsift_hip_verifier* v, const Frame& f, const float* pts, int n)
{
    auto* const d_pts = (const v4f*)(v->d_buf + f.o_pts);
    auto* const d_bounds = (uint32_t*)v->d_buf;
    memcpy(v->h_buf, pts, f.b_pts);
    if (ok(hipMemcpyAsync(v->d_buf + f.o_pts, v->h_buf, f.b_pts, hipMemcpyHostToDevice, v->stream)) &&
        ok(hipMemsetAsync(d_bounds, 0, 32, v->stream)))
        hipLaunchKernelGGL(k_ransac_bounds, dim3(std::min((n + 255) / 256, 512)), dim3(256), 0, v->stream, d_pts, n, d_bounds);
    return ok.good();
}

/* the record, the mask for a caller that takes it, and b_own bytes of the call's own arrays from o_own come down.  True
 * when they have arrived: the record at h_buf + g_down, the own bytes at h_buf + h_own, the mask in the caller's array */
bool download(Status& ok, popsift_hip_verifier* v, const Frame& f, int n, uint8_t* inlier, size_t o_own, size_t b_own)
{
    const size_t down = HEAD + (inlier ? (size_t)n : 0);
    ok.good() && ok(hipMemcpyAsync(v->h_buf + f.g_down, v->d_buf + f.o_head, down, hipMemcpyDeviceToHost, v->stream));
    if (ok.good() && b_own) ok(hipMemcpyAsync(v->h_buf + f.h_own, v->d_buf + o_own, b_own, hipMemcpyDeviceToHost, v->stream));
    if (!ok.good() || !ok(hipStreamSynchronize(v->stream))) return false;
    if (inlier) memcpy(inlier, v->h_buf + f.g_down + HEAD, (size_t)n);
    return true;
}

/* popsift_hip_ransac, popsift_hip_epipolar and their traces: the same launches but for the model kernel and the inlier
 * rule; a trace downloads three more arrays.  The layout of the scratch is a function of (n, T, kind) and every byte a
 * call reads it has written before, so nothing of an earlier call, whatever its kind, reaches a later one. */
template <int KIND>
int run(popsift_hip_verifier* v, const float* pts, int n, const Fit& fit, popsift_hip_ransac_result* res, uint8_t* inlier,
        bool trace, int32_t* samples, float* models, int32_t* counts)
{
    typedef Kind<KIND>        K;
    typedef typename K::Rule Rule;
    if (!args_valid(v, pts, n) || (!trace && !res)) return POPSIFT_HIP_ERR_INVALID;
    const int T = fit.hypotheses;
    if (n < K::m) { /* no sample exists */
        if (res) {
            memset(res, 0, sizeof *res);
            res->hypothesis = -1;
        }
        if (inlier && n > 0) memset(inlier, 0, (size_t)n);
        if (samples) memset(samples, 0xff, sizeof(int32_t) * K::row * (size_t)T);
        if (models) memset(models, 0, sizeof(float) * 9 * (size_t)T);
        if (counts) memset(counts, 0xff, sizeof(int32_t) * (size_t)T);
        return POPSIFT_HIP_OK;
    }
    if (hipSetDevice(v->device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    Status       ok;
    const Frame  f = frame(n);
    const size_t b_models = round16(sizeof(float) * 9 * (size_t)T), b_samples = sizeof(int) * K::row * (size_t)T,
                 b_counts = round16(sizeof(int) * (size_t)T), b_trace = b_models + b_samples + b_counts;
    /* the call's own arrays: [models][samples][counts], contiguous for the trace */
    const size_t o_models = f.d_own, o_samples = o_models + b_models, o_counts = o_samples + b_samples;
    if (!grow(ok, v, o_counts + b_counts, f.h_own + b_trace)) return ok.rc;
    hipStream_t const s = v->stream;
    char* const       d = v->d_buf;
    auto* const       d_bounds = (uint32_t*)d;
    auto* const       d_res = (popsift_hip_ransac_result*)(d + f.o_head);
    auto* const       d_mask = (uint32_t*)(d + f.o_mask);
    auto* const       d_pts = (const v4f*)(d + f.o_pts);
    auto* const       d_models = (float*)(d + o_models);
    auto* const       d_samples = (int*)(d + o_samples);
    auto* const       d_counts = (int*)(d + o_counts);
    const float       max_err2 = fit.max_err * fit.max_err;

    if (upload(ok, v, f, pts, n)) {
        const dim3 g_models((T + 63) / 64), g_score((T + S_HYP - 1) / S_HYP, (n + S_CHUNK - 1) / S_CHUNK), g_mask((n + 1023) / 1024);
        if constexpr (KIND == FIT_EPIPOLAR)
            hipLaunchKernelGGL(k_epipolar_models, g_models, dim3(64), 0, s, d_pts, n, T, fit.seed, d_bounds, d_models, d_samples,
                               d_counts);
        else
            hipLaunchKernelGGL(k_ransac_models<KIND>, g_models, dim3(64), 0, s, d_pts, n, T, fit.seed, d_bounds, d_models,
                               d_samples, d_counts);
        hipLaunchKernelGGL(k_ransac_score<Rule>, g_score, dim3(S_BLOCK), 0, s, d_pts, n, d_models, T, max_err2, d_counts);
        hipLaunchKernelGGL(k_ransac_select, dim3(1), dim3(256), 0, s, d_counts, d_models, T, K::m, d_res);
        hipLaunchKernelGGL(k_ransac_mask<Rule>, g_mask, dim3(256), 0, s, d_pts, n, d_res, max_err2, d_mask);
        ok(hipGetLastError());
    }
    if (download(ok, v, f, n, inlier, o_models, trace ? b_trace : 0)) {
        if (res) memcpy(res, v->h_buf + f.g_down, sizeof *res);
        const char* tr = v->h_buf + f.h_own;
        if (models) memcpy(models, tr, sizeof(float) * 9 * (size_t)T);
        if (samples) memcpy(samples, tr + b_models, b_samples);
        if (counts) memcpy(counts, tr + b_models + b_samples, sizeof(int) * (size_t)T);
    }
    return ok.rc;
}

/* popsift_hip_ransac and its trace: the model of the options becomes the kind here */
int run_ransac(popsift_hip_verifier* v, const float* pts, int n, const popsift_hip_ransac_opts* o, popsift_hip_ransac_result* res,
               uint8_t* inlier, bool trace, int32_t* samples, float* models, int32_t* counts)
{
    if (!opts_valid(o)) return POPSIFT_HIP_ERR_INVALID;
    const Fit fit{o->hypotheses, o->max_err, o->seed};
    return o->model == FIT_AFFINE ? run<FIT_AFFINE>(v, pts, n, fit, res, inlier, trace, samples, models, counts)
                                  : run<FIT_HOMOGRAPHY>(v, pts, n, fit, res, inlier, trace, samples, models, counts);
}

int run_epipolar(popsift_hip_verifier* v, const float* pts, int n, const popsift_hip_epipolar_opts* o,
                 popsift_hip_ransac_result* res, uint8_t* inlier, bool trace, int32_t* samples, float* models, int32_t* counts)
{
    if (!epipolar_opts_valid(o)) return POPSIFT_HIP_ERR_INVALID;
    return run<FIT_EPIPOLAR>(v, pts, n, Fit{o->hypotheses, o->max_err, o->seed}, res, inlier, trace, samples, models, counts);
}

/* ---- popsift_hip_ransac_many */

constexpr int MAX_LISTS = 1 << 20;

bool many_opts_valid(const popsift_hip_ransac_many_opts* o)
{
    return o && o->kind >= FIT_HOMOGRAPHY && o->kind <= FIT_EPIPOLAR && o->hypotheses >= 1 && o->hypotheses <= MAX_HYP &&
           std::isfinite(o->max_err) && o->max_err > 0.0f && o->reserved[0] == 0 && o->reserved[1] == 0 && o->reserved[2] == 0 &&
           o->reserved[3] == 0;
}

bool many_args_valid(const popsift_hip_verifier* v, const float* pts, const int32_t* offsets, int n_lists)
{
    if (!v || !offsets || n_lists < 0 || n_lists > MAX_LISTS || offsets[0] != 0) return false;
    for (int m = 0; m < n_lists; m++)
        if (offsets[m + 1] < offsets[m]) return false;
    return offsets[n_lists] <= MAX_PAIRS && (offsets[n_lists] == 0 || pts);
}

/* One upload (points, offsets, segments), the bounds of every list, then per group of consecutive lists the models, the
 * scores and the winners in that group's scratch, the masks of all lists, one download (records, masks) and one
 * synchronisation.  A trace brings each group's three arrays down before the next group overwrites them.
 * device: [bounds 32 / list][records][mask][points][offsets][segments][models][samples][counts], the last three for the
 * largest group; pinned: [points][offsets][segments][records][mask][the trace's models][samples][counts].  As in run()
 * the layout is a function of the arguments and every byte a call reads it has written before. */
template <int KIND>
int run_many(popsift_hip_verifier* v, const float* pts, const int32_t* offsets, int n_lists, const Fit& fit,
             popsift_hip_ransac_result* res, uint8_t* inlier, bool trace, int32_t* samples, float* models, int32_t* counts)
{
    typedef Kind<KIND>        K;
    typedef typename K::Rule Rule;
    const int    T = fit.hypotheses;
    const size_t P = (size_t)offsets[n_lists];
    const int    group = v->many_group > 0 ? v->many_group : POPSIFT_HIP_RANSAC_MANY_GROUP;
    const int    per_group = std::min(std::max(1, group / T), n_lists); /* lists of a group: at least one */
    const int    n_groups = (n_lists + per_group - 1) / per_group;
    size_t       n_seg = 0;
    for (int m = 0; m < n_lists; m++) n_seg += ((size_t)(offsets[m + 1] - offsets[m]) + G_SEG - 1) / G_SEG;

    const size_t recs = (size_t)per_group * T, all = (size_t)n_lists * T;
    const size_t b_bounds = 32 * (size_t)n_lists, b_res = round16(sizeof(popsift_hip_ransac_result) * (size_t)n_lists),
                 b_mask = round16(P), b_pts = sizeof(float) * 4 * P, b_off = round16(sizeof(int32_t) * ((size_t)n_lists + 1)),
                 b_segs = sizeof(Segment) * n_seg, b_up = b_pts + b_off + b_segs;
    const size_t o_res = b_bounds, o_mask = o_res + b_res, o_pts = o_mask + b_mask, o_off = o_pts + b_pts, o_segs = o_off + b_off,
                 o_models = o_segs + b_segs, o_samples = o_models + round16(sizeof(float) * 9 * recs),
                 o_counts = o_samples + sizeof(int) * K::row * recs, d_need = o_counts + round16(sizeof(int) * recs);
    const size_t h_res = b_up, h_models = h_res + b_res + b_mask, h_samples = h_models + round16(sizeof(float) * 9 * all),
                 h_counts = h_samples + sizeof(int) * K::row * all, h_need = trace ? h_counts + sizeof(int) * all : h_models;
    if (hipSetDevice(v->device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    Status ok;
    if (!grow(ok, v, d_need, h_need)) return ok.rc;
    hipStream_t const s = v->stream;
    char* const       d = v->d_buf;
    char* const       h = v->h_buf;
    auto* const       d_bounds = (uint32_t*)d;
    auto* const       d_res = (popsift_hip_ransac_result*)(d + o_res);
    auto* const       d_mask = (uint8_t*)(d + o_mask);
    auto* const       d_pts = (const v4f*)(d + o_pts);
    auto* const       d_off = (const int*)(d + o_off);
    auto* const       d_segs = (const Segment*)(d + o_segs);
    auto* const       d_models = (float*)(d + o_models);
    auto* const       d_samples = (int*)(d + o_samples);
    auto* const       d_counts = (int*)(d + o_counts);
    const float       max_err2 = fit.max_err * fit.max_err;

    /* the pinned block going up; seg0[g]: the first segment of group g */
    std::unique_ptr<size_t[]> seg0(new (std::nothrow) size_t[(size_t)n_groups + 1]);
    if (!seg0) return POPSIFT_HIP_ERR_OOM;
    if (b_pts) memcpy(h, pts, b_pts);
    memset(h + b_pts, 0, b_off);
    memcpy(h + b_pts, offsets, sizeof(int32_t) * ((size_t)n_lists + 1));
    Segment* sg = (Segment*)(h + b_pts + b_off);
    size_t   k = 0;
    for (int m = 0; m < n_lists; m++) {
        if (m % per_group == 0) seg0[m / per_group] = k;
        const int n = offsets[m + 1] - offsets[m];
        for (int i = 0; i < n; i += G_SEG) sg[k++] = Segment{m, offsets[m] + i, std::min(G_SEG, n - i), n <= G_SEG ? 1 : 0};
    }
    seg0[n_groups] = k;

    if (ok(hipMemcpyAsync(d + o_pts, h, b_up, hipMemcpyHostToDevice, s)) && ok(hipMemsetAsync(d_bounds, 0, b_bounds, s))) {
        if (n_seg) hipLaunchKernelGGL(k_many_bounds, dim3((unsigned)n_seg), dim3(G_BLOCK), 0, s, d_pts, d_segs, d_bounds);
        for (int g = 0; g < n_groups && ok.good(); g++) {
            const int    list0 = g * per_group, L = std::min(per_group, n_lists - list0);
            const size_t ns = seg0[g + 1] - seg0[g], r0 = (size_t)list0 * T, nr = (size_t)L * T;
            hipLaunchKernelGGL(k_many_models<KIND>, dim3(L, (T + 63) / 64), dim3(64), 0, s, d_pts, d_off, list0, T, fit.seed, d_bounds,
                               d_models, d_samples, d_counts);
            if (ns)
                hipLaunchKernelGGL(k_many_score<Rule>, dim3((unsigned)ns, (T + G_BLOCK - 1) / G_BLOCK), dim3(G_BLOCK), 0, s, d_pts,
                                   d_segs + seg0[g], list0, d_models, T, max_err2, d_counts);
            hipLaunchKernelGGL(k_many_select, dim3(L), dim3(256), 0, s, d_counts, d_models, T, K::m, d_res + list0);
            if (trace)
                ok(hipMemcpyAsync(h + h_models + sizeof(float) * 9 * r0, d_models, sizeof(float) * 9 * nr, hipMemcpyDeviceToHost, s)) &&
                    ok(hipMemcpyAsync(h + h_samples + sizeof(int) * K::row * r0, d_samples, sizeof(int) * K::row * nr,
                                      hipMemcpyDeviceToHost, s)) &&
                    ok(hipMemcpyAsync(h + h_counts + sizeof(int) * r0, d_counts, sizeof(int) * nr, hipMemcpyDeviceToHost, s));
        }
        if (n_seg && inlier)
            hipLaunchKernelGGL(k_many_mask<Rule>, dim3((unsigned)n_seg), dim3(G_BLOCK), 0, s, d_pts, d_segs, d_res, max_err2, d_mask);
        ok(hipGetLastError());
    }
    /* the records and, for a caller that takes them, the masks behind them */
    if (ok.good() && ok(hipMemcpyAsync(h + h_res, d + o_res, b_res + (inlier ? P : 0), hipMemcpyDeviceToHost, s)) &&
        ok(hipStreamSynchronize(s))) {
        if (res) memcpy(res, h + h_res, sizeof *res * (size_t)n_lists);
        if (inlier && P) memcpy(inlier, h + h_res + b_res, P);
        if (models) memcpy(models, h + h_models, sizeof(float) * 9 * all);
        if (samples) memcpy(samples, h + h_samples, sizeof(int) * K::row * all);
        if (counts) memcpy(counts, h + h_counts, sizeof(int) * all);
    }
    return ok.rc;
}

int ransac_many(popsift_hip_verifier* v, const float* pts, const int32_t* offsets, int n_lists, const popsift_hip_ransac_many_opts* o,
                popsift_hip_ransac_result* res, uint8_t* inlier, bool trace, int32_t* samples, float* models, int32_t* counts)
{
    if (!many_opts_valid(o) || !many_args_valid(v, pts, offsets, n_lists) || (!trace && !res)) return POPSIFT_HIP_ERR_INVALID;
    if (n_lists == 0) return POPSIFT_HIP_OK;
    const Fit fit{o->hypotheses, o->max_err, o->seed};
    return o->kind == FIT_HOMOGRAPHY ? run_many<FIT_HOMOGRAPHY>(v, pts, offsets, n_lists, fit, res, inlier, trace, samples, models, counts)
           : o->kind == FIT_AFFINE   ? run_many<FIT_AFFINE>(v, pts, offsets, n_lists, fit, res, inlier, trace, samples, models, counts)
                                     : run_many<FIT_EPIPOLAR>(v, pts, offsets, n_lists, fit, res, inlier, trace, samples, models, counts);
}

bool refit_opts_valid(const popsift_hip_refit_opts* o)
{
    if (!o || o->model < POPSIFT_HIP_REFIT_HOMOGRAPHY || o->model > POPSIFT_HIP_REFIT_EPIPOLAR || o->rounds < 1 ||
        o->rounds > F_ROUNDS || !std::isfinite(o->max_err) || !(o->max_err > 0.0f))
        return false;
    for (int i = 0; i < 9; i++)
        if (!std::isfinite(o->M[i])) return false;
    return o->reserved[0] == 0 && o->reserved[1] == 0 && o->reserved[2] == 0 && o->reserved[3] == 0;
}

/* popsift_hip_refit and its trace for one kind.  As in run() the layout of the scratch is a function of the arguments, and
 * every byte the call reads it has written before. */
template <int KIND>
int run_refit(popsift_hip_verifier* v, const float* pts, int n, const popsift_hip_refit_opts* o, popsift_hip_refit_result* res,
              uint8_t* inlier, bool trace, double* sums, float* models, int32_t* counts, int32_t* accepted)
{
    typedef typename Kind<KIND>::Rule Rule;
    constexpr int                     m = Kind<KIND>::m;
    if (!args_valid(v, pts, n) || !res) return POPSIFT_HIP_ERR_INVALID;
    const int R = o->rounds;
    if (n < m) { /* no model of this kind has support */
        memcpy(res->M, o->M, sizeof res->M);
        res->n_inliers = res->n_start = res->rounds = 0;
        res->stop = POPSIFT_HIP_REFIT_STOP_NO_SUPPORT;
        if (inlier && n > 0) memset(inlier, 0, (size_t)n);
        if (sums) memset(sums, 0, sizeof(double) * F_SLOTS * (size_t)R);
        if (models) memset(models, 0, sizeof(float) * 9 * (size_t)R);
        if (counts) memset(counts, 0xff, sizeof(int32_t) * (size_t)R);
        if (accepted) memset(accepted, 0, sizeof(int32_t) * (size_t)R);
        return POPSIFT_HIP_OK;
    }
    if (hipSetDevice(v->device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    Status       ok;
    const Frame  f = frame(n);
    const int    chunks = (n + F_CHUNK - 1) / F_CHUNK;
    const size_t b_trace = round16(sizeof(RefitTrace)), b_blocks = round16(sizeof(double) * F_SLOTS * (size_t)chunks),
                 b_spare = round16(sizeof(double) * F_SLOTS * (((size_t)chunks + 1) / 2));
    /* the call's own arrays: [trace][chunk sums][spare] */
    const size_t o_trace = f.d_own, o_blocks = o_trace + b_trace, o_spare = o_blocks + b_blocks;
    if (!grow(ok, v, o_spare + b_spare, f.h_own + b_trace)) return ok.rc;
    hipStream_t const s = v->stream;
    char* const       d = v->d_buf;
    auto* const       d_bounds = (uint32_t*)d;
    auto* const       d_st = (RefitState*)(d + f.o_head);
    auto* const       d_mask = (uint32_t*)(d + f.o_mask);
    auto* const       d_pts = (const v4f*)(d + f.o_pts);
    auto* const       d_tr = (RefitTrace*)(d + o_trace);
    auto* const       d_blocks = (double*)(d + o_blocks);
    auto* const       d_spare = (double*)(d + o_spare);
    const float       max_err2 = o->max_err * o->max_err;

    if (upload(ok, v, f, pts, n) && ok(hipMemsetAsync(d_tr, 0, b_trace, s))) {
        RefitStart start;
        memcpy(start.M, o->M, sizeof start.M);
        const dim3 g_quads((n + 1023) / 1024), g_chunks(chunks), wg(256);
        hipLaunchKernelGGL(k_refit_init, dim3(1), dim3(64), 0, s, start, d_st, d_tr);
        hipLaunchKernelGGL(k_refit_count<Rule>, g_quads, wg, 0, s, d_pts, n, d_st->H, max_err2, &d_st->n_inliers, &d_st->done);
        hipLaunchKernelGGL(k_refit_decide, dim3(1), dim3(64), 0, s, d_st, d_tr, -1, m);
        for (int r = 0; r < R; r++) {
            hipLaunchKernelGGL(k_refit_accumulate<KIND>, g_chunks, wg, 0, s, d_pts, n, d_bounds, d_st, max_err2, d_blocks);
            hipLaunchKernelGGL(k_refit_solve<KIND>, dim3(1), wg, 0, s, d_blocks, d_spare, chunks, d_bounds, d_st, d_tr, r);
            hipLaunchKernelGGL(k_refit_count<Rule>, g_quads, wg, 0, s, d_pts, n, d_tr->models[r], max_err2, &d_tr->counts[r],
                               &d_st->done);
            hipLaunchKernelGGL(k_refit_decide, dim3(1), dim3(64), 0, s, d_st, d_tr, r, m);
        }
        hipLaunchKernelGGL(k_ransac_mask<Rule>, g_quads, wg, 0, s, d_pts, n, (const popsift_hip_ransac_result*)d_st, max_err2, d_mask);
        ok(hipGetLastError());
    }
    if (download(ok, v, f, n, inlier, o_trace, trace ? sizeof(RefitTrace) : 0)) {
        RefitState st;
        memcpy(&st, v->h_buf + f.g_down, sizeof st);
        memcpy(res->M, st.H, sizeof res->M);
        res->n_inliers = st.n_inliers;
        res->n_start = st.n_start;
        res->rounds = st.rounds;
        res->stop = st.stop;
        const RefitTrace* tr = (const RefitTrace*)(v->h_buf + f.h_own);
        if (sums) memcpy(sums, tr->sums, sizeof(double) * F_SLOTS * (size_t)R);
        if (models) memcpy(models, tr->models, sizeof(float) * 9 * (size_t)R);
        if (counts) memcpy(counts, tr->counts, sizeof(int32_t) * (size_t)R);
        if (accepted) memcpy(accepted, tr->accepted, sizeof(int32_t) * (size_t)R);
    }
    return ok.rc;
}

/* popsift_hip_refit and its trace: the model of the options becomes the kind here */
int refit(popsift_hip_verifier* v, const float* pts, int n, const popsift_hip_refit_opts* o, popsift_hip_refit_result* res,
          uint8_t* inlier, bool trace, double* sums, float* models, int32_t* counts, int32_t* accepted)
{
    if (!refit_opts_valid(o)) return POPSIFT_HIP_ERR_INVALID;
    return o->model == FIT_HOMOGRAPHY ? run_refit<FIT_HOMOGRAPHY>(v, pts, n, o, res, inlier, trace, sums, models, counts, accepted)
           : o->model == FIT_AFFINE   ? run_refit<FIT_AFFINE>(v, pts, n, o, res, inlier, trace, sums, models, counts, accepted)
                                      : run_refit<FIT_EPIPOLAR>(v, pts, n, o, res, inlier, trace, sums, models, counts, accepted);
}

}  // namespace

extern "C" {

void popsift_hip_default_refit_opts(popsift_hip_refit_opts* o)
{
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->model = POPSIFT_HIP_REFIT_HOMOGRAPHY;
    o->rounds = 4;
    o->max_err = 2.0f;
    o->M[0] = o->M[4] = o->M[8] = 1.0f;
}

int popsift_hip_refit(popsift_hip_verifier* v, const float* pts, int n, const popsift_hip_refit_opts* o,
                      popsift_hip_refit_result* res, uint8_t* inlier)
{
    return refit(v, pts, n, o, res, inlier, false, nullptr, nullptr, nullptr, nullptr);
}

int popsift_hip_refit_trace(popsift_hip_verifier* v, const float* pts, int n, const popsift_hip_refit_opts* o,
                            popsift_hip_refit_result* res, uint8_t* inlier, double* sums, float* models, int32_t* counts,
                            int32_t* accepted)
{
    return refit(v, pts, n, o, res, inlier, true, sums, models, counts, accepted);
}

int popsift_hip_verifier_create(int device, popsift_hip_verifier** out)
{
    if (!out) return POPSIFT_HIP_ERR_INVALID;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return POPSIFT_HIP_ERR_NO_DEVICE;
    if (device < 0 || device >= count) return POPSIFT_HIP_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    popsift_hip_verifier* v = new (std::nothrow) popsift_hip_verifier();
    if (!v) return POPSIFT_HIP_ERR_OOM;
    v->device = device;
    if (hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking) != hipSuccess) {
        delete v;
        return POPSIFT_HIP_ERR_DEVICE;
    }
    *out = v;
    return POPSIFT_HIP_OK;
}

int popsift_hip_verifier_free(popsift_hip_verifier* v)
{
    if (!v) return POPSIFT_HIP_OK;
    (void)hipSetDevice(v->device);
    if (v->stream) (void)hipStreamDestroy(v->stream);
    if (v->d_buf) (void)hipFree(v->d_buf);
    if (v->h_buf) (void)hipHostFree(v->h_buf);
    delete v;
    return POPSIFT_HIP_OK;
}

void popsift_hip_default_ransac_opts(popsift_hip_ransac_opts* o)
{
    if (!o) return;
    o->model = POPSIFT_HIP_MODEL_HOMOGRAPHY;
    o->hypotheses = 2048;
    o->max_err = 2.0f;
    o->seed = 0;
    o->reserved[0] = o->reserved[1] = 0;
}

int popsift_hip_ransac(popsift_hip_verifier* v, const float* pts, int n, const popsift_hip_ransac_opts* o,
                       popsift_hip_ransac_result* res, uint8_t* inlier)
{
    return run_ransac(v, pts, n, o, res, inlier, false, nullptr, nullptr, nullptr);
}

int popsift_hip_ransac_trace(popsift_hip_verifier* v, const float* pts, int n, const popsift_hip_ransac_opts* o, int32_t* samples,
                             float* models, int32_t* counts)
{
    return run_ransac(v, pts, n, o, nullptr, nullptr, true, samples, models, counts);
}

void popsift_hip_default_epipolar_opts(popsift_hip_epipolar_opts* o)
{
    if (!o) return;
    o->hypotheses = 2048;
    o->max_err = 2.0f;
    o->seed = 0;
    o->reserved[0] = o->reserved[1] = o->reserved[2] = 0;
}

int popsift_hip_epipolar(popsift_hip_verifier* v, const float* pts, int n, const popsift_hip_epipolar_opts* o,
                         popsift_hip_ransac_result* res, uint8_t* inlier)
{
    return run_epipolar(v, pts, n, o, res, inlier, false, nullptr, nullptr, nullptr);
}

int popsift_hip_epipolar_trace(popsift_hip_verifier* v, const float* pts, int n, const popsift_hip_epipolar_opts* o,
                               int32_t* samples, float* models, int32_t* counts)
{
    return run_epipolar(v, pts, n, o, nullptr, nullptr, true, samples, models, counts);
}

void popsift_hip_default_ransac_many_opts(popsift_hip_ransac_many_opts* o)
{
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->kind = POPSIFT_HIP_REFIT_HOMOGRAPHY;
    o->hypotheses = 2048;
    o->max_err = 2.0f;
}

int popsift_hip_ransac_many(popsift_hip_verifier* v, const float* pts, const int32_t* offsets, int n_lists,
                            const popsift_hip_ransac_many_opts* o, popsift_hip_ransac_result* res, uint8_t* inlier)
{
    return ransac_many(v, pts, offsets, n_lists, o, res, inlier, false, nullptr, nullptr, nullptr);
}

int popsift_hip_ransac_many_trace(popsift_hip_verifier* v, const float* pts, const int32_t* offsets, int n_lists,
                                  const popsift_hip_ransac_many_opts* o, popsift_hip_ransac_result* res, uint8_t* inlier,
                                  int32_t* samples, float* models, int32_t* counts)
{
    return ransac_many(v, pts, offsets, n_lists, o, res, inlier, true, samples, models, counts);
}

int popsift_hip_verifier_debug_set_group(popsift_hip_verifier* v, int records)
{
    if (!v || records < 0) return POPSIFT_HIP_ERR_INVALID;
    v->many_group = records;
    return POPSIFT_HIP_OK;
}

int popsift_hip_pair_points(const popsift_hip_devfeatures* lc,const popsift_hip_devfeatures* r, const popsift_hip_pair* pairs,
                            int n, float* pts)
{
    if (!lc || !r || n < 0 || (n > 0 && (!pairs || !pts))) return POPSIFT_HIP_ERR_INVALID;
    for (int i = 0; i < n; i++)
        if (pairs[i].l < 0 || pairs[i].l >= lc->n_desc || pairs[i].r < 0 || pairs[i].r >= r->n_desc) return POPSIFT_HIP_ERR_INVALID;
    if (n == 0) return POPSIFT_HIP_OK;
    popsift_hip_devfeatures* l = const_cast<popsift_hip_devfeatures*>(lc);
    if (hipSetDevice(l->device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    Status            ok;
    hipStream_t const s = stream_of(ok, *l);
    /* device block and its pinned twin: a flag, the pairs, the points */
    const size_t b_pairs = sizeof(popsift_hip_pair) * (size_t)n, b_pts = sizeof(float) * 4 * (size_t)n, need = 16 + b_pairs + b_pts;
    grow_twin(ok, l->v_buf, l->v_host, l->v_cap, need);
    /* a right set on another GPU: its feature records and its map come over for the call */
    const DevFeature* rf = r->d_feat;
    const int*        rrev = r->d_rev;
    PeerCopy          peer;
    if (peer.fetch(ok, l->device, r->device,
                   {{r->d_feat, sizeof(DevFeature) * (size_t)std::max(r->n_feat, 1)}, {r->d_rev, sizeof(int) * (size_t)r->n_desc}})) {
        rf = (const DevFeature*)peer.at[0];
        rrev = (const int*)peer.at[1];
    }
    if (ok.good()) {
        char* const d = (char*)l->v_buf;
        char* const h = (char*)l->v_host;
        memset(h, 0, 16);
        memcpy(h + 16, pairs, b_pairs);
        if (ok(hipMemcpyAsync(d, h, 16 + b_pairs, hipMemcpyHostToDevice, s))) {
            hipLaunchKernelGGL(k_pair_points, dim3((n + 255) / 256), dim3(256), 0, s, (const popsift_hip_pair*)(d + 16), n,
                               l->d_feat, l->d_rev, l->n_feat, rf, rrev, r->n_feat, (v4f*)(d + 16 + b_pairs), (int*)d);
            ok(hipGetLastError());
        }
        /* the flag and the points come down; the pairs in between stay */
        if (ok.good() && ok(hipMemcpyAsync(h, d, 16, hipMemcpyDeviceToHost, s)) &&
            ok(hipMemcpyAsync(h + 16 + b_pairs, d + 16 + b_pairs, b_pts, hipMemcpyDeviceToHost, s)) && ok(hipStreamSynchronize(s))) {
            if (*(const int*)h != 0) ok.rc = POPSIFT_HIP_ERR_INVALID;
            else memcpy(pts, h + 16 + b_pairs, b_pts);
        }
    }
    return ok.rc;
}

} /* extern "C" */
