/*
 * epipolar_ref.c -- CPU restatement of the epipolar verifier's rule (include/popsift_hip.h, popsift_hip_epipolar), steps 1
 * to 7, one IEEE operation per line of the rule.  Build with gcc -O2 -ffp-contract=off (tests/epipolar_rule.py): fma() /
 * fmaf() are the only fused operations.
 *
 * `variant` deliberately breaks one step, so that tests can show that a scene depends on it:
 *   1  ties of the selection go to the HIGHEST hypothesis index
 *   2  the inlier test drops `g > 0`, also where it meets the all-zero model of an invalid hypothesis
 *   4  the pivot search stays in column k (partial pivoting): the last unknown is fixed to 1
 *   8  no rank-2 step
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define M 8

/* ---- 1. sample */

static uint32_t mix(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352dU;
    x ^= x >> 15;
    x *= 0x846ca68bU;
    x ^= x >> 16;
    return x;
}

/* 8 indices, -1 from the first slot that found no new index in its 9 draws; returns 0 for such a sample */
static int sample(uint32_t seed, int t, int n, int32_t idx[M])
{
    const uint32_t base = mix(mix(seed + 0x9e3779b9U) ^ (uint32_t)t);
    uint32_t       c = 0;
    for (int k = 0; k < M; k++) idx[k] = -1;
    for (int k = 0; k < M; k++) {
        int got = 0;
        for (int draw = 0; draw < 9 && !got; draw++) {
            c++;
            const uint32_t h = mix(base + 0x9e3779b9U * c);
            const int32_t  i = (int32_t)(((uint64_t)h * (uint64_t)(uint32_t)n) >> 32);
            int            seen = 0;
            for (int j = 0; j < k; j++) seen |= idx[j] == i;
            if (!seen) {
                idx[k] = i;
                got = 1;
            }
        }
        if (!got) return 0;
    }
    return 1;
}

/* ---- 2. normalise */

typedef struct Norm {
    double cx, cy, s, k; /* centre, scale (half extent, or 1), 1 / s */
} Norm;

/* float bits as an unsigned key that orders like the value, -0 below +0 */
static uint32_t order_key(float f)
{
    uint32_t b;
    memcpy(&b, &f, 4);
    return (b & 0x80000000U) ? ~b : (b | 0x80000000U);
}
static float key_value(uint32_t k)
{
    const uint32_t b = (k & 0x80000000U) ? (k & 0x7fffffffU) : ~k;
    float          f;
    memcpy(&f, &b, 4);
    return f;
}

static void bounds(const float* pts, int n, int col, double* centre, double* half)
{
    uint32_t lo = 0xffffffffU, hi = 0;
    int      any = 0;
    for (int i = 0; i < n; i++) {
        const float f = pts[4 * (size_t)i + col];
        if (!isfinite(f)) continue;
        const uint32_t k = order_key(f);
        if (k < lo) lo = k;
        if (k > hi) hi = k;
        any = 1;
    }
    if (!any) {
        *centre = 0.0;
        *half = 0.0;
        return;
    }
    const double a = (double)key_value(lo), b = (double)key_value(hi);
    *centre = (a + b) * 0.5;
    *half = (b - a) * 0.5;
}

static Norm normaliser(const float* pts, int n, int col)
{
    Norm   q;
    double hx, hy;
    bounds(pts, n, col, &q.cx, &hx);
    bounds(pts, n, col + 1, &q.cy, &hy);
    const double e = hx > hy ? hx : hy;
    q.s = e > 0.0 ? e : 1.0;
    q.k = 1.0 / q.s;
    return q;
}

/* ---- 3. solve: the null vector of the 8 x 9 system by Gaussian elimination with complete pivoting; 0 when a pivot is 0 */

static int null_vector(double a[M][9], double f[9], int variant)
{
    int perm[9];
    for (int j = 0; j < 9; j++) perm[j] = j;
    for (int k = 0; k < M; k++) {
        int    pr = k, pc = k;
        double best = fabs(a[k][k]);
        const int c_end = (variant & 4) ? k + 1 : 9;
        for (int c = k; c < c_end; c++) /* column-major: the lowest column, then the lowest row, wins a tie */
            for (int r = k; r < M; r++) {
                const double v = fabs(a[r][c]);
                if (v > best) {
                    best = v;
                    pr = r;
                    pc = c;
                }
            }
        if (pr != k)
            for (int j = 0; j < 9; j++) {
                const double tmp = a[k][j];
                a[k][j] = a[pr][j];
                a[pr][j] = tmp;
            }
        if (pc != k) {
            for (int r = 0; r < M; r++) {
                const double tmp = a[r][k];
                a[r][k] = a[r][pc];
                a[r][pc] = tmp;
            }
            const int tmp = perm[k];
            perm[k] = perm[pc];
            perm[pc] = tmp;
        }
        if (a[k][k] == 0.0) return 0;
        for (int r = k + 1; r < M; r++) {
            const double q = a[r][k] / a[k][k];
            for (int j = k + 1; j < 9; j++) a[r][j] = fma(-q, a[k][j], a[r][j]);
        }
    }
    double z[9];
    z[8] = 1.0; /* the free column's unknown */
    for (int i = M - 1; i >= 0; i--) {
        double s = -a[i][8];
        for (int j = i + 1; j < M; j++) s = fma(-a[i][j], z[j], s);
        z[i] = s / a[i][i];
    }
    for (int j = 0; j < 9; j++) f[perm[j]] = z[j];
    return 1;
}

/* ---- 4. rank 2: f <- f - (f v) v^T, v the eigenvector of f^T f under its smallest eigenvalue (cyclic Jacobi) */

static void rotate(double m[3][3], double v[3][3], int p, int q, int o)
{
    if (m[p][q] == 0.0) return;
    const double d = m[q][q] - m[p][p];
    const double e = 2.0 * m[p][q];
    const double theta = d / e;
    const double root = sqrt(fma(theta, theta, 1.0));
    const double den = fabs(theta) + root;
    const double t = copysign(1.0, theta) / den;
    const double c = 1.0 / sqrt(fma(t, t, 1.0));
    const double s = t * c;
    m[p][p] = fma(-t, m[p][q], m[p][p]);
    m[q][q] = fma(t, m[p][q], m[q][q]);
    m[p][q] = m[q][p] = 0.0;
    const double mp = m[o][p], mq = m[o][q];
    m[o][p] = m[p][o] = fma(-s, mq, c * mp);
    m[o][q] = m[q][o] = fma(s, mp, c * mq);
    for (int r = 0; r < 3; r++) {
        const double vp = v[r][p], vq = v[r][q];
        v[r][p] = fma(-s, vq, c * vp);
        v[r][q] = fma(s, vp, c * vq);
    }
}

static void rank2(double f[9])
{
    double m[3][3], v[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = i; j < 3; j++) m[i][j] = m[j][i] = fma(f[i], f[j], fma(f[3 + i], f[3 + j], f[6 + i] * f[6 + j]));
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 6; sweep++) {
        rotate(m, v, 0, 1, 2);
        rotate(m, v, 0, 2, 1);
        rotate(m, v, 1, 2, 0);
    }
    int b = 0;
    if (m[1][1] < m[b][b]) b = 1;
    if (m[2][2] < m[b][b]) b = 2;
    for (int i = 0; i < 3; i++) {
        const double w = fma(f[3 * i], v[0][b], fma(f[3 * i + 1], v[1][b], f[3 * i + 2] * v[2][b]));
        for (int j = 0; j < 3; j++) f[3 * i + j] = fma(-w, v[j][b], f[3 * i + j]);
    }
}

/* the model of one sample: 9 floats, or 0 */
static int solve(const float* pts, const int32_t idx[M], const Norm* L, const Norm* Rn, int variant, float F[9])
{
    double a[M][9], f[9];
    for (int i = 0; i < M; i++) {
        const float* p = pts + 4 * (size_t)idx[i];
        const double x = ((double)p[0] - L->cx) * L->k;
        const double y = ((double)p[1] - L->cy) * L->k;
        const double u = ((double)p[2] - Rn->cx) * Rn->k;
        const double v = ((double)p[3] - Rn->cy) * Rn->k;
        a[i][0] = u * x; a[i][1] = u * y; a[i][2] = u;
        a[i][3] = v * x; a[i][4] = v * y; a[i][5] = v;
        a[i][6] = x; a[i][7] = y; a[i][8] = 1.0;
    }
    if (!null_vector(a, f, variant)) return 0;
    if (!(variant & 8)) rank2(f);
    /* ---- 5. denormalise: G = Fn * Tl, then H = Tr^T * G; scale by the entry of largest magnitude */
    double g[9], h[9];
    for (int i = 0; i < 3; i++) {
        g[3 * i] = f[3 * i] * L->k;
        g[3 * i + 1] = f[3 * i + 1] * L->k;
        g[3 * i + 2] = fma(-g[3 * i], L->cx, fma(-g[3 * i + 1], L->cy, f[3 * i + 2]));
    }
    for (int j = 0; j < 3; j++) {
        h[j] = g[j] * Rn->k;
        h[3 + j] = g[3 + j] * Rn->k;
        h[6 + j] = fma(-h[j], Rn->cx, fma(-h[3 + j], Rn->cy, g[6 + j]));
    }
    int    b = 0;
    double best = fabs(h[0]);
    for (int i = 1; i < 9; i++) {
        const double v = fabs(h[i]);
        if (v > best) {
            best = v;
            b = i;
        }
    }
    const double d = h[b];
    if (d == 0.0) return 0;
    int ok = 1;
    for (int i = 0; i < 9; i++) {
        F[i] = (float)(h[i] / d);
        ok &= isfinite(F[i]) != 0;
    }
    return ok;
}

/* ---- 6. score */

static int inlier(const float* F, const float* p, float max_err, int variant)
{
    const float x = p[0], y = p[1], xr = p[2], yr = p[3];
    const float a = fmaf(F[0], x, fmaf(F[1], y, F[2]));
    const float b = fmaf(F[3], x, fmaf(F[4], y, F[5]));
    const float c = fmaf(F[6], x, fmaf(F[7], y, F[8]));
    const float d = fmaf(F[0], xr, fmaf(F[3], yr, F[6]));
    const float e = fmaf(F[1], xr, fmaf(F[4], yr, F[7]));
    const float r = fmaf(a, xr, fmaf(b, yr, c));
    const float g = fmaf(a, a, fmaf(b, b, fmaf(d, d, e * e)));
    const float lim = (max_err * max_err) * g;
    return ((variant & 2) || g > 0.0f) && g < INFINITY && r * r <= lim;
}

/*
 * The whole rule.  samples: T x 8, models: T x 9, counts: T (any may be null).  result: F[9] as floats, then n_inliers,
 * hypothesis, n_valid, 0 as int32 (the 52 bytes of popsift_hip_ransac_result).  mask: n bytes or null.
 */
void er_epipolar(const float* pts, int n, int T, float max_err, uint32_t seed, int variant, int32_t* samples, float* models,
                 int32_t* counts, void* result, uint8_t* mask)
{
    float bestF[9] = {0};
    int   best = -1, best_t = -1, n_valid = 0;
    Norm  L, R;
    if (n >= M) {
        L = normaliser(pts, n, 0);
        R = normaliser(pts, n, 2);
    }
    for (int t = 0; t < T; t++) {
        int32_t idx[M] = {-1, -1, -1, -1, -1, -1, -1, -1};
        float   F[9] = {0};
        int     cnt = -1;
        if (n >= M && sample(seed, t, n, idx)) {
            if (solve(pts, idx, &L, &R, variant, F)) {
                cnt = 0;
                for (int i = 0; i < n; i++) cnt += inlier(F, pts + 4 * (size_t)i, max_err, variant);
            } else {
                memset(F, 0, sizeof F);
            }
        }
        /* variant 2: what scoring the stored all-zero model of an invalid hypothesis adds to its -1 without `g > 0` */
        if ((variant & 2) && n >= M && cnt < 0)
            for (int i = 0; i < n; i++) cnt += inlier(F, pts + 4 * (size_t)i, max_err, variant);
        if (samples) memcpy(samples + M * (size_t)t, idx, sizeof idx);
        if (models) memcpy(models + 9 * (size_t)t, F, sizeof F);
        if (counts) counts[t] = cnt;
        if (cnt >= 0) n_valid++;
        if (cnt > best || ((variant & 1) && cnt >= 0 && cnt == best)) {
            best = cnt;
            best_t = t;
            memcpy(bestF, F, sizeof F);
        }
    }
    if (best < M) { /* ---- 7. select: no winner below a sample's size */
        best_t = -1;
        best = 0;
        memset(bestF, 0, sizeof bestF);
    }
    if (mask)
        for (int i = 0; i < n; i++) mask[i] = best_t >= 0 ? (uint8_t)inlier(bestF, pts + 4 * (size_t)i, max_err, variant) : 0;
    if (result) {
        int32_t tail[4] = {best, best_t, n_valid, 0};
        memcpy(result, bestF, sizeof bestF);
        memcpy((char*)result + sizeof bestF, tail, sizeof tail);
    }
}

/* the sampler alone: T x 8 indices, valid[t] = 1 when the sample is complete */
void er_samples(uint32_t seed, int n, int T, int32_t* samples, int32_t* valid)
{
    for (int t = 0; t < T; t++) valid[t] = sample(seed, t, n, samples + M * (size_t)t);
}
