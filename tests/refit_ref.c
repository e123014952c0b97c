/*
 * refit_ref.c -- CPU restatement of the verifier's least-squares refit (include/popsift_hip.h, popsift_hip_refit), steps 1
 * to 5, one IEEE operation per line of the rule.  Build with gcc -O2 -ffp-contract=off (tests/refit_rule.py): fma() /
 * fmaf() are the only fused operations.
 *
 * `variant` deliberately breaks one step, so that tests can show that a scene depends on it:
 *   1   the sums run over all pairs, not over the inliers of the current model
 *   2   a sum is formed left to right, not as the pairwise tree
 *   4   a candidate with fewer inliers than the current model is accepted
 *   8   the transfer test drops `w > 0`
 *   16  a pair with a coordinate that is not finite enters the sums
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

enum { KIND_HOMOGRAPHY = 0, KIND_AFFINE = 1, KIND_EPIPOLAR = 2 };
enum { STOP_ROUNDS = 0, STOP_CONVERGED = 1, STOP_NOT_BETTER = 2, STOP_NO_FIT = 3, STOP_NO_SUPPORT = 4 };
#define SLOTS 45

/* ---- 1. normalise (step 2 of popsift_hip_ransac) */

typedef struct Norm {
    double cx, cy, s, k; /* centre, scale (half extent, or 1), 1 / s */
} Norm;

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

/* ---- 2. the kinds' inlier tests: step 4 of popsift_hip_ransac, step 6 of popsift_hip_epipolar */

static int inlier(int kind, const float* M, const float* p, float max_err, int variant)
{
    const float x = p[0], y = p[1], xr = p[2], yr = p[3];
    if (kind == KIND_EPIPOLAR) {
        const float a = fmaf(M[0], x, fmaf(M[1], y, M[2]));
        const float b = fmaf(M[3], x, fmaf(M[4], y, M[5]));
        const float c = fmaf(M[6], x, fmaf(M[7], y, M[8]));
        const float d = fmaf(M[0], xr, fmaf(M[3], yr, M[6]));
        const float e = fmaf(M[1], xr, fmaf(M[4], yr, M[7]));
        const float r = fmaf(a, xr, fmaf(b, yr, c));
        const float g = fmaf(a, a, fmaf(b, b, fmaf(d, d, e * e)));
        const float lim = (max_err * max_err) * g;
        return g > 0.0f && g < INFINITY && r * r <= lim;
    }
    const float u = fmaf(M[0], x, fmaf(M[1], y, M[2]));
    const float v = fmaf(M[3], x, fmaf(M[4], y, M[5]));
    const float w = fmaf(M[6], x, fmaf(M[7], y, M[8]));
    const float dx = fmaf(-w, xr, u);
    const float dy = fmaf(-w, yr, v);
    const float e = fmaf(dx, dx, dy * dy);
    const float lim = (max_err * max_err) * (w * w);
    return ((variant & 8) || w > 0.0f) && e <= lim;
}

static int count(int kind, const float* M, const float* pts, int n, float max_err, int variant)
{
    int c = 0;
    for (int i = 0; i < n; i++) c += inlier(kind, M, pts + 4 * (size_t)i, max_err, variant);
    return c;
}

/* ---- 3a. the terms of one pair, in the slot layout of the header */

static void terms(int kind, const float* p, const Norm* L, const Norm* Rn, double t[SLOTS])
{
    const double x = ((double)p[0] - L->cx) * L->k;
    const double y = ((double)p[1] - L->cy) * L->k;
    const double u = ((double)p[2] - Rn->cx) * Rn->k;
    const double v = ((double)p[3] - Rn->cy) * Rn->k;
    for (int j = 0; j < SLOTS; j++) t[j] = 0.0;
    if (kind == KIND_EPIPOLAR) {
        const double a[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1.0};
        int          s = 0;
        for (int j = 0; j < 9; j++)
            for (int k = j; k < 9; k++) t[s++] = a[j] * a[k];
        return;
    }
    t[0] = x * x; t[1] = x * y; t[2] = x; t[3] = y * y; t[4] = y; t[5] = 1.0;
    t[21] = x * u; t[22] = y * u; t[23] = u; t[24] = x * v; t[25] = y * v; t[26] = v;
    if (kind == KIND_AFFINE) return;
    const double p6 = -u * x, p7 = -u * y, q6 = -v * x, q7 = -v * y;
    t[6] = x * p6; t[7] = x * p7; t[8] = y * p6; t[9] = y * p7; t[10] = p6; t[11] = p7;
    t[12] = x * q6; t[13] = x * q7; t[14] = y * q6; t[15] = y * q7; t[16] = q6; t[17] = q7;
    t[18] = fma(p6, p6, q6 * q6);
    t[19] = fma(p6, p7, q6 * q7);
    t[20] = fma(p7, p7, q7 * q7);
    t[27] = fma(p6, u, q6 * v);
    t[28] = fma(p7, u, q7 * v);
}

/* ---- 3b. the sums: the pairwise tree over the pair index, fed pair by pair.  level[l] holds tree(a, 2^l) of the last
 * complete block of 2^l pairs whose right sibling is still open; pair i closes as many levels as i has trailing one bits. */

static void sums_of(int kind, const float* cur, const float* pts, int n, const Norm* L, const Norm* Rn, float max_err,
                    int variant, double sum[SLOTS])
{
    static double level[26][SLOTS];
    double        t[SLOTS];
    int           P = 1;
    while (P < n) P *= 2;
    for (int j = 0; j < SLOTS; j++) sum[j] = 0.0;
    for (int i = 0; i < P; i++) {
        int in = 0;
        if (i < n) {
            const float* p = pts + 4 * (size_t)i;
            in = (variant & 1) || inlier(kind, cur, p, max_err, variant);
            if ((variant & 16) && !(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && isfinite(p[3]))) in = 1;
            if (in) terms(kind, p, L, Rn, t);
        }
        for (int j = 0; j < SLOTS; j++) t[j] = in ? t[j] + 0.0 : 0.0; /* a term of -0.0 enters as +0.0 */
        if (variant & 2) {
            for (int j = 0; j < SLOTS; j++) sum[j] = sum[j] + t[j];
            continue;
        }
        int l = 0;
        for (int b = i; b & 1; b >>= 1, l++)
            for (int j = 0; j < SLOTS; j++) t[j] = level[l][j] + t[j];
        for (int j = 0; j < SLOTS; j++) level[l][j] = t[j];
        if (i == P - 1)
            for (int j = 0; j < SLOTS; j++) sum[j] = t[j];
    }
}

/* ---- 3c. solve */

/* partial pivoting on an R x (R + NB) augmented system (step 3 of popsift_hip_ransac); 0 when a pivot is exactly 0 */
static int eliminate(double a[8][9], int R, int NB)
{
    const int C = R + NB;
    for (int c = 0; c < R; c++) {
        int    p = c;
        double best = fabs(a[c][c]);
        for (int r = c + 1; r < R; r++) {
            const double v = fabs(a[r][c]);
            if (v > best) {
                best = v;
                p = r;
            }
        }
        if (p != c)
            for (int j = 0; j < C; j++) {
                const double tmp = a[c][j];
                a[c][j] = a[p][j];
                a[p][j] = tmp;
            }
        if (a[c][c] == 0.0) return 0;
        for (int r = c + 1; r < R; r++) {
            const double f = a[r][c] / a[c][c];
            for (int j = c + 1; j < C; j++) a[r][j] = fma(-f, a[c][j], a[r][j]);
        }
    }
    for (int b = 0; b < NB; b++)
        for (int i = R - 1; i >= 0; i--) {
            double s = a[i][R + b];
            for (int j = i + 1; j < R; j++) s = fma(-a[i][j], a[j][R + b], s);
            a[i][R + b] = s / a[i][i];
        }
    return 1;
}

/* complete pivoting on the 9 x 9 normal matrix, eight steps (step 3 of popsift_hip_epipolar with a ninth row) */
static int null_vector(double a[9][9], double f[9])
{
    int perm[9];
    for (int j = 0; j < 9; j++) perm[j] = j;
    for (int k = 0; k < 8; k++) {
        int    pr = k, pc = k;
        double best = fabs(a[k][k]);
        for (int c = k; c < 9; c++)
            for (int r = k; r < 9; r++) {
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
            for (int r = 0; r < 9; r++) {
                const double tmp = a[r][k];
                a[r][k] = a[r][pc];
                a[r][pc] = tmp;
            }
            const int tmp = perm[k];
            perm[k] = perm[pc];
            perm[pc] = tmp;
        }
        if (a[k][k] == 0.0) return 0;
        for (int r = k + 1; r < 9; r++) {
            const double q = a[r][k] / a[k][k];
            for (int j = k + 1; j < 9; j++) a[r][j] = fma(-q, a[k][j], a[r][j]);
        }
    }
    double z[9];
    z[8] = 1.0; /* row 8 is dropped; the unknown of the column left over */
    for (int i = 7; i >= 0; i--) {
        double s = -a[i][8];
        for (int j = i + 1; j < 8; j++) s = fma(-a[i][j], z[j], s);
        z[i] = s / a[i][i];
    }
    for (int j = 0; j < 9; j++) f[perm[j]] = z[j];
    return 1;
}

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

/* the candidate of one round's sums: 9 floats, or 0 */
static int solve(int kind, const double s[SLOTS], const Norm* L, const Norm* Rn, float out[9])
{
    double h[9];
    if (kind == KIND_EPIPOLAR) {
        double a[9][9], f[9], g[9];
        int    k = 0;
        for (int i = 0; i < 9; i++)
            for (int j = i; j < 9; j++) a[i][j] = a[j][i] = s[k++];
        if (!null_vector(a, f)) return 0;
        rank2(f);
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
        for (int i = 0; i < 9; i++) h[i] = h[i] / d;
    } else {
        double a[8][9], g[9];
        if (kind == KIND_AFFINE) {
            const double n3[3][3] = {{s[0], s[1], s[2]}, {s[1], s[3], s[4]}, {s[2], s[4], s[5]}};
            for (int i = 0; i < 3; i++) {
                for (int j = 0; j < 3; j++) a[i][j] = n3[i][j];
                a[i][3] = s[21 + i];
                a[i][4] = s[24 + i];
            }
            if (!eliminate(a, 3, 2)) return 0;
            for (int i = 0; i < 3; i++) {
                g[i] = a[i][3];
                g[3 + i] = a[i][4];
            }
            g[6] = 0.0;
            g[7] = 0.0;
        } else {
            const double n3[3][3] = {{s[0], s[1], s[2]}, {s[1], s[3], s[4]}, {s[2], s[4], s[5]}};
            for (int i = 0; i < 8; i++)
                for (int j = 0; j < 8; j++) a[i][j] = 0.0;
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) a[i][j] = a[3 + i][3 + j] = n3[i][j];
            for (int i = 0; i < 3; i++) {
                a[i][6] = a[6][i] = s[6 + 2 * i];
                a[i][7] = a[7][i] = s[7 + 2 * i];
                a[3 + i][6] = a[6][3 + i] = s[12 + 2 * i];
                a[3 + i][7] = a[7][3 + i] = s[13 + 2 * i];
            }
            a[6][6] = s[18];
            a[6][7] = a[7][6] = s[19];
            a[7][7] = s[20];
            for (int i = 0; i < 8; i++) a[i][8] = s[21 + i];
            if (!eliminate(a, 8, 1)) return 0;
            for (int i = 0; i < 8; i++) g[i] = a[i][8];
        }
        g[8] = 1.0;
        double mm[9];
        for (int i = 0; i < 3; i++) {
            mm[3 * i] = g[3 * i] * L->k;
            mm[3 * i + 1] = g[3 * i + 1] * L->k;
            mm[3 * i + 2] = fma(-mm[3 * i], L->cx, fma(-mm[3 * i + 1], L->cy, g[3 * i + 2]));
        }
        for (int j = 0; j < 3; j++) {
            h[j] = fma(Rn->s, mm[j], Rn->cx * mm[6 + j]);
            h[3 + j] = fma(Rn->s, mm[3 + j], Rn->cy * mm[6 + j]);
            h[6 + j] = mm[6 + j];
        }
    }
    int ok = 1;
    for (int i = 0; i < 9; i++) {
        out[i] = (float)h[i];
        ok &= isfinite(out[i]) != 0;
    }
    return ok;
}

/*
 * The whole rule.  sums: rounds x 45, models: rounds x 9, counts: rounds, accepted: rounds (any may be null).  result: M[9]
 * as floats, then n_inliers, n_start, rounds, stop as int32 (the 52 bytes of popsift_hip_refit_result).  mask: n bytes or
 * null.
 */
void rf_refit(const float* pts, int n, int kind, int rounds, float max_err, const float* M, int variant, double* sums,
              float* models, int32_t* counts, int32_t* accepted, void* result, uint8_t* mask)
{
    const int m = kind == KIND_EPIPOLAR ? 8 : kind == KIND_AFFINE ? 3 : 4;
    float     cur[9];
    int       c_cur = 0, n_start = 0, done_rounds = 0, stop = STOP_ROUNDS;
    memcpy(cur, M, sizeof cur);
    if (sums) memset(sums, 0, sizeof(double) * SLOTS * (size_t)rounds);
    if (models) memset(models, 0, sizeof(float) * 9 * (size_t)rounds);
    if (accepted) memset(accepted, 0, sizeof(int32_t) * (size_t)rounds);
    if (counts)
        for (int r = 0; r < rounds; r++) counts[r] = -1;
    if (n < m) { /* answered without looking at the points */
        stop = STOP_NO_SUPPORT;
        if (mask && n > 0) memset(mask, 0, (size_t)n);
    } else {
        const Norm L = normaliser(pts, n, 0), Rn = normaliser(pts, n, 2);
        c_cur = n_start = count(kind, cur, pts, n, max_err, variant);
        if (c_cur < m) stop = STOP_NO_SUPPORT;
        for (int r = 0; r < rounds && stop == STOP_ROUNDS; r++) {
            double s[SLOTS];
            float  cand[9];
            sums_of(kind, cur, pts, n, &L, &Rn, max_err, variant, s);
            if (sums) memcpy(sums + SLOTS * (size_t)r, s, sizeof s);
            if (!solve(kind, s, &L, &Rn, cand)) {
                stop = STOP_NO_FIT;
                break;
            }
            const int c_new = count(kind, cand, pts, n, max_err, variant);
            if (models) memcpy(models + 9 * (size_t)r, cand, sizeof cand);
            if (counts) counts[r] = c_new;
            if (memcmp(cand, cur, sizeof cur) == 0) {
                stop = STOP_CONVERGED;
            } else if (c_new < c_cur && !(variant & 4)) {
                stop = STOP_NOT_BETTER;
            } else {
                memcpy(cur, cand, sizeof cur);
                c_cur = c_new;
                done_rounds++;
                if (accepted) accepted[r] = 1;
            }
        }
        if (mask)
            for (int i = 0; i < n; i++) mask[i] = (uint8_t)inlier(kind, cur, pts + 4 * (size_t)i, max_err, variant);
    }
    if (result) {
        int32_t tail[4] = {c_cur, n_start, done_rounds, stop};
        memcpy(result, cur, sizeof cur);
        memcpy((char*)result + sizeof cur, tail, sizeof tail);
    }
}

/* the inliers of M under the kind's test: n bytes */
void rf_mask(const float* pts, int n, int kind, float max_err, const float* M, uint8_t* mask)
{
    for (int i = 0; i < n; i++) mask[i] = (uint8_t)inlier(kind, M, pts + 4 * (size_t)i, max_err, 0);
}

/* the terms of every pair (n x 45), whether inlier or not, for tests that restate the tree */
void rf_terms(const float* pts, int n, int kind, double* out)
{
    const Norm L = normaliser(pts, n, 0), Rn = normaliser(pts, n, 2);
    for (int i = 0; i < n; i++) {
        terms(kind, pts + 4 * (size_t)i, &L, &Rn, out + SLOTS * (size_t)i);
        for (int j = 0; j < SLOTS; j++) out[SLOTS * (size_t)i + j] = out[SLOTS * (size_t)i + j] + 0.0;
    }
}
