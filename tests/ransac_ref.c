/*
 * ransac_ref.c -- CPU restatement of the verifier's rule (include/popsift_hip.h, popsift_hip_ransac), steps 1 to 5, one
 * IEEE operation per line of the rule.  Build with gcc -O2 -ffp-contract=off (tests/ransac_rule.py): fma() / fmaf() are
 * the only fused operations.
 *
 * `variant` deliberately breaks one step, so that tests can show that a scene depends on it:
 *   1  ties of the selection go to the HIGHEST hypothesis index
 *   2  the inlier test drops `w > 0`
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define MODEL_HOMOGRAPHY 0
#define MODEL_AFFINE 1

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

/* m indices into idx[0 .. m-1], the rest -1; returns 0 when a slot found no new index in its 9 draws */
static int sample(uint32_t seed, int t, int n, int m, int32_t idx[4])
{
    const uint32_t base = mix(mix(seed + 0x9e3779b9U) ^ (uint32_t)t);
    uint32_t       c = 0;
    idx[0] = idx[1] = idx[2] = idx[3] = -1;
    for (int k = 0; k < m; k++) {
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

/* ---- 3. solve: Gaussian elimination with partial pivoting on an R x (R + NB) augmented system, in place; the solution
 * of right-hand side b is left in column R + b.  Returns 0 when a pivot is exactly 0. */
#define MAXR 8
#define MAXC 9
static int eliminate(double a[MAXR][MAXC], int R, int NB)
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

/* the model of one sample: 9 floats, or 0 */
static int solve(const float* pts, const int32_t idx[4], int model, const Norm* L, const Norm* Rn, float H[9])
{
    double a[MAXR][MAXC];
    double g[9];
    const int m = model == MODEL_AFFINE ? 3 : 4;
    double x[4], y[4], u[4], v[4];
    for (int i = 0; i < m; i++) {
        const float* p = pts + 4 * (size_t)idx[i];
        x[i] = ((double)p[0] - L->cx) * L->k;
        y[i] = ((double)p[1] - L->cy) * L->k;
        u[i] = ((double)p[2] - Rn->cx) * Rn->k;
        v[i] = ((double)p[3] - Rn->cy) * Rn->k;
    }
    if (model == MODEL_AFFINE) {
        for (int i = 0; i < 3; i++) {
            a[i][0] = x[i];
            a[i][1] = y[i];
            a[i][2] = 1.0;
            a[i][3] = u[i];
            a[i][4] = v[i];
        }
        if (!eliminate(a, 3, 2)) return 0;
        for (int i = 0; i < 3; i++) {
            g[i] = a[i][3];
            g[3 + i] = a[i][4];
        }
        g[6] = 0.0;
        g[7] = 0.0;
    } else {
        for (int i = 0; i < 4; i++) {
            double* r0 = a[2 * i];
            double* r1 = a[2 * i + 1];
            r0[0] = x[i]; r0[1] = y[i]; r0[2] = 1.0; r0[3] = 0.0; r0[4] = 0.0; r0[5] = 0.0;
            r0[6] = -u[i] * x[i]; r0[7] = -u[i] * y[i]; r0[8] = u[i];
            r1[0] = 0.0; r1[1] = 0.0; r1[2] = 0.0; r1[3] = x[i]; r1[4] = y[i]; r1[5] = 1.0;
            r1[6] = -v[i] * x[i]; r1[7] = -v[i] * y[i]; r1[8] = v[i];
        }
        if (!eliminate(a, 8, 1)) return 0;
        for (int i = 0; i < 8; i++) g[i] = a[i][8];
    }
    g[8] = 1.0;
    /* denormalise: M = G * Tl, then H = Tr^-1 * M */
    double mm[9], h[9];
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
    int ok = 1;
    for (int i = 0; i < 9; i++) {
        H[i] = (float)h[i];
        ok &= isfinite(H[i]) != 0;
    }
    return ok;
}

/* ---- 4. score */

static int inlier(const float* H, const float* p, float max_err, int variant)
{
    const float x = p[0], y = p[1], xr = p[2], yr = p[3];
    const float u = fmaf(H[0], x, fmaf(H[1], y, H[2]));
    const float v = fmaf(H[3], x, fmaf(H[4], y, H[5]));
    const float w = fmaf(H[6], x, fmaf(H[7], y, H[8]));
    const float dx = fmaf(-w, xr, u);
    const float dy = fmaf(-w, yr, v);
    const float e = fmaf(dx, dx, dy * dy);
    const float lim = (max_err * max_err) * (w * w);
    return ((variant & 2) || w > 0.0f) && e <= lim;
}

/*
 * The whole rule.  samples: T x 4, models: T x 9, counts: T (any may be null).  result: H[9] as floats, then
 * n_inliers, hypothesis, n_valid, 0 as int32 (the 52 bytes of popsift_hip_ransac_result).  mask: n bytes or null.
 */
void rr_ransac(const float* pts, int n, int model, int T, float max_err, uint32_t seed, int variant, int32_t* samples,
               float* models, int32_t* counts, void* result, uint8_t* mask)
{
    const int m = model == MODEL_AFFINE ? 3 : 4;
    float     bestH[9] = {0};
    int       best = -1, best_t = -1, n_valid = 0;
    Norm      L, R;
    if (n >= m) {
        L = normaliser(pts, n, 0);
        R = normaliser(pts, n, 2);
    }
    for (int t = 0; t < T; t++) {
        int32_t idx[4] = {-1, -1, -1, -1};
        float   H[9] = {0};
        int     cnt = -1;
        if (n >= m && sample(seed, t, n, m, idx)) {
            if (solve(pts, idx, model, &L, &R, H)) {
                cnt = 0;
                for (int i = 0; i < n; i++) cnt += inlier(H, pts + 4 * (size_t)i, max_err, variant);
            } else {
                memset(H, 0, sizeof H);
            }
        }
        if (samples) memcpy(samples + 4 * (size_t)t, idx, sizeof idx);
        if (models) memcpy(models + 9 * (size_t)t, H, sizeof H);
        if (counts) counts[t] = cnt;
        if (cnt >= 0) n_valid++;
        if (cnt > best || ((variant & 1) && cnt >= 0 && cnt == best)) {
            best = cnt;
            best_t = t;
            memcpy(bestH, H, sizeof H);
        }
    }
    if (best < m) {
        best_t = -1;
        best = 0;
        memset(bestH, 0, sizeof bestH);
    }
    if (mask)
        for (int i = 0; i < n; i++) mask[i] = best_t >= 0 ? (uint8_t)inlier(bestH, pts + 4 * (size_t)i, max_err, variant) : 0;
    if (result) {
        int32_t tail[4] = {best, best_t, n_valid, 0};
        memcpy(result, bestH, sizeof bestH);
        memcpy((char*)result + sizeof bestH, tail, sizeof tail);
    }
}

/* the sampler alone: T x 4 indices, valid[t] = 1 when the sample is complete */
void rr_samples(uint32_t seed, int n, int model, int T, int32_t* samples, int32_t* valid)
{
    const int m = model == MODEL_AFFINE ? 3 : 4;
    for (int t = 0; t < T; t++) valid[t] = sample(seed, t, n, m, samples + 4 * (size_t)t);
}
