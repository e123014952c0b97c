/* CPU restatement of the guided matcher's rule (include/popsift_hip.h, popsift_hip_match_guided): the candidate test for
 * both models, the distance, the rows, the rows of the search the other way round and the pairs.  Serial loops in the
 * header's own words; build with -ffp-contract=off so that every FMA is one written here. */
#include <math.h>
#include <stdint.h>

typedef struct {
    int32_t best, second, accept;
    float   dist_best, dist_second;
} gr_match;

typedef struct {
    int32_t l, r;
    float   dist_best, dist_second;
} gr_pair;

/* model 0: step 4 of popsift_hip_ransac with H = M; model 1: step 6 of popsift_hip_epipolar with F = M */
int gr_ok(int model, const float* M, float max_err, float x, float y, float xr, float yr)
{
    if (model == 0) {
        const float u = fmaf(M[0], x, fmaf(M[1], y, M[2]));
        const float v = fmaf(M[3], x, fmaf(M[4], y, M[5]));
        const float w = fmaf(M[6], x, fmaf(M[7], y, M[8]));
        const float dx = fmaf(-w, xr, u);
        const float dy = fmaf(-w, yr, v);
        const float e = fmaf(dx, dx, dy * dy);
        const float lim = (max_err * max_err) * (w * w);
        return w > 0.0f && e <= lim;
    }
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

/* ok(k, k) of n pairs (x, y, x', y'): the verifiers' inlier mask under the same model and max_err */
void gr_ok_pairs(int model, const float* M, float max_err, const float* pts, int n, uint8_t* mask)
{
    for (int k = 0; k < n; k++) mask[k] = (uint8_t)gr_ok(model, M, max_err, pts[4 * k], pts[4 * k + 1], pts[4 * k + 2], pts[4 * k + 3]);
}

float gr_dist(const float* l, const float* r)
{
    float p[32];
    for (int c = 0; c < 32; c++) {
        const float x = l[4 * c] - r[4 * c], y = l[4 * c + 1] - r[4 * c + 1], z = l[4 * c + 2] - r[4 * c + 2],
                    w = l[4 * c + 3] - r[4 * c + 3];
        p[c] = fmaf(w, w, fmaf(z, z, fmaf(y, y, x * x)));
    }
    for (int s = 16; s >= 1; s >>= 1)
        for (int i = 0; i < s; i++) p[i] = p[i] + p[i + s];
    return p[0];
}

static int lex_less(float d, int i, float e, int j) { return d < e || (d == e && i < j); }

static void insert(gr_match* m, float d, int j)
{
    if (m->best < 0 || lex_less(d, j, m->dist_best, m->best)) {
        m->second = m->best;
        m->dist_second = m->dist_best;
        m->best = j;
        m->dist_best = d;
    } else if (m->second < 0 || lex_less(d, j, m->dist_second, m->second)) {
        m->second = j;
        m->dist_second = d;
    }
}

/* back = 0: a row per left descriptor i over { j : ok(i, j) }, under (d, j); ncand[i] = its candidates (before the
 * distance's own condition).  back = 1: a row per right descriptor j over { i : ok(i, j) }, under (d, i). */
void gr_rows(int model, const float* M, float max_err, const float* ldesc, const float* lxy, int nl, const float* rdesc,
             const float* rxy, int nr, int back, gr_match* out, int32_t* ncand)
{
    const int n_rows = back ? nr : nl, n_cols = back ? nl : nr;
    for (int a = 0; a < n_rows; a++) {
        gr_match m = {-1, -1, 0, INFINITY, INFINITY};
        int      n = 0;
        for (int b = 0; b < n_cols; b++) {
            const int i = back ? b : a, j = back ? a : b;
            if (!gr_ok(model, M, max_err, lxy[2 * i], lxy[2 * i + 1], rxy[2 * j], rxy[2 * j + 1])) continue;
            n++;
            const float d = gr_dist(ldesc + 128 * (long)i, rdesc + 128 * (long)j);
            if (d < INFINITY) insert(&m, d, b);
        }
        m.accept = m.dist_best / m.dist_second < 0.8f;
        out[a] = m;
        if (ncand) ncand[a] = n;
    }
}

/* the rule of popsift_hip_match_pairs on the rows F (and B, or null without the cross-check); returns the count */
int gr_pairs(const gr_match* F, int nl, const gr_match* B, float ratio, float max_dist2, gr_pair* out)
{
    int n = 0;
    for (int i = 0; i < nl; i++) {
        const gr_match m = F[i];
        if (m.best < 0) continue;
        if (!(ratio == 0.0f || m.dist_best / m.dist_second < ratio)) continue;
        if (!(m.dist_best <= max_dist2)) continue;
        if (B && B[m.best].best != i) continue;
        out[n].l = i;
        out[n].r = m.best;
        out[n].dist_best = m.dist_best;
        out[n].dist_second = m.dist_second;
        n++;
    }
    return n;
}
