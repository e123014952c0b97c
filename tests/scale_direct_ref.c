/*
 * scale_direct_ref.c -- CPU restatement of the Gaussian pyramid in both scaling modes, the yardstick of
 * tests/test_scale_direct.py and tests/test_gpu_scale_direct.py.
 *
 * ScaleDefault (scale_direct = 0): octave 0's level 0 is the input image, upscaled bilinearly (CUDA linear-filter
 * fetch: clamp addressing, 1.8 fixed-point weights) and blurred with inc[0]; level 0 of octave o >= 1 is every second
 * pixel of level L-3 of octave o-1; level l >= 1 is level l-1 blurred with the incremental taps inc[l].
 * ScaleDirect (scale_direct = 1): level 0 of EVERY octave o is the input image sampled at octave o's own size
 * ((x + shift_o) / w_o), blurred horizontally with dd[o] (outermost tap first, centre last, x 255) and vertically with
 * inc[0]; shift_o is octave 0's upscale shift for o = 0 and 0.5 otherwise.  Levels l >= 1 as in the default mode.
 *
 * Horizontal pass from a plane: centre tap first, then (left + right) * g[k] from the outermost tap in; vertical pass:
 * outermost tap first, upper then lower sample, centre last; clamp addressing.  Compile with -ffp-contract=off: an FMA
 * happens exactly where fmaf() is written.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define GA 32         /* taps per table row */
#define MAX_OCT 20    /* rows of the dd table */

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static int imin(int a, int b) { return a < b ? a : b; }

/* half-filter width incl. the centre: VLFeat rule (ceil(4 sigma) + 1), or the OpenCV rule (gauss_mode 3) */
static int span_of(int gauss_mode, float sigma)
{
    if (gauss_mode == 3) {
        int s = (int)roundf(2.0f * 4.0f * sigma + 1.0f) | 1;
        return imin((s >> 1) + 1, GA - 1);
    }
    return imin((int)(ceilf(4.0f * sigma) + 1.0f), GA - 1);
}

/* normalised half filters: f[0] = 1, f[x] = exp(-x^2 / 2 sigma^2), divided by their double sum */
static void filters(int n, const float* sigma, int gauss_mode, float* f, int* span)
{
    for (int l = 0; l < n; l++) {
        const float sig = sigma[l];
        const int   spn = span_of(gauss_mode, sig);
        float*      row = f + l * GA;
        double      sum = 1.0;
        span[l] = spn;
        row[0] = 1.0f;
        for (int x = 1; x < spn; x++) {
            row[x] = (float)exp(-0.5 * pow((double)x / sig, 2.0));
            sum += 2.0f * row[x];
        }
        for (int x = 0; x < spn; x++) row[x] = (float)(row[x] / sum);
        for (int x = spn; x < GA; x++) row[x] = 0.0f;
    }
}

/* The incremental table (inc, L = levels + 3 rows) and the dd table (MAX_OCT rows); returns L. */
int sdr_tables(float sigma0, int levels, int assume_initial_blur, float initial_blur, float upscale_factor, int gauss_mode,
               float* inc_f, int* inc_span, float* inc_sigma, float* dd_f, int* dd_span, float* dd_sigma)
{
    const int   L = levels + 3;
    const float ib = assume_initial_blur ? initial_blur * powf(2.0f, upscale_factor) : 0.0f;
    inc_sigma[0] = assume_initial_blur ? sqrtf(fabsf(sigma0 * sigma0 - ib * ib)) : sigma0;
    for (int l = 1; l < L; l++) {
        const float sp = sigma0 * powf(2.0f, (float)(l - 1) / (float)levels);
        const float ss = sigma0 * powf(2.0f, (float)l / (float)levels);
        inc_sigma[l] = sqrtf(ss * ss - sp * sp);
    }
    /* sigma0 * 2^o less the assumed input blur, in octave-o pixels */
    for (int o = 0; o < MAX_OCT; o++) {
        const float s = ldexpf(sigma0, o);
        dd_sigma[o] = ldexpf(sqrtf(fabsf(s * s - ib * ib)), -o);
    }
    filters(L, inc_sigma, gauss_mode, inc_f, inc_span);
    filters(MAX_OCT, dd_sigma, gauss_mode, dd_f, dd_span);
    return L;
}

typedef struct {
    const uint8_t* u8;
    const float*   f32;
    int            w, h, pitch;
} image;

static float texel(const image* im, int x, int y)
{
    x = clampi(x, 0, im->w - 1);
    y = clampi(y, 0, im->h - 1);
    if (im->u8) return (float)im->u8[(size_t)y * im->pitch + x] / 255.0f;
    return im->f32[(size_t)y * im->pitch + x];
}

/* normalised coordinate r on an axis of n texels: first texel and its 1.8 fixed-point weight */
static void sample_at(float r, int n, int* i0, float* wt)
{
    const float p = r * (float)n - 0.5f;
    const float fl = floorf(p);
    *i0 = (int)fl;
    *wt = floorf((p - fl) * 256.0f + 0.5f) * (1.0f / 256.0f);
}

/* input image sampled at dw x dh -> horizontal blur (taps g, span) -> tmp */
static void h_from_input(const image* im, float shift, const float* g, int span, float* tmp, int dw, int dh)
{
    float* u = (float*)malloc(sizeof(float) * (size_t)(dw + 2 * span));
    for (int y = 0; y < dh; y++) {
        int   iy;
        float b;
        sample_at(((float)y + shift) / (float)dh, im->h, &iy, &b);
        for (int x = -span; x < dw + span; x++) {
            int   ix;
            float a;
            sample_at(((float)x + shift) / (float)dw, im->w, &ix, &a);
            const float top = (1.0f - a) * texel(im, ix, iy) + a * texel(im, ix + 1, iy);
            const float bot = (1.0f - a) * texel(im, ix, iy + 1) + a * texel(im, ix + 1, iy + 1);
            u[x + span] = (1.0f - b) * top + b * bot;
        }
        for (int x = 0; x < dw; x++) {
            float acc = 0.0f;
            for (int k = span - 1; k > 0; k--) acc = fmaf(u[x - k + span] + u[x + k + span], g[k], acc);
            acc = fmaf(u[x + span], g[0], acc);
            tmp[(size_t)y * dw + x] = acc * 255.0f;
        }
    }
    free(u);
}

/* plane -> horizontal blur, centre tap first, clamp addressing */
static void h_from_plane(const float* src, const float* g, int span, float* tmp, int w, int h)
{
    for (int y = 0; y < h; y++) {
        const float* row = src + (size_t)y * w;
        for (int x = 0; x < w; x++) {
            float acc = row[x] * g[0];
            for (int k = span - 1; k > 0; k--) acc = fmaf(row[clampi(x - k, 0, w - 1)] + row[clampi(x + k, 0, w - 1)], g[k], acc);
            tmp[(size_t)y * w + x] = acc;
        }
    }
}

/* vertical blur: outermost tap first, upper then lower sample, centre last, clamp addressing */
static void v_pass(const float* tmp, const float* g, int span, float* dst, int w, int h)
{
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            float acc = 0.0f;
            for (int k = span - 1; k > 0; k--) {
                acc = fmaf(tmp[(size_t)clampi(y - k, 0, h - 1) * w + x], g[k], acc);
                acc = fmaf(tmp[(size_t)clampi(y + k, 0, h - 1) * w + x], g[k], acc);
            }
            dst[(size_t)y * w + x] = fmaf(tmp[(size_t)y * w + x], g[0], acc);
        }
}

/*
 * The Gaussian planes of n_oct octaves of sizes ow[o] x oh[o] (the library's plan), written contiguously to out:
 * octave o, level l at out + sum_{p < o} L * ow[p] * oh[p] + l * ow[o] * oh[o].  One of u8 / f32 is the input.
 * shift: octave 0's upscale sample offset (0.5 * 2^upscale_factor in PopSift / VLFeat sift mode, 0.5 in OpenCV mode).
 * Returns 0, or -1 when out of memory.
 */
int sdr_pyramid(const uint8_t* u8, const float* f32, int w, int h, int pitch, float shift, int L, const float* inc_f,
                const int* inc_span, const float* dd_f, const int* dd_span, int scale_direct, int n_oct, const int* ow,
                const int* oh, float* out)
{
    const image im = {u8, f32, w, h, pitch};
    float*      tmp = (float*)malloc(sizeof(float) * (size_t)ow[0] * oh[0]);
    if (!tmp) return -1;
    float* prev = NULL; /* the octave before */
    for (int o = 0; o < n_oct; o++) {
        const int    W = ow[o], H = oh[o];
        const size_t n = (size_t)W * H;
        float*       pl = out;
        for (int l = 0; l < L; l++) {
            float* dst = pl + l * n;
            if (l == 0 && (o == 0 || scale_direct)) {
                const float* g = scale_direct ? dd_f + o * GA : inc_f;
                const int    s = scale_direct ? dd_span[o] : inc_span[0];
                h_from_input(&im, o == 0 ? shift : 0.5f, g, s, tmp, W, H);
                v_pass(tmp, inc_f, inc_span[0], dst, W, H);
            } else if (l == 0) {
                const int    pw = ow[o - 1], ph = oh[o - 1];
                const float* src = prev + (size_t)(L - 3) * pw * ph;
                for (int y = 0; y < H; y++)
                    for (int x = 0; x < W; x++) dst[(size_t)y * W + x] = src[(size_t)imin(2 * y, ph - 1) * pw + imin(2 * x, pw - 1)];
            } else {
                h_from_plane(dst - n, inc_f + l * GA, inc_span[l], tmp, W, H);
                v_pass(tmp, inc_f + l * GA, inc_span[l], dst, W, H);
            }
        }
        prev = pl;
        out += (size_t)L * n;
    }
    free(tmp);
    return 0;
}
