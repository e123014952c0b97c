/* Stand-alone sanitizer pass over tests/guided_ref.c, the CPU reference of the guided matcher:
 *     gcc -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all guided_san_main.c -lm
 * Seeded scenes at the sizes where the loops end (0, 1, odd counts), both models, both directions and the pair rule;
 * NaN and infinite positions included.  Prints a checksum of the rows and the pairs, the same with and without the
 * sanitizers (tests/test_guided_rule.py compares them). */
#include <stdio.h>
#include <stdlib.h>

#include "../guided_ref.c"

static uint32_t state = 12345u;
static float    rnd(void)
{
    state = state * 1664525u + 1013904223u;
    return (float)(state >> 8) / 16777216.0f;
}

int main(void)
{
    const int    sizes[][2] = {{0, 0}, {0, 5}, {5, 0}, {1, 1}, {7, 33}, {65, 129}};
    const float  H[9] = {1.0f, 0.01f, 4.0f, -0.02f, 1.0f, -3.0f, 1e-5f, 0.0f, 1.0f};
    const float  F[9] = {0.0f, 0.0f, 5.0f, 0.0f, 0.0f, -10.0f, -5.0f, 10.0f, 0.0f};
    unsigned long sum = 0;
    for (unsigned s = 0; s < sizeof sizes / sizeof sizes[0]; s++) {
        const int nl = sizes[s][0], nr = sizes[s][1];
        /* exact sizes, so that one element past an end is outside its allocation */
        float*    l = malloc(sizeof(float) * 128 * (size_t)nl + 1);
        float*    r = malloc(sizeof(float) * 128 * (size_t)nr + 1);
        float*    lxy = malloc(sizeof(float) * 2 * (size_t)nl + 1);
        float*    rxy = malloc(sizeof(float) * 2 * (size_t)nr + 1);
        gr_match* fwd = malloc(sizeof(gr_match) * (size_t)nl + 1);
        gr_match* back = malloc(sizeof(gr_match) * (size_t)nr + 1);
        gr_pair*  pairs = malloc(sizeof(gr_pair) * (size_t)nl + 1);
        int32_t*  ncand = malloc(sizeof(int32_t) * (size_t)nl + 1);
        for (int i = 0; i < 128 * nl; i++) l[i] = rnd();
        for (int i = 0; i < 128 * nr; i++) r[i] = rnd();
        for (int i = 0; i < 2 * nl; i++) lxy[i] = 40.0f * rnd();
        for (int i = 0; i < 2 * nr; i++) rxy[i] = 40.0f * rnd();
        if (nl > 3) lxy[2] = NAN, lxy[5] = INFINITY;
        if (nr > 3) rxy[3] = NAN, rxy[4] = -INFINITY;
        for (int model = 0; model < 2; model++) {
            const float* M = model ? F : H;
            gr_rows(model, M, 6.0f, l, lxy, nl, r, rxy, nr, 0, fwd, ncand);
            gr_rows(model, M, 6.0f, l, lxy, nl, r, rxy, nr, 1, back, NULL);
            for (int cross = 0; cross < 2; cross++) {
                const int n = gr_pairs(fwd, nl, cross ? back : NULL, cross ? 0.0f : 0.8f, INFINITY, pairs);
                sum = sum * 31 + (unsigned long)n;
                for (int k = 0; k < n; k++) sum = sum * 31 + (unsigned long)(pairs[k].l * 1000 + pairs[k].r);
            }
            for (int i = 0; i < nl; i++) sum = sum * 31 + (unsigned long)(fwd[i].best + 2) + (unsigned long)ncand[i];
            for (int j = 0; j < nr; j++) sum = sum * 31 + (unsigned long)(back[j].best + 2);
        }
        free(l), free(r), free(lxy), free(rxy), free(fwd), free(back), free(pairs), free(ncand);
    }
    printf("guided_san ok: %lu\n", sum);
    return 0;
}
