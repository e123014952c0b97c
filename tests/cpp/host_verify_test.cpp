// popsift::Verifier and FeaturesDev::pairPoints through the C++ API.
//   host_verify_test scene.bin l.pgm r.pgm points.out
// scene.bin: int32 n, n x 4 floats (x, y, x', y'), n planted mask bytes (tests/ransac_rule.py, planted()): the homography
// verified with 1000 hypotheses at 0.5 px must return exactly the planted mask, twice, and a second verifier the same.
// The two images go through PopSift in MatchingMode; the points of their cross-checked pairs are written to points.out
// (the test compares them with the C ABI's) and verified with the affine model.
// Prints "host_verify ok: <pairs> <inliers> <H, nine numbers>".
#include <popsift/features.h>
#include <popsift/popsift.h>
#include <popsift/verify.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../popsift_amd/host/pgmread.h"

#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);        \
            return 1;                                                      \
        }                                                                  \
    } while (0)

typedef popsift::FeaturesDev Dev;

int main(int argc, char** argv)
{
    if (argc != 5) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    CHECK(f);
    int n = 0;
    CHECK(std::fread(&n, 4, 1, f) == 1 && n > 0);
    std::vector<float>         pts(4 * (size_t)n);
    std::vector<unsigned char> planted((size_t)n);
    CHECK(std::fread(pts.data(), 16, (size_t)n, f) == (size_t)n && std::fread(planted.data(), 1, (size_t)n, f) == (size_t)n);
    std::fclose(f);
    int n_planted = 0;
    for (unsigned char b : planted) n_planted += b;

    popsift::RansacOptions opts;
    opts.hypotheses = 1000;
    opts.maxErr = 0.5f;
    opts.seed = 5;
    popsift::Verifier           verifier, second;
    const popsift::RansacResult a = verifier.ransac(pts, opts);
    CHECK(a.hypothesis >= 0 && a.inliers == n_planted && a.valid > 900 && a.mask == planted);
    const popsift::RansacResult b = verifier.ransac(pts, opts), c = second.ransac(pts, opts);
    CHECK(b.mask == a.mask && std::memcmp(b.H, a.H, sizeof a.H) == 0 && b.hypothesis == a.hypothesis);
    CHECK(c.mask == a.mask && std::memcmp(c.H, a.H, sizeof a.H) == 0 && c.hypothesis == a.hypothesis);
    /* too few pairs: no winner */
    const popsift::RansacResult none = verifier.ransac(std::vector<float>(pts.begin(), pts.begin() + 12), opts);
    CHECK(none.hypothesis == -1 && none.inliers == 0 && none.mask.size() == 3 && none.H[8] == 0.0f);
    CHECK(verifier.ransac(std::vector<float>()).hypothesis == -1);

    int            w[2], h[2];
    unsigned char* img[2];
    for (int k = 0; k < 2; k++) {
        img[k] = readPGMfile(argv[2 + k], w[k], h[k]);
        if (!img[k]) return 3;
    }
    popsift::Config cfg;
    PopSift         sift(cfg, popsift::Config::MatchingMode);
    SiftJob*        jl = sift.enqueue(w[0], h[0], img[0]);
    SiftJob*        jr = sift.enqueue(w[1], h[1], img[1]);
    Dev*            l = jl->getDev();
    Dev*            r = jr->getDev();
    CHECK(l && r);
    Dev::MatchOptions cc;
    cc.crossCheck = true;
    const std::vector<Dev::Pair> pairs = l->matchPairs(r, cc);
    CHECK(pairs.size() >= 8);
    const std::vector<float> pp = l->pairPoints(r, pairs);
    CHECK(pp.size() == 4 * pairs.size());
    CHECK(l->pairPoints(r, std::vector<Dev::Pair>()).empty());
    f = std::fopen(argv[4], "wb");
    CHECK(f && std::fwrite(pp.data(), 4, pp.size(), f) == pp.size());
    std::fclose(f);
    popsift::RansacOptions aff;
    aff.model = popsift::RansacOptions::Affine;
    const popsift::RansacResult fit = verifier.ransac(pp, aff);
    CHECK(fit.hypothesis >= 0 && fit.mask.size() == pairs.size());
    std::printf("host_verify ok: %zu %d", pairs.size(), fit.inliers);
    for (int i = 0; i < 9; i++) std::printf(" %.9g", fit.H[i]);
    std::printf("\n");
    delete l;
    delete r;
    delete jl;
    delete jr;
    sift.uninit();
    delete[] img[0];
    delete[] img[1];
    return 0;
}
