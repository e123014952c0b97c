// popsift::Verifier::refit through the C++ API.
//   host_refit_test l.pgm r.pgm result.out
// The two images go through PopSift in MatchingMode; the points of their cross-checked pairs (FeaturesDev::pairPoints) are
// verified with each kind of model and the winner is refitted with RefitOptions(winner, kind, 2 px).  result.out: int32 n,
// the n x 4 points, then per kind (homography, affine, epipolar) the start model (9 floats) and the refit's M (9 floats),
// inliers, start, rounds, stop (int32) and mask (n bytes): the test repeats the calls through the C ABI on the same points.
// Prints "host_refit ok: <pairs>".
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
    if (argc != 4) return 2;
    int            w[2], h[2];
    unsigned char* img[2];
    for (int k = 0; k < 2; k++) {
        img[k] = readPGMfile(argv[1 + k], w[k], h[k]);
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
    const int                n = (int)pairs.size();
    std::FILE*               f = std::fopen(argv[3], "wb");
    CHECK(f && std::fwrite(&n, 4, 1, f) == 1 && std::fwrite(pp.data(), 4, pp.size(), f) == pp.size());

    popsift::Verifier verifier;
    /* the defaults: the identity, 4 rounds, 2 px */
    const popsift::RefitOptions plain;
    CHECK(plain.kind == popsift::RefitOptions::Homography && plain.rounds == 4 && plain.maxErr == 2.0f && plain.M[0] == 1.0f &&
          plain.M[1] == 0.0f && plain.M[4] == 1.0f && plain.M[8] == 1.0f);
    /* too few pairs: the start model comes back */
    const popsift::RefitResult none = verifier.refit(std::vector<float>(pp.begin(), pp.begin() + 8), plain);
    CHECK(none.stop == popsift::RefitResult::NoSupport && none.inliers == 0 && none.mask.size() == 2 && none.M[0] == 1.0f);
    for (int kind = 0; kind < 3; kind++) {
        popsift::RansacResult fit;
        if (kind == 2) {
            fit = verifier.epipolar(pp);
        } else {
            popsift::RansacOptions o;
            o.model = kind == 1 ? popsift::RansacOptions::Affine : popsift::RansacOptions::Homography;
            fit = verifier.ransac(pp, o);
        }
        CHECK(fit.hypothesis >= 0);
        const popsift::RefitOptions ro(fit, (popsift::RefitOptions::Kind)kind, 2.0f);
        CHECK(ro.rounds == 4 && std::memcmp(ro.M, fit.H, sizeof fit.H) == 0);
        const popsift::RefitResult again = verifier.refit(pp, ro);
        CHECK(again.start == fit.inliers && again.inliers >= again.start && again.mask.size() == pairs.size());
        const int tail[4] = {again.inliers, again.start, again.rounds, (int)again.stop};
        CHECK(std::fwrite(fit.H, 4, 9, f) == 9 && std::fwrite(again.M, 4, 9, f) == 9 && std::fwrite(tail, 4, 4, f) == 4 &&
              std::fwrite(again.mask.data(), 1, again.mask.size(), f) == again.mask.size());
    }
    std::fclose(f);
    std::printf("host_refit ok: %zu\n", pairs.size());
    delete l;
    delete r;
    delete jl;
    delete jr;
    sift.uninit();
    delete[] img[0];
    delete[] img[1];
    return 0;
}
