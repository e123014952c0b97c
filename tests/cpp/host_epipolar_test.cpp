// popsift::Verifier::epipolar through the C++ API.
//   host_epipolar_test scene.bin result.out
// scene.bin: int32 n, n x 4 floats (x, y, x', y'), n planted mask bytes (tests/epipolar_rule.py, two_view()).  The scene is
// verified with 1500 hypotheses at 0.5 px, seed 0: the planted mask must come back, twice, the second time after a
// homography call on the same verifier, and from a second verifier.  result.out receives H (nine floats), inliers,
// hypothesis, valid (three int32) and the mask: the test compares them with the C call's bytes.
// Prints "host_epipolar ok: <inliers> <hypothesis>".
#include <popsift/verify.h>

#include <cstdio>
#include <cstring>
#include <vector>

#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);        \
            return 1;                                                      \
        }                                                                  \
    } while (0)

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
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

    popsift::EpipolarOptions opts;
    CHECK(opts.hypotheses == 2048 && opts.maxErr == 2.0f && opts.seed == 0);
    opts.hypotheses = 1500;
    opts.maxErr = 0.5f;
    popsift::Verifier           verifier, second;
    const popsift::RansacResult a = verifier.epipolar(pts, opts);
    CHECK(a.hypothesis >= 0 && a.inliers == n_planted && a.valid > 1400 && a.mask == planted);
    popsift::RansacOptions hom;
    hom.hypotheses = 100;
    const popsift::RansacResult h = verifier.ransac(pts, hom);
    CHECK(h.mask.size() == (size_t)n);
    const popsift::RansacResult b = verifier.epipolar(pts, opts), c = second.epipolar(pts, opts);
    CHECK(b.mask == a.mask && std::memcmp(b.H, a.H, sizeof a.H) == 0 && b.hypothesis == a.hypothesis && b.inliers == a.inliers);
    CHECK(c.mask == a.mask && std::memcmp(c.H, a.H, sizeof a.H) == 0 && c.hypothesis == a.hypothesis && c.valid == a.valid);
    /* too few pairs: no winner */
    const popsift::RansacResult none = verifier.epipolar(std::vector<float>(pts.begin(), pts.begin() + 28), opts);
    CHECK(none.hypothesis == -1 && none.inliers == 0 && none.mask.size() == 7 && none.H[8] == 0.0f);
    CHECK(verifier.epipolar(std::vector<float>()).hypothesis == -1);

    f = std::fopen(argv[2], "wb");
    const int tail[3] = {a.inliers, a.hypothesis, a.valid};
    CHECK(f && std::fwrite(a.H, 4, 9, f) == 9 && std::fwrite(tail, 4, 3, f) == 3 &&
          std::fwrite(a.mask.data(), 1, a.mask.size(), f) == a.mask.size());
    std::fclose(f);
    std::printf("host_epipolar ok: %d %d\n", a.inliers, a.hypothesis);
    return 0;
}
