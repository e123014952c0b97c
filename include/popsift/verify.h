/*
 * popsift/verify.h -- extension: geometric verification of correspondences on the GPU (popsift_hip_ransac,
 * include/popsift_hip.h, which states the rule).  No counterpart in the reference, whose matching demo stops at the
 * descriptor pairs.
 *
 *     std::vector<FeaturesDev::Pair> pairs = l->matchPairs(r, opts);
 *     popsift::Verifier              verifier;
 *     popsift::RansacResult          fit = verifier.ransac(l->pairPoints(r, pairs), popsift::RansacOptions());
 */
#pragma once

#include <vector>

struct popsift_hip_verifier;

namespace popsift {

struct RansacOptions {
    enum Model { Homography = 0, Affine = 1 }; /* 4 / 3 pairs per sample */
    Model    model = Homography;
    int      hypotheses = 2048; /* 1 .. 65536 */
    float    maxErr = 2.0f;     /* inlier: transfer error in the right image <= maxErr pixels */
    unsigned seed = 0;
};

struct RansacResult {
    float                      H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; /* row major, right ~ H * left; zeros without a winner */
    int                        inliers = 0;
    int                        hypothesis = -1; /* index of the winning hypothesis, -1: none */
    int                        valid = 0;       /* hypotheses that produced a model */
    std::vector<unsigned char> mask;            /* one byte per pair: 1 = inlier of H */
};

/* A stream and grow-only scratch on one GPU; one call at a time.  The result is a function of (points, options) alone. */
class Verifier {
    popsift_hip_verifier* _v;

    Verifier(const Verifier&);
    Verifier& operator=(const Verifier&);

public:
    explicit Verifier(int device = 0);
    ~Verifier();

    /* pts: (x, y, x', y') per pair, as FeaturesDev::pairPoints returns them */
    RansacResult ransac(const std::vector<float>& pts, const RansacOptions& opts);
    RansacResult ransac(const std::vector<float>& pts) { return ransac(pts, RansacOptions()); }
};

}  // namespace popsift
