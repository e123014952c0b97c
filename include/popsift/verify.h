/*
 * popsift/verify.h -- extension: geometric verification of correspondences on the GPU (popsift_hip_ransac and
 * popsift_hip_epipolar, include/popsift_hip.h, which states the rules).  No counterpart in the reference, whose matching demo stops at the
 * descriptor pairs.
 *
 *     std::vector<FeaturesDev::Pair> pairs = l->matchPairs(r, opts);
 *     popsift::Verifier              verifier;
 *     popsift::RansacResult          fit = verifier.ransac(l->pairPoints(r, pairs), popsift::RansacOptions());
 *     popsift::RansacResult          two = verifier.epipolar(l->pairPoints(r, pairs), popsift::EpipolarOptions());
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

/* Two views of a 3-D scene: the fundamental matrix by the 8-point algorithm, 8 pairs per sample.  A clean sample has
 * probability w^8 for an inlier share w, so this takes more hypotheses than a homography at the same share. */
struct EpipolarOptions {
    int      hypotheses = 2048; /* 1 .. 65536 */
    float    maxErr = 2.0f;     /* inlier: Sampson distance <= maxErr pixels */
    unsigned seed = 0;
};

struct RansacResult {
    /* row major, right ~ H * left; from Verifier::epipolar the fundamental matrix F, [x' y' 1] F [x y 1]^T = 0; zeros
     * without a winner */
    float                      H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
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
    /* the same points; the result's H holds F and its mask the pairs within maxErr of their epipolar lines */
    RansacResult epipolar(const std::vector<float>& pts, const EpipolarOptions& opts);
    RansacResult epipolar(const std::vector<float>& pts) { return epipolar(pts, EpipolarOptions()); }
};

}  // namespace popsift
