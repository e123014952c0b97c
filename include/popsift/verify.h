/*
 * popsift/verify.h -- extension: geometric verification of correspondences on the GPU (popsift_hip_ransac,
 * popsift_hip_epipolar and popsift_hip_refit, include/popsift_hip.h, which states the rules).  No counterpart in the reference, whose matching demo stops at the
 * descriptor pairs.
 *
 *     std::vector<FeaturesDev::Pair> pairs = l->matchPairs(r, opts);
 *     popsift::Verifier              verifier;
 *     popsift::RansacResult          fit = verifier.ransac(l->pairPoints(r, pairs), popsift::RansacOptions());
 *     popsift::RansacResult          two = verifier.epipolar(l->pairPoints(r, pairs), popsift::EpipolarOptions());
 *     popsift::RefitResult           best = verifier.refit(l->pairPoints(r, pairs),
 *                                                          popsift::RefitOptions(fit, popsift::RefitOptions::Homography, 2.0f));
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

/* Many pair lists in one call (popsift_hip_ransac_many): the lists of a gallery, each verified as ransac() / epipolar()
 * verifies it alone, with the same hypotheses, maxErr and seed for every list. */
struct ManyOptions {
    enum Kind { Homography = 0, Affine = 1, Epipolar = 2 };
    Kind     kind = Homography;
    int      hypotheses = 2048; /* 1 .. 65536 */
    float    maxErr = 2.0f;     /* the kind's inlier limit in pixels */
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

/* Least squares on the inliers: the model of a minimal sample carries that sample's noise; the refit fits the kind's model
 * to all inliers of the current model and repeats on the new model's inliers while their number does not drop. */
struct RefitOptions {
    enum Kind { Homography = 0, Affine = 1, Epipolar = 2 };
    Kind  kind = Homography;
    int   rounds = 4;     /* 1 .. 16 */
    float maxErr = 2.0f;  /* the kind's inlier limit, as in the call the model came from */
    float M[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}; /* the start model, row major */

    RefitOptions() {}
    /* start from the winner of Verifier::ransac / Verifier::epipolar */
    RefitOptions(const RansacResult& start, Kind k, float max_err) : kind(k), maxErr(max_err)
    {
        for (int i = 0; i < 9; i++) M[i] = start.H[i];
    }
};

struct RefitResult {
    enum Stop { Rounds = 0, Converged = 1, NotBetter = 2, NoFit = 3, NoSupport = 4 };
    float                      M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; /* the refitted model, row major */
    int                        inliers = 0;                        /* >= start */
    int                        start = 0;                          /* inliers of the start model */
    int                        rounds = 0;                         /* accepted rounds */
    Stop                       stop = NoSupport;
    std::vector<unsigned char> mask;                               /* one byte per pair: 1 = inlier of M */
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
    /* the same points and the model to start from */
    RefitResult refit(const std::vector<float>& pts, const RefitOptions& opts);
    /* list m is the pairs offsets[m] .. offsets[m + 1] of pts, as Gallery::pairPoints returns both; result m is what
     * ransac() / epipolar() returns for list m alone, from one upload, one download and a number of launches that does
     * not depend on the number of lists */
    std::vector<RansacResult> ransacMany(const std::vector<float>& pts, const std::vector<int>& offsets, const ManyOptions& opts);
};

}  // namespace popsift
