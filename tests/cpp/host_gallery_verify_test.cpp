// A gallery verified through the C++ API: Gallery::add(FeaturesDev*), Gallery::pairPoints and Verifier::ransacMany.
//   host_gallery_verify_test q.pgm a.pgm b.pgm   three images through PopSift in MatchingMode with norm_multi = 9.  The
//                                                gallery holds a and b as float sets.  Its pair lists must equal those of a
//                                                gallery of their byte sets, its points FeaturesDev::pairPoints(q, member)
//                                                per member, and for a homography and a fundamental matrix every record and
//                                                mask of Verifier::ransacMany those of Verifier::ransac / Verifier::epipolar
//                                                on the member's points, bit for bit.
// Prints "host_gallery_verify ok: <inliers of a> <inliers of b>" of the homography (512 hypotheses, max_err 2, seed 3).
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

typedef popsift::FeaturesDev Set;

static bool same(const popsift::RansacResult& a, const popsift::RansacResult& b)
{
    return memcmp(a.H, b.H, sizeof a.H) == 0 && a.inliers == b.inliers && a.hypothesis == b.hypothesis && a.valid == b.valid &&
           a.mask == b.mask;
}

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    popsift::Config cfg;
    cfg.setNormalizationMultiplier(9);
    PopSift sift(cfg, popsift::Config::MatchingMode);
    Set*    sets[3];
    for (int k = 0; k < 3; k++) {
        int            w, h;
        unsigned char* img = readPGMfile(argv[1 + k], w, h);
        if (!img) return 3;
        SiftJob* job = sift.enqueue(w, h, img);
        sets[k] = job->getDev();
        CHECK(sets[k] && sets[k]->getDescriptorCount() > 100);
        delete job;
        delete[] img;
    }
    Set*                       q = sets[0];
    popsift::FeaturesDevBytes* qb = q->toBytes();
    popsift::Gallery           gallery(q->getDevice()), bytes(q->getDevice());
    for (int m = 0; m < 2; m++) {
        popsift::FeaturesDevBytes* b = sets[1 + m]->toBytes();
        CHECK(gallery.add(sets[1 + m]) == m && bytes.add(b) == m);
        delete b;
    }
    Set::MatchOptions mo;
    mo.crossCheck = true;
    const std::vector<std::vector<Set::Pair>> pairs = gallery.matchPairs(qb, mo), want = bytes.matchPairs(qb, mo);
    CHECK(pairs.size() == 2 && want.size() == 2);
    for (size_t m = 0; m < 2; m++) {
        CHECK(pairs[m].size() == want[m].size() && pairs[m].size() > 10);
        CHECK(memcmp(pairs[m].data(), want[m].data(), sizeof(Set::Pair) * pairs[m].size()) == 0);
    }
    std::vector<int>         offsets;
    const std::vector<float> pts = gallery.pairPoints(q, pairs, offsets);
    CHECK(offsets.size() == 3 && offsets[0] == 0 && offsets[1] == (int)pairs[0].size() &&
          offsets[2] == (int)(pairs[0].size() + pairs[1].size()) && pts.size() == 4 * (size_t)offsets[2]);
    std::vector<float> each[2];
    for (size_t m = 0; m < 2; m++) {
        each[m] = q->pairPoints(sets[1 + m], pairs[m]);
        CHECK(each[m].size() == 4 * pairs[m].size());
        CHECK(memcmp(each[m].data(), pts.data() + 4 * (size_t)offsets[m], sizeof(float) * each[m].size()) == 0);
    }
    /* a gallery of byte sets matches alike, and has no points for a pair */
    std::vector<std::vector<Set::Pair>> nothing(2);
    CHECK(bytes.pairPoints(q, nothing, offsets).empty() && offsets.size() == 3 && offsets[2] == 0);
    gallery.pairPoints(q, pairs, offsets);

    popsift::Verifier    verifier(q->getDevice());
    popsift::ManyOptions many;
    many.hypotheses = 512;
    many.seed = 3;
    std::vector<popsift::RansacResult> fits = verifier.ransacMany(pts, offsets, many);
    CHECK(fits.size() == 2);
    popsift::RansacOptions ro;
    ro.hypotheses = 512;
    ro.seed = 3;
    for (size_t m = 0; m < 2; m++) CHECK(same(fits[m], verifier.ransac(each[m], ro)) && fits[m].mask.size() == pairs[m].size());
    CHECK(fits[0].hypothesis >= 0 && fits[0].inliers > fits[1].inliers);
    const int inliers[2] = {fits[0].inliers, fits[1].inliers};

    many.kind = popsift::ManyOptions::Epipolar;
    popsift::EpipolarOptions eo;
    eo.hypotheses = 512;
    eo.seed = 3;
    fits = verifier.ransacMany(pts, offsets, many);
    for (size_t m = 0; m < 2; m++) CHECK(same(fits[m], verifier.epipolar(each[m], eo)));
    CHECK(verifier.ransacMany(std::vector<float>(), std::vector<int>(), many).empty());

    std::printf("host_gallery_verify ok: %d %d\n", inliers[0], inliers[1]);
    delete qb;
    for (int k = 0; k < 3; k++) delete sets[k];
    sift.uninit();
    return 0;
}
