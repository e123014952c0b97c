// popsift::Gallery through the C++ API.
//   host_gallery_test q.pgm a.pgm b.pgm    three images through PopSift in MatchingMode with norm_multi = 9; the sets go to
//                                          bytes on the GPU.  The gallery holds a, an empty set and b.  For several option
//                                          sets Gallery::matchPairs(q) must equal FeaturesDevBytes::matchPairs(q, member),
//                                          field by field and member by member, and counts() the lists' lengths; the members
//                                          are deleted before the gallery is matched.
// Prints "host_gallery ok: <pairs of a> <pairs of the empty set> <pairs of b>" with the default ratio and the cross-check.
#include <popsift/features.h>
#include <popsift/popsift.h>

#include <popsift_hip.h>

#include <cstdio>
#include <vector>

#include "../../popsift_amd/host/pgmread.h"

#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);        \
            return 1;                                                      \
        }                                                                  \
    } while (0)

typedef popsift::FeaturesDevBytes Bytes;

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    popsift::Config cfg;
    cfg.setNormalizationMultiplier(9);
    PopSift sift(cfg, popsift::Config::MatchingMode);
    Bytes*  sets[3];
    for (int k = 0; k < 3; k++) {
        int            w, h;
        unsigned char* img = readPGMfile(argv[1 + k], w, h);
        if (!img) return 3;
        SiftJob*              job = sift.enqueue(w, h, img);
        popsift::FeaturesDev* f = job->getDev();
        CHECK(f && f->getDescriptorCount() > 100);
        sets[k] = f->toBytes();
        CHECK(sets[k] && sets[k]->getDescriptorCount() == f->getDescriptorCount());
        delete f;
        delete job;
        delete[] img;
    }
    Bytes* q = sets[0];
    Bytes  none((const unsigned char*)0, 0, q->getDevice());
    Bytes* members[3] = {sets[1], &none, sets[2]};

    Bytes::MatchOptions opts[4];
    opts[1].ratio = 0.6f;
    opts[2].crossCheck = true;
    opts[3].ratio = 0.0f;
    opts[3].crossCheck = true;
    std::vector<std::vector<Bytes::Pair>> want[4];
    for (int k = 0; k < 4; k++)
        for (int m = 0; m < 3; m++) want[k].push_back(q->matchPairs(members[m], opts[k]));

    popsift::Gallery gallery(q->getDevice());
    CHECK(gallery.size() == 0 && gallery.matchPairs(q).empty() && gallery.counts(q, opts[0]).empty());
    for (int m = 0; m < 3; m++) CHECK(gallery.add(members[m]) == m);
    CHECK(gallery.size() == 3);
    delete sets[1]; /* the gallery holds copies */
    delete sets[2];

    for (int k = 0; k < 4; k++) {
        const std::vector<std::vector<Bytes::Pair>> got = gallery.matchPairs(q, opts[k]);
        const std::vector<int>                      n = gallery.counts(q, opts[k]);
        CHECK(got.size() == 3 && n.size() == 3);
        for (int m = 0; m < 3; m++) {
            const std::vector<Bytes::Pair>& w = want[k][(size_t)m];
            const std::vector<Bytes::Pair>& g = got[(size_t)m];
            CHECK(g.size() == w.size() && (size_t)n[(size_t)m] == w.size());
            for (size_t i = 0; i < g.size(); i++)
                CHECK(g[i].l == w[i].l && g[i].r == w[i].r && g[i].distBest == w[i].distBest && g[i].distSecond == w[i].distSecond);
        }
    }
    CHECK(want[0][1].empty() && want[0][0].size() > 10 && want[1][0].size() < want[0][0].size());
    CHECK(gallery.matchPairs(q).size() == 3 && gallery.matchPairs(q)[0].size() == want[0][0].size());
    std::printf("host_gallery ok: %zu %zu %zu\n", want[2][0].size(), want[2][1].size(), want[2][2].size());
    delete q;
    sift.uninit();
    return 0;
}
