// popsift::Gallery over links through the C++ API.
//   host_links_test a.pgm b.pgm c.pgm    three images through PopSift in MatchingMode with norm_multi = 9.  The gallery holds
//                                        a, b, an empty byte set and c; a, b and c as float sets, with their positions.  For
//                                        several option sets Gallery::matchPairs(links) must equal
//                                        FeaturesDevBytes::matchPairs(member a, member b) link by link and field by field,
//                                        over all a < b, a sequence, and a list with a == b, a reversed and a repeated link;
//                                        Gallery::pairPoints(links) must equal FeaturesDev::pairPoints per link.
// Prints "host_links ok: <pairs of (a, b)> <pairs of (a, c)> <pairs of (b, c)>" with the default ratio and the cross-check.
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
typedef popsift::Gallery::Link    Link;

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    popsift::Config cfg;
    cfg.setNormalizationMultiplier(9);
    PopSift               sift(cfg, popsift::Config::MatchingMode);
    popsift::FeaturesDev* floats[4] = {0, 0, 0, 0}; /* by member; member 2 is the empty byte set */
    Bytes*                bytes[4] = {0, 0, 0, 0};
    for (int k = 0; k < 3; k++) {
        const int      m = k < 2 ? k : 3;
        int            w, h;
        unsigned char* img = readPGMfile(argv[1 + k], w, h);
        if (!img) return 3;
        SiftJob* job = sift.enqueue(w, h, img);
        floats[m] = job->getDev();
        CHECK(floats[m] && floats[m]->getDescriptorCount() > 100);
        bytes[m] = floats[m]->toBytes();
        delete job;
        delete[] img;
    }
    Bytes none((const unsigned char*)0, 0, floats[0]->getDevice());
    bytes[2] = &none;

    popsift::Gallery gallery(floats[0]->getDevice());
    CHECK(gallery.matchPairs(std::vector<Link>()).empty());
    for (int m = 0; m < 4; m++) CHECK((m == 2 ? gallery.add(bytes[m]) : gallery.add(floats[m])) == m);

    const std::vector<Link> all = popsift::Gallery::allLinks(4), seq = popsift::Gallery::sequentialLinks(4, 1);
    CHECK(all.size() == 6 && all[0].a == 0 && all[0].b == 1 && all[2].b == 3 && all[3].a == 1 && all[5].a == 2 && all[5].b == 3);
    CHECK(seq.size() == 3 && seq[2].a == 2 && seq[2].b == 3 && popsift::Gallery::sequentialLinks(4, 9).size() == 6);
    CHECK(popsift::Gallery::allLinks(1).empty() && popsift::Gallery::sequentialLinks(3, 2).size() == 3);
    const std::vector<Link> mixed = {{3, 0}, {1, 1}, {2, 0}, {0, 3}, {3, 0}, {1, 2}};
    const std::vector<Link> lists[3] = {all, seq, mixed};

    Bytes::MatchOptions opts[4];
    opts[1].ratio = 0.6f;
    opts[2].crossCheck = true;
    opts[3].ratio = 0.0f;
    opts[3].crossCheck = true;
    size_t shown[3] = {0, 0, 0};
    for (int k = 0; k < 4; k++)
        for (int t = 0; t < 3; t++) {
            const std::vector<Link>&                    links = lists[t];
            const std::vector<std::vector<Bytes::Pair>> got = gallery.matchPairs(links, opts[k]);
            CHECK(got.size() == links.size());
            for (size_t e = 0; e < links.size(); e++) {
                const std::vector<Bytes::Pair> w = bytes[links[e].a]->matchPairs(bytes[links[e].b], opts[k]);
                const std::vector<Bytes::Pair>& g = got[e];
                CHECK(g.size() == w.size());
                for (size_t i = 0; i < g.size(); i++)
                    CHECK(g[i].l == w[i].l && g[i].r == w[i].r && g[i].distBest == w[i].distBest && g[i].distSecond == w[i].distSecond);
                if (links[e].a == 2 || links[e].b == 2) CHECK(g.empty());
            }
            /* the points of the lists, link by link */
            std::vector<int>         offsets;
            const std::vector<float> pts = gallery.pairPoints(links, got, offsets);
            CHECK(offsets.size() == links.size() + 1 && offsets[0] == 0 && pts.size() == 4 * (size_t)offsets.back());
            for (size_t e = 0; e < links.size(); e++) {
                CHECK((size_t)(offsets[e + 1] - offsets[e]) == got[e].size());
                if (got[e].empty()) continue;
                const std::vector<float> w = floats[links[e].a]->pairPoints(floats[links[e].b], got[e]);
                CHECK(w.size() == 4 * got[e].size());
                for (size_t i = 0; i < w.size(); i++) CHECK(pts[4 * (size_t)offsets[e] + i] == w[i]);
            }
            if (k == 2 && t == 0) {
                shown[0] = got[0].size();
                shown[1] = got[2].size();
                shown[2] = got[4].size();
                CHECK(got[0].size() > 10);
            }
        }
    CHECK(gallery.matchPairs(all).size() == 6);
    std::printf("host_links ok: %zu %zu %zu\n", shown[0], shown[1], shown[2]);
    for (int m = 0; m < 4; m++) {
        if (m == 2) continue;
        delete bytes[m];
        delete floats[m];
    }
    sift.uninit();
    return 0;
}
