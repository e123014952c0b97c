// FeaturesDev::matchPairs through the C++ API.
//   host_match_pairs_test l.pgm r.pgm    both images through PopSift in MatchingMode; for several option sets matchPairs
//                                        must equal matchAndGet in both directions filtered on the host by the rule of
//                                        include/popsift_hip.h, field by field.
// Prints "host_match_pairs ok: <pairs with the default ratio and the cross-check>".
#include <popsift/features.h>
#include <popsift/popsift.h>

#include <cmath>
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

static std::vector<Dev::Pair> by_rule(const std::vector<Dev::Match>& F, const std::vector<Dev::Match>& B,
                                      const Dev::MatchOptions& o)
{
    std::vector<Dev::Pair> out;
    if (B.empty()) return out;
    for (size_t i = 0; i < F.size(); i++) {
        const Dev::Match& m = F[i];
        if (o.ratio != 0.0f && !(m.dist_best / m.dist_second < o.ratio)) continue;
        if (!(m.dist_best <= o.maxDist2)) continue;
        if (o.crossCheck && B[(size_t)m.best].best != (int)i) continue;
        out.push_back(Dev::Pair{(int)i, m.best, m.dist_best, m.dist_second});
    }
    return out;
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
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
    CHECK(l && r && l->getDescriptorCount() > 100 && r->getDescriptorCount() > 100);

    const std::vector<Dev::Match> F = l->matchAndGet(r), B = r->matchAndGet(l);
    /* a cap that splits the accepted rows: their mean squared distance */
    double sum = 0.0;
    int    n_acc = 0;
    for (const Dev::Match& m : F)
        if (m.accept) {
            sum += m.dist_best;
            n_acc++;
        }
    CHECK(n_acc > 10);
    const float cap = (float)(sum / n_acc);

    Dev::MatchOptions opts[5];
    opts[1].ratio = 0.6f;
    opts[2].ratio = 0.0f;
    opts[2].maxDist2 = cap;
    opts[3].ratio = 0.0f;
    opts[3].crossCheck = true;
    opts[4].maxDist2 = cap;
    opts[4].crossCheck = true;
    size_t sizes[5];
    for (int k = 0; k < 5; k++) {
        const std::vector<Dev::Pair> want = by_rule(F, B, opts[k]);
        const std::vector<Dev::Pair> got = l->matchPairs(r, opts[k]);
        CHECK(got.size() == want.size());
        CHECK(want.empty() || std::memcmp(got.data(), want.data(), sizeof(Dev::Pair) * want.size()) == 0);
        sizes[k] = got.size();
    }
    /* the defaults are matchAndGet's accepted rows; every filter removes something here */
    CHECK(l->matchPairs(r).size() == (size_t)n_acc && sizes[0] == (size_t)n_acc);
    CHECK(sizes[1] < sizes[0] && sizes[4] < sizes[3] && sizes[4] > 0 && sizes[2] < F.size() && sizes[3] < F.size());
    /* the sweeps' own results are untouched by the calls in between */
    const std::vector<Dev::Match> F2 = l->matchAndGet(r);
    CHECK(F2.size() == F.size());
    for (size_t i = 0; i < F.size(); i++)
        CHECK(F2[i].best == F[i].best && F2[i].second == F[i].second && F2[i].accept == F[i].accept &&
              F2[i].dist_best == F[i].dist_best);

    Dev::MatchOptions cc;
    cc.crossCheck = true;
    std::printf("host_match_pairs ok: %zu\n", l->matchPairs(r, cc).size());
    delete l;
    delete r;
    delete jl;
    delete jr;
    sift.uninit();
    delete[] img[0];
    delete[] img[1];
    return 0;
}
