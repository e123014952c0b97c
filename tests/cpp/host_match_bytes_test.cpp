// FeaturesDevBytes through the C++ API.
//   host_match_bytes_test l.pgm r.pgm    both images through PopSift in MatchingMode with norm_multi = 9; the sets go to
//                                        bytes on the GPU (FeaturesDev::toBytes).  matchAndGet must equal the C call's rows and
//                                        matchPairs the C call's pairs, field by field, for several option sets; matchPairs
//                                        must also equal matchAndGet in both directions filtered on the host by the rule of
//                                        include/popsift_hip.h; a set rebuilt from the downloaded bytes must match alike.
// Prints "host_match_bytes ok: <pairs with the default ratio and the cross-check>".
#include <popsift/features.h>
#include <popsift/popsift.h>

#include <popsift_hip.h>

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

typedef popsift::FeaturesDevBytes Bytes;

static std::vector<Bytes::Pair> by_rule(const std::vector<Bytes::Match>& F, const std::vector<Bytes::Match>& B,
                                        const Bytes::MatchOptions& o)
{
    std::vector<Bytes::Pair> out;
    if (B.empty()) return out;
    for (size_t i = 0; i < F.size(); i++) {
        const Bytes::Match& m = F[i];
        if (o.ratio != 0.0f && !(m.dist_best / m.dist_second < o.ratio)) continue;
        if (!(m.dist_best <= o.maxDist2)) continue;
        if (o.crossCheck && B[(size_t)m.best].best != (int)i) continue;
        out.push_back(Bytes::Pair{(int)i, m.best, m.dist_best, m.dist_second});
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
    cfg.setNormalizationMultiplier(9);
    PopSift               sift(cfg, popsift::Config::MatchingMode);
    SiftJob*              jl = sift.enqueue(w[0], h[0], img[0]);
    SiftJob*              jr = sift.enqueue(w[1], h[1], img[1]);
    popsift::FeaturesDev* fl = jl->getDev();
    popsift::FeaturesDev* fr = jr->getDev();
    CHECK(fl && fr && fl->getDescriptorCount() > 100 && fr->getDescriptorCount() > 100);
    Bytes* l = fl->toBytes();
    Bytes* r = fr->toBytes();
    CHECK(l && r && l->getDescriptorCount() == fl->getDescriptorCount() && r->getDescriptorCount() == fr->getDescriptorCount());
    CHECK(l->getDevice() == fl->getDevice());
    const int nl = l->getDescriptorCount(), nr = r->getDescriptorCount();

    /* rows: the C call's, field by field; the distances are integers */
    const std::vector<Bytes::Match> F = l->matchAndGet(r), B = r->matchAndGet(l);
    std::vector<popsift_hip_match>  raw((size_t)nl);
    CHECK(popsift_hip_match_bytes(l->getHandle(), r->getHandle(), raw.data()) == POPSIFT_HIP_OK);
    CHECK(F.size() == (size_t)nl && B.size() == (size_t)nr);
    double sum = 0.0;
    int    n_acc = 0;
    for (int i = 0; i < nl; i++) {
        const Bytes::Match& m = F[(size_t)i];
        CHECK(m.best == raw[(size_t)i].best && m.second == raw[(size_t)i].second && m.accept == (raw[(size_t)i].accept != 0) &&
              m.dist_best == raw[(size_t)i].dist_best && m.dist_second == raw[(size_t)i].dist_second);
        CHECK(m.dist_best == std::floor(m.dist_best) && m.dist_best <= 8323200.0f && m.dist_best <= m.dist_second);
        if (m.accept) {
            sum += m.dist_best;
            n_acc++;
        }
    }
    CHECK(n_acc > 10);
    const float cap = (float)(sum / n_acc); /* splits the accepted rows: their mean squared distance */

    Bytes::MatchOptions opts[5];
    opts[1].ratio = 0.6f;
    opts[2].ratio = 0.0f;
    opts[2].maxDist2 = cap;
    opts[3].ratio = 0.0f;
    opts[3].crossCheck = true;
    opts[4].maxDist2 = cap;
    opts[4].crossCheck = true;
    size_t sizes[5];
    for (int k = 0; k < 5; k++) {
        const std::vector<Bytes::Pair> want = by_rule(F, B, opts[k]);
        const std::vector<Bytes::Pair> got = l->matchPairs(r, opts[k]);
        popsift_hip_match_opts         o;
        popsift_hip_default_match_opts(&o);
        o.ratio = opts[k].ratio;
        o.max_dist2 = opts[k].maxDist2;
        o.cross_check = opts[k].crossCheck ? 1 : 0;
        std::vector<popsift_hip_pair> c((size_t)nl);
        int                           n = -1;
        CHECK(popsift_hip_match_pairs_bytes(l->getHandle(), r->getHandle(), &o, c.data(), c.size(), &n) == POPSIFT_HIP_OK);
        CHECK(n >= 0 && got.size() == (size_t)n && got.size() == want.size());
        for (size_t i = 0; i < got.size(); i++) {
            CHECK(got[i].l == c[i].l && got[i].r == c[i].r && got[i].distBest == c[i].dist_best &&
                  got[i].distSecond == c[i].dist_second);
            CHECK(got[i].l == want[i].l && got[i].r == want[i].r && got[i].distBest == want[i].distBest &&
                  got[i].distSecond == want[i].distSecond);
        }
        sizes[k] = got.size();
    }
    CHECK(l->matchPairs(r).size() == (size_t)n_acc && sizes[0] == (size_t)n_acc);
    CHECK(sizes[1] < sizes[0] && sizes[4] < sizes[3] && sizes[4] > 0 && sizes[2] < F.size() && sizes[3] < F.size());

    /* the same bytes from host memory: the same rows */
    std::vector<unsigned char> lb((size_t)nl * 128), rb((size_t)nr * 128);
    CHECK(popsift_hip_bytefeatures_download(l->getHandle(), lb.data(), 0) == POPSIFT_HIP_OK);
    CHECK(popsift_hip_bytefeatures_download(r->getHandle(), rb.data(), 0) == POPSIFT_HIP_OK);
    {
        Bytes                           l2(lb.data(), nl, l->getDevice()), r2(rb.data(), nr, r->getDevice());
        const std::vector<Bytes::Match> F2 = l2.matchAndGet(&r2);
        CHECK(F2.size() == F.size());
        for (size_t i = 0; i < F.size(); i++)
            CHECK(F2[i].best == F[i].best && F2[i].second == F[i].second && F2[i].accept == F[i].accept &&
                  F2[i].dist_best == F[i].dist_best && F2[i].dist_second == F[i].dist_second);
    }

    Bytes::MatchOptions cc;
    cc.crossCheck = true;
    std::printf("host_match_bytes ok: %zu\n", l->matchPairs(r, cc).size());
    delete l;
    delete r;
    delete fl;
    delete fr;
    delete jl;
    delete jr;
    sift.uninit();
    delete[] img[0];
    delete[] img[1];
    return 0;
}
