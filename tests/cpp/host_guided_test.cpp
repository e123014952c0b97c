// FeaturesDev::fromHostPoints / matchGuided / matchGuidedRows through the C++ API.
//   host_guided_test scene.bin result.out
// scene.bin: int32 nl, nr, model; nine floats M; float max_err; then l (nl x 128 floats), lxy (nl x 2), r (nr x 128),
// rxy (nr x 2) (tests/guided_rule.py, scene()).  result.out receives the rows (nl x 20 bytes), then for the options
// {defaults, ratio 0.8 + cross-check}: int32 count and the pairs (16 bytes each): the test compares them with the C
// calls' bytes.  Prints "host_guided ok: <pairs> <pairs with the cross-check>".
#include <popsift/features.h>

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

typedef popsift::FeaturesDev Dev;

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    CHECK(f);
    int   head[3] = {0, 0, 0};
    float M[9], max_err = 0;
    CHECK(std::fread(head, 4, 3, f) == 3 && std::fread(M, 4, 9, f) == 9 && std::fread(&max_err, 4, 1, f) == 1);
    const int nl = head[0], nr = head[1];
    CHECK(nl > 0 && nr > 0);
    std::vector<float> l(128 * (size_t)nl), lxy(2 * (size_t)nl), r(128 * (size_t)nr), rxy(2 * (size_t)nr);
    CHECK(std::fread(l.data(), 4, l.size(), f) == l.size() && std::fread(lxy.data(), 4, lxy.size(), f) == lxy.size());
    CHECK(std::fread(r.data(), 4, r.size(), f) == r.size() && std::fread(rxy.data(), 4, rxy.size(), f) == rxy.size());
    std::fclose(f);

    Dev* L = Dev::fromHostPoints(l.data(), lxy.data(), nl);
    Dev* R = Dev::fromHostPoints(r.data(), rxy.data(), nr);
    CHECK(L && R && L->getFeatureCount() == nl && L->getDescriptorCount() == nl && R->getDescriptorCount() == nr);

    Dev::GuidedOptions o;
    CHECK(o.model == Dev::GuidedOptions::Homography && o.maxErr == 2.0f && o.ratio == 0.8f && !o.crossCheck && o.M[0] == 1.0f &&
          o.M[1] == 0.0f && o.M[8] == 1.0f);
    o.model = head[2] ? Dev::GuidedOptions::Epipolar : Dev::GuidedOptions::Homography;
    std::memcpy(o.M, M, sizeof M);
    o.maxErr = max_err;
    const std::vector<Dev::Match> rows = L->matchGuidedRows(R, o);
    const std::vector<Dev::Pair>  plain = L->matchGuided(R, o);
    o.crossCheck = true;
    const std::vector<Dev::Pair> crossed = L->matchGuided(R, o), again = L->matchGuided(R, o);
    CHECK(rows.size() == (size_t)nl && !plain.empty() && crossed.size() <= plain.size());
    CHECK(again.size() == crossed.size() && std::memcmp(again.data(), crossed.data(), crossed.size() * sizeof(Dev::Pair)) == 0);
    /* the pairs are the accepted rows */
    size_t accepted = 0;
    for (size_t i = 0; i < rows.size(); i++) {
        if (!rows[i].accept) continue;
        CHECK(accepted < plain.size() && plain[accepted].l == (int)i && plain[accepted].r == rows[i].best &&
              plain[accepted].distBest == rows[i].dist_best);
        accepted++;
    }
    CHECK(accepted == plain.size());
    /* the sets serve the unguided calls too, and pairPoints returns the positions given */
    const std::vector<float> pts = L->pairPoints(R, plain);
    for (size_t k = 0; k < plain.size(); k++)
        CHECK(pts[4 * k] == lxy[2 * (size_t)plain[k].l] && pts[4 * k + 3] == rxy[2 * (size_t)plain[k].r + 1]);
    /* an empty set on either side */
    Dev* E = Dev::fromHostPoints(nullptr, nullptr, 0);
    CHECK(E->matchGuided(R, o).empty() && L->matchGuided(E, o).empty() && E->matchGuidedRows(R, o).empty());
    const std::vector<Dev::Match> none = L->matchGuidedRows(E, o);
    CHECK(none.size() == (size_t)nl && none[0].best == -1 && none[0].second == -1 && !none[0].accept);

    f = std::fopen(argv[2], "wb");
    CHECK(f);
    for (const Dev::Match& m : rows) {
        const int   i[3] = {m.best, m.second, m.accept ? 1 : 0};
        const float d[2] = {m.dist_best, m.dist_second};
        CHECK(std::fwrite(i, 4, 3, f) == 3 && std::fwrite(d, 4, 2, f) == 2);
    }
    for (const std::vector<Dev::Pair>* p : {&plain, &crossed}) {
        const int n = (int)p->size();
        CHECK(std::fwrite(&n, 4, 1, f) == 1 && std::fwrite(p->data(), sizeof(Dev::Pair), p->size(), f) == p->size());
    }
    std::fclose(f);
    std::printf("host_guided ok: %zu %zu\n", plain.size(), crossed.size());
    delete E;
    delete L;
    delete R;
    return 0;
}
