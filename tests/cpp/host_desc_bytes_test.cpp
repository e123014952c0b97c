// Config::ByteDescriptors through the C++ API.
//   host_desc_bytes_test                       (built with -DDESC_BYTES_CPU_ONLY) Config and FeaturesHost, no GPU
//   host_desc_bytes_test a.pgm b.pgm ...       every image through PopSift in the float format and in the byte format
//                                              (one object each, norm multiplier 9); the byte results must equal the
//                                              rule of include/popsift_hip.h applied to the float results, feature by
//                                              feature, and MatchingMode must ignore the format.
// The feature order differs between runs (atomic compaction), so features are matched by their (x, y, sigma,
// orientation) bits.  Prints "host_desc_bytes ok" / "host_desc_bytes cpu ok".
#include <popsift/features.h>
#include <popsift/popsift.h>

#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../popsift_amd/host/pgmread.h"

#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);        \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static uint8_t q(float d)
{
    if (std::isnan(d) || d <= 0.0f) return 0;
    if (d >= 255.0f) return 255;
    return (uint8_t)roundf(d);
}

static uint32_t bits(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

static int cpu_checks()
{
    popsift::Config a, b;
    CHECK(a.getDescriptorFormat() == popsift::Config::FloatDescriptors);
    CHECK(a.equal(b));
    b.setDescriptorFormat(popsift::Config::ByteDescriptors);
    CHECK(b.getDescriptorFormat() == popsift::Config::ByteDescriptors);
    CHECK(!a.equal(b) && a != b);

    popsift::FeaturesHost f;
    f.resetBytes(3, 4);
    CHECK(f.hasDescriptorBytes() && f.getDescriptorBytes() != nullptr && f.getDescriptors() == nullptr);
    CHECK(f.getFeatureCount() == 3 && f.getDescriptorCount() == 4);
    popsift::Feature* ft = f.getFeatures();
    int*              idx = f.getDescriptorIndices();
    for (int i = 0; i < 3; i++) {
        ft[i].xpos = 10.0f + i;
        ft[i].ypos = 20.0f;
        ft[i].sigma = 2.0f;
        ft[i].num_ori = i == 1 ? 2 : 1;
        for (int k = 0; k < 4; k++) ft[i].desc[k] = nullptr;
    }
    idx[0 * 4 + 0] = 0;
    idx[1 * 4 + 0] = 1;
    idx[1 * 4 + 1] = 2;
    idx[2 * 4 + 0] = 3;
    for (int d = 0; d < 4; d++)
        for (int k = 0; k < 128; k++) f.getDescriptorBytes()[d * 128 + k] = (unsigned char)(d * 60 + k);
    CHECK(f.descriptorBytes(1, 1) == f.getDescriptorBytes() + 2 * 128);
    CHECK(f.descriptorBytes(1, 2) == nullptr && f.descriptorBytes(0, 1) == nullptr && f.descriptorBytes(3, 0) == nullptr);
    std::ostringstream os;
    f.print(os, false);
    std::istringstream is(os.str());
    std::string        line;
    int                rows = 0;
    while (std::getline(is, line)) {
        std::istringstream ls(line);
        std::vector<double> v;
        double              x;
        while (ls >> x) v.push_back(x);
        CHECK(v.size() == 133);
        const int d = rows; /* rows come in descriptor order here */
        for (int k = 0; k < 128; k++) CHECK(v[5 + k] == (double)(unsigned char)(d * 60 + k));
        rows++;
    }
    CHECK(rows == 4);
    /* back to floats: the byte block is gone */
    f.reset(2, 2);
    CHECK(!f.hasDescriptorBytes() && f.getDescriptors() != nullptr && f.descriptorBytes(0, 0) == nullptr);
    std::printf("host_desc_bytes cpu ok\n");
    return 0;
}

#ifndef DESC_BYTES_CPU_ONLY
typedef std::array<uint32_t, 5> Key;

static Key key(const popsift::Feature& f, int o)
{
    return Key{bits(f.xpos), bits(f.ypos), bits(f.sigma), bits(f.orientation[o]), (uint32_t)o};
}

struct Img {
    int            w, h;
    unsigned char* p;
};

static int gpu_checks(const std::vector<Img>& imgs)
{
    popsift::Config fc;
    fc.setNormalizationMultiplier(9);
    popsift::Config bc = fc;
    bc.setDescriptorFormat(popsift::Config::ByteDescriptors);
    PopSift fs(fc), bs(bc);
    std::vector<SiftJob*> fj, bj;
    for (const Img& im : imgs) {
        fj.push_back(fs.enqueue(im.w, im.h, im.p));
        bj.push_back(bs.enqueue(im.w, im.h, im.p));
    }
    long long checked = 0, saturated = 0;
    for (size_t i = 0; i < imgs.size(); i++) {
        popsift::FeaturesHost* ff = fj[i]->get();
        popsift::FeaturesHost* bf = bj[i]->get();
        CHECK(ff && bf && !ff->hasDescriptorBytes() && bf->hasDescriptorBytes());
        CHECK(ff->getFeatureCount() == bf->getFeatureCount() && ff->getDescriptorCount() == bf->getDescriptorCount());
        CHECK(bf->getDescriptors() == nullptr);
        std::map<Key, std::array<uint8_t, 128>> want;
        for (int n = 0; n < ff->getFeatureCount(); n++) {
            const popsift::Feature& f = ff->getFeatures()[n];
            for (int o = 0; o < f.num_ori; o++) {
                std::array<uint8_t, 128> b;
                for (int k = 0; k < 128; k++) b[(size_t)k] = q(f.desc[o]->features[k]);
                want[key(f, o)] = b;
            }
        }
        for (int n = 0; n < bf->getFeatureCount(); n++) {
            const popsift::Feature& f = bf->getFeatures()[n];
            for (int o = 0; o < 4; o++) CHECK(f.desc[o] == nullptr);
            CHECK(bf->descriptorBytes(n, f.num_ori) == nullptr);
            for (int o = 0; o < f.num_ori; o++) {
                const unsigned char* b = bf->descriptorBytes(n, o);
                CHECK(b != nullptr);
                auto it = want.find(key(f, o));
                CHECK(it != want.end());
                CHECK(std::memcmp(b, it->second.data(), 128) == 0);
                for (int k = 0; k < 128; k++) saturated += b[k] == 255;
                checked++;
            }
        }
        delete ff;
        delete bf;
        delete fj[i];
        delete bj[i];
    }
    fs.uninit();
    bs.uninit();
    CHECK(checked > 0);

    /* MatchingMode ignores the format: device-resident float sets */
    PopSift                ms(bc, popsift::Config::MatchingMode);
    SiftJob*               j = ms.enqueue(imgs[0].w, imgs[0].h, imgs[0].p);
    popsift::FeaturesDev*  dev = j->getDev();
    CHECK(dev != nullptr && dev->getDescriptorCount() > 0 && dev->getDescriptors() != nullptr);
    delete dev;
    delete j;
    ms.uninit();
    std::printf("host_desc_bytes ok: %lld descriptors, %lld saturated bytes\n", checked, saturated);
    return 0;
}
#endif

int main(int argc, char** argv)
{
    if (int rc = cpu_checks()) return rc;
#ifndef DESC_BYTES_CPU_ONLY
    std::vector<Img> imgs;
    for (int i = 1; i < argc; i++) {
        Img im;
        im.p = readPGMfile(argv[i], im.w, im.h);
        if (!im.p) return 3;
        imgs.push_back(im);
    }
    if (!imgs.empty())
        if (int rc = gpu_checks(imgs)) return rc;
#else
    (void)argc;
    (void)argv;
#endif
    return 0;
}
