// GPU test driver for PopSift::enqueueMasked: one PopSift object in raster feature order extracts the image dir/img.u8 or
// dir/img.f32 (w x h) in R jobs.  Job j is masked with dir/mask.u8 (w x h bytes) when j % 3 != 1 and unmasked (a null mask,
// which behaves like enqueue) when j % 3 == 1, so that with POPSIFT_BATCH > 1 a worker batches masked and unmasked jobs
// together.  Every job's features (as popsift_hip_feature records: desc[] as indices into the job's descriptor array) and
// descriptors go to dir/job<j>.feat / dir/job<j>.desc for the comparison with the C ABI.
//   host_mask_test <dir> <w> <h> <float 0|1> <R>
#include <popsift/features.h>
#include <popsift/popsift.h>

#include <popsift_hip.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

template <class T>
static bool read_all(const std::string& path, std::vector<T>& v)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    const bool ok = fread(v.data(), sizeof(T), v.size(), f) == v.size();
    fclose(f);
    return ok;
}

int main(int argc, char** argv)
{
    if (argc != 6) {
        fprintf(stderr, "usage: host_mask_test dir w h float repeats\n");
        return 2;
    }
    const std::string dir = argv[1];
    const int         w = atoi(argv[2]), h = atoi(argv[3]), rep = atoi(argv[5]);
    const bool        is_float = atoi(argv[4]) != 0;
    std::vector<unsigned char> img8((size_t)w * h), mask((size_t)w * h);
    std::vector<float>         img32((size_t)w * h);
    if (!read_all(dir + "/mask.u8", mask)) return 3;
    if (!(is_float ? read_all(dir + "/img.f32", img32) : read_all(dir + "/img.u8", img8))) return 3;

    popsift::Config cfg;
    cfg.setFeatureOrder(popsift::Config::RasterOrder);
    PopSift               ps(cfg, popsift::Config::ExtractingMode, is_float ? PopSift::FloatImages : PopSift::ByteImages);
    std::vector<SiftJob*> jobs;
    for (int j = 0; j < rep; j++) {
        const unsigned char* m = (j % 3 != 1) ? mask.data() : nullptr;
        jobs.push_back(is_float ? ps.enqueueMasked(w, h, img32.data(), m) : ps.enqueueMasked(w, h, img8.data(), m));
    }
    for (int j = 0; j < rep; j++) {
        popsift::FeaturesHost*           fh = jobs[(size_t)j]->get();
        std::vector<popsift_hip_feature> out((size_t)fh->size());
        for (int i = 0; i < fh->size(); i++) {
            const popsift::Feature& s = fh->getFeatures()[i];
            popsift_hip_feature&    d = out[(size_t)i];
            d.debug_octave = s.debug_octave;
            d.xpos = s.xpos;
            d.ypos = s.ypos;
            d.sigma = s.sigma;
            d.num_ori = s.num_ori;
            for (int k = 0; k < POPSIFT_HIP_ORI_MAX; k++) {
                d.orientation[k] = s.orientation[k];
                d.desc_idx[k] = s.desc[k] ? (int)(s.desc[k] - fh->getDescriptors()) : -1;
            }
        }
        const std::string base = dir + "/job" + std::to_string(j);
        FILE*             f = fopen((base + ".feat").c_str(), "wb");
        if (!f || fwrite(out.data(), sizeof(popsift_hip_feature), out.size(), f) != out.size()) return 4;
        fclose(f);
        f = fopen((base + ".desc").c_str(), "wb");
        const size_t nd = (size_t)fh->getDescriptorCount();
        if (!f || fwrite(fh->getDescriptors(), 128 * sizeof(float), nd, f) != nd) return 4;
        fclose(f);
        delete fh;
        delete jobs[(size_t)j];
    }
    ps.uninit();
    printf("host_mask_test ok\n");
    return 0;
}
