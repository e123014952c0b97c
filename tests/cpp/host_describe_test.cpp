// GPU test driver for PopSift::enqueue(w, h, img, frames): one PopSift object describes the frames of dir/frames.bin in the
// u8 image dir/img.u8 (w x h), in R describe jobs with an extraction job after every third (a worker batches describe jobs
// with describe jobs only), and writes every describe job's features (as popsift_hip_feature records: desc[] as indices into the job's
// descriptor array) and descriptors to dir/job<j>.feat / dir/job<j>.desc for the comparison with the C ABI.  Job j
// describes the first n - j * n / (2 R) frames.
//   host_describe_test <dir> <w> <h> <n_frames> <compute_orientation 0|1> <R>
#include <popsift/features.h>
#include <popsift/popsift.h>

#include <popsift_hip.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 7) {
        fprintf(stderr, "usage: host_describe_test dir w h n_frames compute_orientation repeats\n");
        return 2;
    }
    const std::string dir = argv[1];
    const int         w = atoi(argv[2]), h = atoi(argv[3]), n = atoi(argv[4]), rep = atoi(argv[6]);
    const bool        compute = atoi(argv[5]) != 0;
    std::vector<unsigned char>  img((size_t)w * h);
    std::vector<popsift::Frame> frames((size_t)n);
    FILE*                       f = fopen((dir + "/img.u8").c_str(), "rb");
    if (!f || fread(img.data(), 1, img.size(), f) != img.size()) return 3;
    fclose(f);
    f = fopen((dir + "/frames.bin").c_str(), "rb");
    if (!f || fread(frames.data(), sizeof(popsift::Frame), frames.size(), f) != frames.size()) return 3;
    fclose(f);

    popsift::Config cfg;
    PopSift         ps(cfg, popsift::Config::ExtractingMode, PopSift::ByteImages);
    std::vector<SiftJob*> jobs, extractions;
    for (int j = 0; j < rep; j++) {
        const std::vector<popsift::Frame> sub(frames.begin(), frames.begin() + (n - j * n / (2 * rep)));
        jobs.push_back(ps.enqueue(w, h, img.data(), sub, compute));
        if (j % 3 == 2) extractions.push_back(ps.enqueue(w, h, img.data()));
    }
    for (int j = 0; j < rep; j++) {
        popsift::FeaturesHost* fh = jobs[(size_t)j]->get();
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
        f = fopen((base + ".feat").c_str(), "wb");
        if (!f || fwrite(out.data(), sizeof(popsift_hip_feature), out.size(), f) != out.size()) return 4;
        fclose(f);
        f = fopen((base + ".desc").c_str(), "wb");
        const size_t nd = (size_t)fh->getDescriptorCount();
        if (!f || fwrite(fh->getDescriptors(), 128 * sizeof(float), nd, f) != nd) return 4;
        fclose(f);
        delete fh;
        delete jobs[(size_t)j];
    }
    for (SiftJob* e : extractions) {
        popsift::FeaturesHost* fh = e->get();
        if (fh->size() == 0) return 5;
        delete fh;
        delete e;
    }
    ps.uninit();
    printf("host_describe_test ok\n");
    return 0;
}
