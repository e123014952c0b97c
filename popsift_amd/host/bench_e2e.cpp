/*
 * popsift-bench -- steady-state throughput of the drop-in C++ API, host image in -> host features out
 * (SURVEY 8(d) "T_e2e": wall time per image through enqueue() ... get() with many images in flight).
 * PCIe-inclusive: every image is uploaded and its features + descriptors (about 53 MB for the dense
 * synthetic 1080p image) are downloaded into a FeaturesHost.  Never the headline `value` of bench.py.
 *   popsift-bench [--images N] [--width W] [--height H] [--inflight K] [--callers C] [--seed S] [--pgm a.pgm,b.pgm,...]
 *                 [--threshold T] [--desc-bytes] [--feature-order arrival|raster]
 * --callers: threads that enqueue and drain (each its share of the images and of the in-flight budget; default 1, the
 * reference's demo loop -- bench.py passes one per GPU: a single caller copies about 10 GB/s of images, enough for one GPU
 * on dense images and not for eight).  The line reports what a caller thread spends per image: in enqueue() (the copy of
 * the image into a pinned block), blocked in get(), and in the two deletes.
 * --threshold: popsift::Config::setThreshold (0.04 by default; 0.17 leaves ~2 features per 1000 pixels of the synthetic
 * images -- the keypoint-sparse regime, where the results are a few MB and PCIe is no longer the limit).
 * --desc-bytes: popsift::Config::ByteDescriptors -- the descriptors are quantized on the GPU and 128 bytes instead of 512
 * cross PCIe per descriptor (d2h_mb_per_image reports the results' bytes of either format).
 * --feature-order: popsift::Config::setFeatureOrder -- raster adds the ordering pass (order.hip) to every extraction.
 * --pgm: the images to cycle through (bench.py passes the popsift_amd/synth.py images of the headline workload);
 * without it a cheap built-in generator is used.
 * Contexts per GPU come from POPSIFT_CONTEXTS_PER_DEVICE, GPUs from POPSIFT_DEVICES.
 */
#include <popsift/features.h>
#include <popsift/popsift.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <random>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "pgmread.h"

/* built-in stand-in for popsift_amd/synth.py (used when no --pgm files are given): smoothed noise, deterministic */
static std::vector<unsigned char> make_image(int w, int h, unsigned seed)
{
    std::mt19937                          rng(seed);
    std::uniform_real_distribution<float> uni(0.0f, 1.0f);
    std::vector<float>                    a((size_t)w * h), b((size_t)w * h);
    for (float& v : a) v = uni(rng);
    for (int pass = 0; pass < 2; pass++) { /* two box blurs */
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const int x0 = x > 0 ? x - 1 : x, x1 = x < w - 1 ? x + 1 : x;
                b[(size_t)y * w + x] = (a[(size_t)y * w + x0] + a[(size_t)y * w + x] + a[(size_t)y * w + x1]) / 3.0f;
            }
        for (int y = 0; y < h; y++) {
            const int y0 = y > 0 ? y - 1 : y, y1 = y < h - 1 ? y + 1 : y;
            for (int x = 0; x < w; x++)
                a[(size_t)y * w + x] = (b[(size_t)y0 * w + x] + b[(size_t)y * w + x] + b[(size_t)y1 * w + x]) / 3.0f;
        }
    }
    std::vector<unsigned char> img((size_t)w * h);
    for (size_t i = 0; i < img.size(); i++) {
        const float v = 128.0f + (a[i] - 0.5f) * 700.0f;
        img[i] = (unsigned char)(v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v));
    }
    return img;
}

int main(int argc, char** argv)
{
    int images = 64, w = 1920, h = 1080, inflight = 16, callers = 1;
    unsigned seed = 1;
    float    threshold = -1.0f;
    bool     desc_bytes = false, raster = false;
    std::string pgm;
    for (int i = 1; i < argc; i += 2) {
        if (!strcmp(argv[i], "--desc-bytes")) { /* the one option without a value */
            desc_bytes = true;
            i--;
            continue;
        }
        if (i + 1 >= argc) break;
        if (!strcmp(argv[i], "--pgm")) pgm = argv[i + 1];
        else if (!strcmp(argv[i], "--images")) images = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--width")) w = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--height")) h = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--inflight")) inflight = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--callers")) callers = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--seed")) seed = (unsigned)atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--threshold")) threshold = (float)atof(argv[i + 1]);
        else if (!strcmp(argv[i], "--feature-order")) {
            if (strcmp(argv[i + 1], "arrival") && strcmp(argv[i + 1], "raster")) {
                fprintf(stderr, "popsift-bench: --feature-order arrival|raster, not %s\n", argv[i + 1]);
                return 2;
            }
            raster = !strcmp(argv[i + 1], "raster");
        }
    }
    std::vector<std::vector<unsigned char>> pool;
    if (!pgm.empty()) {
        std::stringstream ss(pgm);
        std::string       f;
        while (std::getline(ss, f, ',')) {
            int            pw = 0, ph = 0;
            unsigned char* p = readPGMfile(f, pw, ph);
            if (!p) return 2;
            if (pool.empty()) {
                w = pw;
                h = ph;
            } else if (pw != w || ph != h) {
                fprintf(stderr, "popsift-bench: %s is not %d x %d\n", f.c_str(), w, h);
                return 2;
            }
            pool.emplace_back(p, p + (size_t)pw * ph);
            delete[] p;
        }
    }
    if (pool.empty())
        for (int k = 0; k < 4; k++) pool.push_back(make_image(w, h, seed + k));

    popsift::Config config;
    if (threshold >= 0.0f) config.setThreshold(threshold);
    if (desc_bytes) config.setDescriptorFormat(popsift::Config::ByteDescriptors);
    if (raster) config.setFeatureOrder(popsift::Config::RasterOrder);
    PopSift         sift(config, popsift::Config::ExtractingMode, PopSift::ByteImages);

    if (callers < 1) callers = 1;
    if (inflight < callers) inflight = callers;
    struct CallerTime {
        double    enqueue = 0, get = 0, del = 0;
        long long feats = 0, descs = 0;
    };
    typedef std::chrono::steady_clock clk;
    auto since = [](clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); };
    /* caller t takes images t, t + callers, ... and keeps at most inflight / callers jobs in flight */
    auto run_caller = [&](int t, int n, CallerTime& ct) {
        std::deque<SiftJob*> q;
        const int            mine = inflight / callers + (t < inflight % callers ? 1 : 0);
        auto                 drain_one = [&]() {
            SiftJob* j = q.front();
            q.pop_front();
            clk::time_point    t0 = clk::now();
            popsift::Features* f = j->get();
            ct.get += since(t0);
            ct.feats += f->getFeatureCount();
            ct.descs += f->getDescriptorCount();
            t0 = clk::now();
            delete f;
            delete j;
            ct.del += since(t0);
        };
        for (int i = t; i < n; i += callers) {
            const clk::time_point t0 = clk::now();
            SiftJob*              j = sift.enqueue(w, h, pool[(size_t)i % pool.size()].data());
            ct.enqueue += since(t0);
            q.push_back(j);
            if ((int)q.size() >= mine) drain_one();
        }
        while (!q.empty()) drain_one();
    };
    auto run = [&](int n, CallerTime& sum) {
        std::vector<CallerTime>  cts((size_t)callers);
        std::vector<std::thread> th;
        for (int t = 1; t < callers; t++) th.emplace_back(run_caller, t, n, std::ref(cts[(size_t)t]));
        run_caller(0, n, cts[0]);
        for (auto& x : th) x.join();
        sum = CallerTime();
        for (const CallerTime& c : cts) {
            sum.enqueue += c.enqueue;
            sum.get += c.get;
            sum.del += c.del;
            sum.feats += c.feats;
            sum.descs += c.descs;
        }
    };
    CallerTime warm, ct;
    /* warm-up: device buffers and one pinned result block per job that can be in flight (allocating pinned
     * memory takes tens of milliseconds per block and stalls every context while it happens) */
    std::string warm_rates; /* Mpix/s of every warm-up pass: shows a ramp (pools) or a disturbance if there is one */
    auto        timed_warm = [&](int n) {
        const auto w1 = clk::now();
        run(n, warm);
        char buf[32];
        snprintf(buf, sizeof(buf), "%s%.0f", warm_rates.empty() ? "" : ", ", (double)n * w * h / since(w1) / 1e6);
        warm_rates += buf;
    };
    timed_warm(inflight + sift.getContextCount() + 2);
    /* ... and at least a quarter of a second of work at the measured load; the rate of every pass is reported
     * (warmup_passes_mpix_s): a run disturbed from outside shows there -- bench.py's first child process, started right
     * after the parent had released ~50 GB of device memory, read half the rate in EVERY pass */
    {
        const auto w0 = clk::now();
        for (int k = 0; k < 16 && since(w0) < 0.25; k++) timed_warm(std::max(inflight, 32));
    }
    const auto t0 = clk::now();
    run(images, ct);
    const double sec = since(t0);
    printf("{\"e2e_host_api_mpix_s\": %.1f, \"images\": %d, \"width\": %d, \"height\": %d, \"contexts\": %d, "
           "\"in_flight\": %d, \"callers\": %d, \"ms_per_image\": %.3f, \"features_per_image\": %.0f, "
           "\"descriptors_per_image\": %.0f, \"caller_us_per_image\": {\"enqueue\": %.1f, \"get_blocked\": %.1f, "
           "\"delete\": %.1f}, \"warmup_passes_mpix_s\": [%s], \"input\": \"%s\", \"desc_format\": \"%s\", "
           "\"d2h_mb_per_image\": %.2f}\n",
           (double)images * w * h / sec / 1e6, images, w, h, sift.getContextCount(), inflight, callers, sec * 1e3 / images,
           (double)ct.feats / images, (double)ct.descs / images, ct.enqueue * 1e6 / images, ct.get * 1e6 / images,
           ct.del * 1e6 / images, warm_rates.c_str(), pgm.empty() ? "built-in generator" : "pgm files", desc_bytes ? "u8" : "f32",
           /* what the downloads carry: the 52-byte POD feature records and 128 floats or 128 bytes per descriptor */
           ((double)ct.feats * 52 + (double)ct.descs * (desc_bytes ? 128 : 512)) / images / 1e6);
    sift.uninit();
    return 0;
}
