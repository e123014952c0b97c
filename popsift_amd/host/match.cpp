/*
 * popsift-match -- the reference's matching demo (src/application/match.cpp:47-276) against this
 * library: extract two images in Config::MatchingMode (features stay on the GPU), print the counts,
 * brute-force match left against right (one accept / reject line per left descriptor).
 * Extension: --pairs [--ratio R] [--max-dist D] [--cross-check] prints the correspondences instead.
 * Extension: --bytes quantizes both sets on the GPU and matches the byte descriptors (exact integer distances).
 * Extension: --verify homography|affine|epipolar [--hypotheses T] [--max-err E] [--seed S] with --pairs fits the model to
 * the pairs by RANSAC on the GPU (popsift::Verifier) and prints it with its inlier count after the pair lines; epipolar is
 * the fundamental matrix of two views of a 3-D scene.
 * Extension: --guided [--guided-err E] with --verify matches again under the model just found (FeaturesDev::matchGuided)
 * and prints those pairs after the model block.
 * Extension: --refit [--refit-rounds N] with --verify refits the model RANSAC found to all its inliers by least squares
 * (Verifier::refit) and prints the refitted model under the RANSAC block; with --guided the refitted model is the guide.
 * Extension: --gallery FILE (repeatable, instead of -r; implies --bytes --pairs) matches the left image against every
 * gallery image in one pass (popsift::Gallery) and prints, per gallery image in the order given, its pair count and pairs.
 * Extension: --gallery-verify homography|affine|epipolar [--hypotheses T] [--max-err E] [--seed S] with --gallery fits the
 * model to every gallery image's pairs in one call (Gallery::pairPoints, Verifier::ransacMany) and prints it with its inlier
 * count under the image's pair lines, then, after the total, the gallery images ranked by their inliers.
 * Extension: --all-pairs or --sequential K with --gallery (and without -l) matches the gallery images with each other in one
 * pass -- every a < b, or every image with its K successors (Gallery::matchPairs over links) -- and prints one line per link:
 * its pair count and, with --gallery-verify, its inlier count and model (Gallery::pairPoints over links,
 * Verifier::ransacMany).
 */
#include <popsift/common/device_prop.h>
#include <popsift/features.h>
#include <popsift/popsift.h>
#include <popsift/sift_conf.h>
#include <popsift/verify.h>

#include <popsift_hip.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <functional>
#include <iostream>
#include <string>
#include <vector>

#include "cli_options.h"
#include "pgmread.h"

using namespace std;

static bool print_dev_info = false;
static bool print_time_info = false;
static bool write_as_uchar = false;
static bool dont_write = false;
static bool pgmread_loading = false;
static bool print_pairs = false;
static bool match_bytes = false;
static popsift::FeaturesDev::MatchOptions pair_opts;
static bool verify_pairs = false;
static popsift::RansacOptions verify_opts;
static bool verify_epipolar = false;
static bool guided_pairs = false;
static float guided_err = 0.0f; /* 0: --max-err */
static bool refit_model = false;
static int refit_rounds = 4;
static vector<string> gallery_files;
static string gallery_verify; /* empty: off */
static bool all_pairs = false;
static int sequential_k = 0; /* 0: off */

static void parseargs(int argc, char** argv, popsift::Config& config, string& lFile, string& rFile)
{
    cli::Options o;
    /* match.cpp:50-60 */
    o.flag("help", 'h', "Options", "Print usage", [] {});
    o.flag("verbose", 'v', "Options", "", [&] { config.setVerbose(); });
    o.flag("log", 0, "Options", "Write debugging files", [&] { config.setLogMode(popsift::Config::All); });
    o.val("left", 'l', "Options", "\"Left\"  input file", [&](const string& v) { lFile = v; });
    o.val("right", 'r', "Options", "\"Right\" input file (required without --gallery)", [&](const string& v) { rFile = v; });
    /* match.cpp:61-73 */
    o.ival("octaves", "Parameters", "Number of octaves", [&](int v) { config.octaves = v; });
    o.ival("levels", "Parameters", "Number of levels per octave", [&](int v) { config.levels = v; });
    o.fval("sigma", "Parameters", "Initial sigma value", [&](float f) { config.setSigma(f); });
    o.fval("threshold", "Parameters", "Contrast threshold", [&](float f) { config.setThreshold(f); });
    o.fval("edge-threshold", "Parameters", "On-edge threshold", [&](float f) { config.setEdgeLimit(f); });
    o.fval("edge-limit", "Parameters", "On-edge threshold", [&](float f) { config.setEdgeLimit(f); });
    o.fval("downsampling", "Parameters", "Downscale width and height of input by 2^N",
           [&](float f) { config.setDownsampling(f); });
    o.fval("initial-blur", "Parameters", "Assume initial blur, subtract when blurring first time",
           [&](float f) { config.setInitialBlur(f); });
    /* match.cpp:74-112 */
    o.val("gauss-mode", 0, "Modes", popsift::Config::getGaussModeUsage(), [&](const string& s) { config.setGaussMode(s); });
    o.val("desc-mode", 0, "Modes", "Choice of descriptor extraction modes:\nloop, iloop, grid, igrid, notile\nDefault is loop",
          [&](const string& s) { config.setDescMode(s); });
    o.flag("popsift-mode", 0, "Modes", "PopSift's own refinement and upscale rules (default)",
           [&] { config.setMode(popsift::Config::PopSift); });
    o.flag("vlfeat-mode", 0, "Modes", "VLFeat-like refinement (levels stay fixed)", [&] { config.setMode(popsift::Config::VLFeat); });
    o.flag("opencv-mode", 0, "Modes", "OpenCV-like upscale shift, refinement steps and filter widths",
           [&] { config.setMode(popsift::Config::OpenCV); });
    o.flag("direct-scaling", 0, "Modes", "Direct each octave from upscaled orig instead of blurred level.",
           [&] { config.setScalingMode(popsift::Config::ScaleDirect); });
    o.ival("norm-multi", "Modes", "Multiply the descriptor by pow(2,<int>).", [&](int i) { config.setNormalizationMultiplier(i); });
    o.val("norm-mode", 0, "Modes", popsift::Config::getNormModeUsage(), [&](const string& s) { config.setNormMode(s); });
    o.flag("root-sift", 0, "Modes", popsift::Config::getNormModeUsage(), [&] { config.setNormMode(popsift::Config::RootSift); });
    o.ival("filter-max-extrema", "Modes", "Approximate max number of extrema.", [&](int f) { config.setFilterMaxExtrema(f); });
    o.ival("filter-grid", "Modes", "Grid edge length for extrema filtering (ie. value 4 leads to a 4x4 grid)",
           [&](int f) { config.setFilterGridSize(f); });
    o.val("filter-sort", 0, "Modes", "Sort extrema in each cell by scale, either random (default), up or down",
          [&](const string& s) { config.setFilterSorting(s); });
    /* match.cpp:114-125 */
    o.flag("print-gauss-tables", 0, "Informational", "A debug output printing Gauss filter size and tables",
           [&] { config.setPrintGaussTables(); });
    o.flag("print-dev-info", 0, "Informational", "A debug output printing CUDA device information", [&] { print_dev_info = true; });
    o.flag("print-time-info", 0, "Informational", "A debug output printing image processing time after load()",
           [&] { print_time_info = true; });
    o.flag("write-as-uchar", 0, "Informational", "Output descriptors rounded to int", [&] { write_as_uchar = true; });
    o.flag("dont-write", 0, "Informational", "Suppress descriptor output", [&] { dont_write = true; });
    o.flag("pgmread-loading", 0, "Informational", "Use the old image loader instead of LibDevIL", [&] { pgmread_loading = true; });
    /* extension: correspondences (FeaturesDev::matchPairs) instead of the reference's line per left descriptor */
    o.flag("pairs", 0, "Matching", "Print the matching pairs only: one line per pair, then their count", [&] { print_pairs = true; });
    o.fval("ratio", "Matching", "With --pairs: a pair needs best / second squared distance below this (default 0.8, 0 = off)",
           [&](float f) { pair_opts.ratio = f; });
    o.fval("max-dist", "Matching", "With --pairs: a pair needs an L2 distance of at most this",
           [&](float f) { pair_opts.maxDist2 = f * f; });
    o.flag("cross-check", 0, "Matching", "With --pairs: keep mutual nearest neighbours only", [&] { pair_opts.crossCheck = true; });
    o.flag("bytes", 0, "Matching",
           "Match byte descriptors: both sets are quantized on the GPU (0 .. 255, rounded) and matched with exact integer\n"
           "distances; --max-dist is then in byte units.  Needs --norm-multi (9 gives VLFeat-style bytes)",
           [&] { match_bytes = true; });
    o.val("verify", 0, "Matching",
          "With --pairs: fit a model to the pairs by RANSAC on the GPU, homography, affine or epipolar (the fundamental\n"
          "matrix F of two views, x'^T F x = 0); prints the 3 x 3 model and the number of inliers after the pair lines",
          [&](const string& v) {
              if (v != "homography" && v != "affine" && v != "epipolar") {
                  cerr << "--verify: homography, affine or epipolar, not " << v << endl;
                  exit(-1);
              }
              verify_pairs = true;
              verify_epipolar = v == "epipolar";
              verify_opts.model = v == "affine" ? popsift::RansacOptions::Affine : popsift::RansacOptions::Homography;
          });
    o.ival("hypotheses", "Matching", "With --verify: sampled hypotheses, 1 .. 65536 (default 2048)",
           [&](int v) { verify_opts.hypotheses = v; });
    o.fval("max-err", "Matching", "With --verify: an inlier lies within this many pixels of its image, or of its epipolar line (default 2)",
           [&](float f) { verify_opts.maxErr = f; });
    o.ival("seed", "Matching", "With --verify: seed of the sampler (default 0)", [&](int v) { verify_opts.seed = (unsigned)v; });
    o.flag("guided", 0, "Matching",
           "With --verify: match again under the model just found -- each left descriptor among the right ones within\n"
           "--guided-err pixels of its image (homography, affine) or of its epipolar line -- with --ratio, --max-dist and\n"
           "--cross-check as given; prints those pairs after the model, then their count",
           [&] { guided_pairs = true; });
    o.fval("guided-err", "Matching", "With --guided: the distance in pixels (default: --max-err)", [&](float f) { guided_err = f; });
    o.flag("refit", 0, "Matching",
           "With --verify: refit the model to all its inliers by least squares, again on the new model's inliers while\n"
           "their number does not drop; prints the refitted model, its inliers, the rounds and why it stopped under the\n"
           "RANSAC lines; --guided then matches under the refitted model",
           [&] { refit_model = true; });
    o.ival("refit-rounds", "Matching", "With --refit: the most rounds, 1 .. 16 (default 4)", [&](int v) { refit_rounds = v; });
    o.val("gallery", 0, "Matching",
          "Match the left image against this image too; repeatable, replaces --right and implies --bytes --pairs.  All\n"
          "gallery images are matched in one pass on the GPU; prints per image, in the order given, a line\n"
          "'gallery <k> <file>: <n> pairs' and its pair lines, then the total.  Not with --verify or --guided (see\n"
          "--gallery-verify)",
          [&](const string& v) { gallery_files.push_back(v); });
    o.val("gallery-verify", 0, "Matching",
          "With --gallery: fit a model (homography, affine or epipolar) to every gallery image's pairs by RANSAC, all\n"
          "images in one call on the GPU, with --hypotheses, --max-err and --seed as for --verify; prints the model and\n"
          "the number of inliers under each image's pair lines and, after the total, the images ranked by inliers",
          [&](const string& v) {
              if (v != "homography" && v != "affine" && v != "epipolar") {
                  cerr << "--gallery-verify: homography, affine or epipolar, not " << v << endl;
                  exit(-1);
              }
              gallery_verify = v;
          });
    o.flag("all-pairs", 0, "Matching",
           "With --gallery and without --left: match the gallery images with each other, every a < b, in one pass on the\n"
           "GPU; prints one line per link, 'link <a> <b>: <n> pairs', with --gallery-verify followed by its inliers and\n"
           "its model, then the total",
           [&] { all_pairs = true; });
    o.ival("sequential", "Matching", "As --all-pairs, but every gallery image with its K successors only", [&](int k) {
        if (k < 1) o.error("the argument ('" + to_string(k) + "') for option '--sequential' is invalid");
        sequential_k = k;
    });
    o.val("feature-order", 0, "Extensions",
          "Order of the features of an image: arrival (default; differs from run to run) or raster (by octave, pixel row,\n"
          "pixel column, level: the same bytes on every run)",
          [&](const string& s) {
              if (s == "arrival") config.setFeatureOrder(popsift::Config::ArrivalOrder);
              else if (s == "raster") config.setFeatureOrder(popsift::Config::RasterOrder);
              else o.error("the argument ('" + s + "') for option '--feature-order' is invalid");
          });
    o.ival("keep-strongest", "Extensions",
           "Match only the N keypoints of every image with the largest DoG response (ties with the N-th included),\n"
           "thinned on the GPU before orientation; 0 (default): off.  Does not combine with --filter-max-extrema",
           [&](int n) {
               if (n < 0) o.error("the argument ('" + to_string(n) + "') for option '--keep-strongest' is invalid");
               config.setKeepStrongest(n);
           });
    o.parse(argc, argv);
    const bool links = all_pairs || sequential_k > 0;
    if (links && (all_pairs && sequential_k > 0)) {
        cerr << "--all-pairs or --sequential: give one or the other" << endl;
        exit(-1);
    }
    if (links && (gallery_files.empty() || !lFile.empty())) {
        cerr << "--all-pairs and --sequential match the --gallery images with each other: give them, and no --left" << endl;
        exit(-1);
    }
    if (!links && lFile.empty()) o.error("the option '--left' is required but missing");
    if (gallery_files.empty() && rFile.empty()) o.error("the option '--right' is required but missing");
    if (!gallery_files.empty()) {
        if (!rFile.empty()) {
            cerr << "--gallery replaces --right: give one or the other" << endl;
            exit(-1);
        }
        if (verify_pairs || guided_pairs) {
            cerr << "--gallery matches byte sets, which hold no positions: no --verify or --guided over a gallery" << endl;
            exit(-1);
        }
        match_bytes = print_pairs = true;
    }
    if (!gallery_verify.empty() && gallery_files.empty()) {
        cerr << "--gallery-verify verifies the images of a gallery: add --gallery" << endl;
        exit(-1);
    }
    if (verify_pairs && !print_pairs) {
        cerr << "--verify works on the pairs: add --pairs" << endl;
        exit(-1);
    }
    if (guided_pairs && !verify_pairs) {
        cerr << "--guided matches under the model --verify finds: add --verify" << endl;
        exit(-1);
    }
    if (refit_model && !verify_pairs) {
        cerr << "--refit refits the model --verify finds: add --verify" << endl;
        exit(-1);
    }
    if (refit_rounds < 1 || refit_rounds > 16) {
        cerr << "--refit-rounds: 1 .. 16, not " << refit_rounds << endl;
        exit(-1);
    }
    if (guided_pairs && match_bytes) {
        cerr << "--guided needs positions, which byte sets do not hold: drop --bytes" << endl;
        exit(-1);
    }
}

/* the reverse map (descriptor -> feature) of a float or a byte set */
static vector<int> reverse_map(popsift::FeaturesDev* f)
{
    vector<int> fem((size_t)f->getDescriptorCount());
    popsift_hip_devfeatures_download(f->getHandle(), 0, fem.data());
    return fem;
}
static vector<int> reverse_map(popsift::FeaturesDevBytes* f)
{
    vector<int> fem((size_t)f->getDescriptorCount());
    popsift_hip_bytefeatures_download(f->getHandle(), 0, fem.data());
    return fem;
}

/* --verify: the model fitted to the pairs' points and its inliers.  lf / rf: the float sets the positions come from */
static void print_verification(popsift::FeaturesDev* lf, popsift::FeaturesDev* rf, const vector<popsift::FeaturesDev::Pair>& pairs)
{
    popsift::Verifier        verifier(lf->getDevice());
    const vector<float>      pts = lf->pairPoints(rf, pairs);
    popsift::EpipolarOptions two_view;
    two_view.hypotheses = verify_opts.hypotheses;
    two_view.maxErr = verify_opts.maxErr;
    two_view.seed = verify_opts.seed;
    const popsift::RansacResult fit = verify_epipolar ? verifier.epipolar(pts, two_view) : verifier.ransac(pts, verify_opts);
    printf("Model (%s):\n", verify_epipolar ? "epipolar" : verify_opts.model == popsift::RansacOptions::Affine ? "affine" : "homography");
    for (int i = 0; i < 3; i++) printf("  %.9g %.9g %.9g\n", fit.H[3 * i], fit.H[3 * i + 1], fit.H[3 * i + 2]);
    printf("Number of inliers:     %d of %zu\n", fit.inliers, pairs.size());
    float guide[9];
    for (int i = 0; i < 9; i++) guide[i] = fit.H[i];
    if (refit_model) {
        popsift::RefitOptions ro(fit, verify_epipolar ? popsift::RefitOptions::Epipolar
                                      : verify_opts.model == popsift::RansacOptions::Affine ? popsift::RefitOptions::Affine
                                                                                            : popsift::RefitOptions::Homography,
                                 verify_opts.maxErr);
        ro.rounds = refit_rounds;
        const popsift::RefitResult again = verifier.refit(pts, ro);
        static const char* const why[] = {"all rounds ran", "converged", "no more inliers", "no fit", "no support"};
        printf("Refitted model:\n");
        for (int i = 0; i < 3; i++) printf("  %.9g %.9g %.9g\n", again.M[3 * i], again.M[3 * i + 1], again.M[3 * i + 2]);
        printf("Refit inliers:         %d -> %d of %zu, %d rounds (%s)\n", again.start, again.inliers, pairs.size(), again.rounds,
               why[again.stop]);
        for (int i = 0; i < 9; i++) guide[i] = again.M[i];
    }
    if (!guided_pairs) return;
    /* --guided: the search again, among the right descriptors that agree with the model */
    popsift::FeaturesDev::GuidedOptions g;
    g.model = verify_epipolar ? popsift::FeaturesDev::GuidedOptions::Epipolar : popsift::FeaturesDev::GuidedOptions::Homography;
    for (int i = 0; i < 9; i++) g.M[i] = guide[i];
    g.maxErr = guided_err > 0.0f ? guided_err : verify_opts.maxErr;
    g.ratio = pair_opts.ratio;
    g.maxDist2 = pair_opts.maxDist2;
    g.crossCheck = pair_opts.crossCheck;
    const vector<popsift::FeaturesDev::Pair> guided = lf->matchGuided(rf, g);
    const vector<int>                        l_fem = reverse_map(lf), r_fem = reverse_map(rf);
    for (const popsift::FeaturesDev::Pair& p : guided)
        printf("pair feat %4d [%4d] matches feat %4d [%4d] dist %.3f\n", l_fem[(size_t)p.l], p.l, r_fem[(size_t)p.r], p.r,
               sqrtf(p.distBest));
    printf("Number of guided pairs: %zu\n", guided.size());
}

/* one line per pair through the sets' reverse maps, then the count; lf / rf: the float sets behind l and r */
template <class Set>
static void print_matching_pairs(Set* l, Set* r, popsift::FeaturesDev* lf, popsift::FeaturesDev* rf)
{
    const vector<popsift::FeaturesDev::Pair> pairs = l->matchPairs(r, pair_opts);
    const vector<int>                        l_fem = reverse_map(l), r_fem = reverse_map(r);
    for (const popsift::FeaturesDev::Pair& p : pairs)
        printf("pair feat %4d [%4d] matches feat %4d [%4d] dist %.3f\n", l_fem[(size_t)p.l], p.l, r_fem[(size_t)p.r], p.r,
               sqrtf(p.distBest));
    printf("Number of pairs:       %zu\n", pairs.size());
    if (verify_pairs) print_verification(lf, rf, pairs);
}

/* --bytes without --pairs: FeaturesDev::match's line per left descriptor, from the byte matcher's rows */
static void print_byte_matches(popsift::FeaturesDevBytes* l, popsift::FeaturesDevBytes* r)
{
    if (l->getDescriptorCount() == 0 || r->getDescriptorCount() == 0) return;
    const vector<popsift::FeaturesDevBytes::Match> m = l->matchAndGet(r);
    const vector<int>                              l_fem = reverse_map(l), r_fem = reverse_map(r);
    for (size_t i = 0; i < m.size(); i++)
        printf("%s feat %4d [%4d] matches feat %4d [%4d] ( 2nd feat %4d [%4d] ) dist %.3f vs %.3f\n",
               m[i].accept ? "accept" : "reject", l_fem[i], (int)i, r_fem[(size_t)m[i].best], m[i].best,
               r_fem[(size_t)m[i].second], m[i].second, m[i].dist_best, m[i].dist_second);
}

static SiftJob* process_image(const string& inputFile, PopSift& sift);

/* --gallery: the left image against all gallery images in one pass */
static int match_gallery_files(const string& lFile, PopSift& sift)
{
    SiftJob*              lJob = process_image(lFile, sift);
    popsift::FeaturesDev* lFeatures = lJob->getDev();
    cout << "Number of features:    " << lFeatures->getFeatureCount() << endl;
    cout << "Number of descriptors: " << lFeatures->getDescriptorCount() << endl;
    popsift::FeaturesDevBytes* lBytes = lFeatures->toBytes();
    const vector<int>          l_fem = reverse_map(lBytes);
    popsift::Gallery           gallery(lFeatures->getDevice());
    vector<vector<int>>        r_fem;
    for (const string& f : gallery_files) {
        SiftJob*              job = process_image(f, sift);
        popsift::FeaturesDev* feat = job->getDev();
        cout << "Number of features:    " << feat->getFeatureCount() << endl;
        cout << "Number of descriptors: " << feat->getDescriptorCount() << endl;
        popsift::FeaturesDevBytes* bytes = feat->toBytes();
        r_fem.push_back(reverse_map(bytes));
        /* copied: the set can go.  For --gallery-verify the float set, whose positions the gallery keeps with the bytes */
        if (gallery_verify.empty()) gallery.add(bytes);
        else gallery.add(feat);
        delete bytes;
        delete feat;
        delete job;
    }
    const vector<vector<popsift::Gallery::Pair>> all = gallery.matchPairs(lBytes, pair_opts);
    size_t                                       total = 0;
    vector<popsift::RansacResult>                fits;
    if (!gallery_verify.empty()) {
        popsift::Verifier    verifier(lFeatures->getDevice());
        popsift::ManyOptions mo;
        mo.kind = gallery_verify == "epipolar" ? popsift::ManyOptions::Epipolar
                  : gallery_verify == "affine" ? popsift::ManyOptions::Affine
                                               : popsift::ManyOptions::Homography;
        mo.hypotheses = verify_opts.hypotheses;
        mo.maxErr = verify_opts.maxErr;
        mo.seed = verify_opts.seed;
        vector<int>         offsets;
        const vector<float> pts = gallery.pairPoints(lFeatures, all, offsets);
        fits = verifier.ransacMany(pts, offsets, mo);
    }
    for (size_t k = 0; k < all.size(); k++) {
        printf("gallery %zu %s: %zu pairs\n", k, gallery_files[k].c_str(), all[k].size());
        for (const popsift::Gallery::Pair& p : all[k])
            printf("pair feat %4d [%4d] matches feat %4d [%4d] dist %.3f\n", l_fem[(size_t)p.l], p.l, r_fem[k][(size_t)p.r], p.r,
                   sqrtf(p.distBest));
        total += all[k].size();
        if (fits.empty()) continue;
        printf("Model (%s):\n", gallery_verify.c_str());
        for (int i = 0; i < 3; i++) printf("  %.9g %.9g %.9g\n", fits[k].H[3 * i], fits[k].H[3 * i + 1], fits[k].H[3 * i + 2]);
        printf("Number of inliers:     %d of %zu\n", fits[k].inliers, all[k].size());
    }
    printf("Number of pairs:       %zu\n", total);
    if (!fits.empty()) {
        /* most inliers first, the order given on a tie */
        vector<size_t> rank(fits.size());
        for (size_t k = 0; k < rank.size(); k++) rank[k] = k;
        stable_sort(rank.begin(), rank.end(), [&](size_t a, size_t b) { return fits[a].inliers > fits[b].inliers; });
        printf("Ranking by inliers:   ");
        for (size_t k : rank) printf(" %zu (%d)", k, fits[k].inliers);
        printf("\n");
    }
    delete lBytes;
    delete lFeatures;
    delete lJob;
    return 0;
}

/* --all-pairs / --sequential: the gallery images with each other in one pass */
static int match_gallery_links(PopSift& sift)
{
    popsift::Gallery gallery(0);
    for (const string& f : gallery_files) {
        SiftJob*              job = process_image(f, sift);
        popsift::FeaturesDev* feat = job->getDev();
        cout << "Number of features:    " << feat->getFeatureCount() << endl;
        cout << "Number of descriptors: " << feat->getDescriptorCount() << endl;
        /* copied with its positions: the set can go */
        gallery.add(feat);
        delete feat;
        delete job;
    }
    const int                                    n = (int)gallery_files.size();
    const vector<popsift::Gallery::Link>         links = all_pairs ? popsift::Gallery::allLinks(n)
                                                                   : popsift::Gallery::sequentialLinks(n, sequential_k);
    const vector<vector<popsift::Gallery::Pair>> all = gallery.matchPairs(links, pair_opts);
    vector<popsift::RansacResult>                fits;
    if (!gallery_verify.empty()) {
        popsift::Verifier    verifier(0);
        popsift::ManyOptions mo;
        mo.kind = gallery_verify == "epipolar" ? popsift::ManyOptions::Epipolar
                  : gallery_verify == "affine" ? popsift::ManyOptions::Affine
                                               : popsift::ManyOptions::Homography;
        mo.hypotheses = verify_opts.hypotheses;
        mo.maxErr = verify_opts.maxErr;
        mo.seed = verify_opts.seed;
        vector<int>         offsets;
        const vector<float> pts = gallery.pairPoints(links, all, offsets);
        fits = verifier.ransacMany(pts, offsets, mo);
    }
    size_t total = 0;
    for (size_t e = 0; e < links.size(); e++) {
        printf("link %d %d: %zu pairs", links[e].a, links[e].b, all[e].size());
        if (!fits.empty()) {
            printf(", %d inliers, %s", fits[e].inliers, gallery_verify.c_str());
            for (int i = 0; i < 9; i++) printf(" %.9g", fits[e].H[i]);
        }
        printf("\n");
        total += all[e].size();
    }
    printf("Number of links:       %zu\n", links.size());
    printf("Number of pairs:       %zu\n", total);
    return 0;
}

static SiftJob* process_image(const string& inputFile, PopSift& sift)
{
    int            w, h;
    unsigned char* image_data = readPGMfile(inputFile, w, h);
    if (image_data == 0) exit(-1);
    SiftJob* job = sift.enqueue(w, h, image_data);
    delete[] image_data;
    return job;
}

int main(int argc, char** argv)
{
    popsift::Config config;
    string          lFile = "";
    string          rFile = "";

    parseargs(argc, argv, config, lFile, rFile);
    const bool     links = all_pairs || sequential_k > 0;
    vector<string> inputs = {lFile};
    if (links) {
        std::cout << gallery_files.size() << " gallery images <-> each other" << std::endl;
        inputs = gallery_files;
    } else if (gallery_files.empty()) {
        std::cout << lFile << " <-> " << rFile << std::endl;
        inputs.push_back(rFile);
    } else {
        std::cout << lFile << " <-> " << gallery_files.size() << " gallery images" << std::endl;
        inputs.insert(inputs.end(), gallery_files.begin(), gallery_files.end());
    }

    for (const string& f : inputs) {
        if (filesystem::exists(f) && !filesystem::is_regular_file(f)) {
            cout << "Input file " << f << " is not a regular file, nothing to do" << endl;
            exit(-1);
        }
    }

    popsift::cuda::device_prop_t deviceInfo;
    deviceInfo.set(0, print_dev_info);
    if (print_dev_info) deviceInfo.print();

    PopSift sift(config, popsift::Config::MatchingMode);

    if (!gallery_files.empty()) {
        const int rc = links ? match_gallery_links(sift) : match_gallery_files(lFile, sift);
        sift.uninit();
        return rc;
    }

    SiftJob* lJob = process_image(lFile, sift);
    SiftJob* rJob = process_image(rFile, sift);

    popsift::FeaturesDev* lFeatures = lJob->getDev();
    cout << "Number of features:    " << lFeatures->getFeatureCount() << endl;
    cout << "Number of descriptors: " << lFeatures->getDescriptorCount() << endl;

    popsift::FeaturesDev* rFeatures = rJob->getDev();
    cout << "Number of features:    " << rFeatures->getFeatureCount() << endl;
    cout << "Number of descriptors: " << rFeatures->getDescriptorCount() << endl;

    if (match_bytes) {
        popsift::FeaturesDevBytes* lBytes = lFeatures->toBytes();
        popsift::FeaturesDevBytes* rBytes = rFeatures->toBytes();
        if (print_pairs) print_matching_pairs(lBytes, rBytes, lFeatures, rFeatures);
        else print_byte_matches(lBytes, rBytes);
        delete lBytes;
        delete rBytes;
    } else if (print_pairs) {
        print_matching_pairs(lFeatures, rFeatures, lFeatures, rFeatures);
    } else {
        lFeatures->match(rFeatures);
    }

    delete lFeatures;
    delete rFeatures;
    delete lJob;
    delete rJob;

    sift.uninit();
    return 0;
}
