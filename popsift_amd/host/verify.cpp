/* popsift::Verifier on top of popsift_hip_ransac, popsift_hip_epipolar and popsift_hip_refit (include/popsift/verify.h) */
#include "popsift/verify.h"

#include <cstdlib>
#include <cstring>
#include <iostream>

#include "popsift_hip.h"

namespace popsift {

namespace {
[[noreturn]] void verify_fatal(const char* what, int rc)
{
    std::cerr << __FILE__ << std::endl << "E    " << what << ": " << popsift_hip_strerror(rc) << std::endl;
    exit(-1);
}

void take(RansacResult& out, const popsift_hip_ransac_result& res)
{
    memcpy(out.H, res.H, sizeof out.H);
    out.inliers = res.n_inliers;
    out.hypothesis = res.hypothesis;
    out.valid = res.n_valid;
}
}  // namespace

Verifier::Verifier(int device) : _v(0)
{
    const int rc = popsift_hip_verifier_create(device, &_v);
    if (rc != POPSIFT_HIP_OK) verify_fatal("cannot create the verifier", rc);
}

Verifier::~Verifier() { popsift_hip_verifier_free(_v); }

RansacResult Verifier::ransac(const std::vector<float>& pts, const RansacOptions& opts)
{
    RansacResult              out;
    const int                 n = (int)(pts.size() / 4);
    popsift_hip_ransac_opts   o;
    popsift_hip_ransac_result res;
    popsift_hip_default_ransac_opts(&o);
    o.model = (int)opts.model;
    o.hypotheses = opts.hypotheses;
    o.max_err = opts.maxErr;
    o.seed = opts.seed;
    out.mask.resize((size_t)n);
    const int rc = popsift_hip_ransac(_v, n ? pts.data() : 0, n, &o, &res, n ? out.mask.data() : 0);
    if (rc != POPSIFT_HIP_OK) verify_fatal("verification failed", rc);
    take(out, res);
    return out;
}

RansacResult Verifier::epipolar(const std::vector<float>& pts, const EpipolarOptions& opts)
{
    RansacResult              out;
    const int                 n = (int)(pts.size() / 4);
    popsift_hip_epipolar_opts o;
    popsift_hip_ransac_result res;
    popsift_hip_default_epipolar_opts(&o);
    o.hypotheses = opts.hypotheses;
    o.max_err = opts.maxErr;
    o.seed = opts.seed;
    out.mask.resize((size_t)n);
    const int rc = popsift_hip_epipolar(_v, n ? pts.data() : 0, n, &o, &res, n ? out.mask.data() : 0);
    if (rc != POPSIFT_HIP_OK) verify_fatal("epipolar verification failed", rc);
    take(out, res);
    return out;
}

std::vector<RansacResult> Verifier::ransacMany(const std::vector<float>& pts, const std::vector<int>& offsets,
                                               const ManyOptions& opts)
{
    static_assert(sizeof(int) == sizeof(int32_t), "offsets are int32_t");
    const int                              n_lists = offsets.empty() ? 0 : (int)offsets.size() - 1;
    std::vector<RansacResult>              out((size_t)n_lists);
    std::vector<popsift_hip_ransac_result> res((size_t)n_lists);
    std::vector<unsigned char>             mask(pts.size() / 4);
    popsift_hip_ransac_many_opts           o;
    popsift_hip_default_ransac_many_opts(&o);
    o.kind = (int)opts.kind;
    o.hypotheses = opts.hypotheses;
    o.max_err = opts.maxErr;
    o.seed = opts.seed;
    if (n_lists == 0) return out;
    if (offsets.back() < 0 || (size_t)offsets.back() != mask.size()) verify_fatal("the offsets do not end at the last pair", POPSIFT_HIP_ERR_INVALID);
    const int rc = popsift_hip_ransac_many(_v, pts.empty() ? 0 : pts.data(), offsets.data(), n_lists, &o, res.data(),
                                           mask.empty() ? 0 : mask.data());
    if (rc != POPSIFT_HIP_OK) verify_fatal("verification of the lists failed", rc);
    for (int m = 0; m < n_lists; m++) {
        take(out[(size_t)m], res[(size_t)m]);
        out[(size_t)m].mask.assign(mask.begin() + offsets[(size_t)m], mask.begin() + offsets[(size_t)m + 1]);
    }
    return out;
}

RefitResult Verifier::refit(const std::vector<float>& pts, const RefitOptions& opts)
{
    RefitResult              out;
    const int                n = (int)(pts.size() / 4);
    popsift_hip_refit_opts   o;
    popsift_hip_refit_result res;
    popsift_hip_default_refit_opts(&o);
    o.model = (int)opts.kind;
    o.rounds = opts.rounds;
    o.max_err = opts.maxErr;
    memcpy(o.M, opts.M, sizeof o.M);
    out.mask.resize((size_t)n);
    const int rc = popsift_hip_refit(_v, n ? pts.data() : 0, n, &o, &res, n ? out.mask.data() : 0);
    if (rc != POPSIFT_HIP_OK) verify_fatal("refit failed", rc);
    memcpy(out.M, res.M, sizeof out.M);
    out.inliers = res.n_inliers;
    out.start = res.n_start;
    out.rounds = res.rounds;
    out.stop = (RefitResult::Stop)res.stop;
    return out;
}

}  // namespace popsift
