/*
 * sets.hip -- the device-resident feature sets of the C ABI (include/popsift_hip.h): popsift_hip_devfeatures (float
 * descriptors, FeaturesDev of features.h:98-118) and popsift_hip_bytefeatures (byte descriptors): every entry point that
 * makes, reads or frees a set without an extraction context.  The two clone calls that fill a set from a context's slot are
 * ctx.hip; the calls that match sets are match_sets.hip, match_guided.hip and ransac.hip.  The set types, and what each
 * owns, are devfeatures.h.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "devfeatures.h"
#include "kernels.h"

namespace popsift_hip {

int check_device(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return POPSIFT_HIP_ERR_NO_DEVICE;
    return device < 0 || device >= n ? POPSIFT_HIP_ERR_INVALID : POPSIFT_HIP_OK;
}

int devfeatures_new(int device, int n_feat, int n_desc, popsift_hip_devfeatures** out)
{
    if (hipSetDevice(device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    popsift_hip_devfeatures* f = new (std::nothrow) popsift_hip_devfeatures();
    if (!f) return POPSIFT_HIP_ERR_OOM;
    f->device = device;
    f->n_feat = n_feat;
    f->n_desc = n_desc;
    const size_t nf = (size_t)std::max(n_feat, 1), nd = (size_t)std::max(n_desc, 1);
    if (hipMalloc((void**)&f->d_feat, sizeof(DevFeature) * nf) != hipSuccess ||
        hipMalloc((void**)&f->d_desc, sizeof(float) * 128 * nd) != hipSuccess ||
        hipMalloc((void**)&f->d_rev, sizeof(int) * nd) != hipSuccess) {
        delete f;
        return POPSIFT_HIP_ERR_OOM;
    }
    *out = f;
    return POPSIFT_HIP_OK;
}

int bytefeatures_new(int device, int n, popsift_hip_bytefeatures** out)
{
    if (hipSetDevice(device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    popsift_hip_bytefeatures* f = new (std::nothrow) popsift_hip_bytefeatures();
    if (!f) return POPSIFT_HIP_ERR_OOM;
    f->device = device;
    f->n_desc = n;
    const size_t nd = (size_t)std::max(n, 1);
    if (hipMalloc((void**)&f->d_desc, 128 * nd) != hipSuccess || hipMalloc((void**)&f->d_rev, sizeof(int) * nd) != hipSuccess) {
        delete f;
        return POPSIFT_HIP_ERR_OOM;
    }
    *out = f;
    return POPSIFT_HIP_OK;
}

}  // namespace popsift_hip

using namespace popsift_hip;

namespace {

/* A float set's descriptors as bytes into d_u8 (128 per descriptor, on the set's GPU, which is current).  The null stream:
 * the pass is ordered after whatever wrote the set, and a blocking copy or a wait for the null stream after the pass. */
void set_bytes(Status& ok, const popsift_hip_devfeatures* f, uint8_t* d_u8)
{
    if (ok.good() && f->n_desc > 0) ok(launch_desc_bytes(f->d_desc, f->n_desc, d_u8, nullptr));
}

}  // namespace

extern "C" {

int popsift_hip_devfeatures_free(popsift_hip_devfeatures* f)
{
    if (!f) return POPSIFT_HIP_OK;
    (void)hipSetDevice(f->device);
    delete f;
    return POPSIFT_HIP_OK;
}

int popsift_hip_devfeatures_info(const popsift_hip_devfeatures* f, int* device, int* n_features, int* n_descriptors)
{
    if (!f) return POPSIFT_HIP_ERR_INVALID;
    if (device) *device = f->device;
    if (n_features) *n_features = f->n_feat;
    if (n_descriptors) *n_descriptors = f->n_desc;
    return POPSIFT_HIP_OK;
}

int popsift_hip_devfeatures_ptrs(const popsift_hip_devfeatures* f, void** d_features, void** d_descriptors,
                                 void** d_reverse_map)
{
    if (!f) return POPSIFT_HIP_ERR_INVALID;
    if (d_features) *d_features = f->d_feat;
    if (d_descriptors) *d_descriptors = f->d_desc;
    if (d_reverse_map) *d_reverse_map = f->d_rev;
    return POPSIFT_HIP_OK;
}

int popsift_hip_devfeatures_alloc(int device, int n_feat, int n_desc, popsift_hip_devfeatures** out)
{
    if (!out || n_feat < 0 || n_desc < 0) return POPSIFT_HIP_ERR_INVALID;
    *out = nullptr;
    popsift_hip_devfeatures* f = nullptr;
    if (int rc = check_device(device)) return rc;
    if (int rc = devfeatures_new(device, n_feat, n_desc, &f)) return rc;
    const size_t nf = (size_t)std::max(n_feat, 1), nd = (size_t)std::max(n_desc, 1);
    Status       ok;
    ok(hipMemset(f->d_feat, 0, sizeof(DevFeature) * nf)) && ok(hipMemset(f->d_desc, 0, sizeof(float) * 128 * nd)) &&
        ok(hipMemset(f->d_rev, 0, sizeof(int) * nd));
    return hand_over(ok.rc, f, out);
}

int popsift_hip_devfeatures_from_host(int device, const float* desc, int n, popsift_hip_devfeatures** out)
{
    if (!out || n < 0 || (n > 0 && !desc)) return POPSIFT_HIP_ERR_INVALID;
    *out = nullptr;
    popsift_hip_devfeatures* f = nullptr;
    if (int rc = check_device(device)) return rc;
    if (int rc = devfeatures_new(device, 0, n, &f)) return rc;
    Status ok;
    if (n > 0)
        ok(hipMemcpy(f->d_desc, desc, sizeof(float) * 128 * (size_t)n, hipMemcpyHostToDevice)) &&
            ok(hipMemset(f->d_rev, 0xff, sizeof(int) * (size_t)n)); /* -1: no feature behind it */
    return hand_over(ok.rc, f, out);
}

int popsift_hip_devfeatures_from_host_points(int device, const float* desc, const float* xy, int n, popsift_hip_devfeatures** out)
{
    if (!out || n < 0 || (n > 0 && (!desc || !xy))) return POPSIFT_HIP_ERR_INVALID;
    *out = nullptr;
    popsift_hip_devfeatures* f = nullptr;
    if (int rc = check_device(device)) return rc;
    if (int rc = devfeatures_new(device, n, n, &f)) return rc;
    Status ok;
    if (n > 0) {
        /* the records are built here: one feature per descriptor, its desc[0] pointing into the device array */
        std::vector<DevFeature> feat((size_t)n);
        std::vector<int>        rev((size_t)n);
        for (int i = 0; i < n; i++) {
            DevFeature& o = feat[(size_t)i];
            memset(&o, 0, sizeof o);
            o.xpos = xy[2 * (size_t)i];
            o.ypos = xy[2 * (size_t)i + 1];
            o.num_ori = 1;
            o.desc[0] = f->d_desc + (size_t)i * 128;
            rev[(size_t)i] = i;
        }
        ok(hipMemcpy(f->d_desc, desc, sizeof(float) * 128 * (size_t)n, hipMemcpyHostToDevice)) &&
            ok(hipMemcpy(f->d_feat, feat.data(), sizeof(DevFeature) * (size_t)n, hipMemcpyHostToDevice)) &&
            ok(hipMemcpy(f->d_rev, rev.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    }
    return hand_over(ok.rc, f, out);
}

int popsift_hip_devfeatures_download(const popsift_hip_devfeatures* f, float* desc, int32_t* rev)
{
    if (!f) return POPSIFT_HIP_ERR_INVALID;
    if (hipSetDevice(f->device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    Status ok;
    if (f->n_desc > 0 && desc) ok(hipMemcpy(desc, f->d_desc, sizeof(float) * 128 * (size_t)f->n_desc, hipMemcpyDeviceToHost));
    if (f->n_desc > 0 && rev && ok.good()) ok(hipMemcpy(rev, f->d_rev, sizeof(int) * (size_t)f->n_desc, hipMemcpyDeviceToHost));
    return ok.rc;
}

int popsift_hip_devfeatures_download_u8(const popsift_hip_devfeatures* f, uint8_t* desc)
{
    if (!f || (f->n_desc > 0 && !desc)) return POPSIFT_HIP_ERR_INVALID;
    if (f->n_desc <= 0) return POPSIFT_HIP_OK;
    if (hipSetDevice(f->device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    const size_t bytes = (size_t)f->n_desc * 128;
    uint8_t*     d_u8 = nullptr;
    if (hipMalloc((void**)&d_u8, bytes) != hipSuccess) return POPSIFT_HIP_ERR_OOM;
    Status ok;
    set_bytes(ok, f, d_u8);
    if (ok.good()) ok(hipMemcpy(desc, d_u8, bytes, hipMemcpyDeviceToHost));
    (void)hipFree(d_u8);
    return ok.rc;
}

/* ---- byte sets */

int popsift_hip_bytefeatures_free(popsift_hip_bytefeatures* f)
{
    if (!f) return POPSIFT_HIP_OK;
    (void)hipSetDevice(f->device);
    delete f;
    return POPSIFT_HIP_OK;
}

int popsift_hip_bytefeatures_from_host(int device, const uint8_t* desc, int n, popsift_hip_bytefeatures** out)
{
    if (!out || n < 0 || (n > 0 && !desc)) return POPSIFT_HIP_ERR_INVALID;
    *out = nullptr;
    popsift_hip_bytefeatures* f = nullptr;
    if (int rc = check_device(device)) return rc;
    if (int rc = bytefeatures_new(device, n, &f)) return rc;
    Status ok;
    if (n > 0)
        ok(hipMemcpy(f->d_desc, desc, (size_t)128 * (size_t)n, hipMemcpyHostToDevice)) &&
            ok(hipMemset(f->d_rev, 0xff, sizeof(int) * (size_t)n)) && /* -1: no feature behind it */
            ok(hipDeviceSynchronize());
    return hand_over(ok.rc, f, out);
}

int popsift_hip_bytefeatures_from_set(const popsift_hip_devfeatures* src, popsift_hip_bytefeatures** out)
{
    if (!src || !out) return POPSIFT_HIP_ERR_INVALID;
    *out = nullptr;
    popsift_hip_bytefeatures* f = nullptr;
    if (int rc = bytefeatures_new(src->device, src->n_desc, &f)) return rc;
    /* the set's own match stream does not wait for the null stream, so the call returns with the bytes in place */
    Status ok;
    set_bytes(ok, src, f->d_desc);
    if (ok.good() && src->n_desc > 0)
        ok(hipMemcpyAsync(f->d_rev, src->d_rev, sizeof(int) * (size_t)src->n_desc, hipMemcpyDeviceToDevice, nullptr)) &&
            ok(hipStreamSynchronize(nullptr));
    return hand_over(ok.rc, f, out);
}

int popsift_hip_bytefeatures_info(const popsift_hip_bytefeatures* f, int* device, int* n_descriptors)
{
    if (!f) return POPSIFT_HIP_ERR_INVALID;
    if (device) *device = f->device;
    if (n_descriptors) *n_descriptors = f->n_desc;
    return POPSIFT_HIP_OK;
}

int popsift_hip_bytefeatures_download(const popsift_hip_bytefeatures* f, uint8_t* desc, int32_t* rev)
{
    if (!f) return POPSIFT_HIP_ERR_INVALID;
    if (f->n_desc <= 0) return POPSIFT_HIP_OK;
    if (hipSetDevice(f->device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    Status ok;
    if (desc) ok(hipMemcpy(desc, f->d_desc, (size_t)128 * (size_t)f->n_desc, hipMemcpyDeviceToHost));
    if (rev && ok.good()) ok(hipMemcpy(rev, f->d_rev, sizeof(int) * (size_t)f->n_desc, hipMemcpyDeviceToHost));
    return ok.rc;
}

} /* extern "C" */
