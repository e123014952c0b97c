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

/* ---- galleries of byte sets */

namespace {

constexpr int64_t GALLERY_MAX_DESC = (int64_t)1 << 30;
constexpr int     GALLERY_MAX_MEMBERS = 1 << 20;

/* Room for n more descriptors and one more member.  New buffers are filled device to device and swapped in only when
 * every allocation has succeeded: a failure leaves the gallery as it was. */
int gallery_reserve(popsift_hip_gallery* g, int n, bool with_xy, hipStream_t s)
{
    if ((size_t)g->n_members + 1 > g->tab_cap) {
        const size_t   cap = std::max<size_t>(2 * g->tab_cap, 64);
        int64_t* const first = (int64_t*)malloc(sizeof(int64_t) * cap);
        int* const     count = (int*)malloc(sizeof(int) * cap);
        uint8_t* const has_xy = (uint8_t*)malloc(cap);
        if (!first || !count || !has_xy) {
            free(first);
            free(count);
            free(has_xy);
            return POPSIFT_HIP_ERR_OOM;
        }
        if (g->n_members > 0) {
            memcpy(first, g->first, sizeof(int64_t) * (size_t)g->n_members);
            memcpy(count, g->count, sizeof(int) * (size_t)g->n_members);
            memcpy(has_xy, g->has_xy, (size_t)g->n_members);
        }
        free(g->first);
        free(g->count);
        free(g->has_xy);
        g->first = first;
        g->count = count;
        g->has_xy = has_xy;
        g->tab_cap = cap;
    }
    /* the positions exist from the first member that brings some, and are as long as the descriptors from then on */
    const bool   xy = with_xy || g->d_xy;
    const size_t need = (size_t)g->n_desc + (size_t)n;
    if (need <= g->cap && (!xy || g->d_xy)) return POPSIFT_HIP_OK;
    const bool   more = need > g->cap;
    const size_t cap = more ? std::max(need, std::max<size_t>(2 * g->cap, 1024)) : g->cap;
    uint8_t*     desc = nullptr;
    int*         norm = nullptr;
    float*       pos = nullptr;
    Status       ok;
    if (more && ok(hipMalloc((void**)&desc, 128 * cap)) && ok(hipMalloc((void**)&norm, sizeof(int) * cap)) && g->n_desc > 0)
        ok(hipMemcpyAsync(desc, g->d_desc, 128 * (size_t)g->n_desc, hipMemcpyDeviceToDevice, s)) &&
            ok(hipMemcpyAsync(norm, g->d_norm, sizeof(int) * (size_t)g->n_desc, hipMemcpyDeviceToDevice, s));
    if (xy && ok.good() && ok(hipMalloc((void**)&pos, sizeof(float) * 2 * std::max<size_t>(cap, 1))) && g->d_xy && g->n_desc > 0)
        ok(hipMemcpyAsync(pos, g->d_xy, sizeof(float) * 2 * (size_t)g->n_desc, hipMemcpyDeviceToDevice, s));
    if (ok.good()) ok(hipStreamSynchronize(s));
    if (!ok.good()) {
        free_bufs({desc, norm, pos});
        return ok.rc;
    }
    if (more) {
        free_bufs({g->d_desc, g->d_norm});
        g->d_desc = desc;
        g->d_norm = norm;
        g->cap = cap;
    }
    if (xy) {
        free_bufs({g->d_xy});
        g->d_xy = pos;
    }
    return POPSIFT_HIP_OK;
}

/* a new member of n descriptors from `src` (device memory of src_device, or host memory with src_device < 0); xy: its
 * n x 2 positions in device memory of src_device, or NULL for a member without positions */
int gallery_append(popsift_hip_gallery* g, const uint8_t* src, int src_device, int n, const float* xy, int* member)
{
    if (g->n_desc + n > GALLERY_MAX_DESC || g->n_members + 1 > GALLERY_MAX_MEMBERS) return POPSIFT_HIP_ERR_INVALID;
    if (hipSetDevice(g->device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    hipStream_t const s = (hipStream_t)g->stream;
    if (int rc = gallery_reserve(g, n, xy != nullptr, s)) return rc;
    if (n > 0) {
        uint8_t* const dst = g->d_desc + 128 * (size_t)g->n_desc;
        const size_t   bytes = 128 * (size_t)n;
        Status         ok;
        if (src_device < 0) ok(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
        else if (src_device == g->device) ok(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
        else ok(hipMemcpyPeer(dst, g->device, src, src_device, bytes));
        if (ok.good() && xy) {
            float* const pos = g->d_xy + 2 * (size_t)g->n_desc;
            if (src_device == g->device) ok(hipMemcpyAsync(pos, xy, sizeof(float) * 2 * (size_t)n, hipMemcpyDeviceToDevice, s));
            else ok(hipMemcpyPeer(pos, g->device, xy, src_device, sizeof(float) * 2 * (size_t)n));
        }
        if (ok.good()) ok(launch_norms_u8(dst, n, g->d_norm + g->n_desc, s));
        if (ok.good()) ok(hipStreamSynchronize(s));
        if (!ok.good()) return ok.rc;
    }
    g->first[g->n_members] = g->n_desc;
    g->count[g->n_members] = n;
    g->has_xy[g->n_members] = xy != nullptr;
    if (member) *member = g->n_members;
    g->n_members += 1;
    g->n_desc += n;
    return POPSIFT_HIP_OK;
}

/* (xpos, ypos) of the feature behind each of a set's n descriptors; *bad = 1 when a map entry names no feature */
__global__ __launch_bounds__(256) void k_member_xy(const DevFeature* __restrict__ feat, const int* __restrict__ rev, int n_feat,
                                                   int n, float2* __restrict__ xy, int* __restrict__ bad)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int f = rev[i];
    if (f < 0 || f >= n_feat) {
        *bad = 1;
        xy[i] = make_float2(0.0f, 0.0f);
        return;
    }
    xy[i] = make_float2(feat[f].xpos, feat[f].ypos);
}

/* item = (descriptor of l, row of the gallery): the point pair (x, y of the feature behind l's descriptor, the gallery's
 * position of the row); *bad = 1 when l's map names no feature */
__global__ __launch_bounds__(256) void k_gallery_points(const int2* __restrict__ items, int n, const DevFeature* __restrict__ lf,
                                                        const int* __restrict__ lrev, int l_nfeat, const float2* __restrict__ xy,
                                                        float4* __restrict__ out, int* __restrict__ bad)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int2 it = items[i];
    const int  f = lrev[it.x];
    if (f < 0 || f >= l_nfeat) {
        *bad = 1;
        out[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float2 r = xy[it.y];
    out[i] = make_float4(lf[f].xpos, lf[f].ypos, r.x, r.y);
}

}  // namespace

extern "C" {

int popsift_hip_gallery_add_set(popsift_hip_gallery* g, const popsift_hip_devfeatures* f, int* member)
{
    if (!g || !f) return POPSIFT_HIP_ERR_INVALID;
    /* on the set's GPU: its bytes (those of popsift_hip_bytefeatures_from_set) and, behind a flag, its positions */
    popsift_hip_bytefeatures* b = nullptr;
    if (int rc = popsift_hip_bytefeatures_from_set(f, &b)) return rc;
    const int n = f->n_desc;
    char*     d_xy = nullptr;
    int       bad = 0;
    Status    ok;
    if (ok(hipMalloc((void**)&d_xy, 16 + sizeof(float2) * (size_t)std::max(n, 1))) && ok(hipMemsetAsync(d_xy, 0, 16, nullptr)) &&
        n > 0) {
        hipLaunchKernelGGL(k_member_xy, dim3((n + 255) / 256), dim3(256), 0, nullptr, f->d_feat, f->d_rev, f->n_feat, n,
                           (float2*)(d_xy + 16), (int*)d_xy);
        ok(hipGetLastError());
    }
    if (ok.good()) ok(hipMemcpy(&bad, d_xy, sizeof bad, hipMemcpyDeviceToHost));
    if (ok.good() && bad) ok.rc = POPSIFT_HIP_ERR_INVALID;
    if (ok.good()) ok.rc = gallery_append(g, b->d_desc, b->device, n, (const float*)(d_xy + 16), member);
    (void)hipSetDevice(f->device);
    if (d_xy) (void)hipFree(d_xy);
    (void)popsift_hip_bytefeatures_free(b);
    return ok.rc;
}

int popsift_hip_gallery_pair_points(const popsift_hip_devfeatures* l, popsift_hip_gallery* g, const popsift_hip_pair* pairs,
                                    const int32_t* offsets, float* pts)
{
    if (!l || !g || !offsets || offsets[0] != 0) return POPSIFT_HIP_ERR_INVALID;
    for (int m = 0; m < g->n_members; m++)
        if (offsets[m + 1] < offsets[m]) return POPSIFT_HIP_ERR_INVALID;
    const int n = offsets[g->n_members];
    if (n > 0 && (!pairs || !pts)) return POPSIFT_HIP_ERR_INVALID;
    for (int m = 0; m < g->n_members; m++) {
        if (offsets[m + 1] > offsets[m] && !g->has_xy[m]) return POPSIFT_HIP_ERR_INVALID;
        for (int i = offsets[m]; i < offsets[m + 1]; i++)
            if (pairs[i].l < 0 || pairs[i].l >= l->n_desc || pairs[i].r < 0 || pairs[i].r >= g->count[m]) return POPSIFT_HIP_ERR_INVALID;
    }
    if (n == 0) return POPSIFT_HIP_OK;
    if (hipSetDevice(g->device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    Status            ok;
    hipStream_t const s = (hipStream_t)g->stream;
    /* device block and its pinned twin: a flag, the items, the points */
    const size_t b_items = round16(sizeof(int2) * (size_t)n), b_pts = sizeof(float) * 4 * (size_t)n;
    grow_twin(ok, g->xy_dev, g->xy_host, g->xy_cap, 16 + b_items + b_pts);
    /* a query set on another GPU: its feature records and its map come over for the call */
    const DevFeature* lf = l->d_feat;
    const int*        lrev = l->d_rev;
    PeerCopy          peer;
    if (peer.fetch(ok, g->device, l->device,
                   {{l->d_feat, sizeof(DevFeature) * (size_t)std::max(l->n_feat, 1)}, {l->d_rev, sizeof(int) * (size_t)l->n_desc}})) {
        lf = (const DevFeature*)peer.at[0];
        lrev = (const int*)peer.at[1];
    }
    if (ok.good()) {
        char* const d = (char*)g->xy_dev;
        char* const h = (char*)g->xy_host;
        memset(h, 0, 16);
        int2* const items = (int2*)(h + 16);
        for (int m = 0; m < g->n_members; m++)
            for (int i = offsets[m]; i < offsets[m + 1]; i++) items[i] = make_int2(pairs[i].l, (int)(g->first[m] + pairs[i].r));
        if (ok(hipMemcpyAsync(d, h, 16 + b_items, hipMemcpyHostToDevice, s))) {
            hipLaunchKernelGGL(k_gallery_points, dim3((n + 255) / 256), dim3(256), 0, s, (const int2*)(d + 16), n, lf, lrev, l->n_feat,
                               (const float2*)g->d_xy, (float4*)(d + 16 + b_items), (int*)d);
            ok(hipGetLastError());
        }
        /* the flag and the points come down; the items in between stay */
        if (ok.good() && ok(hipMemcpyAsync(h, d, 16, hipMemcpyDeviceToHost, s)) &&
            ok(hipMemcpyAsync(h + 16 + b_items, d + 16 + b_items, b_pts, hipMemcpyDeviceToHost, s)) && ok(hipStreamSynchronize(s))) {
            if (*(const int*)h != 0) ok.rc = POPSIFT_HIP_ERR_INVALID;
            else memcpy(pts, h + 16 + b_items, b_pts);
        }
    }
    return ok.rc;
}

int popsift_hip_gallery_create(int device, popsift_hip_gallery** out)
{
    if (!out) return POPSIFT_HIP_ERR_INVALID;
    *out = nullptr;
    if (int rc = check_device(device)) return rc;
    if (hipSetDevice(device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    popsift_hip_gallery* g = new (std::nothrow) popsift_hip_gallery();
    if (!g) return POPSIFT_HIP_ERR_OOM;
    g->device = device;
    Status      ok;
    hipStream_t s = nullptr;
    hipEvent_t  e = nullptr;
    if (ok(hipStreamCreateWithFlags(&s, hipStreamNonBlocking))) g->stream = s;
    if (ok.good() && ok(hipEventCreateWithFlags(&e, hipEventDisableTiming))) g->w_event = e;
    return hand_over(ok.rc, g, out);
}

int popsift_hip_gallery_free(popsift_hip_gallery* g)
{
    if (!g) return POPSIFT_HIP_OK;
    (void)hipSetDevice(g->device);
    delete g;
    return POPSIFT_HIP_OK;
}

int popsift_hip_gallery_add(popsift_hip_gallery* g, const popsift_hip_bytefeatures* f, int* member)
{
    if (!g || !f) return POPSIFT_HIP_ERR_INVALID;
    return gallery_append(g, f->d_desc, f->device, f->n_desc, nullptr, member);
}

int popsift_hip_gallery_add_host(popsift_hip_gallery* g, const uint8_t* desc, int n_descriptors, int* member)
{
    if (!g || n_descriptors < 0 || (n_descriptors > 0 && !desc)) return POPSIFT_HIP_ERR_INVALID;
    return gallery_append(g, desc, -1, n_descriptors, nullptr, member);
}

int popsift_hip_gallery_info(const popsift_hip_gallery* g, int* device, int* n_members, int64_t* n_descriptors)
{
    if (!g) return POPSIFT_HIP_ERR_INVALID;
    if (device) *device = g->device;
    if (n_members) *n_members = g->n_members;
    if (n_descriptors) *n_descriptors = g->n_desc;
    return POPSIFT_HIP_OK;
}

int popsift_hip_gallery_member(const popsift_hip_gallery* g, int m, int64_t* first, int* count)
{
    if (!g || m < 0 || m >= g->n_members) return POPSIFT_HIP_ERR_INVALID;
    if (first) *first = g->first[m];
    if (count) *count = g->count[m];
    return POPSIFT_HIP_OK;
}

int popsift_hip_gallery_download(const popsift_hip_gallery* g, int m, uint8_t* desc)
{
    if (!g || m < 0 || m >= g->n_members || (g->count[m] > 0 && !desc)) return POPSIFT_HIP_ERR_INVALID;
    if (g->count[m] == 0) return POPSIFT_HIP_OK;
    if (hipSetDevice(g->device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    Status ok;
    ok(hipMemcpy(desc, g->d_desc + 128 * (size_t)g->first[m], 128 * (size_t)g->count[m], hipMemcpyDeviceToHost));
    return ok.rc;
}

int popsift_hip_gallery_debug_set_group_rows(popsift_hip_gallery* g, int rows)
{
    if (!g || rows < 0) return POPSIFT_HIP_ERR_INVALID;
    g->group_rows = rows;
    return POPSIFT_HIP_OK;
}

} /* extern "C" */
