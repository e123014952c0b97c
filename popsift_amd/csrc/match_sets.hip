/*
 * match_sets.hip -- the host driver of the descriptor matchers: popsift_hip_match_sets / _bytes (2-NN rows) and
 * popsift_hip_match_pairs / _bytes (pair lists) over two device-resident sets.  The kernels are match.hip, match_mfma.hip,
 * match_u8.hip and match_pairs.hip; the sets' scratch record and the helpers shared with the guided matcher and the
 * verifier are devfeatures.h.  Nothing here touches an extraction context.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "devfeatures.h"
#include "kernels.h"
#include "top2.h"

using namespace popsift_hip;

namespace {

std::atomic<int> g_match_path{POPSIFT_HIP_MATCH_AUTO};

/* large problems: matrix-core screening + exact re-rank (match_mfma.hip); small ones and POPSIFT_HIP_MATCH_EXACT: the
 * exact brute-force kernel alone (match.hip) */
bool match_screens(int path, int l_len, int r_len)
{
    return path == POPSIFT_HIP_MATCH_SCREEN || (path == POPSIFT_HIP_MATCH_AUTO && (double)l_len * (double)r_len >= 4.0e6);
}

/* |x|^2 of the set's own descriptors (and launch_norms' flag behind them), computed on first use */
void match_own_norms(Status& ok, popsift_hip_devfeatures* f, hipStream_t s)
{
    if (ok.good() && !f->d_norm && ok(hipMalloc((void**)&f->d_norm, sizeof(float) * ((size_t)f->n_desc + 1))))
        ok(launch_norms(f->d_desc, f->n_desc, f->d_norm, s));
}

void match_own_norms(Status& ok, popsift_hip_bytefeatures* f, hipStream_t s)
{
    if (ok.good() && !f->d_norm && ok(hipMalloc((void**)&f->d_norm, sizeof(int) * (size_t)f->n_desc)))
        ok(launch_norms_u8(f->d_desc, f->n_desc, f->d_norm, s));
}

/* One 2-NN sweep of l_len descriptors against r_len on stream s: d_out[l_len] on the device.  The candidate buffer is
 * `own`'s; with screening the norms of both sides are ready and redo = [count, rows the screening pass leaves to the
 * exact kernel ...] has room for l_len rows. */
void match_sweep(Status& ok, popsift_hip_devfeatures* own, bool screen, const float* ldesc, int l_len, const float* lnorm,
                 const float* rdesc, int r_len, const float* rnorm, popsift_hip_match* d_out, int* redo, hipStream_t s)
{
    const int n_split = splits(l_len, r_len, M_LT, M_RT, M_GROUPS);
    const int s_split = screen ? splits(l_len, r_len, S_LB, S_RB, S_GROUPS) : 1;
    /* rows the screening pass cannot decide are few: the first REDO_CAP of them are matched with the right set split
     * over many workgroups, a second launch (normally empty) covers the rest of the list */
    const int REDO_CAP = 2048;
    const int redo_split = std::min(256, std::max((r_len + 63) / 64, 1));
    size_t    need = partial_bytes(l_len, n_split, sizeof(Top2<float>));
    if (screen) need = std::max(need, partial_bytes(l_len, s_split, S_CAND_BYTES));
    if (screen) need = std::max(need, partial_bytes(REDO_CAP, redo_split, sizeof(Top2<float>)));
    if (!grow(ok, own->m_partial, own->m_partial_cap, need, 1)) return;
    if (screen) {
        ok(launch_match_screen(ldesc, l_len, rdesc, r_len, lnorm, rnorm, s_split, own->m_partial, d_out, redo + 1, redo, s)) &&
            ok(launch_match(ldesc, l_len, rdesc, r_len, redo_split, own->m_partial, d_out, redo + 1, redo, 0, REDO_CAP, s)) &&
            ok(launch_match(ldesc, l_len, rdesc, r_len, n_split, own->m_partial, d_out, redo + 1, redo, REDO_CAP, l_len, s));
    } else {
        ok(launch_match(ldesc, l_len, rdesc, r_len, n_split, own->m_partial, d_out, nullptr, nullptr, 0, 0, s));
    }
}

/* byte sets (match_u8.hip): one exact kernel, no path choice */
void match_sweep_u8(Status& ok, popsift_hip_bytefeatures* own, const uint8_t* ldesc, int l_len, const int* lnorm,
                    const uint8_t* rdesc, int r_len, const int* rnorm, popsift_hip_match* d_out, hipStream_t s)
{
    const int n_split = splits(l_len, r_len, U_LB, U_RB, U_GROUPS);
    if (!grow(ok, own->m_partial, own->m_partial_cap, partial_bytes(l_len, n_split, sizeof(Top2<int>)), 1)) return;
    ok(launch_match_u8(ldesc, l_len, lnorm, rdesc, r_len, rnorm, n_split, own->m_partial, d_out, s));
}

/* What both forward sweeps begin with (l->n_desc > 0, l's GPU current): l's stream, its row buffer, r's descriptors on l's
 * GPU (returned; a copy lives as long as `peer`) and rnorm_bytes for the norms of r.  The right set may be the left set of
 * another thread's match: its norms go to this buffer of this call, never into r. */
template <class Set, class Elem = typename std::remove_pointer<decltype(Set::d_desc)>::type>
const Elem* match_begin(Status& ok, Set* l, const Set* r, PeerCopy& peer, size_t rnorm_bytes)
{
    stream_of(ok, *l);
    if (ok.good() && !l->m_out) ok(hipMalloc(&l->m_out, sizeof(popsift_hip_match) * (size_t)l->n_desc));
    const Elem* rdesc = r->d_desc;
    if (r->n_desc > 0 && peer.fetch(ok, l->device, r->device, {{r->d_desc, sizeof(Elem) * 128 * (size_t)r->n_desc}}))
        rdesc = (const Elem*)peer.at[0];
    grow(ok, l->m_rnorm, l->m_rnorm_cap, rnorm_bytes, 1);
    return rdesc;
}

/* The sweep of l against r into l->m_out, enqueued on l's stream; returns r's descriptors on l's GPU.  Float sets: norms
 * and the redo list only when screening. */
const float* match_forward(Status& ok, popsift_hip_devfeatures* l, const popsift_hip_devfeatures* r, int path, PeerCopy& peer)
{
    const bool         screen = match_screens(path, l->n_desc, r->n_desc);
    const float* const rdesc = match_begin(ok, l, r, peer, screen ? sizeof(float) * ((size_t)r->n_desc + 1) : 0);
    hipStream_t const  s = (hipStream_t)l->m_stream;
    if (ok.good() && screen) {
        if (!l->m_redo) ok(hipMalloc((void**)&l->m_redo, sizeof(int) * ((size_t)l->n_desc + 1)));
        match_own_norms(ok, l, s);
        if (ok.good()) ok(launch_norms(rdesc, r->n_desc, (float*)l->m_rnorm, s));
    }
    if (ok.good())
        match_sweep(ok, l, screen, l->d_desc, l->n_desc, l->d_norm, rdesc, r->n_desc, (const float*)l->m_rnorm,
                    (popsift_hip_match*)l->m_out, l->m_redo, s);
    return rdesc;
}

/* byte sets: always norms */
const uint8_t* match_forward(Status& ok, popsift_hip_bytefeatures* l, const popsift_hip_bytefeatures* r, int /*path*/,
                             PeerCopy& peer)
{
    const uint8_t* const rdesc = match_begin(ok, l, r, peer, sizeof(int) * (size_t)r->n_desc);
    hipStream_t const    s = (hipStream_t)l->m_stream;
    match_own_norms(ok, l, s);
    if (ok.good()) ok(launch_norms_u8(rdesc, r->n_desc, (int*)l->m_rnorm, s));
    if (ok.good())
        match_sweep_u8(ok, l, l->d_desc, l->n_desc, l->d_norm, rdesc, r->n_desc, (const int*)l->m_rnorm,
                       (popsift_hip_match*)l->m_out, s);
    return rdesc;
}

/* The reverse sweep of the cross-check: the n_list right descriptors of `list` (ascending) against all of l, on l's
 * stream; returns their rows, in list order, in l's p_back. */
const popsift_hip_match* match_reverse(Status& ok, popsift_hip_devfeatures* l, const float* rdesc, const int* list, int n_list,
                                       int path)
{
    const int    l_len = l->n_desc;
    hipStream_t  s = (hipStream_t)l->m_stream;
    /* per member of J: 128 floats, a result row, a norm and a redo slot (+ the norms' flag and the redo count) */
    const size_t per = sizeof(float) * 128 + sizeof(popsift_hip_match) + sizeof(float) + sizeof(int);
    if (!grow(ok, l->p_back, l->p_back_cap, (size_t)n_list + 1, per)) return nullptr;
    float* const gdesc = (float*)l->p_back;
    auto* const  rows = (popsift_hip_match*)(gdesc + 128 * (size_t)n_list);
    float* const gnorm = (float*)(rows + n_list);
    int* const   redo = (int*)(gnorm + n_list + 1);
    const bool   screen = match_screens(path, n_list, l_len);
    ok(launch_gather_rows(rdesc, list, n_list, gdesc, s));
    if (screen) {
        match_own_norms(ok, l, s);
        if (ok.good()) ok(launch_norms(gdesc, n_list, gnorm, s));
    }
    if (ok.good()) match_sweep(ok, l, screen, gdesc, n_list, gnorm, l->d_desc, l_len, l->d_norm, rows, redo, s);
    return rows;
}

const popsift_hip_match* match_reverse(Status& ok, popsift_hip_bytefeatures* l, const uint8_t* rdesc, const int* list,
                                       int n_list, int /*path*/)
{
    hipStream_t  s = (hipStream_t)l->m_stream;
    /* per member of J: 128 bytes, a result row and a norm */
    const size_t per = 128 + sizeof(popsift_hip_match) + sizeof(int);
    if (!grow(ok, l->p_back, l->p_back_cap, (size_t)n_list, per)) return nullptr;
    uint8_t* const gdesc = (uint8_t*)l->p_back;
    auto* const    rows = (popsift_hip_match*)(gdesc + 128 * (size_t)n_list);
    int* const     gnorm = (int*)(rows + n_list);
    ok(launch_gather_rows(rdesc, list, n_list, gdesc, s)) && ok(launch_norms_u8(gdesc, n_list, gnorm, s));
    if (ok.good()) match_sweep_u8(ok, l, gdesc, n_list, gnorm, l->d_desc, l->n_desc, l->d_norm, rows, s);
    return rows;
}

/* popsift_hip_match_sets / popsift_hip_match_bytes */
template <class Set>
int match_rows(const Set* lc, const Set* r, popsift_hip_match* out, int path)
{
    if (!lc || !r || (lc->n_desc > 0 && !out)) return POPSIFT_HIP_ERR_INVALID;
    if (lc->n_desc == 0) return POPSIFT_HIP_OK;
    Set* l = const_cast<Set*>(lc);
    if (hipSetDevice(l->device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    Status       ok;
    PeerCopy     peer;
    const size_t out_bytes = sizeof(popsift_hip_match) * (size_t)l->n_desc;
    match_forward(ok, l, r, path, peer);
    if (ok.good() && !l->m_host) ok(hipHostMalloc(&l->m_host, out_bytes, hipHostMallocDefault));
    hipStream_t s = (hipStream_t)l->m_stream;
    if (ok.good() && ok(hipMemcpyAsync(l->m_host, l->m_out, out_bytes, hipMemcpyDeviceToHost, s)) && ok(hipStreamSynchronize(s)))
        memcpy(out, l->m_host, out_bytes);
    return ok.rc;
}

/* popsift_hip_match_pairs / popsift_hip_match_pairs_bytes */
template <class Set>
int match_pairs(const Set* lc, const Set* r, const popsift_hip_match_opts* opts, popsift_hip_pair* pairs, size_t cap,
                int* n_pairs, int path)
{
    if (!lc || !r || !opts || !n_pairs || (cap > 0 && !pairs)) return POPSIFT_HIP_ERR_INVALID;
    if (!(opts->ratio >= 0.0f) || std::isinf(opts->ratio) || std::isnan(opts->max_dist2) || opts->reserved != 0 ||
        (opts->cross_check != 0 && opts->cross_check != 1))
        return POPSIFT_HIP_ERR_INVALID;
    *n_pairs = 0;
    if (lc->n_desc == 0 || r->n_desc == 0) return POPSIFT_HIP_OK;
    Set* l = const_cast<Set*>(lc);
    if (hipSetDevice(l->device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    const int         l_len = l->n_desc, r_len = r->n_desc;
    Status            ok;
    PeerCopy          peer;
    const auto* const rdesc = match_forward(ok, l, r, path, peer);
    hipStream_t       s = (hipStream_t)l->m_stream;
    const auto*       fwd = (const popsift_hip_match*)l->m_out;
    pair_block(ok, *l, l_len);
    int* const   d_count = (int*)l->p_pairs; /* [0] pairs, [1] |J| */
    const size_t n_counts = (size_t)std::max(pair_count_blocks(l_len), pair_count_blocks(r_len));
    grow(ok, l->p_idx, l->p_idx_cap, n_counts + (opts->cross_check ? 3 * (size_t)r_len : 0), sizeof(int));
    int*                     counts = l->p_idx;
    const popsift_hip_match* back = nullptr;
    const int*               rank = nullptr;
    size_t                   most = std::min(cap, (size_t)l_len); /* pairs the download has to cover */
    if (ok.good() && opts->cross_check) {
        /* J: the right descriptors a passing row points to.  Only their nearest left neighbours matter. */
        int* const flags = l->p_idx + n_counts;
        int* const list = flags + 2 * (size_t)r_len;
        rank = flags + r_len;
        int n_list = 0;
        /* |J| sizes the reverse sweep's launches and buffers: one 4-byte read-back between the sweeps */
        if (ok(launch_pair_targets(fwd, l_len, r_len, opts->ratio, opts->max_dist2, flags, counts, list, (int*)rank,
                                   d_count + 1, s)) &&
            ok(hipMemcpyAsync(l->p_host, d_count + 1, sizeof(int), hipMemcpyDeviceToHost, s)) && ok(hipStreamSynchronize(s)))
            n_list = *(const int*)l->p_host;
        if (ok.good() && n_list == 0) return POPSIFT_HIP_OK; /* no row passes */
        back = match_reverse(ok, l, rdesc, list, n_list, path);
        most = std::min(most, (size_t)n_list); /* every member of J has one nearest left descriptor */
    }
    if (ok.good() && ok(launch_pair_emit(fwd, l_len, opts->ratio, opts->max_dist2, back, rank, counts,
                                         (popsift_hip_pair*)l->p_pairs + 1, d_count, s)))
        download_pairs(ok, *l, most, -1, pairs, cap, n_pairs, s);
    return ok.rc;
}

}  // namespace

extern "C" {

int popsift_hip_match_set_path(int path)
{
    if (path < POPSIFT_HIP_MATCH_AUTO || path > POPSIFT_HIP_MATCH_SCREEN) return POPSIFT_HIP_ERR_INVALID;
    g_match_path.store(path);
    return POPSIFT_HIP_OK;
}

int popsift_hip_match_sets(const popsift_hip_devfeatures* l, const popsift_hip_devfeatures* r, popsift_hip_match* out)
{
    return match_rows(l, r, out, g_match_path.load());
}

int popsift_hip_devfeatures_debug_redo_count(const popsift_hip_devfeatures* l, int* count)
{
    if (!l || !count) return POPSIFT_HIP_ERR_INVALID;
    *count = -1;
    if (!l->m_redo) return POPSIFT_HIP_OK;
    if (hipSetDevice(l->device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    if (hipStreamSynchronize((hipStream_t)l->m_stream) != hipSuccess ||
        hipMemcpy(count, l->m_redo, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
        return POPSIFT_HIP_ERR_DEVICE;
    return POPSIFT_HIP_OK;
}

int popsift_hip_match_bytes(const popsift_hip_bytefeatures* l, const popsift_hip_bytefeatures* r, popsift_hip_match* out)
{
    return match_rows(l, r, out, 0);
}

void popsift_hip_default_match_opts(popsift_hip_match_opts* o)
{
    if (!o) return;
    o->ratio = 0.8f;
    o->max_dist2 = INFINITY;
    o->cross_check = 0;
    o->reserved = 0;
}

int popsift_hip_match_pairs(const popsift_hip_devfeatures* l, const popsift_hip_devfeatures* r,
                            const popsift_hip_match_opts* opts, popsift_hip_pair* pairs, size_t cap, int* n_pairs)
{
    return match_pairs(l, r, opts, pairs, cap, n_pairs, g_match_path.load());
}

int popsift_hip_match_pairs_bytes(const popsift_hip_bytefeatures* l, const popsift_hip_bytefeatures* r,
                                  const popsift_hip_match_opts* opts, popsift_hip_pair* pairs, size_t cap, int* n_pairs)
{
    return match_pairs(l, r, opts, pairs, cap, n_pairs, 0);
}

} /* extern "C" */
