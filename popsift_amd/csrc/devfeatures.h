/* devfeatures.h -- device-resident result sets (internal; the C ABI sees opaque pointers), the scratch record a set keeps
 * for the calls that have it on the left, and the host helpers those calls share (sets.hip, match_sets.hip,
 * match_guided.hip, ransac.hip).  A set owns everything its fields point to: whichever file makes a buffer, the set's
 * destructor here is the one place that frees it. */
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "sift_types.h"

/* popsift::Feature as laid out on an LP64 host (features.h:22-34): 72 bytes, the four
 * Descriptor* point into `desc` of the same set */
struct DevFeature {
    int    debug_octave;
    float  xpos, ypos, sigma;
    int    num_ori;
    float  orientation[POPSIFT_HIP_ORI_MAX];
    int    pad;
    float* desc[POPSIFT_HIP_ORI_MAX];
};
static_assert(sizeof(DevFeature) == 72, "popsift::Feature layout");

/* device and pinned buffers of a set go; its GPU is current (popsift_hip_*features_free) */
inline void free_bufs(std::initializer_list<void*> dev, std::initializer_list<void*> pinned = {})
{
    for (void* p : dev)
        if (p) (void)hipFree(p);
    for (void* p : pinned)
        if (p) (void)hipHostFree(p);
}

/* Scratch of the matchers with this set on the left, kept between calls (one match at a time per left set, like one image
 * at a time per context).  Both set types embed it. */
struct MatchScratch {
    void*  m_stream = nullptr;  /* hipStream_t */
    void*  m_partial = nullptr; /* the sweeps' per-split candidates */
    size_t m_partial_cap = 0;   /* bytes */
    void*  m_out = nullptr;     /* popsift_hip_match[n_desc] */
    void*  m_host = nullptr;    /* pinned staging of the same size */
    void*  m_rnorm = nullptr;   /* norms of the right set of the current call, in the set's norm type */
    size_t m_rnorm_cap = 0;     /* bytes */
    /* of popsift_hip_match_pairs* */
    void*  p_pairs = nullptr;   /* a 16-byte header ([0] = pair count, [1] = |J|, [2] = the guided matcher's map flag) and
                                   popsift_hip_pair[n_desc] */
    void*  p_host = nullptr;    /* pinned staging of the same size */
    int*   p_idx = nullptr;     /* over the right set: flags, ranks, the list J; and the compaction's block counts */
    size_t p_idx_cap = 0;       /* ints */
    void*  p_back = nullptr;    /* of J: gathered descriptors, their norms, the reverse sweep's rows (and its redo list) */
    size_t p_back_cap = 0;      /* rows */

    MatchScratch() = default;
    MatchScratch(const MatchScratch&) = delete;
    MatchScratch& operator=(const MatchScratch&) = delete;
    ~MatchScratch()
    {
        if (m_stream) (void)hipStreamDestroy((hipStream_t)m_stream);
        free_bufs({m_partial, m_out, m_rnorm, p_pairs, p_idx, p_back}, {m_host, p_host});
    }
};

struct popsift_hip_devfeatures : MatchScratch {
    int         device = 0;
    int         n_feat = 0, n_desc = 0;
    DevFeature* d_feat = nullptr; /* n_feat      */
    float*      d_desc = nullptr; /* n_desc * 128 */
    int*        d_rev = nullptr;  /* n_desc: descriptor -> feature (feat_to_ext_map) */
    float*      d_norm = nullptr; /* |x|^2 per descriptor, computed on first use by a match */
    int*        m_redo = nullptr; /* [0] = count, [1 ..] = rows the screening pass left to the exact kernel */
    /* scratch of popsift_hip_pair_points with this set on the left: a flag, the pairs, the points */
    void*  v_buf = nullptr;
    void*  v_host = nullptr;    /* pinned twin */
    size_t v_cap = 0;           /* bytes */
    /* scratch of the guided matcher with this set on the left (match_guided.hip): a 16-byte header ([0] = a map entry
     * names no feature) and the forward rows, then both sets' positions, the reverse rows and the compaction's counts */
    void*  g_buf = nullptr;
    size_t g_cap = 0;           /* bytes */
    void*  g_host = nullptr;    /* pinned twin of the header and the forward rows */

    ~popsift_hip_devfeatures() { free_bufs({d_feat, d_desc, d_rev, d_norm, m_redo, v_buf, g_buf}, {v_host, g_host}); }
};

/* A set of byte descriptors (popsift_hip_bytefeatures); a zero-filled block reads as an empty set. */
struct popsift_hip_bytefeatures : MatchScratch {
    int      device = 0;
    int      n_desc = 0;
    uint8_t* d_desc = nullptr; /* n_desc * 128, the caller's bytes */
    int*     d_rev = nullptr;  /* n_desc: descriptor -> feature, -1 = none */
    int*     d_norm = nullptr; /* |x - 128|^2 per descriptor, computed on first use by a match */

    ~popsift_hip_bytefeatures() { free_bufs({d_desc, d_rev, d_norm}); }
};

/* A gallery of byte sets (popsift_hip_gallery): the members' bytes end to end with their norms, the member table on the
 * host, and the scratch of the two gallery matchers (match_gallery.hip), which belongs to the gallery and not to the query.
 * Plain pointers and counts only: a zero-filled block reads as a gallery without members.  sets.hip makes and fills it,
 * the destructor here frees everything. */
struct popsift_hip_gallery {
    int      device = 0;
    int      n_members = 0;
    int64_t  n_desc = 0;
    uint8_t* d_desc = nullptr;  /* cap * 128 */
    int*     d_norm = nullptr;  /* cap: |x - 128|^2, computed when the member is added */
    size_t   cap = 0;           /* descriptors the two buffers hold */
    int64_t* first = nullptr;   /* host, tab_cap: first descriptor of member m */
    int*     count = nullptr;   /* host, tab_cap */
    uint8_t* has_xy = nullptr;  /* host, tab_cap: 1 = the member came from a float set and has positions */
    size_t   tab_cap = 0;
    float*   d_xy = nullptr;    /* cap * 2: (xpos, ypos) per descriptor; allocated with the first member that has positions */
    void*    xy_dev = nullptr;  /* scratch of popsift_hip_gallery_pair_points: a flag, the (l, gallery row) items, the points */
    void*    xy_host = nullptr; /* pinned twin */
    size_t   xy_cap = 0;        /* bytes */
    int      group_rows = 0;    /* popsift_hip_gallery_debug_set_group_rows; 0 = POPSIFT_HIP_GALLERY_GROUP_ROWS */
    void*    stream = nullptr;  /* hipStream_t */
    /* scratch of a match, grow-only */
    void*  w_dev = nullptr;     /* a group's member table and work items ... */
    void*  w_host = nullptr;    /* ... and the pinned block they are built in */
    size_t w_cap = 0;           /* bytes */
    void*  w_event = nullptr;   /* hipEvent_t: the upload of w_host has been read */
    int*   lnorm = nullptr;     /* the query's norms */
    size_t lnorm_cap = 0;       /* ints */
    void*  partial = nullptr;   /* the sweeps' per-split candidates */
    size_t partial_cap = 0;     /* bytes */
    void*  rows = nullptr;      /* popsift_hip_match of one group, member-major */
    size_t rows_cap = 0;        /* rows */
    void*  rows_host = nullptr; /* pinned: all rows of popsift_hip_match_gallery */
    size_t rows_host_cap = 0;   /* rows */
    void*  res = nullptr;       /* offsets, the running pair count, |J|; then the pairs */
    void*  res_host = nullptr;  /* pinned twin */
    size_t res_cap = 0;         /* bytes */
    int*   idx = nullptr;       /* over a group's gallery rows: flags, ranks, the list J; and the compactions' block counts */
    size_t idx_cap = 0;         /* ints */
    void*  back = nullptr;      /* of J: gathered descriptors, the reverse sweep's rows, norms */
    size_t back_cap = 0;        /* rows */
    /* of the link matchers (match_links.hip), which share w_*, partial, rows, rows_host, idx, back and xy_* with the above */
    void*  lk_rev = nullptr;      /* a group's link table and work items of the reverse sweep ... */
    void*  lk_rev_host = nullptr; /* ... and the pinned block they are built in */
    size_t lk_rev_cap = 0;        /* bytes */
    void*  lk_res = nullptr;      /* the running pair count, the links' offsets; then the pairs */
    size_t lk_res_cap = 0;        /* bytes */
    void*  lk_host = nullptr;     /* pinned: J's segment starts of a group; the head of lk_res; the pairs found */
    size_t lk_host_cap = 0;       /* bytes */

    popsift_hip_gallery() = default;
    popsift_hip_gallery(const popsift_hip_gallery&) = delete;
    popsift_hip_gallery& operator=(const popsift_hip_gallery&) = delete;
    ~popsift_hip_gallery()
    {
        if (w_event) (void)hipEventDestroy((hipEvent_t)w_event);
        if (stream) (void)hipStreamDestroy((hipStream_t)stream);
        free_bufs({d_desc, d_norm, d_xy, xy_dev, w_dev, lnorm, partial, rows, res, idx, back, lk_rev, lk_res},
                  {xy_host, w_host, rows_host, res_host, lk_rev_host, lk_host});
        free(first);
        free(count);
        free(has_xy);
    }
};

namespace popsift_hip {

/* the first failing HIP call decides the status; the calls after it are skipped */
struct Status {
    int  rc = POPSIFT_HIP_OK;
    bool good() const { return rc == POPSIFT_HIP_OK; }
    bool operator()(hipError_t e)
    {
        if (e != hipSuccess && rc == POPSIFT_HIP_OK) rc = (e == hipErrorOutOfMemory) ? POPSIFT_HIP_ERR_OOM : POPSIFT_HIP_ERR_DEVICE;
        return e == hipSuccess;
    }
};

inline size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }

/* grow-only device scratch: `cap` counts units of `unit` bytes */
template <class T>
bool grow(Status& ok, T*& p, size_t& cap, size_t need, size_t unit)
{
    if (!ok.good()) return false;
    if (need <= cap) return true;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    if (ok(hipMalloc((void**)&p, need * unit))) cap = need;
    return ok.good();
}

/* ... with a pinned host twin of the same size: one capacity, in bytes, for both */
inline bool grow_twin(Status& ok, void*& dev, void*& host, size_t& cap, size_t need)
{
    if (!ok.good() || need <= cap) return ok.good();
    if (host) (void)hipHostFree(host);
    host = nullptr;
    if (grow(ok, dev, cap, need, 1) && !ok(hipHostMalloc(&host, need, hipHostMallocDefault))) cap = 0;
    return ok.good();
}

/* ERR_NO_DEVICE without a usable GPU, ERR_INVALID for an index out of range (sets.hip) */
int check_device(int device);

/* An uninitialised set on `device`, made current: n_feat feature records and n_desc descriptors with their map, or n
 * byte descriptors with theirs.  Allocations of at least one element keep the pointers valid for empty sets.  A failure
 * leaves nothing behind: ERR_DEVICE (the device cannot be made current) or ERR_OOM.  (sets.hip) */
int devfeatures_new(int device, int n_feat, int n_desc, popsift_hip_devfeatures** out);
int bytefeatures_new(int device, int n, popsift_hip_bytefeatures** out);

/* what a constructor ends with (rc: the status of filling f): the set goes to the caller, or is freed */
template <class Set>
int hand_over(int rc, Set* f, Set** out)
{
    if (rc == POPSIFT_HIP_OK) *out = f;
    else delete f;
    return rc;
}

/* the set's own non-blocking stream, created on first use */
inline hipStream_t stream_of(Status& ok, MatchScratch& m)
{
    if (!m.m_stream) {
        hipStream_t s = nullptr;
        if (ok(hipStreamCreateWithFlags(&s, hipStreamNonBlocking))) m.m_stream = s;
    }
    return (hipStream_t)m.m_stream;
}

/* Arrays of a right set on the left set's GPU for the length of one call (images of one PopSift object may have been
 * extracted on different GPUs; xGMI): one allocation, one hipMemcpyPeer per array, freed with the object. */
struct PeerCopy {
    struct Part {
        const void* src;
        size_t      bytes;
    };
    char* at[3] = {nullptr, nullptr, nullptr}; /* the copy of part k (16-byte aligned); at[0] is the allocation */

    PeerCopy() = default;
    PeerCopy(const PeerCopy&) = delete;
    PeerCopy& operator=(const PeerCopy&) = delete;
    ~PeerCopy()
    {
        if (at[0]) (void)hipFree(at[0]);
    }
    /* true: every part has arrived on dst_device.  False: the devices are the same, or a call failed (see ok) */
    template <size_t N>
    bool fetch(Status& ok, int dst_device, int src_device, const Part (&parts)[N])
    {
        static_assert(N <= 3, "at[] holds three parts");
        if (!ok.good() || dst_device == src_device) return false;
        size_t off[N + 1] = {0};
        for (size_t k = 0; k < N; k++) off[k + 1] = off[k] + round16(parts[k].bytes);
        if (!ok(hipMalloc((void**)&at[0], off[N]))) return false;
        for (size_t k = 0; k < N; k++) {
            at[k] = at[0] + off[k];
            if (!ok(hipMemcpyPeer(at[k], dst_device, parts[k].src, src_device, parts[k].bytes))) return false;
        }
        return true;
    }
};

/* the pair block of a left set of l_len descriptors and its pinned twin, allocated on first use */
inline void pair_block(Status& ok, MatchScratch& m, int l_len)
{
    const size_t block = sizeof(popsift_hip_pair) * ((size_t)l_len + 1); /* the header has the size of a pair */
    if (ok.good() && !m.p_pairs) ok(hipMalloc(&m.p_pairs, block));
    if (ok.good() && !m.p_host) ok(hipHostMalloc(&m.p_host, block, hipHostMallocDefault));
}

/* The pair block of a set ([16-byte header][popsift_hip_pair ...], MatchScratch::p_pairs) comes down through its pinned
 * twin: the header and the `most` pairs the call can need.  Header int [0] is the number of pairs found; header int
 * [bad_at] != 0 (bad_at < 0: the call has no such flag) says that a map entry names no feature.  min(found, cap) pairs are
 * copied out; more found than cap is POPSIFT_HIP_ERR_TOO_SMALL. */
inline void download_pairs(Status& ok, MatchScratch& m, size_t most, int bad_at, popsift_hip_pair* pairs, size_t cap,
                           int* n_pairs, hipStream_t s)
{
    const size_t head = sizeof(popsift_hip_pair);
    if (!ok.good() || !ok(hipMemcpyAsync(m.p_host, m.p_pairs, head + sizeof(popsift_hip_pair) * most, hipMemcpyDeviceToHost, s)) ||
        !ok(hipStreamSynchronize(s)))
        return;
    const int* h = (const int*)m.p_host;
    if (bad_at >= 0 && h[bad_at] != 0) {
        ok.rc = POPSIFT_HIP_ERR_INVALID;
        return;
    }
    const int total = h[0];
    *n_pairs = total;
    const size_t n = std::min((size_t)total, cap);
    if (n > 0) memcpy(pairs, (const char*)m.p_host + head, sizeof(popsift_hip_pair) * n);
    if ((size_t)total > cap) ok.rc = POPSIFT_HIP_ERR_TOO_SMALL;
}

}  // namespace popsift_hip
