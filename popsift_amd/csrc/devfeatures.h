/* devfeatures.h -- device-resident result set (internal; the C ABI sees an opaque pointer). */
#pragma once
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

struct popsift_hip_devfeatures {
    int         device = 0;
    int         n_feat = 0, n_desc = 0;
    DevFeature* d_feat = nullptr; /* n_feat      */
    float*      d_desc = nullptr; /* n_desc * 128 */
    int*        d_rev = nullptr;  /* n_desc: descriptor -> feature (feat_to_ext_map) */
    /* scratch of popsift_hip_match_sets with this set on the left, kept between calls */
    void*  m_stream = nullptr;  /* hipStream_t */
    void*  m_partial = nullptr;
    size_t m_partial_cap = 0;
    void*  m_out = nullptr;     /* popsift_hip_match[n_desc] */
    void*  m_host = nullptr;    /* pinned staging of the same size */
    int*   m_redo = nullptr;    /* [0] = count, [1 ..] = rows the screening pass left to the exact kernel */
    float* d_norm = nullptr;    /* |x|^2 per descriptor, computed on first use by a match */
    float* m_rnorm = nullptr;   /* norms of the right set of the current call */
    size_t m_rnorm_cap = 0;
    /* scratch of popsift_hip_match_pairs with this set on the left */
    void*  p_pairs = nullptr;   /* a 16-byte header ([0] = pair count, [1] = |J|) and popsift_hip_pair[n_desc] */
    void*  p_host = nullptr;    /* pinned staging of the same size */
    int*   p_idx = nullptr;     /* over the right set: flags, ranks, the list J; and the compaction's block counts */
    size_t p_idx_cap = 0;       /* ints */
    void*  p_back = nullptr;    /* of J: gathered descriptors, their norms, the reverse sweep's rows and its redo list */
    size_t p_back_cap = 0;      /* rows */
    /* scratch of popsift_hip_pair_points with this set on the left: a flag, the pairs, the points */
    void*  v_buf = nullptr;
    void*  v_host = nullptr;    /* pinned twin */
    size_t v_cap = 0;           /* bytes */
    /* scratch of the guided matcher with this set on the left (match_guided.hip): a 16-byte header ([0] = a map entry
     * names no feature) and the forward rows, then both sets' positions, the reverse rows and the compaction's counts */
    void*  g_buf = nullptr;
    size_t g_cap = 0;           /* bytes */
    void*  g_host = nullptr;    /* pinned twin of the header and the forward rows */
};

/* A set of byte descriptors (popsift_hip_bytefeatures).  The scratch members mean what their namesakes above mean; a
 * zero-filled block reads as an empty set. */
struct popsift_hip_bytefeatures {
    int      device = 0;
    int      n_desc = 0;
    uint8_t* d_desc = nullptr; /* n_desc * 128, the caller's bytes */
    int*     d_rev = nullptr;  /* n_desc: descriptor -> feature, -1 = none */
    void*    m_stream = nullptr;
    void*    m_partial = nullptr;
    size_t   m_partial_cap = 0;
    void*    m_out = nullptr;
    void*    m_host = nullptr;
    int*     d_norm = nullptr;  /* |x - 128|^2 per descriptor, computed on first use by a match */
    int*     m_rnorm = nullptr;
    size_t   m_rnorm_cap = 0;
    void*    p_pairs = nullptr;
    void*    p_host = nullptr;
    int*     p_idx = nullptr;
    size_t   p_idx_cap = 0;
    void*    p_back = nullptr; /* of J: gathered descriptors, the reverse sweep's rows, their norms */
    size_t   p_back_cap = 0;
};
