/*
 * ctx.hip -- C-ABI implementation of libpopsift_hip (include/popsift_hip.h):
 * per-GPU extraction context, Gauss / constant tables, HBM arena, the
 * per-image launch sequence and the ways its results leave the context
 * (fetch, fetch_begin, device pointers, clones).  No device code.  The
 * device-resident sets the clones make are sets.hip, the calls that match
 * sets match_sets.hip; the set types are devfeatures.h.
 *
 * Replaces the host side of the reference's L3 layer:
 *   init_filter / init_constants      gauss_filter.cu:127-257, sift_constants.cu:22-53
 *   Pyramid::Pyramid / Octave::alloc  sift_pyramid.cu:108-165, sift_octave.cu:33-53
 *   Pyramid::step1 / build_pyramid    sift_pyramid.cu:226-230, s_pyramid_build.cu:460-596
 *   Pyramid::step2                    sift_pyramid.cu:232-239
 *   Pyramid::get_descriptors          sift_pyramid.cu:281-321
 * with no process-global state: every context owns its stream, arena and
 * counters, so any number of contexts can run per process / per GPU.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "devfeatures.h"
#include "ext_list.h"
#include "kernels.h"
#include "sift_types.h"
#include "trace.h"

using namespace popsift_hip;

namespace {

constexpr int PITCH_ALIGN = 64; /* floats: rows start on 256 B */
constexpr int PROFILE_REPS = 4; /* launches per event pair in profile mode */

/* N rows of a Gauss table: inc and abs_o0 have one row per level, dd (ScaleDirect) one per octave -- row o blurs octave
 * o's level 0 straight from the input image */
template <int N>
struct GaussRows {
    float filter[N * PS_GA];
    int   span[N];
    float sigma[N];
};

struct EventPair {
    hipEvent_t a, b;
    double     bytes;
    bool       big; /* level launch (MODE 0) with 64-row tiles */
};

/* A grow-only device buffer of `cap` units of PER elements each, grown by grow().  A failed grow or free leaves p and
 * cap consistent: null with capacity 0, or the old buffer. */
template <class T, size_t PER = 1>
struct DevBuf {
    T*     p = nullptr;
    size_t cap = 0;
    hipError_t release()
    {
        const hipError_t e = p ? hipFree(p) : hipSuccess;
        if (e == hipSuccess) {
            p = nullptr;
            cap = 0;
        }
        return e;
    }
};

}  // namespace

/* Device memory of ONE image of a batch (sift_types.h, Slot): what a single-image context owned.  Grow-only. */
struct ImageSlot {
    DevBuf<char> input;
    void*        h_input = nullptr; /* pinned staging: submit() copies the caller's image before returning */
    size_t       h_input_cap = 0;
    DevBuf<float>       arena;
    DevBuf<InitExt>     iext;
    DevBuf<InitExt>     iext2; /* grid filter output (filter enabled only) */
    DevBuf<FilterState> fstate;
    DevBuf<int>         fhist;
    DevBuf<InitExt>     otmp;  /* raster feature order only (order.hip): scratch list, never the filter's iext2 */
    DevBuf<int>         orows; /* ... and the row counters */
    /* keep-strongest pass only (strongest.hip; its output list is iext2): responses before / after thinning in flattened
     * list order, the selection's state, the chunk offsets */
    DevBuf<float>       sresp_in, sresp;
    DevBuf<StrongState> sstate;
    DevBuf<int>         schunk;
    DevBuf<Ext>         ext;
    DevBuf<popsift_hip_feature> feats;
    /* the descriptor group, grown as one (slot_desc_cap): desc_cap() descriptors */
    DevBuf<float, 128> desc;
    DevBuf<int>        map;
    DevBuf<float2>     rot;  /* (cos, sin) of every descriptor's orientation, correctly rounded (k_scan_apply) */
    DevBuf<DescRec>    drec; /* per-descriptor constants of the loop descriptor (k_scan_apply -> k_descriptor) */
    DevBuf<int2>       cand;
    DevBuf<int>        partial; /* one partial sum per scan chunk */
    DevBuf<int>        ovf;     /* detection strips handed to the slow pass */
    bool               sized = false; /* the buffers fit the context's current geometry */
    /* second result slab (popsift_hip_fetch_begin_item): the download of this image reads one slab on copy_stream while the
     * kernels of the next batch write the other.  fetch_begin grows the alt buffers to the current slab's and swaps */
    DevBuf<popsift_hip_feature> alt_feats;
    DevBuf<float, 128>          alt_desc;
    bool moved = false; /* the finished image's results went to fetch_begin: the current slab is stale */
    /* descriptors as bytes (popsift_hip_fetch*_u8), allocated on the first byte request and grown with the slab.  One
     * buffer, not swapped: every path that writes it waits for a pending download first */
    DevBuf<uint8_t, 128> desc_u8;
    bool u8_read = false; /* a popsift_hip_fetch_begin*_u8 download reads desc_u8 (until copy_stream is waited for) */
    /* describe (popsift_hip_describe_batch) only, grown on the first describe: the frames (device copy and pinned staging),
     * the per-chunk counts of the partition, list position <-> frame, k_scan_apply's records in list order */
    DevBuf<popsift_hip_frame>   frames;
    popsift_hip_frame*          h_frames = nullptr;
    DevBuf<int>                 fcounts, perm, inv;
    DevBuf<popsift_hip_feature> lfeats;
    int n_frames = 0; /* frames of the described image */
    /* extraction masks (popsift_hip_submit_batch_masked) only, grown on the first mask this slot sees: the packed w x h
     * device copy k_refine reads and the pinned staging of a pageable mask */
    DevBuf<uint8_t> mask;
    void*           h_mask = nullptr;
    size_t          h_mask_cap = 0;

    /* the descriptor group's capacity: 0 after a failed grow of any of its buffers */
    size_t desc_cap() const { return std::min({desc.cap, map.cap, rot.cap, drec.cap}); }

    /* every buffer of the slot (popsift_hip_ctx_destroy) */
    void release()
    {
        auto each = [](auto&... b) { ((void)b.release(), ...); };
        each(input, arena, iext, iext2, fstate, fhist, otmp, orows, sresp_in, sresp, sstate, schunk, ext, feats, desc, map, rot, drec, cand, partial, ovf, alt_feats,
             alt_desc, desc_u8, frames, fcounts, perm, inv, lfeats, mask);
        if (h_input) (void)hipHostFree(h_input);
        if (h_mask) (void)hipHostFree(h_mask);
        if (h_frames) (void)hipHostFree(h_frames);
    }
};

struct popsift_hip_ctx {
    int                device = 0;
    popsift_hip_params p{};
    int                levels = 3, L = 6;
    GaussRows<POPSIFT_HIP_MAX_LEVELS> tab{};
    GaussRows<POPSIFT_HIP_MAX_LEVELS> abs0{}; /* vlfeat-direct (gauss_mode 2): abs_o0, octave 0's levels from the input image */
    float*             d_abs0 = nullptr; /* abs0.filter on the device (the fused kernel's taps), gauss_mode 2 only */
    int                direct_path = 0;  /* DIRECT_PATH debug switch: 0 fused octave-0 kernel, 1 one level-0 launch per level */
    GaussRows<POPSIFT_HIP_MAX_OCTAVES> dd{}; /* ScaleDirect (params.scale_direct = 1): dd, every octave's level 0 from the input */
    float*             d_dd = nullptr;   /* dd.filter on the device (the level-0 launch's horizontal taps), ScaleDirect only */
    int                scale_path = 0;   /* SCALE_PATH debug switch: 0 all-octave launches, 1 per-octave launches */
    SiftConsts         sc{};
    hipStream_t        stream = nullptr;
    hipEvent_t         ev_begin = nullptr, ev_end = nullptr;
    hipEvent_t         ev_stage[POPSIFT_HIP_STAGE_COUNT + 1] = {}; /* profile mode 2: boundaries of the stages */

    /* image geometry (one for all images of a batch) */
    int  in_w = 0, in_h = 0;
    int  frozen_octaves = -1;
    bool have_image = false, finished = false;
    bool batch_ok = false; /* the last submit enqueued everything it had to: there are (or will be) results to wait for */
    int  nb = 1; /* images of the submitted batch */
    bool describe = false;  /* the batch in the context is a describe (popsift_hip_describe_batch), not an extraction */
    int  ori_given = 0;     /* ... with POPSIFT_HIP_ORI_GIVEN */
    int  frames_max = 0;    /* ... and the most frames of one of its images */
    bool masked = false;    /* an image of the batch in the context has a mask (popsift_hip_submit_batch_masked): re-runs apply */
    MaskArgs ma{};          /* ... these again; a plain submit or a describe clears them */

    /* one slot per image of a batch; a plain submit uses slot 0 */
    ImageSlot slot[PS_MAX_BATCH];
    BatchDesc bd{}; /* the kernels' view of the slots in use (a kernel argument, passed by value) */
    PyrDesc   pd{};
    int       kp_waves = 65536; /* launch size of the keypoint kernels in waves (8 per wave slot of the device) */
    int       det_qcap = 1 << 30;  /* popsift_hip_debug_set hooks, see popsift_hip.h */
    int       desc_rows = 1 << 30;
    int       desc_list = 1 << 30;
    BlurTune  blur_tune{0, 0, 0}; /* BLUR_PATH / BLUR_SEG / BLUR_TILE_H debug switches */
    int       keep_strongest = 0; /* popsift_hip_set_keep_strongest: 0 off, n: the next enqueue keeps the n strongest */
    int       batch_keep = 0;     /* ... and what the keypoint stages of the batch in the context were enqueued with */
    int       order_coarse = 0; /* ORDER_COARSE: row bits the ordering pass drops from its bucket key */
    int       pyr_tail = 0;    /* PYR_TAIL: 0 the smallest octaves in one launch where they fit, 1 level launches only */
    int       cand_cap_init = 1 << 20;
    bool      cand_cap_user = false;
    int       ohist_cap_init = 0;
    int       desc_cap_init = 0; /* DESC_CAP debug switch: initial descriptor capacity (0 = 2 * max_extrema) */
    size_t    ext_cap = 0; /* entries every one of iext/ext/feats(/iext2) of the sized slots holds */
    /* capacities the kernels are told: the smallest over the slots of the batch (refresh_caps) */
    int       cand_cap = 0, desc_cap = 0;
    /* extrema k_orientation gives orientations to in one pass: no buffer (a group's histograms stay in its wave's LDS), a
     * bound the host keeps, grow-only like the buffers; finish() raises it and re-runs when an image has more */
    size_t    ohist_cap = 0;
    hipStream_t copy_stream = nullptr;
    hipEvent_t  ev_u8 = nullptr;    /* the byte pass of a fetch_begin*_u8 on `stream` -> its copies on copy_stream */
    bool     copy_pending = false;  /* fetch_begin downloads have not been waited for */
    unsigned long submit_seq = 0, copy_seq = 0; /* the batch now in the context / the batch whose downloads are pending */
    Counters* d_ct = nullptr; /* PS_MAX_BATCH counter blocks, one per slot */
    Counters* h_ct = nullptr; /* pinned mirror */
    PyrDesc*  d_pd = nullptr; /* device copy of pd (kernels index octaves dynamically) */
    PyrDesc*  h_pd = nullptr; /* pinned staging for d_pd */
    int       n_feat[PS_MAX_BATCH] = {}, n_desc[PS_MAX_BATCH] = {}; /* results of the finished batch */

    /* profiling */
    int                    fail_alloc_in = 0; /* test hook (popsift_hip_debug_fail_alloc): the n-th device allocation from now fails */
    int                    profile = 0;
    std::vector<EventPair> blur_events;
    size_t                 blur_events_used = 0;
    popsift_hip_report     rep{};

    char err[256] = {0};
};

namespace {

int fail(popsift_hip_ctx* c, int code, const char* fmt, ...)
{
    if (c) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(c->err, sizeof(c->err), fmt, ap);
        va_end(ap);
    }
    return code;
}

#define HIP_TRY(c, call)                                                                              \
    do {                                                                                              \
        hipError_t e__ = (call);                                                                      \
        if (e__ != hipSuccess)                                                                        \
            return fail((c), e__ == hipErrorOutOfMemory ? POPSIFT_HIP_ERR_OOM : POPSIFT_HIP_ERR_DEVICE, \
                        "%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e__));          \
    } while (0)

/* POP_SYNC_CHK (common/debug_macros.h:25-29): in a SYNC_CHECK build every launch of the per-image sequence is followed
 * by a stream synchronisation and an error check, so a faulting kernel is named where it was launched */
#ifdef POPSIFT_SYNC_CHECK
#define SYNC_CHK(c, what)                                                                                     \
    do {                                                                                                      \
        hipError_t e__ = hipStreamSynchronize((c)->stream);                                                   \
        if (e__ == hipSuccess) e__ = hipGetLastError();                                                       \
        if (e__ != hipSuccess) {                                                                              \
            fprintf(stderr, "%s:%d sync check after %s: %s\n", __FILE__, __LINE__, what, hipGetErrorString(e__)); \
            return fail((c), POPSIFT_HIP_ERR_DEVICE, "sync check after %s: %s", what, hipGetErrorString(e__)); \
        }                                                                                                     \
    } while (0)
#else
#define SYNC_CHK(c, what) \
    do {                  \
    } while (0)
#endif

/* GaussInfo::getSpan, gauss_filter.cu:274-328 */
int span_for(int gauss_mode, float sigma)
{
    if (gauss_mode == POPSIFT_HIP_GAUSS_OPENCV_COMPUTE) {
        int span = int(roundf(2.0f * 4.0f * sigma + 1.0f)) | 1;
        span >>= 1;
        span += 1;
        return std::min<int>(span, PS_GA - 1);
    }
    return std::min<int>(ceilf(4.0f * sigma) + 1, PS_GA - 1);
}

/* GaussTable::computeBlurTable (gauss_filter.cu:340-372): spans and normalised half filters of the N rows of t.sigma */
template <int N>
void compute_filter_rows(GaussRows<N>& t, int gauss_mode)
{
    for (int level = 0; level < N; level++) {
        t.span[level] = std::min(span_for(gauss_mode, t.sigma[level]), PS_GA - 1);
        const float sig = t.sigma[level];
        const int   spn = t.span[level];
        float*      f = &t.filter[level * PS_GA];
        double      sum = 1.0;
        f[0] = 1.0f;
        for (int x = 1; x < spn; x++) {
            const float val = (float)exp(-0.5 * (pow(double(x) / sig, 2.0)));
            f[x] = val;
            sum += 2.0f * val;
        }
        for (int x = 0; x < spn; x++) f[x] = (float)(f[x] / sum);
        for (int x = spn; x < PS_GA; x++) f[x] = 0.0f;
    }
}

/* init_filter (inc table; dd[0] is identical to inc[0]) gauss_filter.cu:163-181,340-372
 * and init_constants sift_constants.cu:22-31 */
void init_tables(popsift_hip_ctx* c)
{
    const popsift_hip_params& p = c->p;
    const float sigma0 = p.sigma;
    const int   levels = c->levels;
    const float initial_blur = p.assume_initial_blur ? p.initial_blur * powf(2.0f, p.upscale_factor) : 0.0f;
    auto&       t = c->tab;
    memset(&t, 0, sizeof(t));
    t.sigma[0] = p.assume_initial_blur ? sqrtf(fabsf(sigma0 * sigma0 - initial_blur * initial_blur)) : sigma0;
    for (int lvl = 1; lvl < c->L; lvl++) {
        const float sigmaP = sigma0 * powf(2.0f, (float)(lvl - 1) / (float)levels);
        const float sigmaS = sigma0 * powf(2.0f, (float)(lvl) / (float)levels);
        t.sigma[lvl] = sqrtf(sigmaS * sigmaS - sigmaP * sigmaP);
    }
    compute_filter_rows(t, p.gauss_mode);
    /* abs_o0 (gauss_filter.cu:190-199): octave 0's level l straight from the input image, sigma relative to the assumed
     * blur of the input; spans by the VLFeat rule (GaussInfo::getSpan for VLFeat_Relative_All).  abs0.sigma[0] equals
     * tab.sigma[0] (sqrt(RN(s * s)) == s), so level 0 is the default mode's level 0. */
    auto& a0 = c->abs0;
    memset(&a0, 0, sizeof(a0));
    if (p.gauss_mode == POPSIFT_HIP_GAUSS_VLFEAT_RELATIVE_ALL) {
        for (int lvl = 0; lvl < c->L; lvl++) {
            const float sigmaS = sigma0 * powf(2.0f, (float)lvl / (float)levels);
            a0.sigma[lvl] = sqrtf(fabsf(sigmaS * sigmaS - initial_blur * initial_blur));
        }
        compute_filter_rows(a0, p.gauss_mode);
    }
    /* dd (gauss_filter.cu:217-236): octave o's level 0 blurred straight from the input image; the blur is sigma0 * 2^o
     * less the assumed blur of the input, in octave-o pixels.  dd.sigma[0] equals tab.sigma[0], so octave 0 is the
     * default mode's octave 0. */
    auto& dd = c->dd;
    memset(&dd, 0, sizeof(dd));
    for (int oct = 0; oct < POPSIFT_HIP_MAX_OCTAVES; oct++) {
        const float oct_sigma = ldexpf(sigma0, oct);
        const float b = sqrtf(fabsf(oct_sigma * oct_sigma - initial_blur * initial_blur));
        dd.sigma[oct] = ldexpf(b, -oct);
    }
    compute_filter_rows(dd, p.gauss_mode);
    SiftConsts& sc = c->sc;
    sc.sigma0 = sigma0;
    sc.sigma_k = powf(2.0f, 1.0f / levels);
    sc.edge_limit = p.edge_limit;
    sc.threshold = p.threshold * 0.5f * 255.0f / levels; /* Config::getPeakThreshold, sift_conf.cu:275-278 */
    sc.max_extrema = p.max_extrema;
    sc.norm_multi = p.norm_multi;
    sc.norm_mode = p.norm_mode;
    sc.sift_mode = p.sift_mode;
    sc.grid_size = p.filter_grid_size > 0 ? p.filter_grid_size : 1;
    sc.up_fac_int = (int)p.upscale_factor;
    sc.desc_mode = p.desc_mode;
    sc.filter_max = p.filter_max_extrema;
    sc.filter_mode = p.filter_sorting;
    sc.det_qcap = c->det_qcap;
    sc.desc_rows = c->desc_rows;
    sc.desc_list = c->desc_list;
}

/* PopSift::private_init, popsift.cpp:89-120 */
void plan_dims(const popsift_hip_params& p, int w, int h, int octaves_cfg, int* n_oct, int* bw, int* bh)
{
    const float scaleFactor = 1.0f / powf(2.0f, -p.upscale_factor);
    int         oct = octaves_cfg;
    if (oct < 0) oct = std::max(int(floorf(logf((float)std::min(w, h)) / logf(2.0f)) - 3.0f + scaleFactor), 1);
    oct = std::min(oct, PS_MAX_OCT);
    *n_oct = oct;
    *bw = (int)ceilf(w * scaleFactor);
    *bh = (int)ceilf(h * scaleFactor);
}

/* Pyramid::Pyramid, sizes only: the octaves of a w x h image under params p (levels = DoG search levels, L = levels + 3
 * Gaussian planes, octaves_cfg < 0: as many as the image allows), their planes as float offsets into one arena, the
 * detection work units and the arena's size in floats.  No device, no context: popsift_hip_plan_arena answers from here
 * as well.  Returns nullptr, or what is wrong with the geometry. */
const char* plan_pyramid(const popsift_hip_params& p, int levels, int L, int octaves_cfg, int w, int h, PyrDesc* out,
                         size_t* arena_floats, int* base_w, int* base_h)
{
    int n_oct, bw, bh;
    memset(out, 0, sizeof(*out));
    *arena_floats = 0;
    plan_dims(p, w, h, octaves_cfg, &n_oct, &bw, &bh);
    *base_w = bw;
    *base_h = bh;
    if (bw < 1 || bh < 1) return "scaled image is empty";
    /* candidates pack (x, y) into 16 bits each; the reference's Plane2D uses short dims too (plane_2d.h:257) */
    if (bw > 32767 || bh > 32767) return "scaled image exceeds 32767 pixels per side";
    PyrDesc& pd = *out;
    size_t   total = 0;
    pd.n_oct = n_oct;
    pd.levels = levels;
    pd.L = L;
    /* DoG planes are not stored (params.store_dog = 0): detection and refinement subtract the Gaussian planes they
     * load -- the same f32 subtraction make_dog does (s_pyramid_build.cu:74-92), so results are bit-identical, with a
     * third fewer bytes per level launch and an octave-0 working set that fits the last-level cache.  An arena then
     * holds L planes per octave plus ONE scratch plane (the size of octave 0's) into which the debug download forms a
     * DoG plane on demand; with store_dog = 1 it holds the reference's 2L-1 planes per octave.  Planes are described
     * by their float offsets from the arena base, the same for every image of a batch (OctDesc::data_off / dog_off;
     * the absolute pointers of OctDesc are not used). */
    pd.dog_fly = p.store_dog ? 0 : 1;
    int ow = bw, oh = bh, tiles = 0;
    for (int o = 0; o < n_oct; o++) {
        OctDesc& od = pd.o[o];
        od.w = ow;
        od.h = oh;
        od.pitch = (ow + PITCH_ALIGN - 1) / PITCH_ALIGN * PITCH_ALIGN;
        od.plane_stride = (int64_t)od.pitch * oh;
        od.tile_begin = tiles;
        tiles += extrema_units(ow, oh);
        od.data_off = (int64_t)total;
        total += (size_t)od.plane_stride * (size_t)L;
        if (!pd.dog_fly) {
            od.dog_off = (int64_t)total;
            total += (size_t)od.plane_stride * (size_t)(L - 1);
        }
        ow = (int)ceilf(ow / 2.0f); /* sift_pyramid.cu:132-133 */
        oh = (int)ceilf(oh / 2.0f);
    }
    if (pd.dog_fly) {
        for (int o = 0; o < n_oct; o++) pd.o[o].dog_off = (int64_t)total; /* download_plane(kind = 1) only */
        total += (size_t)pd.o[0].plane_stride;
    }
    pd.total_tiles = tiles;
    *arena_floats = total;
    /* detection and refinement address a plane element as the arena's base plus an unsigned 32-bit byte offset
     * (extrema.hip), as the keypoint kernels do within a plane */
    if (total * sizeof(float) >= ((size_t)1 << 32)) return "pyramid arena of 4 GiB or more: the image is too large";
    return nullptr;
}

/* every device allocation of a context goes through here, so that tests can make the n-th one fail */
hipError_t ctx_malloc(popsift_hip_ctx* c, void** p, size_t bytes)
{
    if (c->fail_alloc_in > 0 && --c->fail_alloc_in == 0) {
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    return hipMalloc(p, bytes);
}

template <class T, size_t PER>
int grow(popsift_hip_ctx* c, DevBuf<T, PER>& b, size_t need)
{
    if (need <= b.cap) return 0;
    HIP_TRY(c, b.release());
    HIP_TRY(c, ctx_malloc(c, (void**)&b.p, need * PER * sizeof(T)));
    b.cap = need;
    return 0;
}

/* the capacities the kernels are told = the smallest over the slots of the batch, and the kernels' slot table */
void refresh_caps(popsift_hip_ctx* c)
{
    size_t cand = 1 << 30, desc = 1 << 30;
    for (int k = 0; k < c->nb; k++) {
        const ImageSlot& s = c->slot[k];
        cand = std::min(cand, s.cand.cap);
        desc = std::min(desc, s.desc_cap());
        Slot& v = c->bd.s[k];
        v.arena = s.arena.p;
        v.ct = c->d_ct + k;
        v.cand = s.cand.p;
        v.ovf = s.ovf.p;
        v.iext = s.iext.p;
        v.iext2 = s.iext2.p;
        v.fstate = s.fstate.p;
        v.fhist = s.fhist.p;
        v.ext = s.ext.p;
        v.partial = s.partial.p;
        v.map = s.map.p;
        v.rot = s.rot.p;
        v.drec = s.drec.p;
        v.feats = s.feats.p;
        v.desc = s.desc.p;
    }
    c->cand_cap = (int)cand;
    c->desc_cap = (int)desc;
}

/* the descriptor group: all four buffers are freed, then allocated in order, so that a failure anywhere leaves
 * desc_cap() = 0 and the next grow allocates all four again */
int slot_desc_cap(popsift_hip_ctx* c, ImageSlot& s, size_t need)
{
    if (need <= s.desc_cap()) return 0;
    HIP_TRY(c, s.desc.release());
    HIP_TRY(c, s.map.release());
    HIP_TRY(c, s.rot.release());
    HIP_TRY(c, s.drec.release());
    if (int rc = grow(c, s.desc, need)) return rc;
    if (int rc = grow(c, s.map, need)) return rc;
    if (int rc = grow(c, s.rot, need)) return rc;
    return grow(c, s.drec, need);
}

/* grow a buffer of every slot of the batch (grow_slot); the kernels' capacities follow whatever the outcome */
template <typename F>
int ensure_cap(popsift_hip_ctx* c, F grow_slot)
{
    int rc = 0;
    for (int k = 0; k < c->nb && !rc; k++) rc = grow_slot(c->slot[k]);
    refresh_caps(c);
    return rc;
}

/* Pyramid::Pyramid / resetDimensions: sizes for this image size and batch, grow-only buffers.
 * Failure-safe: the context forgets its geometry before anything is freed and commits the new one only after every
 * allocation and the upload of the device copy have been issued, so a submit after a failed one (ERR_OOM is a
 * recoverable status of this ABI) never finds sizes that describe buffers which no longer exist. */
int prepare_geometry(popsift_hip_ctx* c, int w, int h, int nb)
{
    const bool same = c->have_image && w == c->in_w && h == c->in_h && c->pd.n_oct > 0;
    PyrDesc    pd = c->pd;
    int        bw = c->rep.base_w, bh = c->rep.base_h;
    size_t     total = 0;
    if (!same) {
        PyrDesc plan;
        if (const char* why = plan_pyramid(c->p, c->levels, c->L, c->frozen_octaves, w, h, &plan, &total, &bw, &bh))
            return fail(c, POPSIFT_HIP_ERR_INVALID, why);
        if (c->sc.filter_max > 0 && !filter_supported(plan.n_oct, c->sc.max_extrema, c->sc.grid_size))
            return fail(c, POPSIFT_HIP_ERR_INVALID, "grid filter: grid size > 64 or octaves * max_extrema >= 2^25");
        c->frozen_octaves = plan.n_oct; /* popsift.cpp:111: decided by the first image */

        c->in_w = c->in_h = 0;
        c->have_image = false;
        c->pd.n_oct = 0;
        c->ext_cap = 0;
        for (int k = 0; k < PS_MAX_BATCH; k++) c->slot[k].sized = false;

        pd = plan;
    } else {
        const OctDesc& last = pd.o[pd.n_oct - 1];
        total = pd.dog_fly ? (size_t)pd.o[0].dog_off + (size_t)pd.o[0].plane_stride
                           : (size_t)last.dog_off + (size_t)last.plane_stride * (size_t)(c->L - 1);
    }
    const size_t need_ext = (size_t)pd.n_oct * (size_t)c->sc.max_extrema;
    /* orientations: 2 * max_extrema extrema to start with (all octaves together seldom exceed one octave's cap); finish()
     * raises the bound and re-runs the keypoint stages when an image has more */
    c->ohist_cap = std::max(c->ohist_cap, c->ohist_cap_init > 0 ? (size_t)c->ohist_cap_init
                                                                 : std::min(need_ext, (size_t)2 * c->sc.max_extrema));
    for (int k = 0; k < nb; k++) {
        ImageSlot& s = c->slot[k];
        if (s.sized) continue;
        if (int rc = grow(c, s.arena, total)) return rc;
        /* each buffer keeps its own capacity: a failed grow leaves the others consistent */
        if (int rc = grow(c, s.iext, need_ext)) return rc;
        if (int rc = grow(c, s.ext, need_ext)) return rc;
        if (int rc = grow(c, s.feats, need_ext)) return rc;
        if (c->sc.filter_max > 0) {
            if (int rc = grow(c, s.iext2, need_ext)) return rc;
            if (int rc = grow(c, s.fstate, 1)) return rc;
            if (int rc = grow(c, s.fhist, filter_hist_bytes(c->sc.grid_size) / sizeof(int))) return rc;
        }
        if (c->p.feature_order == POPSIFT_HIP_ORDER_RASTER) {
            if (int rc = grow(c, s.otmp, need_ext)) return rc;
            if (int rc = grow(c, s.orows, order_rows(pd))) return rc;
        }
        if (int rc = grow(c, s.partial, (need_ext / scan_chunk() + 2) * scan_partials_per_chunk())) return rc;
        /* sift_pyramid.cu:149: max(2*max_extrema, max_orientations) descriptors to start with */
        const int desc0 = c->desc_cap_init > 0 ? c->desc_cap_init
                                               : std::max(2 * c->sc.max_extrema, c->sc.max_extrema + c->sc.max_extrema / 4);
        if (int rc = slot_desc_cap(c, s, std::max(desc0, c->desc_cap))) return rc;
        /* candidates: 64 region slices of one buffer (extrema.hip); a default-sized buffer grows with the pyramid, so that
         * the first image of a 4K stream does not overflow a slice and re-run (a test's explicit CAND_CAP is taken as is) */
        int cand0 = std::max(c->cand_cap_init, DET_SUBQ);
        if (!c->cand_cap_user) {
            double px = 0;
            for (int o = 0; o < pd.n_oct; o++) px += (double)pd.o[o].w * pd.o[o].h;
            cand0 = std::max(cand0, (int)std::min(px / 8.0, 64.0 * 1024 * 1024));
        }
        if (int rc = grow(c, s.cand, std::max(cand0, c->cand_cap))) return rc;
        if (int rc = grow(c, s.ovf, (size_t)pd.total_tiles + 1)) return rc;
        s.sized = true;
    }
    c->ext_cap = need_ext;
    if (!same) {
        /* the stream is idle here (submit drains the previous batch first), so h_pd is free to reuse */
        *c->h_pd = pd;
        HIP_TRY(c, hipMemcpyAsync(c->d_pd, c->h_pd, sizeof(PyrDesc), hipMemcpyHostToDevice, c->stream));
        c->pd = pd;
        c->in_w = w;
        c->in_h = h;
        c->rep.num_octaves = pd.n_oct;
        c->rep.base_w = bw;
        c->rep.base_h = bh;
        double px = 0;
        for (int o = 0; o < pd.n_oct; o++) px += (double)pd.o[o].w * pd.o[o].h;
        c->rep.pyramid_pixels = px;
    }
    return 0;
}

/* Profile mode 1 brackets PROFILE_REPS back-to-back launches with one event pair: the event-to-kernel gap (~4 us, as large
 * as a small launch itself) is amortised instead of being billed per launch.  Every launch timed here is idempotent (a
 * level launch reads plane l-1, writes plane l and DoG l-1).  big: a level launch (MODE 0) with 64-row tiles. */
template <typename F>
int timed_launch(popsift_hip_ctx* c, double alg_bytes, const char* what, F launch, bool big = false)
{
    if (c->profile == 1) {
        if (c->blur_events_used == c->blur_events.size()) {
            EventPair ep;
            HIP_TRY(c, hipEventCreate(&ep.a));
            HIP_TRY(c, hipEventCreate(&ep.b));
            c->blur_events.push_back(ep);
        }
        EventPair& ep = c->blur_events[c->blur_events_used++];
        ep.bytes = alg_bytes * c->nb;
        ep.big = big;
        HIP_TRY(c, hipEventRecord(ep.a, c->stream));
        for (int rep = 0; rep < PROFILE_REPS; rep++) HIP_TRY(c, launch());
        HIP_TRY(c, hipEventRecord(ep.b, c->stream));
    } else {
        HIP_TRY(c, launch());
        SYNC_CHK(c, what);
    }
    (void)what;
    return 0;
}

/* Rows per tile of the launches on a w x h plane: blur_tile_h's choice by plane size, or the BLUR_TILE_H test switch's for
 * every plane.  The one place the switch applies: the tile grid (set_plane), the kernel (launch_blur) and the pairing
 * into k_blur_duo all take the height from here.  Nothing else depends on it -- a plane's pitch (rows padded to 64
 * floats) and stride come from its size alone (prepare), the kernels clamp their loads to the plane and store only
 * pixels inside it -- so a forced height moves no buffer and changes no value. */
int tile_rows(const popsift_hip_ctx* c, int w, int h) { return c->blur_tune.tile_h ? c->blur_tune.tile_h : blur_tile_h(w, h); }

int blur_launch(popsift_hip_ctx* c, const BlurArgs& a, int mode, int span, int tile_h, double alg_bytes)
{
    return timed_launch(
        c, alg_bytes, "k_blur_tile", [&] { return launch_blur(a, c->bd, c->nb, mode, span, tile_h, c->stream, c->blur_tune); },
        mode == 0 && tile_h == 64);
}

/* the size of octave o's plane and its tile grid for tile_h-row tiles (BlurArgs, DirectArgs) */
template <typename A>
void set_plane(A& a, const OctDesc& od, int tile_h)
{
    a.w = od.w;
    a.h = od.h;
    a.pitch = od.pitch;
    a.tiles_x = (od.w + blur_tile_w() - 1) / blur_tile_w();
    a.tiles_y = (od.h + tile_h - 1) / tile_h;
}

/* arguments of the launch that produces plane `level` (>= 1) of octave o from plane level - 1 */
BlurArgs level_args(const popsift_hip_ctx* c, int o, int level)
{
    const PyrDesc& pd = c->pd;
    const OctDesc& od = pd.o[o];
    BlurArgs       a{};
    set_plane(a, od, tile_rows(c, od.w, od.h));
    memcpy(a.taps.g, &c->tab.filter[level * PS_GA], sizeof(a.taps.g));
    a.dst_off = od.data_off + level * od.plane_stride;
    a.src_off = od.data_off + (level - 1) * od.plane_stride;
    a.dog_off = pd.dog_fly ? -1 : od.dog_off + (level - 1) * od.plane_stride;
    /* level L-3 also writes every second pixel as plane 0 of the next octave (get_by_2_pick_every_second) */
    a.next0_off = (level == pd.L - 3 && o + 1 < pd.n_oct) ? pd.o[o + 1].data_off : -1;
    a.next_pitch = (o + 1 < pd.n_oct) ? pd.o[o + 1].pitch : 0;
    return a;
}

/* the shift of the upscale from the input image (s_pyramid_build.cu:109-114) */
float input_shift(const popsift_hip_ctx* c)
{
    if (c->p.sift_mode == POPSIFT_HIP_SIFT_POPSIFT || c->p.sift_mode == POPSIFT_HIP_SIFT_VLFEAT)
        return 0.5f * powf(2.0f, c->p.upscale_factor - 0);
    return 0.5f;
}

/* Arguments of a launch that samples the input image into level 0 of octave o, tile_h-row tiles (horiz_from_input_image,
 * s_pyramid_build.cu:96-126); the taps are the caller's.  The launch also clears the images' counters
 * (enqueue_keypoint_stages(c, true)). */
BlurArgs input_args(const popsift_hip_ctx* c, int o, int tile_h, int is_f32, int pitch, bool aligned4)
{
    const OctDesc& od = c->pd.o[o];
    BlurArgs       a{};
    set_plane(a, od, tile_h);
    a.dst_off = od.data_off;
    a.src_off = 0;
    a.dog_off = -1;
    a.next0_off = -1;
    a.in_w = c->in_w;
    a.in_h = c->in_h;
    a.in_pitch = pitch;
    a.shift = input_shift(c);
    /* weights of the linear upscale are exactly {0, 1/2}: k_blur_tile's copy / average path */
    a.fast2x = (c->p.upscale_factor == 1.0f && a.shift == 1.0f && od.w == 2 * c->in_w && od.h == 2 * c->in_h) ? 1 : 0;
    /* ... and u8 images whose rows all start on 4-byte boundaries: the texels are fetched as aligned dwords */
    if (a.fast2x && !is_f32 && aligned4) a.fast2x = 2;
    a.zero_words = (int)(sizeof(Counters) / sizeof(int));
    return a;
}

/*
 * Octave 0 of the vlfeat-direct Gauss mode (Pyramid::build_pyramid, s_pyramid_build.cu:545-548): every level l is the
 * input image upscaled and blurred with the abs_o0[l] taps, horizontally (normalizedSource::horiz_all) then vertically
 * (absoluteSource::vert_all_abs0).  Writes the L Gaussian planes, the L-1 DoG planes when they are stored, level 0 of
 * octave 1 (every second pixel of level L-3) and clears the images' counters, like the default mode's octave-0
 * launches.  DIRECT_PATH 0: one fused launch (pyr_direct.hip); 1: the level-0 kernel once per level with the abs_o0
 * taps, then the DoG planes and octave 1's level 0 by launches of their own (the in-tree yardstick of the fused one).
 */
int enqueue_direct_octave0(popsift_hip_ctx* c, int is_f32, int pitch, bool aligned4)
{
    const PyrDesc& pd = c->pd;
    const OctDesc& od = pd.o[0];
    const int      L = pd.L;
    const int64_t  next0_off = pd.n_oct > 1 ? pd.o[1].data_off : -1;
    const double   in_bytes = (double)c->in_w * c->in_h * (is_f32 ? 4 : 1);
    const double   px = (double)od.w * od.h;
    if (c->direct_path == 0) {
        DirectArgs a{};
        set_plane(a, od, pyr_direct_tile_h());
        a.dst_off = od.data_off;
        a.dog_off = pd.dog_fly ? -1 : od.dog_off;
        a.plane_stride = od.plane_stride;
        a.next0_off = next0_off;
        a.taps = c->d_abs0;
        a.next_pitch = pd.n_oct > 1 ? pd.o[1].pitch : 0;
        a.in_w = c->in_w;
        a.in_h = c->in_h;
        a.in_pitch = pitch;
        a.shift = input_shift(c);
        a.L = L;
        for (int l = 0; l < L; l++) a.halo[l] = c->abs0.span[l] - 1;
        a.zero_words = (int)(sizeof(Counters) / sizeof(int));
        const double bytes = in_bytes + 4.0 * px * (L + (pd.dog_fly ? 0 : L - 1)) + (next0_off >= 0 ? px : 0.0);
        return timed_launch(c, bytes, "k_pyr_direct", [&] { return launch_pyr_direct(a, c->bd, c->nb, is_f32, c->stream); });
    }
    const int thd = tile_rows(c, od.w, od.h);
    for (int l = 0; l < L; l++) {
        BlurArgs a = input_args(c, 0, thd, is_f32, pitch, aligned4);
        memcpy(a.taps.g, &c->abs0.filter[l * PS_GA], sizeof(a.taps.g));
        a.dst_off += l * od.plane_stride;
        if (l > 0) a.zero_words = 0; /* the first launch clears the counters */
        const int span = c->abs0.span[l];
        if (int rc = timed_launch(c, in_bytes + 4.0 * px, "k_blur_tile (direct level)",
                                  [&] { return launch_blur(a, c->bd, c->nb, is_f32 ? 2 : 1, span, thd, c->stream, c->blur_tune); }))
            return rc;
    }
    if (!pd.dog_fly)
        for (int l = 0; l + 1 < L; l++) {
            const int64_t lo = od.data_off + l * od.plane_stride, up = lo + od.plane_stride, dg = od.dog_off + l * od.plane_stride;
            if (int rc = timed_launch(c, 12.0 * px, "k_dog_batch",
                                      [&] { return launch_dog_batch(lo, up, dg, od.plane_stride, c->bd, c->nb, c->stream); }))
                return rc;
        }
    if (next0_off >= 0) {
        const OctDesc& o1 = pd.o[1];
        const int64_t  src = od.data_off + (L - 3) * od.plane_stride;
        if (int rc = timed_launch(c, 8.0 * o1.w * o1.h, "k_pick_every_second", [&] {
                return launch_pick_every_second(src, od.w, od.h, od.pitch, o1.data_off, o1.w, o1.h, o1.pitch, c->bd, c->nb, c->stream);
            }))
            return rc;
    }
    return 0;
}

/*
 * The ScaleDirect scaling mode (Pyramid::build_pyramid, s_pyramid_build.cu:499-516), taken before the vlfeat-direct
 * branch, so also for Gauss mode 2: octave o's level 0 is the input image sampled at octave o's size, blurred
 * horizontally with dd[o] and vertically with inc[0]; levels 1 .. L-1 are incremental as in the default mode; no
 * octave's level 0 comes from the octave before.  The octaves are independent, so SCALE_PATH 0 builds the pyramid in
 * L launches for the whole batch: level 0 of every octave (k_pyr_level0_octaves, which also clears the counters), then
 * one launch per level l covering every octave (k_blur_octaves).  SCALE_PATH 1, the yardstick: level 0 of each octave
 * by a launch of its own, then each octave's levels by the default mode's level launches, without next0, duo or tail.
 */
int enqueue_scale_direct(popsift_hip_ctx* c, int is_f32, int pitch, bool aligned4)
{
    const PyrDesc& pd = c->pd;
    const int      L = pd.L;
    const double   in_bytes = (double)c->in_w * c->in_h * (is_f32 ? 4 : 1);
    Taps           vt;
    memcpy(vt.g, &c->tab.filter[0], sizeof(vt.g)); /* inc[0]: every octave's vertical pass of level 0 */
    int halo0 = c->tab.span[0] - 1;
    for (int o = 0; o < pd.n_oct; o++) halo0 = std::max(halo0, c->dd.span[o] - 1);
    double px_all = 0.0;
    for (int o = 0; o < pd.n_oct; o++) px_all += (double)pd.o[o].w * pd.o[o].h;
    const double lvl_bpp = pd.dog_fly ? 8.0 : 12.0; /* read plane l-1, write plane l (and DoG l-1) */
    if (c->scale_path == 0) {
        /* level 0: the input image and octave 0's sampling; the kernel takes each octave's plane and taps */
        const BlurArgs a0 = input_args(c, 0, scale_tile_h(), is_f32, pitch, aligned4);
        if (int rc = timed_launch(c, in_bytes + 4.0 * px_all, "k_pyr_level0_octaves", [&] {
                return launch_pyr_level0_octaves(a0, vt, c->d_dd, c->d_pd, pd, c->bd, c->nb, halo0, is_f32, c->stream);
            }))
            return rc;
        for (int l = 1; l < L; l++) {
            BlurArgs a{};
            memcpy(a.taps.g, &c->tab.filter[l * PS_GA], sizeof(a.taps.g));
            const int halo = c->tab.span[l] - 1;
            if (int rc = timed_launch(c, lvl_bpp * px_all, "k_blur_octaves", [&] {
                    return launch_blur_octaves(a, l, c->d_pd, pd, c->bd, c->nb, halo, c->stream);
                }))
                return rc;
        }
        return 0;
    }
    for (int o = 0; o < pd.n_oct; o++) {
        const OctDesc& od = pd.o[o];
        BlurArgs       a = input_args(c, o, scale_tile_h(), is_f32, pitch, aligned4);
        memcpy(a.taps.g, &c->dd.filter[o * PS_GA], sizeof(a.taps.g));
        if (o > 0) {
            a.shift = 0.5f; /* s_pyramid_build.cu:109-114: octave 0's shift only */
            a.fast2x = 0;
            a.zero_words = 0;
        }
        const int halo = std::max(c->tab.span[0], c->dd.span[o]) - 1;
        if (int rc = timed_launch(c, in_bytes + 4.0 * od.w * od.h, "k_blur_tile_sep",
                                  [&] { return launch_blur_level0_sep(a, vt, c->bd, c->nb, halo, is_f32, c->stream); }))
            return rc;
    }
    for (int o = 0; o < pd.n_oct; o++)
        for (int l = 1; l < L; l++) {
            BlurArgs a = level_args(c, o, l);
            a.next0_off = -1;
            if (int rc = blur_launch(c, a, 0, c->tab.span[l], tile_rows(c, pd.o[o].w, pd.o[o].h), lvl_bpp * pd.o[o].w * pd.o[o].h))
                return rc;
        }
    return 0;
}

/*
 * Pyramid::build_pyramid default branch (s_pyramid_build.cu:549-588), one stream, every launch for all images of the
 * batch (gridDim.y).  Launch order:
 *   octave 0: level 0 (from the input image), levels 1 .. L-1;
 *   octave o >= 1: levels 1 .. L-3 (level 0 came with level L-3 of octave o-1); the two last levels of octave o-1
 *   (they feed nothing but detection) ride along with levels 1 and 2 of octave o in ONE launch (k_blur_duo) when both
 *   octaves use 32-row tiles -- 3 instead of 5 dependent launches per small octave;
 *   finally the two last levels of the last octave.
 */
int enqueue_pyramid(popsift_hip_ctx* c, int is_f32, int pitch, bool aligned4)
{
    POPSIFT_RANGE("popsift_hip: pyramid");
    if (c->p.scale_direct) return enqueue_scale_direct(c, is_f32, pitch, aligned4);
    const PyrDesc& pd = c->pd;
    const int      L = pd.L;
    auto single = [&](int o, int level) -> int {
        const BlurArgs a = level_args(c, o, level);
        const double   px = (double)pd.o[o].w * pd.o[o].h;
        /* read plane l-1 once, write plane l (and DoG l-1 when it is stored) once: 8 (12) B / pixel */
        return blur_launch(c, a, 0, c->tab.span[level], tile_rows(c, pd.o[o].w, pd.o[o].h), (pd.dog_fly ? 8.0 : 12.0) * px);
    };
    const bool direct = c->p.gauss_mode == POPSIFT_HIP_GAUSS_VLFEAT_RELATIVE_ALL;
    if (direct) {
        if (int rc = enqueue_direct_octave0(c, is_f32, pitch, aligned4)) return rc;
    } else {
        const OctDesc& od = pd.o[0];
        const int      thd = tile_rows(c, od.w, od.h);
        BlurArgs       a = input_args(c, 0, thd, is_f32, pitch, aligned4);
        memcpy(a.taps.g, &c->tab.filter[0], sizeof(a.taps.g));
        const double bytes = (double)c->in_w * c->in_h * (is_f32 ? 4 : 1) + 4.0 * (double)od.w * od.h;
        if (int rc = blur_launch(c, a, is_f32 ? 2 : 1, c->tab.span[0], thd, bytes)) return rc;
    }
    /* The smallest octaves -- from the first one whose plane fits the LDS of one workgroup -- are built by ONE launch
     * (pyr_tail.hip) instead of three dependent launches per octave; `n_front` octaves take the level launches. */
    int n_front = pd.n_oct;
    TailArgs ta{};
    if (c->pyr_tail != 1 && c->profile != 1 && pd.dog_fly && L <= PYR_TAIL_MAX_L) {
        bool taps_ok = true;
        for (int l = 1; l < L; l++) taps_ok = taps_ok && c->tab.span[l] - 1 <= PYR_TAIL_PAD && c->tab.span[l] >= 2;
        int first = pd.n_oct;
        for (int o = pd.n_oct - 1; o >= 1 && taps_ok && pyr_tail_fits(pd.o[o].w, pd.o[o].h); o--) first = o;
        if (first < pd.n_oct) {
            n_front = first;
            ta.n_oct = pd.n_oct;
            ta.first_oct = first;
            ta.L = L;
            for (int l = 1; l < L; l++) {
                ta.halo[l] = c->tab.span[l] - 1;
                for (int k = 0; k <= PYR_TAIL_PAD; k++) ta.g[l][k] = k < c->tab.span[l] ? c->tab.filter[l * PS_GA + k] : 0.0f;
            }
            for (int o = 0; o < pd.n_oct; o++) {
                ta.w[o] = pd.o[o].w;
                ta.h[o] = pd.o[o].h;
                ta.pitch[o] = pd.o[o].pitch;
                ta.data_off[o] = pd.o[o].data_off;
                ta.plane_stride[o] = pd.o[o].plane_stride;
            }
        }
    }
    for (int level = 1; level < L && !direct; level++)
        if (int rc = single(0, level)) return rc;
    for (int o = 1; o < n_front; o++) {
        /* per-launch profiling keeps one kernel per event pair; BLUR_PATH = 2 sends every plane-to-plane level through
         * the march kernels, so no level of it is paired into k_blur_duo */
        const bool pair = c->profile != 1 && c->blur_tune.path != 2 && o >= 2 && tile_rows(c, pd.o[o].w, pd.o[o].h) == 32 &&
                          tile_rows(c, pd.o[o - 1].w, pd.o[o - 1].h) == 32;
        for (int level = 1; level <= L - 3; level++) {
            const int trail = L - 3 + level; /* L-2, L-1 of the octave before */
            if (pair && level <= 2) {
                const BlurArgs a = level_args(c, o, level), b = level_args(c, o - 1, trail);
                HIP_TRY(c, launch_blur_duo(a, c->tab.span[level], b, c->tab.span[trail], c->bd, c->nb, c->stream));
                SYNC_CHK(c, "k_blur_duo");
            } else {
                if (int rc = single(o, level)) return rc;
                if (!pair && level <= 2 && o >= 2)
                    if (int rc = single(o - 1, trail)) return rc;
            }
        }
    }
    if (n_front < pd.n_oct) {
        /* reads level 0 of octave n_front, which level L-3 of octave n_front - 1 has just written */
        HIP_TRY(c, launch_pyr_tail(ta, c->bd, c->nb, c->stream));
        SYNC_CHK(c, "k_pyr_tail");
    }
    if (n_front >= 2)
        for (int level = L - 2; level < L; level++)
            if (int rc = single(n_front - 1, level)) return rc;
    return 0;
}

/* Pyramid::step2 + prep_features: extrema -> orientation -> scan -> descriptors -> features */
InitExt* final_iext(popsift_hip_ctx* c, int k = 0)
{
    /* frames are neither grid-filtered nor thinned */
    return (c->sc.filter_max > 0 || c->batch_keep > 0) && !c->describe ? c->slot[k].iext2.p : c->slot[k].iext.p;
}

/* POPSIFT_HIP_ORDER_RASTER: the lists `filtered ? iext2 : iext` of the batch into the header's order */
hipError_t enqueue_order(popsift_hip_ctx* c, bool filtered)
{
    OrderBatch ob{};
    for (int k = 0; k < c->nb; k++) {
        const ImageSlot& sl = c->slot[k];
        ob.s[k].list = filtered ? sl.iext2.p : sl.iext.p;
        ob.s[k].tmp = sl.otmp.p;
        ob.s[k].rows = sl.orows.p;
        ob.s[k].ct = c->d_ct + k;
    }
    return launch_order(c->pd, c->sc, c->order_coarse, ob, c->nb, c->stream);
}

/* popsift_hip_set_keep_strongest: the buffers of the pass for the slots of the batch, grown on the first use */
int prepare_strongest(popsift_hip_ctx* c)
{
    const size_t need = std::max<size_t>(c->ext_cap, 1);
    return ensure_cap(c, [&](ImageSlot& s) {
        if (int rc = grow(c, s.iext2, need)) return rc;
        if (int rc = grow(c, s.sresp_in, need)) return rc;
        if (int rc = grow(c, s.sresp, need)) return rc;
        if (int rc = grow(c, s.sstate, 1)) return rc;
        return grow(c, s.schunk, (size_t)PS_MAX_OCT * strongest_chunks(c->sc.max_extrema));
    });
}

/* the pass on the refined (and ordered) lists iext of the batch -> iext2 */
hipError_t enqueue_strongest(popsift_hip_ctx* c)
{
    StrongBatch sb{};
    for (int k = 0; k < c->nb; k++) {
        const ImageSlot& sl = c->slot[k];
        sb.s[k].arena = sl.arena.p;
        sb.s[k].ct = c->d_ct + k;
        sb.s[k].in = sl.iext.p;
        sb.s[k].out = sl.iext2.p;
        sb.s[k].resp_in = sl.sresp_in.p;
        sb.s[k].resp_out = sl.sresp.p;
        sb.s[k].state = sl.sstate.p;
        sb.s[k].chunk_off = sl.schunk.p;
    }
    return launch_strongest(c->pd, c->d_pd, c->sc, c->batch_keep, sb, c->nb, c->stream);
}

/* What extraction and describe end with: orientation -> scan -> descriptors -> the counters to the host, with their stage
 * marks.  lb: the slot table the scan writes its records through; with_ori: k_orientation runs (otherwise
 * the Ext records and the partial sums are there already, k_frame_place); fb: the frames of a describe, whose records
 * k_frame_out moves to caller order after the descriptor kernel, or null. */
int enqueue_descriptor_stages(popsift_hip_ctx* c, const BatchDesc& lb, bool filtered, bool with_ori, const FrameBatch* fb)
{
    const bool stages = (c->profile == 2);
    auto       mark = [&](int k) -> hipError_t { return stages ? hipEventRecord(c->ev_stage[k], c->stream) : hipSuccess; };
    HIP_TRY(c, mark(POPSIFT_HIP_STAGE_ORIENTATION));
    if (with_ori) {
        HIP_TRY(c, launch_orientation(c->d_pd, c->bd, c->nb, c->sc, filtered, (int)c->ohist_cap, c->kp_waves, c->stream));
        SYNC_CHK(c, "k_orientation");
    }
    HIP_TRY(c, mark(POPSIFT_HIP_STAGE_SCAN));
    const int n_chunks = std::max((int)(((size_t)c->pd.n_oct * c->sc.max_extrema + scan_chunk() - 1) / scan_chunk()), 1);
    HIP_TRY(c, launch_scan_apply(c->d_pd, lb, c->nb, c->sc, n_chunks, c->desc_cap, c->stream));
    SYNC_CHK(c, "k_scan_apply");
    HIP_TRY(c, mark(POPSIFT_HIP_STAGE_DESCRIPTOR));
    HIP_TRY(c, launch_descriptors(c->d_pd, c->bd, c->nb, c->sc, c->desc_cap, c->kp_waves, c->stream));
    SYNC_CHK(c, "descriptor kernel");
    if (fb) {
        /* after the descriptor kernel: k_descriptor_grid / _notile read ext + map[d] with the list positions */
        HIP_TRY(c, launch_frame_out(c->bd, *fb, c->nb, c->desc_cap, c->frames_max, c->stream));
        SYNC_CHK(c, "k_frame_out");
    }
    HIP_TRY(c, mark(POPSIFT_HIP_STAGE_COUNT));
    HIP_TRY(c, hipMemcpyAsync(c->h_ct, c->d_ct, sizeof(Counters) * (size_t)c->nb, hipMemcpyDeviceToHost, c->stream));
    return 0;
}

/* counters_cleared: the level-0 launch of this batch has zeroed the counters (submit); re-runs clear them here */
int enqueue_keypoint_stages(popsift_hip_ctx* c, bool counters_cleared = false)
{
    POPSIFT_RANGE("popsift_hip: keypoint stages");
    const bool stages = (c->profile == 2);
    c->batch_keep = c->keep_strongest;
    if (c->batch_keep > 0)
        if (int rc = prepare_strongest(c)) return rc;
    const bool filtered = c->sc.filter_max > 0 || c->batch_keep > 0; /* the later stages read iext2 */
    auto       mark = [&](int k) -> hipError_t { return stages ? hipEventRecord(c->ev_stage[k], c->stream) : hipSuccess; };
    if (!counters_cleared) HIP_TRY(c, hipMemsetAsync(c->d_ct, 0, sizeof(Counters) * (size_t)c->nb, c->stream));
    HIP_TRY(c, mark(POPSIFT_HIP_STAGE_DETECT)); /* = end of the pyramid stage */
    HIP_TRY(c, launch_extrema(c->pd, c->d_pd, c->bd, c->nb, c->sc, c->cand_cap, filtered, c->stream,
                              stages ? c->ev_stage[POPSIFT_HIP_STAGE_REFINE] : nullptr, c->masked ? &c->ma : nullptr));
    SYNC_CHK(c, "k_detect / k_refine");
    const bool raster = c->p.feature_order == POPSIFT_HIP_ORDER_RASTER;
    if (raster) {
        /* before the filter: its tie-break is the list position */
        HIP_TRY(c, enqueue_order(c, false));
        SYNC_CHK(c, "k_order (refined list)");
    }
    if (c->batch_keep > 0) {
        /* stable: a raster-ordered list stays one */
        HIP_TRY(c, enqueue_strongest(c));
        SYNC_CHK(c, "keep-strongest pass");
    }
    if (c->sc.filter_max > 0) {
        /* Pyramid::orientation's filter hook (s_orientation.cu:353-367); the 10 % test is taken on the device */
        HIP_TRY(c, launch_filter(c->pd.n_oct, c->sc, c->bd, c->nb, c->stream));
        SYNC_CHK(c, "grid filter");
        if (raster) {
            /* k_filter_compact appends its chunks by arrival */
            HIP_TRY(c, enqueue_order(c, true));
            SYNC_CHK(c, "k_order (filtered list)");
        }
    }
    return enqueue_descriptor_stages(c, c->bd, filtered, true, nullptr);
}

/* The keypoint stages of a describe (describe.hip): the frames instead of detection and refinement, then orientation (or
 * the given angles) -> scan -> descriptors as for extraction, then the records in caller order.  Re-runs clear the
 * counters here, as enqueue_keypoint_stages does. */
int enqueue_describe_stages(popsift_hip_ctx* c, bool counters_cleared = false)
{
    POPSIFT_RANGE("popsift_hip: describe stages");
    const bool stages = (c->profile == 2);
    auto       mark = [&](int k) -> hipError_t { return stages ? hipEventRecord(c->ev_stage[k], c->stream) : hipSuccess; };
    c->batch_keep = 0; /* frames are never thinned */
    FrameBatch fb{};
    BatchDesc  lb = c->bd; /* k_scan_apply writes its feature records in list order, k_frame_out moves them */
    for (int k = 0; k < c->nb; k++) {
        const ImageSlot& sl = c->slot[k];
        fb.s[k].frames = sl.frames.p;
        fb.s[k].counts = sl.fcounts.p;
        fb.s[k].perm = sl.perm.p;
        fb.s[k].inv = sl.inv.p;
        fb.s[k].lfeats = sl.lfeats.p;
        fb.s[k].n = sl.n_frames;
        lb.s[k].feats = sl.lfeats.p;
    }
    if (!counters_cleared) HIP_TRY(c, hipMemsetAsync(c->d_ct, 0, sizeof(Counters) * (size_t)c->nb, c->stream));
    HIP_TRY(c, mark(POPSIFT_HIP_STAGE_DETECT));
    HIP_TRY(c, mark(POPSIFT_HIP_STAGE_REFINE)); /* no detection: the resolve-and-partition launches take refinement's place */
    HIP_TRY(c, launch_frame_count(c->d_pd, fb, c->nb, c->sc, c->ori_given, c->frames_max, c->stream));
    SYNC_CHK(c, "k_frame_count");
    HIP_TRY(c, launch_frame_place(c->d_pd, c->bd, fb, c->nb, c->sc, c->ori_given, c->frames_max, c->stream));
    SYNC_CHK(c, "k_frame_place");
    return enqueue_descriptor_stages(c, lb, false, !c->ori_given, &fb);
}

/* the frames of a describe (popsift_hip_describe_batch); null for an extraction */
struct DescribeArgs {
    const popsift_hip_frame* const* frames;
    const int*                      n_frames;
    int                             ori_mode;
};

/* per-slot buffers of a describe, grown on first use (the extraction path allocates none of them) */
int prepare_frames(popsift_hip_ctx* c, ImageSlot& s)
{
    const size_t n = (size_t)c->sc.max_extrema;
    if (int rc = grow(c, s.frames, n)) return rc;
    if (int rc = grow(c, s.fcounts, (size_t)PS_MAX_OCT * frame_chunks(c->sc.max_extrema))) return rc;
    if (int rc = grow(c, s.perm, n)) return rc;
    if (int rc = grow(c, s.inv, n)) return rc;
    if (int rc = grow(c, s.lfeats, n)) return rc;
    if (!s.h_frames) HIP_TRY(c, hipHostMalloc((void**)&s.h_frames, n * sizeof(popsift_hip_frame), hipHostMallocDefault));
    return 0;
}

/* the masks of an extraction (popsift_hip_submit_batch_masked), lying where the images lie; null for a plain submit */
struct MaskSubmit {
    const uint8_t* const* masks;
    int                   pitch; /* bytes */
};

/* The masks of the batch into their slots, packed to pitch w, on the context's stream next to the image upload and by the
 * same route as the images: a pageable mask through pinned staging (copied before submit returns), a pinned or device
 * mask from where it lies.  A batch without a mask leaves the context unmasked and touches nothing. */
int upload_masks(popsift_hip_ctx* c, const MaskSubmit& ms, int nb, int where, int w, int h)
{
    const size_t bytes = (size_t)w * h;
    MaskArgs     ma{};
    bool         any = false;
    for (int k = 0; k < nb; k++) {
        const uint8_t* src = ms.masks[k];
        if (!src) continue;
        ImageSlot& s = c->slot[k];
        if (int rc = grow(c, s.mask, bytes)) return rc;
        if (where == 0) {
            if (bytes > s.h_mask_cap) {
                if (s.h_mask) HIP_TRY(c, hipHostFree(s.h_mask));
                s.h_mask = nullptr;
                s.h_mask_cap = 0;
                HIP_TRY(c, hipHostMalloc(&s.h_mask, bytes, hipHostMallocDefault));
                s.h_mask_cap = bytes;
            }
            for (int y = 0; y < h; y++) memcpy((char*)s.h_mask + (size_t)y * w, src + (size_t)y * ms.pitch, (size_t)w);
            HIP_TRY(c, hipMemcpyAsync(s.mask.p, s.h_mask, bytes, hipMemcpyHostToDevice, c->stream));
        } else {
            HIP_TRY(c, hipMemcpy2DAsync(s.mask.p, (size_t)w, src, (size_t)ms.pitch, (size_t)w, (size_t)h,
                                        where == 1 ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
        }
        ma.m[k] = s.mask.p;
        any = true;
    }
    ma.w = w;
    ma.h = h;
    ma.pitch = w;
    ma.up = c->sc.up_fac_int;
    c->ma = ma;
    c->masked = any;
    return 0;
}

/* where the images of a batch lie: kind = POPSIFT_HIP_IMG_* */
int submit_common(popsift_hip_ctx* c, const void* const* imgs, int nb, int kind, int w, int h, int pitch,
                  const DescribeArgs* da = nullptr, const MaskSubmit* ms = nullptr)
{
    if (!c) return POPSIFT_HIP_ERR_INVALID;
    POPSIFT_RANGE("popsift_hip: submit");
    if (!imgs || nb < 1 || nb > PS_MAX_BATCH || w <= 0 || h <= 0 || pitch < w || kind < 0 || kind > POPSIFT_HIP_IMG_PINNED_F32)
        return fail(c, POPSIFT_HIP_ERR_INVALID, "bad image arguments");
    for (int k = 0; k < nb; k++)
        if (!imgs[k]) return fail(c, POPSIFT_HIP_ERR_INVALID, "bad image arguments");
    for (int k = 0; k < nb && ms; k++)
        if (ms->masks[k] && ms->pitch < w) return fail(c, POPSIFT_HIP_ERR_INVALID, "mask_pitch %d below the width %d", ms->pitch, w);
    const int is_f32 = kind & 1, where = kind >> 1; /* 0 host, 1 device, 2 pinned host */
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->have_image && !c->finished) {
        /* one batch in flight per context: drain the previous one */
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    /* from here until every enqueue below has succeeded the context holds NO results: a submit that fails half-way (an
     * allocation for a new slot of a larger batch of the same size, a pinned staging buffer, a launch) must not leave
     * wait / fetch with the previous batch's counts for slots whose kernels never ran */
    c->batch_ok = false;
    c->finished = false;
    c->masked = false; /* a plain submit and a describe clear the masks of the submit before */
    if (int rc = prepare_geometry(c, w, h, nb)) return rc;
    c->nb = nb;
    refresh_caps(c);
    const size_t esz = is_f32 ? 4 : 1;
    int          dpitch = pitch;
    bool         aligned4 = (pitch & 3) == 0;
    for (int k = 0; k < nb; k++) {
        ImageSlot& s = c->slot[k];
        if (where == 1) {
            c->bd.s[k].input = imgs[k];
            aligned4 = aligned4 && ((uintptr_t)imgs[k] & 3) == 0;
            continue;
        }
        const size_t bytes = (size_t)w * h * esz;
        if (int rc = grow(c, s.input, bytes)) return rc;
        if (where == 2) {
            /* page-locked memory of the caller, valid until wait(): uploaded from where it lies */
            HIP_TRY(c, hipMemcpy2DAsync(s.input.p, (size_t)w * esz, imgs[k], (size_t)pitch * esz, (size_t)w * esz, (size_t)h,
                                        hipMemcpyHostToDevice, c->stream));
        } else {
            /* Like Image::load (s_image.cu:71-79) the caller's buffer is copied into pinned memory before
             * this call returns: the caller may free or reuse it immediately (popsift.cpp:245-247), and an
             * async copy straight from pageable memory would read it later. */
            if (bytes > s.h_input_cap) {
                if (s.h_input) HIP_TRY(c, hipHostFree(s.h_input));
                s.h_input = nullptr;
                s.h_input_cap = 0;
                HIP_TRY(c, hipHostMalloc(&s.h_input, bytes, hipHostMallocDefault));
                s.h_input_cap = bytes;
            }
            for (int y = 0; y < h; y++)
                memcpy((char*)s.h_input + (size_t)y * w * esz, (const char*)imgs[k] + (size_t)y * pitch * esz, (size_t)w * esz);
            HIP_TRY(c, hipMemcpyAsync(s.input.p, s.h_input, bytes, hipMemcpyHostToDevice, c->stream));
        }
        c->bd.s[k].input = s.input.p;
        dpitch = w;
    }
    if (where != 1) aligned4 = (dpitch & 3) == 0; /* hipMalloc'd buffers are aligned */
    if (ms)
        if (int rc = upload_masks(c, *ms, nb, where, w, h)) return rc;
    c->describe = da != nullptr;
    c->ori_given = da && da->ori_mode == POPSIFT_HIP_ORI_GIVEN;
    c->frames_max = 0;
    for (int k = 0; k < nb && da; k++) {
        /* like the images, the caller's frames are copied into pinned memory before this call returns */
        ImageSlot& s = c->slot[k];
        if (int rc = prepare_frames(c, s)) return rc;
        const int nf = da->n_frames[k];
        s.n_frames = nf;
        c->frames_max = std::max(c->frames_max, nf);
        if (nf > 0) {
            memcpy(s.h_frames, da->frames[k], (size_t)nf * sizeof(popsift_hip_frame));
            HIP_TRY(c, hipMemcpyAsync(s.frames.p, s.h_frames, (size_t)nf * sizeof(popsift_hip_frame), hipMemcpyHostToDevice, c->stream));
        }
    }
    c->blur_events_used = 0;
    HIP_TRY(c, hipEventRecord(c->ev_begin, c->stream));
    if (c->profile == 2) HIP_TRY(c, hipEventRecord(c->ev_stage[POPSIFT_HIP_STAGE_PYRAMID], c->stream));
    if (int rc = enqueue_pyramid(c, is_f32, dpitch, aligned4)) return rc;
    if (int rc = da ? enqueue_describe_stages(c, true) : enqueue_keypoint_stages(c, true)) return rc;
    HIP_TRY(c, hipEventRecord(c->ev_end, c->stream));
    c->have_image = true;
    c->finished = false;
    c->batch_ok = true;
    c->submit_seq++;
    for (ImageSlot& sl : c->slot) sl.moved = false;
    return 0;
}

int finish(popsift_hip_ctx* c)
{
    if (!c->have_image || !c->batch_ok) return fail(c, POPSIFT_HIP_ERR_STATE, c->have_image ? "the last submit failed" : "no image submitted");
    if (c->finished) return 0;
    POPSIFT_RANGE("popsift_hip: wait");
    HIP_TRY(c, hipSetDevice(c->device));
    bool rerun = false, fits = false;
    for (int attempt = 0; attempt < 8; attempt++) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        /* the largest need over the images of the batch */
        int  ori_max = 0, qmax = 0;
        long ext_max = 0;
        for (int k = 0; k < c->nb; k++) {
            const Counters& h = c->h_ct[k];
            ori_max = std::max(ori_max, h.ori_total);
            for (int q = 0; q < DET_SUBQ; q++) qmax = std::max(qmax, h.qcnt[q].n);
            long ext_sum = 0; /* ext_total is written by the scan, which may have run on a clipped list: recount */
            for (int o = 0; o < c->pd.n_oct; o++) ext_sum += ext_count(&h, c->sc.max_extrema, o);
            ext_max = std::max(ext_max, ext_sum);
        }
        const bool desc_short = ori_max > c->desc_cap;
        const bool cand_short = qmax > c->cand_cap / DET_SUBQ;
        const bool hist_short = (size_t)ext_max > c->ohist_cap && !c->ori_given; /* given angles need no histograms */
        if (!desc_short && !cand_short && !hist_short) {
            fits = true;
            break;
        }
        /* more candidates / descriptors than the buffers hold (the reference reallocates between
         * stages, sift_pyramid.cu:179-209): grow and redo the keypoint stages of this batch */
        if (desc_short)
            if (int rc = ensure_cap(c, [&](ImageSlot& s) { return slot_desc_cap(c, s, ori_max + ori_max / 8 + 1024); }))
                return rc;
        if (cand_short)
            if (int rc = ensure_cap(c, [&](ImageSlot& s) { return grow(c, s.cand, DET_SUBQ * (qmax + qmax / 8 + 64)); }))
                return rc;
        if (hist_short) c->ohist_cap = std::max(c->ohist_cap, (size_t)ext_max + (size_t)ext_max / 8 + 1024);
        if (int rc = c->describe ? enqueue_describe_stages(c) : enqueue_keypoint_stages(c)) return rc;
        HIP_TRY(c, hipEventRecord(c->ev_end, c->stream));
        rerun = true;
    }
    /* every re-run sizes the buffers from the counts of the run before, so the second attempt fits unless the counts
     * themselves were clipped; eight rounds of growing without fitting is a defect, not a result to hand out clipped */
    if (!fits) return fail(c, POPSIFT_HIP_ERR_DEVICE, "the keypoint buffers still do not fit after 8 grow-and-rerun rounds");
    popsift_hip_report& r = c->rep;
    for (int k = 0; k < c->nb; k++) {
        c->n_feat[k] = c->describe ? c->slot[k].n_frames : c->h_ct[k].ext_total; /* describe: one record per frame */
        c->n_desc[k] = std::min(c->h_ct[k].ori_total, c->desc_cap);
    }
    /* the report describes image 0 of the batch: per-octave descriptor counts from the octave start offsets the scan
     * left (dct.ori_ps / ori_ct) */
    Counters& h0 = c->h_ct[0];
    int       next = h0.ori_total;
    for (int o = PS_MAX_OCT - 1; o >= 0; o--) {
        if (h0.ext_ct[o] > 0) {
            h0.ori_ct[o] = next - h0.ori_ps[o];
            next = h0.ori_ps[o];
        } else {
            h0.ori_ct[o] = 0;
            h0.ori_ps[o] = next;
        }
    }
    for (int o = 0; o < PS_MAX_OCT; o++) {
        r.ext_ct[o] = h0.ext_ct[o];
        r.ori_ct[o] = h0.ori_ct[o];
    }
    r.ext_total = c->h_ct[0].ext_total; /* describe: the valid frames */
    r.ori_total = c->n_desc[0];
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, c->ev_begin, c->ev_end) == hipSuccess) r.ms_device = ms;
    for (int k = 0; k < 8; k++) r.ms_stage[k] = 0.0f;
    /* after a re-run the stage events of the keypoint stages are the re-run's and the pyramid's event pair spans the
     * first attempt as well: no stage times then */
    if (c->profile == 2 && !rerun)
        for (int k = 0; k < POPSIFT_HIP_STAGE_COUNT; k++) {
            float t = 0.0f;
            if (hipEventElapsedTime(&t, c->ev_stage[k], c->ev_stage[k + 1]) == hipSuccess) r.ms_stage[k] = t;
        }
    r.ms_blur = 0.0f;
    r.blur_launches = 0;
    r.blur_alg_bytes = 0.0;
    r.ms_big = 0.0f;
    r.big_launches = 0;
    r.big_alg_bytes = 0.0;
    for (size_t i = 0; i < c->blur_events_used; i++) {
        float t = 0.0f;
        if (hipEventElapsedTime(&t, c->blur_events[i].a, c->blur_events[i].b) == hipSuccess) {
            t /= (float)PROFILE_REPS;
            r.ms_blur += t;
            r.blur_launches++;
            r.blur_alg_bytes += c->blur_events[i].bytes;
            if (c->blur_events[i].big) {
                r.ms_big += t;
                r.big_launches++;
                r.big_alg_bytes += c->blur_events[i].bytes;
            }
        }
    }
    c->finished = true;
    return 0;
}

/* waits for the download popsift_hip_fetch_begin started, if one is pending */
int drain_copy(popsift_hip_ctx* c)
{
    if (!c->copy_pending) return 0;
    c->copy_pending = false;
    HIP_TRY(c, hipStreamSynchronize(c->copy_stream));
    return 0;
}

/* results of the finished batch are readable from the current slabs (not yet handed to fetch_begin) */
int results_here(popsift_hip_ctx* c, int k = 0)
{
    if (int rc = finish(c)) return rc;
    if (k < 0 || k >= c->nb) return fail(c, POPSIFT_HIP_ERR_INVALID, "the batch has %d images", c->nb);
    if (c->slot[k].moved)
        return fail(c, POPSIFT_HIP_ERR_STATE, "the results of this image were handed to popsift_hip_fetch_begin");
    return 0;
}

/* The first n descriptors of a slot as bytes in its desc_u8, by a pass on the compute stream.  The buffer is sized for the
 * slab first, before anything is issued; a writer also waits for a pending fetch_begin*_u8 download that still reads the
 * buffer (the state of that download is left as it is: fetch_end still completes it). */
int slot_bytes(popsift_hip_ctx* c, ImageSlot& sl, int n)
{
    if (sl.u8_read && c->copy_pending) HIP_TRY(c, hipStreamSynchronize(c->copy_stream));
    sl.u8_read = false;
    if (int rc = grow(c, sl.desc_u8, std::max<size_t>(sl.desc_cap(), 1))) return rc;
    if (n > 0) {
        HIP_TRY(c, launch_desc_bytes(sl.desc.p, n, sl.desc_u8.p, c->stream));
        SYNC_CHK(c, "k_desc_bytes");
    }
    return 0;
}

/* What the blocking and the overlapped fetch share: the argument checks, then `prepare` (whatever the caller has to wait
 * for or allocate), then image k's records and its descriptors -- floats, or the bytes of slot_bytes -- on their way to
 * caller memory by copies on stream s.  s is read after prepare, where fetch_begin makes its stream. */
template <typename F>
int fetch_issue(popsift_hip_ctx* c, int k, popsift_hip_feature* feats, size_t feats_cap, void* desc, size_t desc_cap, bool u8,
                const hipStream_t& s, F prepare)
{
    const size_t nf = (size_t)c->n_feat[k], nd = (size_t)c->n_desc[k];
    if ((nf && !feats) || (nd && !desc)) return fail(c, POPSIFT_HIP_ERR_INVALID, "null output buffer");
    if (feats_cap < nf || desc_cap < nd * 128) return fail(c, POPSIFT_HIP_ERR_TOO_SMALL, "output buffer too small");
    HIP_TRY(c, hipSetDevice(c->device));
    ImageSlot& sl = c->slot[k];
    if (int rc = prepare(sl)) return rc;
    /* Bytes: the pass runs on the compute stream -- idle now, and ahead of the next submit's kernels -- and a byte copy
     * on another stream waits for it.  On the copy stream the pass would queue behind other contexts' kernels on a shared
     * hardware queue (keypoint-sparse host to host 6.7-7.4 instead of 9.4-9.5 Gpix/s). */
    const bool apart = u8 && nd && s != c->stream;
    if (u8 && nd)
        if (int rc = slot_bytes(c, sl, (int)nd)) return rc;
    if (apart) HIP_TRY(c, hipEventRecord(c->ev_u8, c->stream));
    if (nf) HIP_TRY(c, hipMemcpyAsync(feats, sl.feats.p, nf * sizeof(popsift_hip_feature), hipMemcpyDeviceToHost, s));
    if (apart) HIP_TRY(c, hipStreamWaitEvent(s, c->ev_u8, 0));
    if (nd && u8) HIP_TRY(c, hipMemcpyAsync(desc, sl.desc_u8.p, nd * 128, hipMemcpyDeviceToHost, s));
    if (nd && !u8) HIP_TRY(c, hipMemcpyAsync(desc, sl.desc.p, nd * 128 * sizeof(float), hipMemcpyDeviceToHost, s));
    return 0;
}

/* image k's results into caller memory, descriptors as floats (u8 = false) or as bytes, on the compute stream */
int fetch_sync(popsift_hip_ctx* c, int k, popsift_hip_feature* feats, size_t feats_cap, void* desc, size_t desc_cap, bool u8)
{
    if (int rc = fetch_issue(c, k, feats, feats_cap, desc, desc_cap, u8, c->stream, [](ImageSlot&) { return 0; })) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
}

/* popsift_hip_fetch_begin_item(_u8) */
int fetch_begin(popsift_hip_ctx* c, int k, popsift_hip_feature* feats, size_t feats_cap, void* desc, size_t desc_cap, bool u8)
{
    auto prepare = [&](ImageSlot& sl) -> int {
        /* the other slabs may still be the source of the downloads of the batch before this one */
        if (c->copy_pending && c->copy_seq != c->submit_seq)
            if (int rc = drain_copy(c)) return rc;
        /* The copy stream is made on first use: the runtime deals its few hardware queues to streams in the order they
         * are created, so a second stream in EVERY context -- used or not -- takes queues from the streams that do the work
         * (four active contexts next to sixteen idle ones: 7.8 -> 6.5 Gpix/s on the sparse workload). */
        if (!c->copy_stream) HIP_TRY(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        /* Nothing has been issued or swapped yet: a failed allocation leaves the results where they are (plain fetch works).
         * That holds for the byte buffer too: slot_bytes, the first to issue anything, grows it before its launch. */
        if (int rc = grow(c, sl.alt_feats, sl.feats.cap)) return rc;
        if (int rc = grow(c, sl.alt_desc, sl.desc_cap())) return rc;
        if (u8 && c->n_desc[k] && !c->ev_u8) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_u8, hipEventDisableTiming));
        return 0;
    };
    /* finish() has synchronised the compute stream: the slab is complete, and copy_stream needs no event to wait on.  A
     * byte pass reads the slab that becomes alt_desc below, which the next batch does not write. */
    if (int rc = fetch_issue(c, k, feats, feats_cap, desc, desc_cap, u8, c->copy_stream, prepare)) return rc;
    ImageSlot& sl = c->slot[k];
    if (u8 && c->n_desc[k]) sl.u8_read = true;
    std::swap(sl.feats, sl.alt_feats);
    std::swap(sl.desc, sl.alt_desc); /* both hold desc_cap() descriptors now; map / rot / drec stay with the slot */
    refresh_caps(c);
    c->copy_pending = true;
    c->copy_seq = c->submit_seq;
    sl.moved = true;
    return 0;
}

/* planes of image 0 of the batch (debug / parity hooks) */
int plane_ptr(popsift_hip_ctx* c, int octave, int kind, int level, float** p, const OctDesc** odp)
{
    if (!c || !c->have_image) return POPSIFT_HIP_ERR_STATE;
    if (octave < 0 || octave >= c->pd.n_oct || level < 0) return fail(c, POPSIFT_HIP_ERR_INVALID, "bad octave/level");
    const OctDesc& od = c->pd.o[octave];
    float*         arena = c->slot[0].arena.p;
    if (kind == 0 && level < c->L)
        *p = arena + od.data_off + level * od.plane_stride;
    else if (kind == 1 && level < c->L - 1)
        *p = arena + od.dog_off + (c->pd.dog_fly ? 0 : level * od.plane_stride); /* not stored: the scratch plane */
    else
        return fail(c, POPSIFT_HIP_ERR_INVALID, "bad plane kind/level");
    *odp = &od;
    return 0;
}

}  // namespace

extern "C" {

void popsift_hip_default_params(popsift_hip_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->octaves = -1;
    p->levels = 3;
    p->sigma = 1.6f;
    p->edge_limit = 10.0f;
    p->threshold = 0.04f;
    p->upscale_factor = 1.0f;
    p->sift_mode = POPSIFT_HIP_SIFT_POPSIFT;
    p->gauss_mode = POPSIFT_HIP_GAUSS_VLFEAT_COMPUTE;
    p->desc_mode = POPSIFT_HIP_DESC_LOOP;
    p->norm_mode = POPSIFT_HIP_NORM_ROOTSIFT;
    p->norm_multi = 0;
    p->max_extrema = 100000;
    p->assume_initial_blur = 1;
    p->initial_blur = 0.5f;
    p->filter_grid_size = 2;
    p->filter_max_extrema = -1;
    p->filter_sorting = POPSIFT_HIP_FILTER_RANDOM;
}

const char* popsift_hip_version(void) { return "popsift_hip 0.1 (gfx950, wave64)"; }

const char* popsift_hip_strerror(int status)
{
    switch (status) {
    case POPSIFT_HIP_OK: return "ok";
    case POPSIFT_HIP_ERR_INVALID: return "invalid argument or unsupported mode";
    case POPSIFT_HIP_ERR_DEVICE: return "HIP runtime error";
    case POPSIFT_HIP_ERR_NO_DEVICE: return "no usable GPU";
    case POPSIFT_HIP_ERR_OOM: return "out of memory";
    case POPSIFT_HIP_ERR_STATE: return "call sequence error";
    case POPSIFT_HIP_ERR_TOO_SMALL: return "buffer too small";
    }
    return "unknown status";
}

const char* popsift_hip_last_error(const popsift_hip_ctx* ctx) { return ctx ? ctx->err : ""; }

int popsift_hip_device_count(int* count)
{
    if (!count) return POPSIFT_HIP_ERR_INVALID;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        *count = 0;
        return POPSIFT_HIP_ERR_NO_DEVICE;
    }
    *count = n;
    return n > 0 ? POPSIFT_HIP_OK : POPSIFT_HIP_ERR_NO_DEVICE;
}

int popsift_hip_get_device_info(int device, popsift_hip_device_info* out)
{
    if (!out) return POPSIFT_HIP_ERR_INVALID;
    if (int rc = check_device(device)) return rc;
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    memset(out, 0, sizeof(*out));
    snprintf(out->name, sizeof(out->name), "%s (%s)", pr.name, pr.gcnArchName);
    out->arch_major = pr.major;
    out->arch_minor = pr.minor;
    out->total_mem = pr.totalGlobalMem;
    out->lds_per_block = pr.sharedMemPerBlock;
    out->wave_size = pr.warpSize;
    out->max_threads_per_block = pr.maxThreadsPerBlock;
    out->max_threads_per_cu = pr.maxThreadsPerMultiProcessor;
    for (int i = 0; i < 3; i++) {
        out->max_block[i] = pr.maxThreadsDim[i];
        out->max_grid[i] = pr.maxGridSize[i];
    }
    out->cu_count = pr.multiProcessorCount;
    out->concurrent_kernels = pr.concurrentKernels;
    out->can_map_host = pr.canMapHostMemory;
    out->unified_addressing = 1; /* HIP on ROCm: one virtual address space for host and device */
    return POPSIFT_HIP_OK;
}

int popsift_hip_device_numa_node(int device, int* node)
{
    if (!node) return POPSIFT_HIP_ERR_INVALID;
    *node = -1;
    if (int rc = check_device(device)) return rc;
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) != hipSuccess) return POPSIFT_HIP_ERR_DEVICE;
    for (char* q = bus; *q; q++)
        if (*q >= 'A' && *q <= 'F') *q = (char)(*q - 'A' + 'a'); /* sysfs spells the address in lower case */
    char path[160];
    snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bus);
    if (FILE* f = fopen(path, "r")) {
        int v = -1;
        if (fscanf(f, "%d", &v) == 1) *node = v;
        fclose(f);
    }
    return POPSIFT_HIP_OK;
}

/* the parameter ranges a context accepts */
static int check_params(const popsift_hip_params* p)
{
    /* gauss_filter.cu:131-144: sigma > 2 or too many levels is fatal in the reference */
    if (!(p->sigma > 0.0f) || p->sigma > 2.0f) return POPSIFT_HIP_ERR_INVALID;
    if (p->levels > POPSIFT_HIP_MAX_LEVELS - 3) return POPSIFT_HIP_ERR_INVALID;
    if (p->gauss_mode != POPSIFT_HIP_GAUSS_VLFEAT_COMPUTE && p->gauss_mode != POPSIFT_HIP_GAUSS_VLFEAT_RELATIVE_ALL &&
        p->gauss_mode != POPSIFT_HIP_GAUSS_OPENCV_COMPUTE)
        return POPSIFT_HIP_ERR_INVALID;
    if (p->desc_mode < POPSIFT_HIP_DESC_LOOP || p->desc_mode > POPSIFT_HIP_DESC_NOTILE) return POPSIFT_HIP_ERR_INVALID;
    if (p->sift_mode < 0 || p->sift_mode > 2 || p->norm_mode < 0 || p->norm_mode > 1) return POPSIFT_HIP_ERR_INVALID;
    if (p->max_extrema < 1 || !(p->edge_limit > 0.0f)) return POPSIFT_HIP_ERR_INVALID;
    if (p->filter_max_extrema > 0 &&
        (p->filter_grid_size < 1 || p->filter_grid_size > 64 || p->filter_sorting < 0 || p->filter_sorting > 2))
        return POPSIFT_HIP_ERR_INVALID;
    if (p->scale_direct != 0 && p->scale_direct != 1) return POPSIFT_HIP_ERR_INVALID;
    if (p->feature_order != POPSIFT_HIP_ORDER_ARRIVAL && p->feature_order != POPSIFT_HIP_ORDER_RASTER)
        return POPSIFT_HIP_ERR_INVALID;
    return POPSIFT_HIP_OK;
}

int popsift_hip_plan_arena(const popsift_hip_params* p, int w, int h, int* n_octaves, int64_t* arena_bytes)
{
    if (!p || w < 1 || h < 1) return POPSIFT_HIP_ERR_INVALID;
    if (int rc = check_params(p)) return rc;
    const int   levels = std::max(2, p->levels);
    PyrDesc     pd;
    size_t      total = 0;
    int         bw, bh;
    const char* why = plan_pyramid(*p, levels, levels + 3, p->octaves, w, h, &pd, &total, &bw, &bh);
    if (n_octaves) *n_octaves = pd.n_oct;
    if (arena_bytes) *arena_bytes = (int64_t)(total * sizeof(float));
    return why ? POPSIFT_HIP_ERR_INVALID : POPSIFT_HIP_OK;
}

int popsift_hip_ctx_create(int device, const popsift_hip_params* p, popsift_hip_ctx** out)
{
    if (!p || !out) return POPSIFT_HIP_ERR_INVALID;
    *out = nullptr;
    if (int rc = check_params(p)) return rc;
    if (int rc = check_device(device)) return rc;

    popsift_hip_ctx* c = new (std::nothrow) popsift_hip_ctx();
    if (!c) return POPSIFT_HIP_ERR_OOM;
    c->device = device;
    c->p = *p;
    c->levels = std::max(2, p->levels); /* popsift.cpp:71 */
    c->L = c->levels + 3;
    c->frozen_octaves = p->octaves;
    init_tables(c);
    int rc = [&]() -> int {
        HIP_TRY(c, hipSetDevice(device));
        {
            int cus = 0;
            HIP_TRY(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
            c->kp_waves = std::max(cus, 8) * 32 * 8; /* a multiple of 32 */
        }
        HIP_TRY(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        HIP_TRY(c, hipEventCreate(&c->ev_begin));
        HIP_TRY(c, hipEventCreate(&c->ev_end));
        for (int k = 0; k <= POPSIFT_HIP_STAGE_COUNT; k++) HIP_TRY(c, hipEventCreate(&c->ev_stage[k]));
        HIP_TRY(c, hipMalloc((void**)&c->d_ct, sizeof(Counters) * PS_MAX_BATCH));
        HIP_TRY(c, hipMalloc((void**)&c->d_pd, sizeof(PyrDesc)));
        HIP_TRY(c, hipHostMalloc((void**)&c->h_pd, sizeof(PyrDesc), hipHostMallocDefault));
        HIP_TRY(c, hipHostMalloc((void**)&c->h_ct, sizeof(Counters) * PS_MAX_BATCH, hipHostMallocDefault));
        memset(c->h_ct, 0, sizeof(Counters) * PS_MAX_BATCH);
        if (c->p.gauss_mode == POPSIFT_HIP_GAUSS_VLFEAT_RELATIVE_ALL) {
            const size_t bytes = sizeof(float) * (size_t)c->L * PS_GA;
            HIP_TRY(c, hipMalloc((void**)&c->d_abs0, bytes));
            HIP_TRY(c, hipMemcpy(c->d_abs0, c->abs0.filter, bytes, hipMemcpyHostToDevice));
        }
        if (c->p.scale_direct) {
            HIP_TRY(c, hipMalloc((void**)&c->d_dd, sizeof(c->dd.filter)));
            HIP_TRY(c, hipMemcpy(c->d_dd, c->dd.filter, sizeof(c->dd.filter), hipMemcpyHostToDevice));
        }
        return 0;
    }();
    if (rc) {
        popsift_hip_ctx_destroy(c);
        return rc;
    }
    *out = c;
    return POPSIFT_HIP_OK;
}

int popsift_hip_ctx_destroy(popsift_hip_ctx* c)
{
    if (!c) return POPSIFT_HIP_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    for (auto& ep : c->blur_events) {
        (void)hipEventDestroy(ep.a);
        (void)hipEventDestroy(ep.b);
    }
    for (int k = 0; k <= POPSIFT_HIP_STAGE_COUNT; k++)
        if (c->ev_stage[k]) (void)hipEventDestroy(c->ev_stage[k]);
    if (c->ev_begin) (void)hipEventDestroy(c->ev_begin);
    if (c->ev_end) (void)hipEventDestroy(c->ev_end);
    for (ImageSlot& sl : c->slot) sl.release();
    if (c->d_ct) (void)hipFree(c->d_ct);
    if (c->d_pd) (void)hipFree(c->d_pd);
    if (c->d_abs0) (void)hipFree(c->d_abs0);
    if (c->d_dd) (void)hipFree(c->d_dd);
    if (c->h_pd) (void)hipHostFree(c->h_pd);
    if (c->h_ct) (void)hipHostFree(c->h_ct);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->ev_u8) (void)hipEventDestroy(c->ev_u8);
    delete c;
    return POPSIFT_HIP_OK;
}

int popsift_hip_get_gauss_table(const popsift_hip_ctx* c, float* filter, int* span, float* sigma, int* n_levels)
{
    if (!c) return POPSIFT_HIP_ERR_INVALID;
    if (filter) memcpy(filter, c->tab.filter, sizeof(float) * (size_t)c->L * PS_GA);
    if (span) memcpy(span, c->tab.span, sizeof(int) * (size_t)c->L);
    if (sigma) memcpy(sigma, c->tab.sigma, sizeof(float) * (size_t)c->L);
    if (n_levels) *n_levels = c->L;
    return POPSIFT_HIP_OK;
}

int popsift_hip_get_gauss_table_abs0(const popsift_hip_ctx* c, float* filter, int* span, float* sigma, int* n_levels)
{
    if (!c) return POPSIFT_HIP_ERR_INVALID;
    if (c->p.gauss_mode != POPSIFT_HIP_GAUSS_VLFEAT_RELATIVE_ALL)
        return fail(const_cast<popsift_hip_ctx*>(c), POPSIFT_HIP_ERR_STATE, "the abs_o0 table exists in the vlfeat-direct Gauss mode only");
    if (filter) memcpy(filter, c->abs0.filter, sizeof(float) * (size_t)c->L * PS_GA);
    if (span) memcpy(span, c->abs0.span, sizeof(int) * (size_t)c->L);
    if (sigma) memcpy(sigma, c->abs0.sigma, sizeof(float) * (size_t)c->L);
    if (n_levels) *n_levels = c->L;
    return POPSIFT_HIP_OK;
}

int popsift_hip_get_gauss_table_dd(const popsift_hip_ctx* c, float* filter, int* span, float* sigma, int* n_octaves)
{
    if (!c) return POPSIFT_HIP_ERR_INVALID;
    if (!c->p.scale_direct)
        return fail(const_cast<popsift_hip_ctx*>(c), POPSIFT_HIP_ERR_STATE, "the dd table exists in the ScaleDirect scaling mode only");
    /* the octaves of the context: fixed by params.octaves or by the first image; all MAX_OCTAVES rows before that */
    const int n = c->frozen_octaves > 0 ? std::min(c->frozen_octaves, (int)POPSIFT_HIP_MAX_OCTAVES) : POPSIFT_HIP_MAX_OCTAVES;
    if (filter) memcpy(filter, c->dd.filter, sizeof(float) * (size_t)n * PS_GA);
    if (span) memcpy(span, c->dd.span, sizeof(int) * (size_t)n);
    if (sigma) memcpy(sigma, c->dd.sigma, sizeof(float) * (size_t)n);
    if (n_octaves) *n_octaves = n;
    return POPSIFT_HIP_OK;
}

int popsift_hip_submit_u8(popsift_hip_ctx* c, const uint8_t* img, int w, int h, int pitch)
{
    const void* one = img;
    return submit_common(c, &one, 1, POPSIFT_HIP_IMG_HOST_U8, w, h, pitch);
}
int popsift_hip_submit_f32(popsift_hip_ctx* c, const float* img, int w, int h, int pitch)
{
    const void* one = img;
    return submit_common(c, &one, 1, POPSIFT_HIP_IMG_HOST_F32, w, h, pitch);
}
int popsift_hip_submit_pinned_u8(popsift_hip_ctx* c, const uint8_t* img, int w, int h, int pitch)
{
    const void* one = img;
    return submit_common(c, &one, 1, POPSIFT_HIP_IMG_PINNED_U8, w, h, pitch);
}
int popsift_hip_submit_pinned_f32(popsift_hip_ctx* c, const float* img, int w, int h, int pitch)
{
    const void* one = img;
    return submit_common(c, &one, 1, POPSIFT_HIP_IMG_PINNED_F32, w, h, pitch);
}
int popsift_hip_submit_dev_u8(popsift_hip_ctx* c, const void* d_img, int w, int h, int pitch)
{
    return submit_common(c, &d_img, 1, POPSIFT_HIP_IMG_DEV_U8, w, h, pitch);
}
int popsift_hip_submit_dev_f32(popsift_hip_ctx* c, const void* d_img, int w, int h, int pitch)
{
    return submit_common(c, &d_img, 1, POPSIFT_HIP_IMG_DEV_F32, w, h, pitch);
}
int popsift_hip_submit_batch(popsift_hip_ctx* c, const void* const* imgs, int n, int kind, int w, int h, int pitch)
{
    return submit_common(c, imgs, n, kind, w, h, pitch);
}

int popsift_hip_submit_batch_masked(popsift_hip_ctx* c, const void* const* imgs, const uint8_t* const* masks, int n, int kind,
                                    int w, int h, int pitch, int mask_pitch)
{
    if (!c) return POPSIFT_HIP_ERR_INVALID;
    if (!masks) return fail(c, POPSIFT_HIP_ERR_INVALID, "null mask list: use popsift_hip_submit_batch");
    const MaskSubmit ms{masks, mask_pitch};
    return submit_common(c, imgs, n, kind, w, h, pitch, nullptr, &ms);
}

int popsift_hip_describe_batch(popsift_hip_ctx* c, const void* const* imgs, const popsift_hip_frame* const* frames,
                               const int* n_frames, int n, int kind, int w, int h, int pitch, int ori_mode)
{
    if (!c) return POPSIFT_HIP_ERR_INVALID;
    if (n < 1 || n > PS_MAX_BATCH || !n_frames || !frames) return fail(c, POPSIFT_HIP_ERR_INVALID, "bad frame arguments");
    if (ori_mode != POPSIFT_HIP_ORI_COMPUTE && ori_mode != POPSIFT_HIP_ORI_GIVEN)
        return fail(c, POPSIFT_HIP_ERR_INVALID, "ori_mode: POPSIFT_HIP_ORI_COMPUTE or POPSIFT_HIP_ORI_GIVEN");
    for (int k = 0; k < n; k++) {
        if (n_frames[k] < 0 || (n_frames[k] > 0 && !frames[k])) return fail(c, POPSIFT_HIP_ERR_INVALID, "bad frame list %d", k);
        /* so that no octave's list can overflow */
        if (n_frames[k] > c->sc.max_extrema)
            return fail(c, POPSIFT_HIP_ERR_INVALID, "%d frames for image %d: more than max_extrema (%d)", n_frames[k], k,
                        c->sc.max_extrema);
    }
    const DescribeArgs da{frames, n_frames, ori_mode};
    return submit_common(c, imgs, n, kind, w, h, pitch, &da);
}

int popsift_hip_wait_batch(popsift_hip_ctx* c, int* n_images, int* n_features, int* n_descriptors)
{
    if (!c) return POPSIFT_HIP_ERR_INVALID;
    if (int rc = finish(c)) return rc;
    if (n_images) *n_images = c->nb;
    for (int k = 0; k < c->nb; k++) {
        if (n_features) n_features[k] = c->n_feat[k];
        if (n_descriptors) n_descriptors[k] = c->n_desc[k];
    }
    return POPSIFT_HIP_OK;
}

int popsift_hip_fetch_item(popsift_hip_ctx* c, int k, popsift_hip_feature* feats, size_t feats_cap, float* desc, size_t desc_cap)
{
    if (!c) return POPSIFT_HIP_ERR_INVALID;
    if (int rc = results_here(c, k)) return rc;
    POPSIFT_RANGE("popsift_hip: fetch");
    return fetch_sync(c, k, feats, feats_cap, desc, desc_cap, false);
}

int popsift_hip_fetch_item_u8(popsift_hip_ctx* c, int k, popsift_hip_feature* feats, size_t feats_cap, uint8_t* desc,
                              size_t desc_cap)
{
    if (!c) return POPSIFT_HIP_ERR_INVALID;
    if (int rc = results_here(c, k)) return rc;
    POPSIFT_RANGE("popsift_hip: fetch_u8");
    return fetch_sync(c, k, feats, feats_cap, desc, desc_cap, true);
}

int popsift_hip_results_dev_item(popsift_hip_ctx* c, int k, const void** d_feats, const void** d_desc)
{
    if (!c) return POPSIFT_HIP_ERR_INVALID;
    if (int rc = results_here(c, k)) return rc;
    if (d_feats) *d_feats = c->slot[k].feats.p;
    if (d_desc) *d_desc = c->slot[k].desc.p;
    return POPSIFT_HIP_OK;
}

int popsift_hip_results_dev_item_u8(popsift_hip_ctx* c, int k, const void** d_feats, const void** d_desc_u8)
{
    if (!c) return POPSIFT_HIP_ERR_INVALID;
    if (int rc = results_here(c, k)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    ImageSlot& sl = c->slot[k];
    if (int rc = slot_bytes(c, sl, c->n_desc[k])) return rc;
    if (c->n_desc[k] > 0) HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (d_feats) *d_feats = sl.feats.p;
    if (d_desc_u8) *d_desc_u8 = sl.desc_u8.p;
    return POPSIFT_HIP_OK;
}

/* The single-image calls are the batch calls for image 0 (finish() sets the report's ori_total from n_desc[0]). */

int popsift_hip_wait(popsift_hip_ctx* c, int* n_features, int* n_descriptors)
{
    if (!c) return POPSIFT_HIP_ERR_INVALID;
    if (int rc = finish(c)) return rc;
    if (n_features) *n_features = c->n_feat[0];
    if (n_descriptors) *n_descriptors = c->n_desc[0];
    return POPSIFT_HIP_OK;
}

int popsift_hip_fetch(popsift_hip_ctx* c, popsift_hip_feature* feats, size_t feats_cap, float* desc, size_t desc_cap)
{
    return popsift_hip_fetch_item(c, 0, feats, feats_cap, desc, desc_cap);
}

int popsift_hip_fetch_u8(popsift_hip_ctx* c, popsift_hip_feature* feats, size_t feats_cap, uint8_t* desc, size_t desc_cap)
{
    return popsift_hip_fetch_item_u8(c, 0, feats, feats_cap, desc, desc_cap);
}

int popsift_hip_fetch_begin_item(popsift_hip_ctx* c, int k, popsift_hip_feature* feats, size_t feats_cap, float* desc,
                                 size_t desc_cap)
{
    if (!c) return POPSIFT_HIP_ERR_INVALID;
    if (int rc = results_here(c, k)) return rc;
    POPSIFT_RANGE("popsift_hip: fetch_begin");
    return fetch_begin(c, k, feats, feats_cap, desc, desc_cap, false);
}

int popsift_hip_fetch_begin_item_u8(popsift_hip_ctx* c, int k, popsift_hip_feature* feats, size_t feats_cap, uint8_t* desc,
                                    size_t desc_cap)
{
    if (!c) return POPSIFT_HIP_ERR_INVALID;
    if (int rc = results_here(c, k)) return rc;
    POPSIFT_RANGE("popsift_hip: fetch_begin_u8");
    return fetch_begin(c, k, feats, feats_cap, desc, desc_cap, true);
}

int popsift_hip_fetch_begin(popsift_hip_ctx* c, popsift_hip_feature* feats, size_t feats_cap, float* desc, size_t desc_cap)
{
    return popsift_hip_fetch_begin_item(c, 0, feats, feats_cap, desc, desc_cap);
}

int popsift_hip_fetch_begin_u8(popsift_hip_ctx* c, popsift_hip_feature* feats, size_t feats_cap, uint8_t* desc, size_t desc_cap)
{
    return popsift_hip_fetch_begin_item_u8(c, 0, feats, feats_cap, desc, desc_cap);
}

int popsift_hip_fetch_end(popsift_hip_ctx* c)
{
    if (!c) return POPSIFT_HIP_ERR_INVALID;
    POPSIFT_RANGE("popsift_hip: fetch_end");
    if (!c->copy_pending) return fail(c, POPSIFT_HIP_ERR_STATE, "no download was started with popsift_hip_fetch_begin");
    HIP_TRY(c, hipSetDevice(c->device));
    return drain_copy(c);
}

int popsift_hip_results_dev(popsift_hip_ctx* c, const void** d_feats, const void** d_desc)
{
    return popsift_hip_results_dev_item(c, 0, d_feats, d_desc);
}

/* ------------------------------------------------------------------ MatchingMode (N3): a finished image as a set (sets.hip) */

int popsift_hip_clone_results(popsift_hip_ctx* c, popsift_hip_devfeatures** out)
{
    if (!c || !out) return POPSIFT_HIP_ERR_INVALID;
    *out = nullptr;
    if (int rc = results_here(c)) return rc;
    const ImageSlot&         sl = c->slot[0];
    const int                nf = c->n_feat[0], nd = c->n_desc[0];
    popsift_hip_devfeatures* f = nullptr;
    if (int rc = devfeatures_new(c->device, nf, nd, &f)) return fail(c, rc, "cannot allocate the set: %s", popsift_hip_strerror(rc));
    return hand_over([&]() -> int {
        /* sift_pyramid.cu:323-345: prep_features into the clone, then the two device-to-device copies */
        HIP_TRY(c, launch_clone_features(sl.feats.p, nf, f->d_desc, f->d_feat, c->stream));
        if (nd > 0) {
            HIP_TRY(c, hipMemcpyAsync(f->d_desc, sl.desc.p, sizeof(float) * 128 * (size_t)nd, hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(f->d_rev, sl.map.p, sizeof(int) * (size_t)nd, hipMemcpyDeviceToDevice, c->stream));
        }
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return 0;
    }(), f, out);
}

int popsift_hip_clone_results_u8(popsift_hip_ctx* c, int k, popsift_hip_bytefeatures** out)
{
    if (!c || !out) return POPSIFT_HIP_ERR_INVALID;
    *out = nullptr;
    if (int rc = results_here(c, k)) return rc;
    ImageSlot&                sl = c->slot[k];
    const int                 n = c->n_desc[k];
    popsift_hip_bytefeatures* f = nullptr;
    if (int rc = bytefeatures_new(c->device, n, &f)) return fail(c, rc, "cannot allocate the byte set: %s", popsift_hip_strerror(rc));
    return hand_over([&]() -> int {
        if (n == 0) return 0;
        /* the bytes the byte fetch calls deliver: the slot's byte buffer, then device to device */
        if (int e = slot_bytes(c, sl, n)) return e;
        HIP_TRY(c, hipMemcpyAsync(f->d_desc, sl.desc_u8.p, (size_t)128 * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(f->d_rev, sl.map.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return 0;
    }(), f, out);
}

void* popsift_hip_host_alloc(size_t bytes)
{
    void* p = nullptr;
    if (bytes == 0) return nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) return nullptr;
    return p;
}

void popsift_hip_host_free(void* p)
{
    if (p) (void)hipHostFree(p);
}

int popsift_hip_get_report(const popsift_hip_ctx* c, popsift_hip_report* rep)
{
    if (!c || !rep) return POPSIFT_HIP_ERR_INVALID;
    *rep = c->rep;
    return POPSIFT_HIP_OK;
}

int popsift_hip_set_profile(popsift_hip_ctx* c, int profile)
{
    if (!c) return POPSIFT_HIP_ERR_INVALID;
    c->profile = (profile == 2) ? 2 : (profile ? 1 : 0);
    return POPSIFT_HIP_OK;
}

int popsift_hip_set_keep_strongest(popsift_hip_ctx* c, int n)
{
    if (!c) return POPSIFT_HIP_ERR_INVALID;
    if (n < 0) return fail(c, POPSIFT_HIP_ERR_INVALID, "keep_strongest: 0 (off) or a positive count");
    if (c->sc.filter_max > 0)
        return fail(c, POPSIFT_HIP_ERR_INVALID, "keep_strongest and the grid filter (filter_max_extrema > 0) do not chain");
    if (c->have_image && c->batch_ok && !c->finished) return fail(c, POPSIFT_HIP_ERR_STATE, "a batch is in flight");
    c->keep_strongest = n;
    return POPSIFT_HIP_OK;
}

int popsift_hip_responses_dev_item(popsift_hip_ctx* c, int k, const void** d_resp)
{
    if (!c) return POPSIFT_HIP_ERR_INVALID;
    if (int rc = results_here(c, k)) return rc;
    if (c->describe || c->batch_keep <= 0)
        return fail(c, POPSIFT_HIP_ERR_STATE, "no responses: the batch was not run with popsift_hip_set_keep_strongest on");
    if (d_resp) *d_resp = c->slot[k].sresp.p;
    return POPSIFT_HIP_OK;
}

int popsift_hip_fetch_responses_item(popsift_hip_ctx* c, int k, float* out, size_t cap)
{
    const void* d_resp = nullptr;
    if (int rc = popsift_hip_responses_dev_item(c, k, &d_resp)) return rc;
    const size_t nf = (size_t)c->n_feat[k];
    if (nf && !out) return fail(c, POPSIFT_HIP_ERR_INVALID, "null output buffer");
    if (cap < nf) return fail(c, POPSIFT_HIP_ERR_TOO_SMALL, "output buffer too small");
    HIP_TRY(c, hipSetDevice(c->device));
    if (nf) HIP_TRY(c, hipMemcpy(out, d_resp, nf * sizeof(float), hipMemcpyDeviceToHost));
    return POPSIFT_HIP_OK;
}

int popsift_hip_octave_dims(const popsift_hip_ctx* c, int octave, int* w, int* h)
{
    if (!c || !c->have_image || octave < 0 || octave >= c->pd.n_oct) return POPSIFT_HIP_ERR_INVALID;
    if (w) *w = c->pd.o[octave].w;
    if (h) *h = c->pd.o[octave].h;
    return POPSIFT_HIP_OK;
}

int popsift_hip_download_plane(popsift_hip_ctx* c, int octave, int kind, int level, float* out)
{
    float*         p = nullptr;
    const OctDesc* od = nullptr;
    if (!out) return POPSIFT_HIP_ERR_INVALID;
    if (int rc = plane_ptr(c, octave, kind, level, &p, &od)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if (kind == 1 && c->pd.dog_fly) /* not stored: DoG(l) = G(l+1) - G(l) into the (otherwise unused) DoG plane */
        HIP_TRY(c, launch_dog_plane(p, c->slot[0].arena.p + od->data_off + (level + 1) * od->plane_stride,
                                    c->slot[0].arena.p + od->data_off + level * od->plane_stride, (size_t)od->plane_stride, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy2D(out, (size_t)od->w * 4, p, (size_t)od->pitch * 4, (size_t)od->w * 4, od->h,
                           hipMemcpyDeviceToHost));
    return POPSIFT_HIP_OK;
}

int popsift_hip_upload_plane(popsift_hip_ctx* c, int octave, int kind, int level, const float* in)
{
    float*         p = nullptr;
    const OctDesc* od = nullptr;
    if (!in) return POPSIFT_HIP_ERR_INVALID;
    if (c && c->have_image && kind == 1 && c->pd.dog_fly)
        return fail(c, POPSIFT_HIP_ERR_STATE, "DoG planes are not stored (params.store_dog = 0): upload Gaussian planes");
    if (int rc = plane_ptr(c, octave, kind, level, &p, &od)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy2D(p, (size_t)od->pitch * 4, in, (size_t)od->w * 4, (size_t)od->w * 4, od->h,
                           hipMemcpyHostToDevice));
    return POPSIFT_HIP_OK;
}

int popsift_hip_download_extrema(popsift_hip_ctx* c, popsift_hip_extremum* out, size_t cap, int* n)
{
    if (!c) return POPSIFT_HIP_ERR_INVALID;
    if (int rc = finish(c)) return rc;
    const int total = c->rep.ext_total;
    if (n) *n = total;
    if (!out) return POPSIFT_HIP_OK;
    if (cap < (size_t)total) return fail(c, POPSIFT_HIP_ERR_TOO_SMALL, "output buffer too small");
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<InitExt> tmp((size_t)std::max(c->sc.max_extrema, 1));
    size_t               k = 0;
    for (int o = 0; o < c->pd.n_oct; o++) {
        const int cnt = c->rep.ext_ct[o];
        if (cnt <= 0) continue;
        HIP_TRY(c, hipMemcpy(tmp.data(), final_iext(c) + (size_t)o * c->sc.max_extrema, (size_t)cnt * sizeof(InitExt),
                             hipMemcpyDeviceToHost));
        for (int i = 0; i < cnt; i++, k++) {
            out[k].xpos = tmp[i].xpos;
            out[k].ypos = tmp[i].ypos;
            out[k].lpos = tmp[i].lpos;
            out[k].sigma = tmp[i].sigma;
            out[k].octave = o;
            out[k].cell = tmp[i].cell;
        }
    }
    return POPSIFT_HIP_OK;
}

int popsift_hip_debug_set(popsift_hip_ctx* c, int what, int value)
{
    if (!c) return POPSIFT_HIP_ERR_INVALID;
    switch (what) {
    case POPSIFT_HIP_DEBUG_DET_QCAP:
        c->det_qcap = c->sc.det_qcap = std::max(value, 0);
        return POPSIFT_HIP_OK;
    case POPSIFT_HIP_DEBUG_CAND_CAP:
        c->cand_cap_init = std::max(value, DET_SUBQ);
        c->cand_cap_user = true;
        return POPSIFT_HIP_OK;
    case POPSIFT_HIP_DEBUG_OHIST_CAP:
        c->ohist_cap_init = std::max(value, 1);
        return POPSIFT_HIP_OK;
    case POPSIFT_HIP_DEBUG_DESC_CAP:
        c->desc_cap_init = std::max(value, 0);
        return POPSIFT_HIP_OK;
    case POPSIFT_HIP_DEBUG_FAIL_ALLOC:
        c->fail_alloc_in = std::max(value, 0);
        return POPSIFT_HIP_OK;
    case POPSIFT_HIP_DEBUG_KP_WAVES:
        c->kp_waves = std::min(std::max(value / 32 * 32, 32), 1 << 20);
        return POPSIFT_HIP_OK;
    case POPSIFT_HIP_DEBUG_BLUR_PATH:
        if (value < 0 || value > 2) return fail(c, POPSIFT_HIP_ERR_INVALID, "BLUR_PATH: 0, 1 or 2");
        c->blur_tune.path = value;
        return POPSIFT_HIP_OK;
    case POPSIFT_HIP_DEBUG_BLUR_SEG:
        c->blur_tune.seg_rows = std::max(value, 0);
        return POPSIFT_HIP_OK;
    case POPSIFT_HIP_DEBUG_BLUR_TILE_H:
        if (value != 0 && value != 32 && value != 64) return fail(c, POPSIFT_HIP_ERR_INVALID, "BLUR_TILE_H: 0, 32 or 64");
        c->blur_tune.tile_h = value;
        return POPSIFT_HIP_OK;
    case POPSIFT_HIP_DEBUG_PYR_TAIL:
        c->pyr_tail = value;
        return POPSIFT_HIP_OK;
    case POPSIFT_HIP_DEBUG_DESC_ROWS:
        c->desc_rows = c->sc.desc_rows = std::max(value, 4);
        return POPSIFT_HIP_OK;
    case POPSIFT_HIP_DEBUG_DESC_LIST:
        c->desc_list = c->sc.desc_list = std::max(value, 64);
        return POPSIFT_HIP_OK;
    case POPSIFT_HIP_DEBUG_DIRECT_PATH:
        if (value < 0 || value > 1) return fail(c, POPSIFT_HIP_ERR_INVALID, "DIRECT_PATH: 0 or 1");
        c->direct_path = value;
        return POPSIFT_HIP_OK;
    case POPSIFT_HIP_DEBUG_SCALE_PATH:
        if (value < 0 || value > 1) return fail(c, POPSIFT_HIP_ERR_INVALID, "SCALE_PATH: 0 or 1");
        c->scale_path = value;
        return POPSIFT_HIP_OK;
    case POPSIFT_HIP_DEBUG_ORDER_COARSE:
        if (value < 0 || value > 15) return fail(c, POPSIFT_HIP_ERR_INVALID, "ORDER_COARSE: 0 .. 15");
        c->order_coarse = value;
        return POPSIFT_HIP_OK;
    }
    return fail(c, POPSIFT_HIP_ERR_INVALID, "unknown debug switch %d", what);
}

int popsift_hip_rerun_keypoint_stages(popsift_hip_ctx* c)
{
    if (!c) return POPSIFT_HIP_ERR_INVALID;
    if (!c->have_image || !c->batch_ok) return fail(c, POPSIFT_HIP_ERR_STATE, "no image submitted");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    /* a download started by fetch_begin may still read the slab the re-run is about to write (the slabs were swapped and
     * `moved` is cleared below without a new submit_seq): wait for it first */
    if (int rc = drain_copy(c)) return rc;
    c->blur_events_used = 0;
    HIP_TRY(c, hipEventRecord(c->ev_begin, c->stream));
    if (int rc = c->describe ? enqueue_describe_stages(c) : enqueue_keypoint_stages(c)) return rc;
    HIP_TRY(c, hipEventRecord(c->ev_end, c->stream));
    c->finished = false;
    for (ImageSlot& sl : c->slot) sl.moved = false;
    return POPSIFT_HIP_OK;
}

} /* extern "C" */
