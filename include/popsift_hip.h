/*
 * popsift_hip.h -- thin C ABI between the C++ host layer (libpopsift) and the
 * HIP/CDNA4 SIFT extraction kernels (libpopsift_hip.so).
 *
 * The reference (10183308/popsift) has no FFI: its boundary is the C++ class API
 * (popsift.h:40-167).  BASELINE.json's north_star asks for "the C++ host ...
 * calling HIP through a thin C-ABI"; SURVEY.md section 8(b) lists the entry points.
 * Each function below cites the reference member function(s) it replaces.
 *
 * Conventions: every function returns 0 on success and a negative
 * popsift_hip_status on failure; no C++ types, no exceptions, no torch types.
 * A context is owned by one host thread at a time; distinct contexts (also on
 * the same device) are fully independent (the reference's process-global
 * counters, sift_pyramid.cu:38-49, do not exist here).
 */
#ifndef POPSIFT_HIP_H
#define POPSIFT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POPSIFT_HIP_MAX_OCTAVES 20 /* sift_conf.h:13 MAX_OCTAVES */
#define POPSIFT_HIP_MAX_LEVELS 12  /* sift_constants.h:35 GAUSS_LEVELS */
#define POPSIFT_HIP_MAX_BATCH 16   /* images of one size a context extracts per submit (popsift_hip_submit_batch) */
#define POPSIFT_HIP_GAUSS_ALIGN 32 /* sift_constants.h:34 GAUSS_ALIGN */
#define POPSIFT_HIP_ORI_MAX 4      /* sift_constants.h:51 ORIENTATION_MAX_COUNT */

typedef enum popsift_hip_status {
    POPSIFT_HIP_OK = 0,
    POPSIFT_HIP_ERR_INVALID = -1,     /* bad argument / unsupported mode        */
    POPSIFT_HIP_ERR_DEVICE = -2,      /* a HIP runtime call failed              */
    POPSIFT_HIP_ERR_NO_DEVICE = -3,   /* no usable GPU                          */
    POPSIFT_HIP_ERR_OOM = -4,         /* host or device allocation failed       */
    POPSIFT_HIP_ERR_STATE = -5,       /* call sequence error (e.g. fetch first) */
    POPSIFT_HIP_ERR_TOO_SMALL = -6    /* caller buffer too small                */
} popsift_hip_status;

/* enum values follow the declaration order in sift_conf.h:32-72 */
enum { POPSIFT_HIP_SIFT_POPSIFT = 0, POPSIFT_HIP_SIFT_OPENCV = 1, POPSIFT_HIP_SIFT_VLFEAT = 2 };
enum { POPSIFT_HIP_GAUSS_VLFEAT_COMPUTE = 0, POPSIFT_HIP_GAUSS_VLFEAT_RELATIVE = 1,
       POPSIFT_HIP_GAUSS_VLFEAT_RELATIVE_ALL = 2, POPSIFT_HIP_GAUSS_OPENCV_COMPUTE = 3,
       POPSIFT_HIP_GAUSS_FIXED9 = 4, POPSIFT_HIP_GAUSS_FIXED15 = 5 };
enum { POPSIFT_HIP_DESC_LOOP = 0, POPSIFT_HIP_DESC_ILOOP = 1, POPSIFT_HIP_DESC_GRID = 2,
       POPSIFT_HIP_DESC_IGRID = 3, POPSIFT_HIP_DESC_NOTILE = 4 };
enum { POPSIFT_HIP_NORM_ROOTSIFT = 0, POPSIFT_HIP_NORM_CLASSIC = 1 };
/* Config::GridFilterMode (sift_conf.h:68-72): which extrema of an over-full cell survive */
enum { POPSIFT_HIP_FILTER_RANDOM = 0, POPSIFT_HIP_FILTER_LARGEST_FIRST = 1, POPSIFT_HIP_FILTER_SMALLEST_FIRST = 2 };

/* Flattened popsift::Config (sift_conf.h:28-310, defaults sift_conf.cu:17-39). */
typedef struct popsift_hip_params {
    int32_t octaves;             /* -1 = auto (popsift.cpp:107-111)            */
    int32_t levels;              /* DoG search levels, clamped to >= 2         */
    float   sigma;               /* 1.6                                        */
    float   edge_limit;          /* 10                                         */
    float   threshold;           /* Config::_threshold, 0.04                   */
    float   upscale_factor;      /* +1 => input stretched by 2                 */
    int32_t sift_mode;           /* POPSIFT_HIP_SIFT_*                         */
    int32_t gauss_mode;          /* POPSIFT_HIP_GAUSS_*                        */
    int32_t desc_mode;           /* POPSIFT_HIP_DESC_*                         */
    int32_t norm_mode;           /* POPSIFT_HIP_NORM_*                         */
    int32_t norm_multi;          /* descriptor *= 2^norm_multi                 */
    int32_t max_extrema;         /* per octave, 100000                         */
    int32_t assume_initial_blur; /* 1                                          */
    float   initial_blur;        /* 0.5                                        */
    int32_t filter_grid_size;    /* 2: the grid filter works on size x size cells */
    int32_t filter_max_extrema;  /* -1 = grid filter off (s_orientation.cu:362)  */
    int32_t filter_sorting;      /* POPSIFT_HIP_FILTER_*                         */
    int32_t store_dog;           /* 0 (default): DoG planes are formed on the fly by their consumers (bit-identical);
                                  * 1: stored as the reference does (s_pyramid_build.cu:74-92), for stage tests     */
    int32_t scale_direct;        /* Config::ScalingMode: 0 (default) ScaleDefault, level 0 of octave o >= 1 is every second
                                  * pixel of level L-3 of octave o-1; 1 ScaleDirect, every octave's level 0 is blurred
                                  * straight from the input image (popsift_hip_get_gauss_table_dd).  Not Config's enum
                                  * values: a zeroed struct keeps the default.  ScaleDirect takes Gauss modes 0, 2, 3. */
    int32_t feature_order;       /* POPSIFT_HIP_ORDER_*: 0 (default, a zeroed struct) arrival order, 1 raster order; see below */
} popsift_hip_params;

/*
 * Feature order.  An extraction always returns the same keypoints, orientations and descriptors; feature_order says in
 * which ORDER.  Features are octave-major in both modes, and within an octave they follow the octave's list of refined
 * extrema (popsift_hip_download_extrema): feature records, descriptor slabs, byte descriptors, cloned sets and their
 * reverse maps all inherit the list order, and the grid filter breaks its ties by list position.
 *
 * POPSIFT_HIP_ORDER_ARRIVAL: the order in which the refinement workgroups appended their survivors: grouped by image
 * region, different from run to run.
 *
 * POPSIFT_HIP_ORDER_RASTER: the result is a function of (image, params) alone: the same bytes on every run, in every
 * batch slot and with every debug switch.  Within octave o the records (xpos, ypos in octave units, lpos, sigma) are in
 * ascending lexicographic order of the tuple
 *     ( iy, ix, lpos, bits(ypos), bits(xpos), bits(sigma) )
 *   iy = pix(ypos), ix = pix(xpos);  pix(v) = 0 if v is NaN or v <= 0, 32767 if v >= 32767, else (int)v (truncation)
 *   lpos compares as the int32 it is
 *   bits(v) is the float's bit pattern compared as uint32
 * i.e. raster order over the pixels of the octave's grid, then level, then the exact sub-pixel position and scale.
 * Refinement lets through only 0 <= xpos <= w - 1, 0 <= ypos <= h - 1 and 0 <= lpos (NaN fails no comparison, so a
 * degenerate 3 x 3 solve can in principle pass one on: pix() and bits() give it a place all the same, and -0.0 sorts by its
 * bits, after every positive value of the pixel).  For the non-negative finite values bits() orders numerically.  Two
 * records equal under the whole tuple are byte-identical (cell is a function of the position), so their mutual order
 * changes no output byte.  A caller can recompute the tuple from popsift_hip_download_extrema; a feature's xpos is its
 * octave's times a power of two.
 *
 * The grid filter (filter_max_extrema > 0) runs on the ordered list, which makes its (scale, list position) selection --
 * the survivor SET in POPSIFT_HIP_FILTER_RANDOM mode included -- a function of the image; its output is ordered again.
 * popsift_hip_rerun_keypoint_stages and the grow-and-rerun paths of popsift_hip_wait order their lists too.
 * popsift_hip_describe_batch accepts the field and is unchanged: its results are in caller order.
 *
 * The max_extrema cap: when more than max_extrema candidates of an octave survive refinement, which of them are kept is
 * decided by arrival, so the surviving set is run-dependent (their order is still the rule's).  The guarantee holds for
 * octaves whose count stays below the cap; a reported ext_ct[o] == max_extrema (popsift_hip_get_report; counts are
 * clamped to the cap) is the sign that it may not have held.
 *
 * The pass (order.hip) runs between refinement and orientation, and again after the grid filter; a workgroup takes
 * POPSIFT_HIP_ORDER_CHUNK records of a list (stated here for the tests of its edges; results do not depend on it).  A
 * context created with POPSIFT_HIP_ORDER_ARRIVAL allocates and launches nothing for it.  Any other value of feature_order:
 * popsift_hip_ctx_create returns POPSIFT_HIP_ERR_INVALID.
 */
enum { POPSIFT_HIP_ORDER_ARRIVAL = 0, POPSIFT_HIP_ORDER_RASTER = 1 };
#define POPSIFT_HIP_ORDER_CHUNK 1024

/* POD mirror of popsift::Feature (features.h:22-34): the four Descriptor*
 * become indices into the descriptor array (-1 = unused slot). */
typedef struct popsift_hip_feature {
    int32_t debug_octave;
    float   xpos;
    float   ypos;
    float   sigma;
    int32_t num_ori;
    float   orientation[POPSIFT_HIP_ORI_MAX];
    int32_t desc_idx[POPSIFT_HIP_ORI_MAX];
} popsift_hip_feature;

/* Pre-orientation extremum (sift_extremum.h:24-33 InitialExtremum), for stage tests. */
typedef struct popsift_hip_extremum {
    float   xpos;
    float   ypos;
    int32_t lpos;
    float   sigma;
    int32_t octave;
    int32_t cell;
} popsift_hip_extremum;

/* Per-image timing / counter report (device side, HIP events). */
typedef struct popsift_hip_report {
    int32_t num_octaves;
    int32_t base_w, base_h;
    int32_t ext_ct[POPSIFT_HIP_MAX_OCTAVES];
    int32_t ori_ct[POPSIFT_HIP_MAX_OCTAVES];
    int32_t ext_total, ori_total;
    float   ms_device;      /* first kernel -> last kernel of the image          */
    float   ms_blur;        /* sum of blur-level kernel durations (profile mode) */
    int32_t blur_launches;  /* number of blur-level launches (profile mode)      */
    double  blur_alg_bytes; /* algorithmic bytes of those launches               */
    double  pyramid_pixels; /* sum over octaves of w*h                           */
    /* the same three for the 64-row-tile instantiation only (k_blur_tile<HALO,0,64>:
     * the level launches of the large octaves, the dominant kernel of the pipeline) */
    double  big_alg_bytes;
    float   ms_big;
    int32_t big_launches;
    /* profile mode 2: device time of the stages of one image, HIP events on the context's stream between the
     * launches (POPSIFT_HIP_STAGE_*); 0 when not collected */
    float   ms_stage[8];
} popsift_hip_report;
enum { POPSIFT_HIP_STAGE_PYRAMID = 0,     /* every k_blur_tile launch                              */
       POPSIFT_HIP_STAGE_DETECT = 1,      /* k_detect (both passes)                                */
       POPSIFT_HIP_STAGE_REFINE = 2,      /* k_refine (+ grid filter / keep-strongest pass when on) */
       POPSIFT_HIP_STAGE_ORIENTATION = 3, /* k_orientation                                         */
       POPSIFT_HIP_STAGE_SCAN = 4,        /* k_scan_apply                                          */
       POPSIFT_HIP_STAGE_DESCRIPTOR = 5,  /* the descriptor kernel                                 */
       POPSIFT_HIP_STAGE_COUNT = 6 };

typedef struct popsift_hip_ctx popsift_hip_ctx;

/* Fills p with the defaults of popsift::Config::Config() (sift_conf.cu:17-39). */
void popsift_hip_default_params(popsift_hip_params* p);

/* Library / build identification string (static storage). */
const char* popsift_hip_version(void);
const char* popsift_hip_strerror(int status);
/* Message of the last failure on this context (static per-context storage). */
const char* popsift_hip_last_error(const popsift_hip_ctx* ctx);

/* Replaces common/device_prop.cu:23-47 (device enumeration). */
int popsift_hip_device_count(int* count);

/* What device_prop_t::print shows (common/device_prop.cu:39-70), as a POD. */
typedef struct popsift_hip_device_info {
    char     name[256];
    int32_t  arch_major, arch_minor; /* "compute capability" slot: gfx major / minor */
    uint64_t total_mem;              /* bytes of HBM */
    uint64_t lds_per_block;          /* "per-block shared mem" */
    int32_t  wave_size;              /* 64 on CDNA */
    int32_t  max_threads_per_block;
    int32_t  max_threads_per_cu;
    int32_t  max_block[3];
    int32_t  max_grid[3];
    int32_t  cu_count;               /* "number of SM(x)s" */
    int32_t  concurrent_kernels;
    int32_t  can_map_host;
    int32_t  unified_addressing;
} popsift_hip_device_info;
int popsift_hip_get_device_info(int device, popsift_hip_device_info* out);
/* NUMA node the GPU hangs off (from its PCI address, /sys/bus/pci/devices/<id>/numa_node), -1 when the host does not
 * say.  The C++ layer binds each worker thread to that node's CPUs, so that the staging copy of the image and the
 * pinned result blocks the worker allocates are node-local; no counterpart in the single-GPU
 * reference. */
int popsift_hip_device_numa_node(int device, int* node);

/* What the pyramid of a w x h image takes under params p, answered without a device: the octaves it gets and the bytes
 * of one image's plane arena (a batch has one arena per image).  POPSIFT_HIP_ERR_INVALID for parameters a context would
 * refuse and for an image a submit would refuse: empty after scaling, a side above 32767 pixels after scaling, or an
 * arena of 4 GiB or more (the detection kernels address the arena with unsigned 32-bit byte offsets); the two outputs
 * are still filled in where the sizes could be formed.  Either output may be NULL. */
int popsift_hip_plan_arena(const popsift_hip_params* p, int w, int h, int* n_octaves, int64_t* arena_bytes);

/* Replaces PopSift::configure (popsift.cpp:63-87: init_filter + init_constants)
 * and Pyramid::Pyramid (sift_pyramid.cu:108-165); buffers are sized lazily on
 * the first image and only grow (contrast sift_octave.cu:55-89). */
int popsift_hip_ctx_create(int device, const popsift_hip_params* p, popsift_hip_ctx** out);
/* Replaces PopSift::uninit / Pyramid::~Pyramid (popsift.cpp:122-137). */
int popsift_hip_ctx_destroy(popsift_hip_ctx* ctx);

/* Gauss tables as uploaded to the device (gauss_filter.cu:127-257), for KATs:
 * filter[(levels+3) * 32], span[levels+3], sigma[levels+3]. */
int popsift_hip_get_gauss_table(const popsift_hip_ctx* ctx, float* filter, int* span, float* sigma,
                                int* n_levels);
/* The abs_o0 table of the vlfeat-direct Gauss mode (POPSIFT_HIP_GAUSS_VLFEAT_RELATIVE_ALL, gauss_filter.cu:190-199):
 * octave 0's level l is blurred straight from the input image with row l.  Same layout as above; ERR_STATE in the other
 * modes. */
int popsift_hip_get_gauss_table_abs0(const popsift_hip_ctx* ctx, float* filter, int* span, float* sigma,
                                     int* n_levels);
/* The dd table of the ScaleDirect scaling mode (params.scale_direct = 1, gauss_filter.cu:217-236): octave o's level 0 is
 * the input image sampled at octave o's size, blurred horizontally with row o and vertically with row 0 of the
 * incremental table; row 0 equals that row.  Same layout as above with one row per octave of the context (fixed by
 * params.octaves or the first image; POPSIFT_HIP_MAX_OCTAVES rows before that); ERR_STATE with scale_direct = 0. */
int popsift_hip_get_gauss_table_dd(const popsift_hip_ctx* ctx, float* filter, int* span, float* sigma,
                                   int* n_octaves);

/* Replaces Image::load + Pyramid::step1 + step2 (s_image.cu:71-79,
 * sift_pyramid.cu:226-239): upload one host image and enqueue the whole
 * extraction asynchronously on the context's stream.  pitch in elements.
 * u8 values are 0..255, f32 values are [0,1) (popsift.h:108-116). */
int popsift_hip_submit_u8(popsift_hip_ctx* ctx, const uint8_t* img, int w, int h, int pitch);
int popsift_hip_submit_f32(popsift_hip_ctx* ctx, const float* img, int w, int h, int pitch);
/* Same for an image in page-locked host memory (popsift_hip_host_alloc): it is uploaded straight from there, without
 * the staging copy Image::load makes (s_image.cu:71-79), so the caller keeps it valid and unchanged until
 * popsift_hip_wait has returned for this image.  PopSift::enqueue's one copy of the caller's image lands in such a
 * block (popsift.cpp:245-247 makes that copy too, and the upload thread a second one). */
int popsift_hip_submit_pinned_u8(popsift_hip_ctx* ctx, const uint8_t* img, int w, int h, int pitch);
int popsift_hip_submit_pinned_f32(popsift_hip_ctx* ctx, const float* img, int w, int h, int pitch);
/* Same, image already resident in this device's memory (bench "inputs in HBM"). */
int popsift_hip_submit_dev_u8(popsift_hip_ctx* ctx, const void* d_img, int w, int h, int pitch);
int popsift_hip_submit_dev_f32(popsift_hip_ctx* ctx, const void* d_img, int w, int h, int pitch);

/*
 * Several images of ONE size per submit (round 3).  The reference's demo enqueues all its images and then collects all
 * the results (src/application/main.cpp:304-326) while its pipeline still extracts them one by one
 * (popsift.cpp:139-213); here up to POPSIFT_HIP_MAX_BATCH images go through the per-image launch sequence TOGETHER --
 * every kernel is launched once for the whole batch, image index in blockIdx.y -- so the latency-bound launches of the
 * small octaves, refinement and the scans are paid once per batch.  Every image has its own planes, lists and result
 * slabs: its results are bit-identical to a submit of its own, whatever it is batched with
 * (tests/test_gpu_batch.py).  kind says where the images lie and what they hold; pointers, w, h, pitch as for the
 * single-image calls above, which are batches of one.  The slots of a context are allocated on first use and kept.
 */
enum { POPSIFT_HIP_IMG_HOST_U8 = 0, POPSIFT_HIP_IMG_HOST_F32 = 1, POPSIFT_HIP_IMG_DEV_U8 = 2, POPSIFT_HIP_IMG_DEV_F32 = 3,
       POPSIFT_HIP_IMG_PINNED_U8 = 4, POPSIFT_HIP_IMG_PINNED_F32 = 5 };
int popsift_hip_submit_batch(popsift_hip_ctx* ctx, const void* const* imgs, int n, int kind, int w, int h, int pitch);
/* blocks until the batch is finished; n_features / n_descriptors: arrays of at least *n_images (= the n submitted) */
int popsift_hip_wait_batch(popsift_hip_ctx* ctx, int* n_images, int* n_features, int* n_descriptors);
/* results of image k of the finished batch (popsift_hip_fetch / popsift_hip_results_dev are k = 0) */
int popsift_hip_fetch_item(popsift_hip_ctx* ctx, int k, popsift_hip_feature* feats, size_t feats_cap, float* desc,
                           size_t desc_cap);
int popsift_hip_results_dev_item(popsift_hip_ctx* ctx, int k, const void** d_feats, const void** d_desc);
/* popsift_hip_fetch_begin (below) for image k of the finished batch: call it for every image whose results are wanted,
 * submit the next batch, then ONE popsift_hip_fetch_end waits for all the downloads */
int popsift_hip_fetch_begin_item(popsift_hip_ctx* ctx, int k, popsift_hip_feature* feats, size_t feats_cap, float* desc,
                                 size_t desc_cap);

/*
 * Extraction masks: keep only the keypoints on visible pixels (OpenCV's detectAndCompute(image, mask, ..), the per-image
 * masks of COLMAP and AliceVision).  The mask acts inside refinement (k_refine, extrema.hip), so a hidden keypoint costs no
 * list slot, no orientation and no descriptor, and max_extrema, keep-strongest and the grid filter are spent on the visible
 * area only.
 *
 * A mask is a w x h array of uint8_t, the size of the input image, with a row pitch of its own in bytes (mask_pitch >= w).
 *
 * For a refined record of octave o at (xpos, ypos) in octave units:
 *
 *     x  = xpos * 2^(o - up),  y = ypos * 2^(o - up)     up = (int)upscale_factor
 *          -- the floats popsift_hip_feature reports for it, bit for bit
 *          -- (keypoint.hip, prep_features; a power-of-two product is exact)
 *     mx = (int)fminf(fmaxf(floorf(x + 0.5f), 0.0f), (float)(w - 1))
 *     my = (int)fminf(fmaxf(floorf(y + 0.5f), 0.0f), (float)(h - 1))
 *     visible = mask[my * mask_pitch + mx] != 0
 *
 * - This is OpenCV's KeyPointsFilter::runByPixelsMask rule, (int)(pt + 0.5f).
 * - The clamp is done on floats, as strongest.hip does, so every input has a defined pixel.  NaN goes to 0 and +inf to the
 *   last column or row.
 * - A caller can recompute the rule from the feature record alone.
 * - A record that is not visible is dropped inside refinement, before it takes a list slot.
 * - Counters::ext_ct[o] counts visible records only.  The max_extrema cap is spent on visible records only.
 * - A NULL mask for an image means every pixel is visible.
 *
 * Consequences:
 * 1. With POPSIFT_HIP_ORDER_RASTER, and no octave's count of ALL refined records reaching the cap, a masked run's results
 *    are byte for byte those of the unmasked run with the hidden records removed and desc_idx renumbered.  That covers
 *    extrema, features, descriptors, byte descriptors, responses and report counts.  It is the statement
 *    popsift_hip_set_keep_strongest makes below.
 * 2. With a cap the unmasked run hits, the masked run still returns every visible record, as long as the visible count of
 *    each octave stays below the cap.
 * 3. An all-non-zero mask returns the unmasked bytes.
 * 4. An all-zero mask returns 0 features and POPSIFT_HIP_OK.
 *
 * popsift_hip_submit_batch_masked: imgs, n, kind, w, h, pitch as in popsift_hip_submit_batch.  masks[k] lies where kind says
 * image k lies: pageable host memory, copied before return; pinned host memory, valid until the wait returns; device memory
 * of the context's GPU, valid until the wait returns.  Any masks[k] may be NULL.  ERR_INVALID, before any GPU call:
 * masks == NULL (use popsift_hip_submit_batch), mask_pitch < w while any mask is non-null, and everything the plain submit
 * refuses.  State rules and all result calls are those of popsift_hip_submit_batch.
 *
 * Each slot keeps its own device copy of the mask, w * h bytes packed to pitch w, grown on first use; the copies are made
 * on the context's stream next to the image upload.  A context that never sees a mask allocates and launches nothing more,
 * and a batch in which no image has a mask launches exactly what popsift_hip_submit_batch launches.
 * popsift_hip_rerun_keypoint_stages and the grow-and-rerun paths of popsift_hip_wait apply the masks of the last submit
 * again.  A later plain submit, or a popsift_hip_describe_batch, clears them.  Describe takes no mask: frames are the
 * caller's own.  popsift_hip_plan_arena is unchanged.  Detection is not masked: a candidate can move during refinement.
 */
int popsift_hip_submit_batch_masked(popsift_hip_ctx* ctx, const void* const* imgs, const uint8_t* const* masks, int n, int kind,
                                    int w, int h, int pitch, int mask_pitch);

/*
 * Keep the n strongest keypoints of every image (OpenCV's nfeatures, KeyPointsFilter::retainBest) and hand out every
 * feature's strength (OpenCV's KeyPoint::response).  A setting of the context, off by default; the pass (strongest.hip)
 * runs on the GPU between refinement and orientation, so orientation and the descriptors see the thinned lists only.
 *
 * The response of a refined extremum record (xpos, ypos, lpos, sigma) of octave o, planes w x h, `levels` search levels:
 *     xi = clamp((int)floorf(xpos + 0.5f), 0, w - 1)     a non-finite xpos or ypos: response = NaN
 *     yi = clamp((int)floorf(ypos + 0.5f), 0, h - 1)
 *     di = clamp(lpos, 1, levels)
 *     response = fabsf(D(xi, yi, di))
 * D(x, y, d) is the DoG value as refinement reads it: the stored plane d of the octave with params.store_dog = 1,
 * otherwise G[d+1] - G[d] formed on the fly, which is bit-identical (popsift_hip_download_plane, kind 1, gives it either
 * way).  So the response is the magnitude of the DoG at the sample nearest to the refined position, in the pyramid's
 * 0 .. 255 units: one load, or one IEEE subtraction, and an absolute value.  (Not the interpolated contrast of the
 * refinement, which mixes the first iteration's centre value with the last iteration's derivatives and cannot be
 * recomputed from a record.)
 *
 * Selection, per image, over all octaves together:
 *     key = 0 if the response is NaN, else the response's bit pattern as uint32 (responses are >= 0: bit order is
 *           numeric order)
 *     total = the records after the max_extrema clamp, n = the setting
 *     total <= n: every record stays.  Otherwise t = the n-th largest key, and a record stays iff key >= t.
 * Every record that ties with the n-th stays (retainBest's rule), so the surviving SET is a function of the records alone,
 * in either feature order and on every run; its size is >= n, and exactly n without a tie at the cut.  Survivors stay in
 * their octave and keep their relative list order: with POPSIFT_HIP_ORDER_RASTER the results are, byte for byte, those of
 * the unthinned run with the dropped records removed (desc_idx renumbered).
 *
 * popsift_hip_set_keep_strongest: n = 0 off; n > 0 on, from the next submit or popsift_hip_rerun_keypoint_stages (the
 * grow-and-rerun paths of popsift_hip_wait include the pass).  A huge n (INT32_MAX) thins nothing and still delivers the
 * responses.  ERR_INVALID: null context, n < 0, or a context whose params enable the grid filter (filter_max_extrema > 0;
 * the two do not chain).  ERR_STATE while a batch is in flight.  popsift_hip_describe_batch ignores the setting: frames
 * are never thinned.  After the pass popsift_hip_download_extrema returns the survivors and popsift_hip_get_report their
 * per-octave counts.  The pass's time counts into POPSIFT_HIP_STAGE_REFINE.  While the setting has never been on, a
 * context allocates and launches nothing for the pass.
 *
 * popsift_hip_fetch_responses_item: the n_features[k] responses of image k of the finished batch, out[i] belonging to
 * feature i; popsift_hip_responses_dev_item: the device array, valid as long as popsift_hip_results_dev_item's pointers.
 * State rules as for popsift_hip_fetch_item; ERR_STATE also when the batch ran with the setting off and for the results
 * of a describe; ERR_TOO_SMALL when cap < n_features[k].
 *
 * A workgroup of the pass's per-record kernels takes POPSIFT_HIP_STRONGEST_CHUNK records of a list (stated here for the
 * tests of its edges; results do not depend on it).
 */
#define POPSIFT_HIP_STRONGEST_CHUNK 1024
int popsift_hip_set_keep_strongest(popsift_hip_ctx* ctx, int n);
int popsift_hip_fetch_responses_item(popsift_hip_ctx* ctx, int k, float* out, size_t cap);
int popsift_hip_responses_dev_item(popsift_hip_ctx* ctx, int k, const void** d_resp);

/*
 * Describe caller-supplied keypoints (vl_sift's 'frames' / 'orientations' options, OpenCV's SIFT::compute): the pyramid
 * of each image is built as for extraction, detection and refinement do not run, and every frame is described where the
 * caller put it.  Results come back through the same calls as an extraction's -- wait / wait_batch, fetch(_item),
 * fetch_begin(_item), results_dev(_item), clone_results -- with n_features[k] == n_frames[k] and feature i belonging to
 * frame i (caller order); desc_idx points into the image's descriptor array as usual, and the reverse map of a cloned
 * set names caller-order feature indices.
 *
 * A frame goes into octave o at x_oct = ldexpf(xpos, up - o) (likewise ypos and sigma), up = (int)upscale_factor, so the
 * feature it gets back reports the frame's own xpos / ypos / sigma.  With octave / level = -1 both are derived from sigma:
 *     t    = log2f(sigma / sigma0) + up
 *     o    = clamp(floor(t - 0.5f / levels), 0, n_oct - 1)
 *     lpos = clamp(roundf(levels * log2f(sigma_oct / sigma0)), 0, L - 1)          (L = levels + 3 Gaussian planes)
 * which inverts refinement's sigma = sigma0 * 2^(sn / levels), lpos = roundf(sn), for sn in [0.5, levels + 0.5).
 *
 * An INVALID frame gets a record with num_ori = 0, desc_idx all -1, debug_octave = -1 and its position and scale echoed;
 * it takes no list slot.  A frame is invalid when a coordinate or sigma is not finite, sigma <= 0, x_oct is outside
 * [0, w_o - 1] or y_oct outside [0, h_o - 1], an octave / level hint is out of range (octave < -1 or >= n_oct, level < -1
 * or >= L), the orientation is not finite (POPSIFT_HIP_ORI_GIVEN), or sigma_oct > POPSIFT_HIP_FRAME_SIGMA_MAX.
 *
 * ori_mode POPSIFT_HIP_ORI_COMPUTE: up to four orientations per frame, exactly as extraction computes them;
 * POPSIFT_HIP_ORI_GIVEN: one orientation (frame.orientation, radians, used as given) and one descriptor per valid frame.
 * n_frames[k] <= params.max_extrema (else ERR_INVALID); 0 is allowed.  Frames are host memory and are copied before the
 * call returns.  The grid filter (filter_max_extrema) does not apply.  download_extrema afterwards returns the resolved
 * frames (ascending octave, caller order within an octave, cell = frame index), get_report their counts,
 * rerun_keypoint_stages re-runs these stages.
 */
typedef struct popsift_hip_frame {   /* 24 bytes */
    float   xpos, ypos;   /* input-image coordinates, as popsift_hip_feature reports them                     */
    float   sigma;        /* input-image units, as popsift_hip_feature::sigma                                  */
    float   orientation;  /* radians, used as given; read only with POPSIFT_HIP_ORI_GIVEN                      */
    int32_t octave;       /* -1: derived from sigma; else the octave to sample (not checked against sigma)     */
    int32_t level;        /* -1: derived from sigma; else the Gaussian level (plane) to sample                 */
} popsift_hip_frame;
enum { POPSIFT_HIP_ORI_COMPUTE = 0, POPSIFT_HIP_ORI_GIVEN = 1 };
/* Largest accepted scale in octave units.  The loop descriptor walks a patch in passes of at most 128 rows whose samples
 * are numbered in signed 16-bit fields (T <= 128 * (5 * sqrt(2) * 3 * sigma + 1) < 2^15 needs sigma < 12.0), and 8 is
 * the largest scale extraction itself produces (sigma0 = 2 at two levels, refinement's sn = levels + 2: the 173-row
 * patches the multi-pass walk was built for).  Orientation's window (4.5 sigma, clipped to the plane) has no tighter
 * limit. */
#define POPSIFT_HIP_FRAME_SIGMA_MAX 8.0f
/* image k of n (one size, kind = POPSIFT_HIP_IMG_*) with its own n_frames[k] frames; a single image is n = 1 */
int popsift_hip_describe_batch(popsift_hip_ctx* ctx, const void* const* imgs, const popsift_hip_frame* const* frames,
                               const int* n_frames, int n, int kind, int w, int h, int pitch, int ori_mode);

/* Replaces the counter read-back of Pyramid::get_descriptors
 * (sift_pyramid.cu:281-294): blocks until the submitted image is finished and
 * returns the feature / descriptor counts. */
int popsift_hip_wait(popsift_hip_ctx* ctx, int* n_features, int* n_descriptors);
/* Replaces prep_features + the two D2H copies (sift_pyramid.cu:249-321).
 * feats: n_features entries; desc: n_descriptors * 128 floats. */
int popsift_hip_fetch(popsift_hip_ctx* ctx, popsift_hip_feature* feats, size_t feats_cap,
                      float* desc, size_t desc_cap);
/* The same download split in two, so that one context overlaps it with the kernels of its next image
 * (the reference serialises them: Pyramid::get_descriptors blocks on its two copies, sift_pyramid.cu:296-321,
 * before PopSift::extractDownloadLoop takes the next job, popsift.cpp:187-213).
 * fetch_begin: requires a finished image (it waits like popsift_hip_wait), starts the two copies on the context's
 * copy stream and returns at once; the context switches to its second result slab, so the next submit / wait may
 * follow immediately.  feats / desc should be pinned (popsift_hip_host_alloc) -- a pageable target makes the copy
 * synchronous -- and must stay untouched until fetch_end returns.
 * fetch_end: blocks until that download has landed.  ERR_STATE without a pending download.
 * After fetch_begin the image's results are no longer in the context: fetch, fetch_begin, results_dev and
 * clone_results return ERR_STATE until another image has been submitted.  A second fetch_begin (for the next image)
 * first waits for the pending download; so does ctx_destroy. */
int popsift_hip_fetch_begin(popsift_hip_ctx* ctx, popsift_hip_feature* feats, size_t feats_cap,
                            float* desc, size_t desc_cap);
int popsift_hip_fetch_end(popsift_hip_ctx* ctx);
/* Device-resident results (FeaturesDev analogue, features.h:98-118): pointers
 * stay valid until the next submit on this context. */
int popsift_hip_results_dev(popsift_hip_ctx* ctx, const void** d_feats, const void** d_desc);

/*
 * Descriptors as bytes (VLFeat's and OpenCV's byte formats, the demo's --write-as-uchar): the GPU quantizes, and only
 * 128 bytes per descriptor cross the link instead of 512.  For each element d of the float descriptor, exactly as the
 * float calls return it (2^norm_multi applied):
 *     q(d) = 0                    if d is NaN or d <= 0      (-0.0 included)
 *            255                  if d >= 255                (+inf included)
 *            (uint8_t) roundf(d)  otherwise                  (ties away from zero, as Feature::print(.., true) rounds)
 * Useful bytes need a scale: norm_multi = 9 (x 512) gives VLFeat-style bytes; with the default 0 every byte is 0 or 1.
 * The float path can hold NaN (the normalisation of a patch without gradient, e.g. a caller frame on a flat region):
 * such elements become 0.
 *
 * Same rules and errors as the float calls above (desc_cap counted in BYTES, >= n_descriptors * 128).  Extraction and
 * describe results alike.  clone_results and the float matcher stay float; byte sets and their own exact matcher are
 * popsift_hip_bytefeatures below.  The float results are untouched: a context that never
 * asks for bytes allocates and launches nothing more.  The pass (desc_bytes.hip) writes a byte buffer of the image's
 * slot, allocated on the first byte request.  It runs on the context's stream; fetch_begin*_u8 enqueues it there before
 * it returns (ahead of the next submit's kernels) and its byte copy on the copy stream waits for it (protocol as above:
 * begin for every image, submit the next batch, one fetch_end).  Every call that writes the buffer first waits for a
 * pending fetch_begin*_u8 download that still reads it.
 * results_dev*_u8: the byte pointer stays valid until the next submit or byte request for that image.
 */
int popsift_hip_fetch_item_u8(popsift_hip_ctx* ctx, int k, popsift_hip_feature* feats, size_t feats_cap, uint8_t* desc,
                              size_t desc_cap);
int popsift_hip_fetch_u8(popsift_hip_ctx* ctx, popsift_hip_feature* feats, size_t feats_cap, uint8_t* desc, size_t desc_cap);
int popsift_hip_fetch_begin_item_u8(popsift_hip_ctx* ctx, int k, popsift_hip_feature* feats, size_t feats_cap, uint8_t* desc,
                                    size_t desc_cap);
int popsift_hip_fetch_begin_u8(popsift_hip_ctx* ctx, popsift_hip_feature* feats, size_t feats_cap, uint8_t* desc,
                               size_t desc_cap);
int popsift_hip_results_dev_item_u8(popsift_hip_ctx* ctx, int k, const void** d_feats, const void** d_desc_u8);

/* Pinned (page-locked) host memory for result buffers: a D2H copy into it runs at PCIe speed
 * without staging.  Replaces FeaturesHost::pin/unpin (cudaHostRegister per image,
 * features.cu:84-109).  Returns NULL on failure / when no GPU runtime is usable. */
void* popsift_hip_host_alloc(size_t bytes);
void  popsift_hip_host_free(void* p);

/* ---- MatchingMode ------------------------------------------------------------
 * Device-resident copy of the last image's results: replaces Pyramid::clone_device_descriptors
 * (sift_pyramid.cu:323-361) and FeaturesDev (features.h:98-118).  The set lives on the context's
 * GPU and is independent of the context afterwards. */
typedef struct popsift_hip_devfeatures popsift_hip_devfeatures;
int popsift_hip_clone_results(popsift_hip_ctx* ctx, popsift_hip_devfeatures** out);
int popsift_hip_devfeatures_free(popsift_hip_devfeatures* f);
int popsift_hip_devfeatures_info(const popsift_hip_devfeatures* f, int* device, int* n_features, int* n_descriptors);
/* Device pointers: features in the 72-byte layout of popsift::Feature (features.h:22-34) whose
 * desc[] point into the descriptor array, descriptors (128 floats each), descriptor -> feature map. */
int popsift_hip_devfeatures_ptrs(const popsift_hip_devfeatures* f, void** d_features, void** d_descriptors,
                                 void** d_reverse_map);
/* An empty (zero-filled) set of the given sizes: FeaturesDev::reset (features.cu:148-160). */
int popsift_hip_devfeatures_alloc(int device, int n_features, int n_descriptors, popsift_hip_devfeatures** out);
/* A set from caller-supplied HOST descriptors (n * 128 floats), for matching without extraction. */
int popsift_hip_devfeatures_from_host(int device, const float* desc, int n_descriptors, popsift_hip_devfeatures** out);
/* Host copies (tests, printing): desc n_descriptors*128 floats, rev n_descriptors ints; either may be NULL. */
int popsift_hip_devfeatures_download(const popsift_hip_devfeatures* f, float* desc, int32_t* rev);
/* The set's descriptors as bytes (n_descriptors * 128, the rule of popsift_hip_fetch_item_u8), quantized on its GPU */
int popsift_hip_devfeatures_download_u8(const popsift_hip_devfeatures* f, uint8_t* desc);

/* One row of the reference's match_matrix (int3, features.cu:178-220) plus the two squared distances. */
typedef struct popsift_hip_match {
    int32_t best;        /* index of the nearest right descriptor        */
    int32_t second;      /* index of the second nearest                  */
    int32_t accept;      /* dist_best / dist_second < 0.8                */
    float   dist_best;   /* squared L2 distances                         */
    float   dist_second;
} popsift_hip_match;
/* Replaces FeaturesDev::match / compute_distance (features.cu:157-300): brute-force 2-NN of every
 * descriptor of `l` among the descriptors of `r`; out has l's descriptor count entries (host memory).
 * Sets on different GPUs are allowed (the right set is copied to the left set's GPU). */
int popsift_hip_match_sets(const popsift_hip_devfeatures* l, const popsift_hip_devfeatures* r, popsift_hip_match* out);
/* Which kernels popsift_hip_match_sets uses, process-wide (tests compare the paths):
 * AUTO (default): matrix-core screening + exact re-rank from 4e6 pairs on, the exact brute-force kernel below;
 * EXACT: the exact kernel only; SCREEN: screening for every size.
 * Every path writes the same bytes for any float input: values of any magnitude and sign, zero rows, NaN and +-Inf
 * elements, and rows whose squared norm overflows while their distances do not.  A pair whose float32 distance is NaN
 * or +Inf is nobody's best or second; a row without two such candidates keeps index 0 and distance +INFINITY in the
 * empty places.  The screening pass decides a row only where its rounding margin holds and the norms it works from are
 * finite; every other row is matched by the exact kernel. */
enum { POPSIFT_HIP_MATCH_AUTO = 0, POPSIFT_HIP_MATCH_EXACT = 1, POPSIFT_HIP_MATCH_SCREEN = 2 };
int popsift_hip_match_set_path(int path);
/* Test hook, not part of the matching interface: *count receives the number of rows that l's last forward sweep on the
 * screening path left to the exact kernel, or -1 when l has never been the left set of a screened sweep.  Waits for l's
 * stream and copies one int; changes nothing.  ERR_INVALID: l or count NULL. */
int popsift_hip_devfeatures_debug_redo_count(const popsift_hip_devfeatures* l, int* count);

/*
 * Correspondences: the rows of the search above, filtered on the GPU into a list of pairs (the expectation SiftGPU's
 * GetSiftMatch(.., distmax, ratiomax, mutual_best_match) and OpenCV's BFMatcher(crossCheck) set).  With F = the rows of
 * match_sets(l, r) and B = the rows of match_sets(r, l), left descriptor i yields the pair
 * (i, F[i].best, F[i].dist_best, F[i].dist_second) iff
 *     1. r has at least one descriptor,
 *     2. ratio == 0, or F[i].dist_best / F[i].dist_second < ratio  (float division; a NaN quotient fails, as in `accept`),
 *     3. F[i].dist_best <= max_dist2,
 *     4. cross_check == 0, or B[F[i].best].best == i  (ties go to the lower index in both directions).
 * Pairs come out in ascending l; the bytes are the same on every run and with every popsift_hip_match_set_path.  With the
 * default options they are the rows of match_sets whose accept is 1.
 *
 * *n_pairs receives the number of pairs found; min(that, cap) of them are written to `pairs` (host memory), and the call
 * returns POPSIFT_HIP_ERR_TOO_SMALL when there are more than cap.  l's descriptor count is always a sufficient cap;
 * cap = 0 with pairs = NULL asks for the count alone.  Empty sets: 0 pairs, POPSIFT_HIP_OK.
 * ERR_INVALID, checked before any GPU call: a NULL set, opts or n_pairs; pairs NULL with cap > 0; ratio negative, NaN or
 * infinite; max_dist2 NaN; reserved != 0; cross_check other than 0 or 1.
 *
 * The forward search is match_sets' own (same kernels, same path choice) and stays on the GPU.  With the cross-check the
 * reverse search runs only for the right descriptors that a row passing 2 and 3 points to: they are compacted into an
 * ascending list, their descriptors gathered, and the same kernels match those rows against l -- on an image pair that
 * mostly does not match this skips nearly all of the second search.  One download brings the count and the pairs.
 * All scratch belongs to l (one match at a time per left set); r may be the left set of another thread's call.  Sets on
 * different GPUs: r's descriptors are copied to l's GPU once and both searches run there.
 * When a model of the image pair is known, popsift_hip_match_pairs_guided (below) searches among the right descriptors that
 * agree with it.
 */
typedef struct popsift_hip_match_opts {
    float   ratio;       /* 0: no ratio test; else a pair needs dist_best / dist_second < ratio (0.8 = match_sets' accept) */
    float   max_dist2;   /* a pair needs dist_best <= max_dist2 (squared L2); +INFINITY: no cap                        */
    int32_t cross_check; /* 1: a pair needs l to be the nearest left descriptor of its best right one                  */
    int32_t reserved;    /* must be 0 */
} popsift_hip_match_opts;
typedef struct popsift_hip_pair {   /* 16 bytes */
    int32_t l, r;                   /* descriptor indices in the left and the right set */
    float   dist_best, dist_second; /* squared L2: to r, and to l's second nearest right descriptor */
} popsift_hip_pair;
void popsift_hip_default_match_opts(popsift_hip_match_opts* opts); /* {0.8f, INFINITY, 0, 0} */
int  popsift_hip_match_pairs(const popsift_hip_devfeatures* l, const popsift_hip_devfeatures* r,
                             const popsift_hip_match_opts* opts, popsift_hip_pair* pairs, size_t cap, int* n_pairs);

/*
 * Byte descriptors on the device, and their matcher.  A popsift_hip_bytefeatures is a device-resident set of n x 128
 * uint8_t descriptors (the format q(d) above produces, VLFeat's and OpenCV's) with its descriptor -> feature map (-1 where
 * no feature stands behind a descriptor) and its own match scratch and stream: a quarter of a float set's memory.  A
 * separate type on purpose: handing a byte set to a float call, or the reverse, does not compile.
 *   from_host         n_descriptors x 128 caller bytes (host memory); the map is all -1
 *   from_set          f's descriptors quantized on f's GPU by q(d) (the pass of the byte fetch calls), f's map copied
 *   clone_results_u8  the same for image k of the finished batch: the bytes popsift_hip_fetch_item_u8 would deliver, copied
 *                     device to device, never through the host; state rules and errors of popsift_hip_fetch_item_u8
 *   download          host copies: desc n x 128 bytes, rev n ints; either may be NULL
 * ERR_INVALID: a NULL set or out, n_descriptors < 0, desc NULL with n_descriptors > 0; a bad device: ERR_NO_DEVICE /
 * ERR_INVALID as for popsift_hip_devfeatures_from_host; a failed allocation: ERR_OOM.
 *
 * popsift_hip_match_bytes: one row per descriptor of l, like popsift_hip_match_sets, from integer arithmetic.
 *     d(i, j)     = sum over k of (l[i][k] - r[j][k])^2, an integer <= 128 * 255^2 = 8 323 200 < 2^24
 *     best, second  the two smallest under lexicographic (d, j): ties go to the lower index
 *     dist_best, dist_second  those integers as float, which is exact
 *     one right descriptor: second = 0, dist_second = +INFINITY (as the float matcher)
 *     accept      = dist_best / dist_second < 0.8f in IEEE float division; 0 / 0 is NaN and fails
 *     l empty: OK, nothing is written.  r empty: every row is {0, 0, 0, +INFINITY, +INFINITY} (as popsift_hip_match_sets).
 * The rows equal popsift_hip_match_sets' on the same values as floats, bit for bit: integer-valued floats below 2^24 make
 * the float matcher's sums exact.  One GEMM on the i8 matrix instructions gives them (match_u8.hip): no screening margin,
 * no re-rank; popsift_hip_match_set_path does not apply.
 *
 * popsift_hip_match_pairs_bytes: the rule of popsift_hip_match_pairs, word for word, on these rows -- conditions 1 to 4,
 * pairs in ascending l, *n_pairs and cap, ERR_TOO_SMALL, and the ERR_INVALID checks before any GPU call.  max_dist2 is in
 * byte units squared.
 *
 * As for float sets: all scratch belongs to l (one match at a time per left set), r may be the left set of another thread's
 * call, and with sets on different GPUs r's bytes are copied to l's GPU once per call.
 *
 * Byte sets hold no positions, so there is no guided byte matcher (popsift_hip_match_pairs_guided): guide the float sets
 * the bytes came from.
 */
typedef struct popsift_hip_bytefeatures popsift_hip_bytefeatures;
int popsift_hip_bytefeatures_from_host(int device, const uint8_t* desc, int n_descriptors, popsift_hip_bytefeatures** out);
int popsift_hip_bytefeatures_from_set(const popsift_hip_devfeatures* f, popsift_hip_bytefeatures** out);
int popsift_hip_clone_results_u8(popsift_hip_ctx* ctx, int k, popsift_hip_bytefeatures** out);
int popsift_hip_bytefeatures_free(popsift_hip_bytefeatures* f);
int popsift_hip_bytefeatures_info(const popsift_hip_bytefeatures* f, int* device, int* n_descriptors);
int popsift_hip_bytefeatures_download(const popsift_hip_bytefeatures* f, uint8_t* desc, int32_t* rev);
int popsift_hip_match_bytes(const popsift_hip_bytefeatures* l, const popsift_hip_bytefeatures* r, popsift_hip_match* out);
int popsift_hip_match_pairs_bytes(const popsift_hip_bytefeatures* l, const popsift_hip_bytefeatures* r,
                                  const popsift_hip_match_opts* opts, popsift_hip_pair* pairs, size_t cap, int* n_pairs);

/*
 * One byte set against many: a popsift_hip_gallery is a device-resident concatenation of byte sets ("members") on one
 * GPU -- the members' bytes end to end, their norms (formed once, when a member is added), the member table first[m],
 * count[m], and a stream and grow-only match scratch of its own.  Byte sets only.
 *   add / add_host    a new member from a byte set (copied device to device, between GPUs with a peer copy; f is not
 *                     referenced afterwards and may be freed) or from n_descriptors x 128 host bytes.  *member (may be
 *                     NULL) receives its index 0, 1, ...  An empty set is a valid member.  The buffers grow
 *                     geometrically; indices and results of earlier members do not change.  A gallery holds no maps,
 *                     and positions only of the members of add_set (below): pair indices are descriptor indices of the
 *                     sets the members came from.
 *   info / member     device, members, descriptors in all; first descriptor and count of member m
 *   download          member m's bytes, count x 128
 * ERR_INVALID, before any GPU call: a NULL gallery, set or out; n_descriptors < 0; desc NULL with n_descriptors > 0; m out
 * of range; an add that would take the gallery past 2^30 descriptors or 2^20 members.  A bad device: as
 * popsift_hip_bytefeatures_from_host.  A failed allocation: ERR_OOM, and the gallery is as it was before the call.
 * One call at a time per gallery (as for a verifier): an add must not run while a match on the gallery is in flight.
 *
 * The two matchers define nothing new; they are stated through the per-pair calls.
 * popsift_hip_match_gallery writes n_members x l_len rows, member-major: out[m * l_len + i] is, bit for bit, row i of
 * popsift_hip_match_bytes(l, member m), with member-local best / second (an empty member: {0, 0, 0, +INFINITY, +INFINITY}
 * rows).  cap_rows < n_members x l_len: ERR_TOO_SMALL and nothing is written.  l empty or no members: OK, nothing written.
 * popsift_hip_match_pairs_gallery returns the pairs in CSR form: those of member m are pairs[offsets[m] .. offsets[m + 1]),
 * offsets[0] = 0, and they are exactly the array popsift_hip_match_pairs_bytes(l, member m, opts, ..) returns (conditions 1
 * to 4, ascending l, member-local r).  *n_pairs = offsets[n_members]; offsets (n_members + 1 ints) is always written in
 * full; the first min(*n_pairs, cap) pairs in that flat order are written, more than cap is ERR_TOO_SMALL with count and
 * offsets valid; n_members x l_len is always a sufficient cap; cap = 0 with pairs = NULL asks for the counts alone (which
 * images match, and how strongly).  An empty l or a gallery without members: all offsets 0, OK.
 * ERR_INVALID, before any GPU call: the checks of popsift_hip_match_pairs_bytes on opts, pairs and n_pairs; a NULL l, g or
 * offsets (out with rows to write); n_members x l_len > INT32_MAX.
 * The results are a function of the bytes, the member order and the options: the same bytes on every run;
 * popsift_hip_match_set_path does not apply.
 *
 * All scratch of the two calls belongs to the gallery (one call at a time per gallery).  l is only read -- its norms are
 * formed in the gallery's scratch on every call -- so l may at the same time be the left or the right set of another
 * thread's call.  With l on another GPU its bytes are copied to the gallery's GPU once per call.
 *
 * Positions.  popsift_hip_gallery_add_set adds a member from a float set: its bytes are
 * popsift_hip_bytefeatures_from_set(f)'s, and with them the gallery keeps per descriptor the (xpos, ypos) of the feature
 * its map names -- the floats popsift_hip_pair_points gathers -- 8 bytes per descriptor next to the 128 of the descriptor,
 * in an array that is allocated with the first such member and grows with the gallery; a gallery that never sees add_set
 * allocates and launches nothing more.  Members added by add / add_host have no positions.  ERR_INVALID also when f's map
 * names no feature for a descriptor; the gallery is then as it was.  Indices, bytes and results of earlier members, and
 * everything popsift_hip_match*_gallery returns, do not change.
 * popsift_hip_gallery_pair_points turns the CSR (pairs, offsets) of popsift_hip_match_pairs_gallery into the points of the
 * verifier (popsift_hip_ransac_many): pts[i] = (x, y of descriptor pairs[i].l of l, x', y' of descriptor pairs[i].r of the
 * member i lies in); l is the float set the query bytes came from.  ERR_INVALID, checked on the host before any GPU call:
 * a NULL l, g or offsets; offsets[0] != 0 or a decreasing offset; pairs or pts NULL with pairs present; a pair index
 * outside l or outside its member; a non-empty list for a member without positions; and, found on the GPU, l's map naming
 * no feature for a descriptor (as popsift_hip_pair_points).  On an error nothing is written.  The gather runs on the
 * gallery's GPU in the gallery's scratch; l on another GPU is copied once per call.
 *
 * The members are walked in groups of max(1, POPSIFT_HIP_GALLERY_GROUP_ROWS / l_len) consecutive members, so that the
 * scratch follows the group and not the gallery; a group costs a fixed number of launches whatever its size
 * (match_gallery.hip).  The define is stated here for the tests of its edges; results do not depend on it.
 * popsift_hip_gallery_debug_set_group_rows replaces it for one gallery from the next call on (0 = the default; < 0:
 * ERR_INVALID).
 */
#define POPSIFT_HIP_GALLERY_GROUP_ROWS (1 << 22)
typedef struct popsift_hip_gallery popsift_hip_gallery;
int popsift_hip_gallery_create(int device, popsift_hip_gallery** out);
int popsift_hip_gallery_free(popsift_hip_gallery* g); /* NULL: OK */
int popsift_hip_gallery_add(popsift_hip_gallery* g, const popsift_hip_bytefeatures* f, int* member);
int popsift_hip_gallery_add_host(popsift_hip_gallery* g, const uint8_t* desc, int n_descriptors, int* member);
int popsift_hip_gallery_add_set(popsift_hip_gallery* g, const popsift_hip_devfeatures* f, int* member);
int popsift_hip_gallery_pair_points(const popsift_hip_devfeatures* l, popsift_hip_gallery* g, const popsift_hip_pair* pairs,
                                    const int32_t* offsets /* n_members + 1 */, float* pts);
int popsift_hip_gallery_info(const popsift_hip_gallery* g, int* device, int* n_members, int64_t* n_descriptors);
int popsift_hip_gallery_member(const popsift_hip_gallery* g, int m, int64_t* first, int* count);
int popsift_hip_gallery_download(const popsift_hip_gallery* g, int m, uint8_t* desc);
int popsift_hip_gallery_debug_set_group_rows(popsift_hip_gallery* g, int rows);
int popsift_hip_match_gallery(const popsift_hip_bytefeatures* l, popsift_hip_gallery* g, popsift_hip_match* out, size_t cap_rows);
int popsift_hip_match_pairs_gallery(const popsift_hip_bytefeatures* l, popsift_hip_gallery* g,
                                    const popsift_hip_match_opts* opts, popsift_hip_pair* pairs, size_t cap,
                                    int32_t* offsets /* n_members + 1 */, int* n_pairs);

/*
 * Members against members: which images of a collection show the same thing as each other (the exhaustive and sequential
 * matching of structure from motion and stitching).  A link is an ordered pair (a, b) of member indices of one gallery:
 * left image a, right image b.  The caller supplies any list of links -- all a < b, (a, a + 1 .. a + k) for a sequence,
 * a retrieval shortlist; a == b and repeated links are allowed and answered like any other link.
 *
 * The three calls define nothing new; they are stated through the per-pair calls.  A_e and B_e are the byte sets
 * popsift_hip_bytefeatures_from_host makes of popsift_hip_gallery_download(g, a_e) and (g, b_e).
 * popsift_hip_match_links writes the rows of every link, link after link: those of link e start at
 * R[e] = sum over e' < e of count[a_e'], and out[R[e] + i] is, bit for bit, row i of popsift_hip_match_bytes(A_e, B_e).
 * An empty B_e gives {0, 0, 0, +INFINITY, +INFINITY} rows, an empty A_e no rows.  cap_rows < R[n_links]: ERR_TOO_SMALL
 * and nothing is written.
 * popsift_hip_match_pairs_links returns the pairs in CSR form: pairs[offsets[e] .. offsets[e + 1]) is exactly the array
 * popsift_hip_match_pairs_bytes(A_e, B_e, opts, ..) returns (conditions 1 to 4, ascending l, l local to a_e, r local to
 * b_e).  offsets[0] = 0 and *n_pairs = offsets[n_links]; offsets (n_links + 1 ints) is always written in full; the first
 * min(*n_pairs, cap) pairs are written, more than cap is ERR_TOO_SMALL with the count and the offsets valid; R[n_links] is
 * always a sufficient cap; cap = 0 with pairs = NULL asks for the counts alone (the edge weights of the view graph).
 * popsift_hip_gallery_link_points turns that CSR into the points popsift_hip_ransac_many takes, unchanged:
 * pts[i] = (x, y of descriptor pairs[i].l of member a_e, x', y' of descriptor pairs[i].r of member b_e), e the link i
 * lies in.  Both positions come from the gallery's position array (popsift_hip_gallery_add_set members): the floats
 * popsift_hip_pair_points gathers from the sets the members came from.
 * The results are a function of the gallery's bytes, the link list and the options: the same bytes on every run.
 *
 * ERR_INVALID, before any GPU call and with nothing written: a NULL gallery, opts, offsets or n_pairs; links NULL with
 * n_links > 0; n_links < 0 or > 2^20 (popsift_hip_ransac_many's limit); an a or b outside 0 .. n_members - 1;
 * R[n_links] > INT32_MAX; pairs (cap > 0) or out (rows to write) NULL; the opts checks of popsift_hip_match_pairs_bytes.
 * popsift_hip_gallery_link_points also: offsets[0] != 0 or a decreasing offset; pairs or pts NULL with pairs present; a
 * pair index outside its member; a non-empty list on a link with a member that has no positions.
 * n_links == 0: OK, *n_pairs = 0 and offsets[0] = 0.
 *
 * One call at a time per gallery, as above; everything lives on the gallery's GPU.  The links are walked in groups of
 * consecutive links holding at most POPSIFT_HIP_GALLERY_GROUP_ROWS left rows (popsift_hip_gallery_debug_set_group_rows
 * applies), always at least one link; a group costs a fixed number of launches and at most one read-back whatever the
 * number of its links (match_links.hip), and results do not depend on the grouping.
 */
typedef struct popsift_hip_link {
    int32_t a, b;
} popsift_hip_link; /* 8 bytes */
int popsift_hip_match_links(popsift_hip_gallery* g, const popsift_hip_link* links, int n_links, popsift_hip_match* out,
                            size_t cap_rows);
int popsift_hip_match_pairs_links(popsift_hip_gallery* g, const popsift_hip_link* links, int n_links,
                                  const popsift_hip_match_opts* opts, popsift_hip_pair* pairs, size_t cap,
                                  int32_t* offsets /* n_links + 1 */, int* n_pairs);
int popsift_hip_gallery_link_points(popsift_hip_gallery* g, const popsift_hip_link* links, int n_links,
                                    const popsift_hip_pair* pairs, const int32_t* offsets /* n_links + 1 */, float* pts);

/*
 * Geometric verification: RANSAC over point pairs (OpenCV's findHomography(.., RANSAC), CudaSift's FindHomography).  Given
 * n pairs (x, y) -> (x', y') the verifier returns the model with the most inliers among T sampled hypotheses, its inlier
 * count and a per-pair inlier mask.  The result is a function of (points, options) alone: the same bytes on every run.
 * With m = 4 pairs per sample for a homography and 3 for an affine map, double = IEEE binary64, float = binary32, every
 * line one IEEE operation, fma / fmaf fused:
 *
 * 1. Sample.  mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16   (uint32_t)
 *    base = mix(mix(seed + 0x9e3779b9) ^ t); draw number c = 1, 2, .. of hypothesis t is the index
 *    (uint64_t)mix(base + 0x9e3779b9 * c) * n >> 32.  Slot k = 0 .. m-1 takes the next draw; a draw equal to an earlier
 *    slot of the sample is redrawn, at most 8 times; a slot whose 9 draws all repeat leaves itself and the later slots -1
 *    and the hypothesis invalid.  The sample depends on (seed, t, n, model) alone.
 * 2. Normalise, per side (left: x, y; right: x', y').  Of every column the smallest and the largest FINITE value, with -0
 *    ordered below +0 (so that no reduction order matters); centre c = ((double)lo + (double)hi) * 0.5, half extent
 *    e = ((double)hi - (double)lo) * 0.5; a column without finite values has c = e = 0.  s = max(e_x, e_y), or 1 when that
 *    is 0; k = 1.0 / s.  A normalised coordinate is ((double)x - c_x) * k.
 * 3. Solve, in double, on the normalised sample (x, y) -> (u, v).  Homography: unknowns g0 .. g7, g8 = 1, pair i gives the
 *    rows [x y 1 0 0 0 -u*x -u*y | u] and [0 0 0 x y 1 -v*x -v*y | v] (rows 2i, 2i+1; -u*x is (-u) * x).  Affine map:
 *    the 3 x 3 system [x y 1] with the two right-hand sides u and v; g6 = g7 = 0, g8 = 1.  Gaussian elimination, column
 *    c = 0, 1, ..: the pivot row is the row r >= c with the largest |a[r][c]|, the lowest such row on a tie ('>' decides, so
 *    a NaN never wins), swapped with row c; for r > c: f = a[r][c] / a[c][c], a[r][j] = fma(-f, a[c][j], a[r][j]) for
 *    j > c.  Back substitution from the last row: s = b[i]; s = fma(-a[i][j], g[j], s) for j = i+1, i+2, ..; g[i] =
 *    s / a[i][i].  Denormalise with the left side's (cx, cy, k) and the right side's (cx', cy', s'): for row i of g,
 *    m[i][0] = g[i][0] * k, m[i][1] = g[i][1] * k, m[i][2] = fma(-m[i][0], cx, fma(-m[i][1], cy, g[i][2])); then
 *    h[0][j] = fma(s', m[0][j], cx' * m[2][j]), h[1][j] = fma(s', m[1][j], cy' * m[2][j]), h[2][j] = m[2][j].  The nine h
 *    are rounded to float: the model H.  The hypothesis is invalid iff a pivot is exactly 0 or one of the nine floats is
 *    not finite.  No conditioning threshold: a near-degenerate sample yields a poor model, which scores low.  The
 *    denominator of H is 1 at the centre of the left bounding box.
 * 4. Score, in float: u = fmaf(h0, x, fmaf(h1, y, h2)), v = fmaf(h3, x, fmaf(h4, y, h5)), w = fmaf(h6, x, fmaf(h7, y, h8)),
 *    dx = fmaf(-w, x', u), dy = fmaf(-w, y', v), e = fmaf(dx, dx, dy * dy), lim = (max_err * max_err) * (w * w).  A pair is
 *    an inlier iff w > 0 && e <= lim (a NaN fails both): its transfer error in the right image is at most max_err pixels,
 *    tested without a division.  The count of a hypothesis is its number of inliers, -1 for an invalid one.
 * 5. Select.  The winner has the largest count, the lowest t on a tie.  No winner when no hypothesis is valid or the best
 *    count is below m.  The mask is step 4 with the winner's H.
 *
 * ERR_INVALID, before any GPU call: a NULL verifier, opts or result; pts NULL with n > 0; n < 0 or n > 2^24; an unknown
 * model; hypotheses outside 1 .. 65536; max_err not finite or <= 0; reserved != 0.  n < m: OK, no winner.  Without a
 * winner hypothesis = -1, n_inliers = 0, H and the mask are zeros.
 *
 * A verifier owns a stream, device scratch and pinned staging, all grow-only, and serves one call at a time.  A call is
 * one upload of the points, a fixed handful of launches (ransac.hip) and one download of the result with the mask.  The
 * scoring kernel gives a workgroup POPSIFT_HIP_RANSAC_CHUNK pairs and POPSIFT_HIP_RANSAC_HYP_BLOCK hypotheses (stated here
 * for the tests of their edges; results do not depend on them).
 *
 * popsift_hip_ransac_trace is the parity hook: the same computation, returning per hypothesis the sample (4 ints, -1 =
 * unused or not found), the model (9 floats, zeros when invalid) and the count; any of the three may be NULL.
 *
 * popsift_hip_pair_points turns the pairs of popsift_hip_match_pairs into the points above: (x, y) of the feature behind
 * descriptor pairs[i].l of l, (x', y') of the one behind pairs[i].r of r, gathered on l's GPU through the sets' maps
 * (scratch belongs to l).  ERR_INVALID also for a pair index outside its set (checked before any GPU call) and for a
 * descriptor whose map entry is -1 (sets made by popsift_hip_devfeatures_from_host).  Byte sets hold no positions: the pair
 * indices of popsift_hip_match_pairs_bytes are the descriptor indices of the float sets the bytes came from
 * (popsift_hip_bytefeatures_from_set, popsift_hip_clone_results_u8), so gather the points from those.
 */
enum { POPSIFT_HIP_MODEL_HOMOGRAPHY = 0 /* 4 pairs */, POPSIFT_HIP_MODEL_AFFINE = 1 /* 3 pairs */ };
#define POPSIFT_HIP_RANSAC_CHUNK 1024
#define POPSIFT_HIP_RANSAC_HYP_BLOCK 64
typedef struct popsift_hip_ransac_opts {
    int32_t  model;        /* POPSIFT_HIP_MODEL_*                                        */
    int32_t  hypotheses;   /* T, 1 .. 65536                                              */
    float    max_err;      /* inlier: transfer error in the right image <= max_err (px)  */
    uint32_t seed;
    int32_t  reserved[2];  /* must be 0 */
} popsift_hip_ransac_opts;
typedef struct popsift_hip_ransac_result {   /* 52 bytes */
    float   H[9];          /* row major, right ~ H * left; zeros when hypothesis == -1   */
    int32_t n_inliers;
    int32_t hypothesis;    /* index of the winner, -1: none                              */
    int32_t n_valid;       /* hypotheses that produced a model                           */
    int32_t reserved;
} popsift_hip_ransac_result;
typedef struct popsift_hip_verifier popsift_hip_verifier;
int  popsift_hip_verifier_create(int device, popsift_hip_verifier** out);
int  popsift_hip_verifier_free(popsift_hip_verifier* v);
void popsift_hip_default_ransac_opts(popsift_hip_ransac_opts* o); /* {HOMOGRAPHY, 2048, 2.0f, 0, {0, 0}} */
/* pts: n x 4 floats (x, y, x', y') in host memory; inlier: n bytes (0 / 1) or NULL */
int  popsift_hip_ransac(popsift_hip_verifier* v, const float* pts, int n, const popsift_hip_ransac_opts* o,
                        popsift_hip_ransac_result* res, uint8_t* inlier);
/* samples: T x 4, models: T x 9, counts: T */
int  popsift_hip_ransac_trace(popsift_hip_verifier* v, const float* pts, int n, const popsift_hip_ransac_opts* o,
                              int32_t* samples, float* models, int32_t* counts);
int  popsift_hip_pair_points(const popsift_hip_devfeatures* l, const popsift_hip_devfeatures* r,
                             const popsift_hip_pair* pairs, int n, float* pts);

/*
 * Epipolar verification: RANSAC for the fundamental matrix of two views of a 3-D scene (OpenCV's findFundamentalMat(..,
 * FM_RANSAC)), on the same verifier under entry points of its own: popsift_hip_ransac and its options do not change.  The
 * pairs of such a scene follow no homography; they satisfy [x' y' 1] F [x y 1]^T = 0.  popsift_hip_epipolar returns the F
 * with the most inliers among T hypotheses of m = 8 pairs each (the 8-point algorithm), its count and the mask; res->H
 * holds F, row major.  Points, mask, result record, "n < m is answered on the host", "one call at a time" and the trace are
 * popsift_hip_ransac's with m = 8 (a sample is 8 ints).  Calls of both kinds may alternate on one verifier: each returns
 * the bytes a fresh verifier returns.  The result is a function of (points, options) alone.  Steps 3 to 5 run in double,
 * step 6 in float; every line one IEEE operation, fma / fmaf fused, sqrt and '/' correctly rounded:
 *
 * 1. Sample.  Step 1 of popsift_hip_ransac with m = 8: the same hash, the same nine draws per slot.
 * 2. Normalise.  Step 2 of popsift_hip_ransac, unchanged: (cx, cy, s, k) of the left side, (cx', cy', s', k') of the right.
 * 3. Solve.  Pair i of the normalised sample (x, y) -> (u, v) gives row i of the 8 x 9 system A f = 0:
 *    [u*x, u*y, u, v*x, v*y, v, x, y, 1].  Gaussian elimination with complete pivoting, k = 0 .. 7; perm[j] = j at first.
 *    The pivot is the entry of largest |a[r][c]| over k <= r <= 7, k <= c <= 8: best = |a[k][k]|, then c = k .. 8 and
 *    within a column r = k .. 7, an entry replaces the pivot when its magnitude > best (the lowest column, then the lowest
 *    row, wins a tie; a NaN never wins).  Row r is swapped with row k; column c with column k in all eight rows, and
 *    perm[c] with perm[k].  For r > k: q = a[r][k] / a[k][k], a[r][j] = fma(-q, a[k][j], a[r][j]) for j > k.  After the
 *    eight steps column 8 is free: z[8] = 1, and for i = 7 .. 0: s = -a[i][8]; s = fma(-a[i][j], z[j], s) for
 *    j = i+1 .. 7; z[i] = s / a[i][i].  f[perm[j]] = z[j].  (Fixing f8 = 1 instead would be wrong: a camera that moves
 *    sideways has F[2][2] = 0.)  Fn is f as a row-major 3 x 3 matrix.
 * 4. Rank 2.  m[i][j] = fma(Fn[0][i], Fn[0][j], fma(Fn[1][i], Fn[1][j], Fn[2][i] * Fn[2][j])) for i <= j (Fn^T Fn,
 *    symmetric), V = identity.  Six sweeps of the Jacobi rotations (p, q) = (0, 1), (0, 2), (1, 2), o the third index.  A
 *    rotation with m[p][q] == 0 is skipped.  Otherwise d = m[q][q] - m[p][p], e = 2 * m[p][q], theta = d / e,
 *    root = sqrt(fma(theta, theta, 1)), den = |theta| + root, t = copysign(1, theta) / den, c = 1 / sqrt(fma(t, t, 1)),
 *    s = t * c; then m[p][p] = fma(-t, m[p][q], m[p][p]), m[q][q] = fma(t, m[p][q], m[q][q]) (both with the old m[p][q]),
 *    m[p][q] = 0, and with the old a = m[o][p], b = m[o][q]: m[o][p] = fma(-s, b, c * a), m[o][q] = fma(s, a, c * b);
 *    for each row r of V with the old a = V[r][p], b = V[r][q]: V[r][p] = fma(-s, b, c * a), V[r][q] = fma(s, a, c * b).
 *    w is the column of V under the smallest m[i][i] ('<' decides from i = 0, so the lowest index wins a tie).  For each
 *    row i: fw = fma(Fn[i][0], w[0], fma(Fn[i][1], w[1], Fn[i][2] * w[2])), Fn[i][j] = fma(-fw, w[j], Fn[i][j]): the
 *    closest matrix of rank 2 in the Frobenius norm, without an SVD.
 * 5. Denormalise and scale: F = Tr^T Fn Tl.  For row i: g[i][0] = Fn[i][0] * k, g[i][1] = Fn[i][1] * k,
 *    g[i][2] = fma(-g[i][0], cx, fma(-g[i][1], cy, Fn[i][2])); for column j: h[0][j] = g[0][j] * k',
 *    h[1][j] = g[1][j] * k', h[2][j] = fma(-h[0][j], cx', fma(-h[1][j], cy', g[2][j])).  d is the h of largest magnitude
 *    in row-major order ('>' decides, the lowest index wins a tie); the model is (float)(h / d), nine values, the largest
 *    exactly 1.  The hypothesis is invalid iff a pivot is exactly 0, d is 0, or one of the nine floats is not finite.  No
 *    conditioning threshold.
 * 6. Score, in float: a = fmaf(F0, x, fmaf(F1, y, F2)), b = fmaf(F3, x, fmaf(F4, y, F5)), c = fmaf(F6, x, fmaf(F7, y, F8)),
 *    d = fmaf(F0, x', fmaf(F3, y', F6)), e = fmaf(F1, x', fmaf(F4, y', F7)), r = fmaf(a, x', fmaf(b, y', c)),
 *    g = fmaf(a, a, fmaf(b, b, fmaf(d, d, e * e))), lim = (max_err * max_err) * g.  A pair is an inlier iff
 *    g > 0 && g < +inf && r * r <= lim: its Sampson distance is at most max_err pixels, tested without a division.  A NaN
 *    fails every test.  An invalid hypothesis is an all-zero model, r = g = 0: `g > 0` keeps it from counting every pair.
 *    A pair with an infinite coordinate has g = +inf (or NaN) and r * r = lim = +inf: `g < +inf` keeps it out.
 * 7. Select.  Step 5 of popsift_hip_ransac with m = 8.
 *
 * ERR_INVALID, before any GPU call: as popsift_hip_ransac, with reserved[0 .. 2] != 0.  A minimal sample of 8 needs more
 * hypotheses than a homography's 4: with an inlier share w a sample is clean with probability w^8.
 */
#define POPSIFT_HIP_EPIPOLAR_SAMPLE 8
typedef struct popsift_hip_epipolar_opts {   /* 24 bytes */
    int32_t  hypotheses;   /* T, 1 .. 65536 */
    float    max_err;      /* inlier: Sampson distance <= max_err (px) */
    uint32_t seed;
    int32_t  reserved[3];  /* must be 0 */
} popsift_hip_epipolar_opts;
void popsift_hip_default_epipolar_opts(popsift_hip_epipolar_opts* o);   /* {2048, 2.0f, 0, {0, 0, 0}} */
/* res->H holds F, row major: [x' y' 1] F [x y 1]^T = 0; zeros when hypothesis == -1 */
int  popsift_hip_epipolar(popsift_hip_verifier* v, const float* pts, int n, const popsift_hip_epipolar_opts* o,
                          popsift_hip_ransac_result* res, uint8_t* inlier);
/* samples: T x 8, models: T x 9, counts: T; any may be NULL */
int  popsift_hip_epipolar_trace(popsift_hip_verifier* v, const float* pts, int n, const popsift_hip_epipolar_opts* o,
                                int32_t* samples, float* models, int32_t* counts);

/*
 * Least-squares refit on the inliers (the step OpenCV's findHomography / findFundamentalMat take after their RANSAC, and
 * LO-RANSAC repeats): popsift_hip_ransac and popsift_hip_epipolar return a model solved from a minimal sample, which carries
 * the noise of those 3, 4 or 8 pairs.  popsift_hip_refit starts from such a model M (or any other), fits the kind's model to
 * ALL inliers of the current model by the normal equations in double, and repeats on the new model's inliers for up to
 * `rounds` rounds, as long as the inlier count does not drop.  A third kind of call on the verifier: the two above, their
 * options, records and bytes do not change, and calls of all kinds may alternate on one verifier.  The result is a function
 * of (points, options) alone.  m = 4 (homography), 3 (affine map) or 8 (epipolar) pairs; every line one IEEE operation, fma /
 * fmaf fused:
 *
 * 1. Normalise.  Step 2 of popsift_hip_ransac over all n pairs: (cx, cy, k) left, (cx', cy', s', k') right.
 * 2. Start.  cur = M; c_cur = the number of inliers of cur under the kind's test, operation for operation: step 4 of
 *    popsift_hip_ransac (homography, affine map), step 6 of popsift_hip_epipolar (epipolar).  n_start = c_cur.  c_cur < m:
 *    stop with NO_SUPPORT.
 * 3. Round r = 0 .. rounds - 1:
 *    a. Terms, of the pairs that are inliers of cur only, from the normalised doubles (x, y) -> (u, v) of step 1.  45 slots;
 *       a slot a kind does not list is the constant +0.0.
 *       Homography -- the normal equations of the rows a = [x y 1 0 0 0 p6 p7 | u], b = [0 0 0 x y 1 q6 q7 | v] of step 3
 *       of popsift_hip_ransac, p6 = (-u) * x, p7 = (-u) * y, q6 = (-v) * x, q7 = (-v) * y; N[j][k] = sum a_j a_k + b_j b_k,
 *       c[j] = sum a_j u + b_j v, a term with one structurally non-zero product is that product:
 *         0 x*x   1 x*y   2 x   3 y*y   4 y   5 1.0          N00 N01 N02 N11 N12 N22, and N[3+j][3+k] = N[j][k], formed once
 *         6 x*p6  7 x*p7  8 y*p6  9 y*p7  10 p6  11 p7       N06 N07 N16 N17 N26 N27
 *         12 x*q6 13 x*q7 14 y*q6 15 y*q7 16 q6  17 q7       N36 N37 N46 N47 N56 N57
 *         18 fma(p6, p6, q6*q6)  19 fma(p6, p7, q6*q7)  20 fma(p7, p7, q7*q7)       N66 N67 N77
 *         21 x*u  22 y*u  23 u  24 x*v  25 y*v  26 v  27 fma(p6, u, q6*v)  28 fma(p7, u, q7*v)       c0 .. c7
 *       N[j][3+k] = 0 for j, k < 3.  Affine map -- slots 0 .. 5 and 21 .. 26 of the above: the 3 x 3 matrix of [x y 1] and its
 *       two right-hand sides.  Epipolar -- the row a = [u*x, u*y, u, v*x, v*y, v, x, y, 1.0] of step 3 of
 *       popsift_hip_epipolar; slot 9j - j(j-1)/2 + (k - j) = a_j * a_k for j <= k: the upper triangle of the 9 x 9 N, row by
 *       row.
 *    b. Sum.  Each slot is the root of a pairwise tree over the pair index: tree(a, 1) = term + 0.0 for a pair a < n that
 *       is an inlier of cur (so a term of -0.0 enters as +0.0), else +0.0; tree(a, 2L) = tree(a, L) + tree(a + L, L); the
 *       root is tree(0, P), P the smallest power of two >= n.  No node is -0.0, so adding +0.0 changes no bit: padding
 *       further, or not at all, gives the same root.  The order is a function of the index alone, not of a launch shape.
 *    c. Solve, in double.  N is mirrored.  Homography: the 8 x 8 system [N | c] by the elimination, back substitution and
 *       denormalisation of step 3 of popsift_hip_ransac, unchanged.  Affine map: the 3 x 3 system with its two right-hand
 *       sides, the same way.  Epipolar: eight steps k = 0 .. 7 of the complete-pivoting elimination of step 3 of
 *       popsift_hip_epipolar on the 9 x 9 N, rows k .. 8 and columns k .. 8 in the search (the same order: columns, within a
 *       column rows, '>' decides) and in the update, column swaps in all nine rows; row 8 is then dropped, z[8] = 1, back
 *       substitution and f[perm[j]] = z[j] as there: the least-squares F with the coefficient the pivoting leaves over fixed
 *       to 1.  Then that rule's rank-2 step 4 and its denormalisation and scaling step 5.  The nine values rounded to float
 *       are the candidate.  It is invalid iff a pivot is exactly 0, the scaling divisor is 0 or a value is not finite: stop
 *       with NO_FIT.
 *    d. Decide.  c' = the inlier count of the candidate (step 2's test).  The candidate equals cur as bytes: stop with
 *       CONVERGED.  c' < c_cur: stop with NOT_BETTER.  Otherwise cur = candidate, c_cur = c', the round is accepted.
 * 4. No stop in `rounds` rounds: stop = ROUNDS.
 * 5. Result: M = cur, n_inliers = c_cur, n_start, rounds = the accepted rounds, stop, and the mask of cur.  Hence
 *    n_inliers >= n_start, and a start model the fit cannot improve comes back unchanged.
 *
 * ERR_INVALID, before any GPU call: a NULL verifier, opts or result; pts NULL with n > 0; n < 0 or n > 2^24; an unknown model;
 * rounds outside 1 .. 16; max_err not finite or <= 0; an entry of M that is not finite; reserved != 0.  n < m: OK, answered
 * on the host: M = the caller's M, n_inliers = n_start = rounds = 0, stop = NO_SUPPORT, the mask zeros.
 *
 * A call is one upload of the points, every launch of every round enqueued up front (ransac.hip: a state record on the
 * device carries cur, c_cur and a `done` flag that the later rounds' kernels read and return on), one download and one
 * synchronisation.  The accumulating kernel gives a workgroup POPSIFT_HIP_REFIT_CHUNK pairs; results do not depend on it.
 *
 * popsift_hip_refit_trace is the parity hook: the same call, returning for each of opts->rounds rounds its 45 sums, its
 * candidate (zeros when invalid), c' (-1 when invalid) and whether it was accepted; a round that did not run is zeros with
 * count -1.  Any of the four may be NULL.
 */
enum { POPSIFT_HIP_REFIT_HOMOGRAPHY = 0, POPSIFT_HIP_REFIT_AFFINE = 1, POPSIFT_HIP_REFIT_EPIPOLAR = 2 };
enum {
    POPSIFT_HIP_REFIT_STOP_ROUNDS = 0,      /* every round ran and was accepted                        */
    POPSIFT_HIP_REFIT_STOP_CONVERGED = 1,   /* a round returned the model it started from              */
    POPSIFT_HIP_REFIT_STOP_NOT_BETTER = 2,  /* a round's candidate has fewer inliers                   */
    POPSIFT_HIP_REFIT_STOP_NO_FIT = 3,      /* a round's system is singular or its solution not finite */
    POPSIFT_HIP_REFIT_STOP_NO_SUPPORT = 4   /* the start model has fewer than m inliers                */
};
#define POPSIFT_HIP_REFIT_CHUNK 1024
#define POPSIFT_HIP_REFIT_MAX_ROUNDS 16
#define POPSIFT_HIP_REFIT_SLOTS 45
typedef struct popsift_hip_refit_opts {     /* 64 bytes */
    int32_t model;         /* POPSIFT_HIP_REFIT_*                                         */
    int32_t rounds;        /* 1 .. POPSIFT_HIP_REFIT_MAX_ROUNDS                           */
    float   max_err;       /* the kind's inlier limit (px), as in the call M came from    */
    float   M[9];          /* the start model, row major                                  */
    int32_t reserved[4];   /* must be 0 */
} popsift_hip_refit_opts;
typedef struct popsift_hip_refit_result {   /* 52 bytes */
    float   M[9];          /* the refitted model, row major                               */
    int32_t n_inliers;
    int32_t n_start;       /* inliers of the start model                                  */
    int32_t rounds;        /* accepted rounds                                             */
    int32_t stop;          /* POPSIFT_HIP_REFIT_STOP_*                                    */
} popsift_hip_refit_result;
void popsift_hip_default_refit_opts(popsift_hip_refit_opts* o);   /* {HOMOGRAPHY, 4, 2.0f, identity, {0, 0, 0, 0}} */
/* pts, inlier: as popsift_hip_ransac */
int  popsift_hip_refit(popsift_hip_verifier* v, const float* pts, int n, const popsift_hip_refit_opts* o,
                       popsift_hip_refit_result* res, uint8_t* inlier);
/* sums: rounds x 45 doubles, models: rounds x 9, counts: rounds, accepted: rounds; any may be NULL */
int  popsift_hip_refit_trace(popsift_hip_verifier* v, const float* pts, int n, const popsift_hip_refit_opts* o,
                             popsift_hip_refit_result* res, uint8_t* inlier, double* sums, float* models, int32_t* counts,
                             int32_t* accepted);

/*
 * Many pair lists in one call: the grouped form of the sampler, for the CSR pair lists of a gallery
 * (popsift_hip_match_pairs_gallery, popsift_hip_gallery_pair_points).  It defines no new numerics; it is stated entirely
 * through the per-list calls.
 *
 * The rule.  res[m], inlier[offsets[m] .. offsets[m+1]) and list m's slice of the trace are, byte for byte, what the
 * per-list call writes for the points pts + 4 * offsets[m] with n = offsets[m+1] - offsets[m] and the same hypotheses,
 * max_err and seed.  The per-list call is popsift_hip_ransac for kinds 0 and 1, and popsift_hip_epipolar for kind 2.
 * This includes a list shorter than the kind's sample: hypothesis -1, zeros, and a trace of -1 / 0 / -1.
 *
 * The per-list calls keep their bytes, their options and their records.  Calls of all kinds may alternate on one verifier,
 * and each returns what a fresh verifier returns.
 *
 * ERR_INVALID, before any GPU call: a NULL verifier, opts, offsets or res (res is not required for the trace); n_lists < 0
 * or > 2^20; offsets[0] != 0, or a decreasing offset; offsets[n_lists] > 2^24; pts NULL with pairs present; an unknown
 * kind; hypotheses outside 1 .. 65536; max_err not finite or <= 0; reserved != 0.  n_lists == 0 returns OK and writes
 * nothing.
 *
 * A call is one upload of all points with the offsets, a number of launches that does not depend on the number of lists
 * within a group (ransac.hip), one download of all records, plus the masks when asked for, and one synchronisation.
 * Scratch is grow-only and belongs to the verifier.  Models, samples and counts cost 36 + 16..32 + 4 bytes per (list,
 * hypothesis), so the lists are walked in groups of consecutive lists, each holding at most POPSIFT_HIP_RANSAC_MANY_GROUP
 * (list, hypothesis) records and always at least one list.  The scoring kernel walks a list in segments of
 * POPSIFT_HIP_RANSAC_MANY_SEGMENT pairs.  The two defines are stated here for the tests of their edges; results do not
 * depend on them.  popsift_hip_verifier_debug_set_group replaces the first for one verifier from the next call on (0 =
 * the default; < 0: ERR_INVALID).
 *
 * popsift_hip_ransac_many_trace is the parity hook: the same call, returning list-major the samples (n_lists x T x 4 ints,
 * x 8 for the epipolar kind), the models (n_lists x T x 9) and the counts (n_lists x T); any of the three, res and inlier
 * may be NULL.
 */
#define POPSIFT_HIP_RANSAC_MANY_GROUP (1 << 20)
#define POPSIFT_HIP_RANSAC_MANY_SEGMENT 256
typedef struct popsift_hip_ransac_many_opts {   /* 32 bytes */
    int32_t  kind;         /* POPSIFT_HIP_REFIT_HOMOGRAPHY / _AFFINE / _EPIPOLAR: the one numbering of the kinds */
    int32_t  hypotheses;   /* T, 1 .. 65536, the same for every list                                             */
    float    max_err;      /* the kind's inlier limit (px)                                                       */
    uint32_t seed;         /* the same for every list: a sample depends on (seed, t, n, kind) alone              */
    int32_t  reserved[4];  /* must be 0 */
} popsift_hip_ransac_many_opts;
void popsift_hip_default_ransac_many_opts(popsift_hip_ransac_many_opts* o);   /* {HOMOGRAPHY, 2048, 2.0f, 0, {0, 0, 0, 0}} */
/* pts: offsets[n_lists] x 4 floats; offsets: n_lists + 1 ints, offsets[0] = 0, non-decreasing (the CSR of
 * popsift_hip_match_pairs_gallery); res: n_lists records; inlier: offsets[n_lists] bytes or NULL */
int  popsift_hip_ransac_many(popsift_hip_verifier* v, const float* pts, const int32_t* offsets, int n_lists,
                             const popsift_hip_ransac_many_opts* o, popsift_hip_ransac_result* res, uint8_t* inlier);
int  popsift_hip_ransac_many_trace(popsift_hip_verifier* v, const float* pts, const int32_t* offsets, int n_lists,
                                   const popsift_hip_ransac_many_opts* o, popsift_hip_ransac_result* res, uint8_t* inlier,
                                   int32_t* samples, float* models, int32_t* counts);
int  popsift_hip_verifier_debug_set_group(popsift_hip_verifier* v, int records);

/*
 * Guided matching: nearest neighbours under a known model (the expectation SiftGPU's GetGuidedSiftMatch(.., H, F, distmax,
 * ratiomax, hsearch_thresh, fsearch_thresh, mutual) sets).  With the homography or the fundamental matrix of an image pair
 * known -- from popsift_hip_ransac / popsift_hip_epipolar, or from anywhere else -- each left descriptor is searched for only
 * among the right descriptors whose POSITION agrees with the model.  This is not "match, then filter": a row whose global
 * nearest neighbour fails the geometry is answered by its nearest candidate, and a row whose second nearest neighbour in
 * the whole right set spoiled the ratio test is measured against the few candidates only.
 *
 * The position of descriptor i of a set is (xpos, ypos) of the feature its descriptor -> feature map names: the floats
 * popsift_hip_pair_points gathers.  M is the caller's 3 x 3 row-major float model; float = IEEE binary32, every line one
 * operation, fmaf fused.
 *
 * Candidate test ok(i, j), left descriptor i at (x, y), right descriptor j at (x', y'):
 *   POPSIFT_HIP_GUIDE_HOMOGRAPHY  step 4 of popsift_hip_ransac with H = M, operation for operation: u, v, w, dx, dy, e, lim
 *                                 as written there; ok = w > 0 && e <= lim.  An affine model is a homography whose last row
 *                                 is 0 0 1.
 *   POPSIFT_HIP_GUIDE_EPIPOLAR    step 6 of popsift_hip_epipolar with F = M, operation for operation;
 *                                 ok = g > 0 && g < +inf && r * r <= lim.
 * A NaN fails every comparison, so a feature with a NaN coordinate is nobody's candidate; so is one with an infinite
 * coordinate as long as lim stays finite (always under the epipolar test, which asks for g < +inf).  Consequence: a pair in
 * the verifier's inlier mask is a candidate under the verifier's own model and max_err.  The test is always evaluated
 * left -> right, also for the cross-check below.
 *
 * Distance d(i, j): the squared L2 distance exactly as popsift_hip_match_sets (POPSIFT_HIP_MATCH_EXACT) forms it.  For chunk
 * c = 0 .. 31 with x, y, z, w = l[4c .. 4c+3] - r[4c .. 4c+3]: p(c) = fmaf(w, w, fmaf(z, z, fmaf(y, y, x * x))); then
 * n1(i) = p(i) + p(i+16), n2(i) = n1(i) + n1(i+8), n3(i) = n2(i) + n2(i+4), n4(i) = n3(i) + n3(i+2), d = n4(0) + n4(1).
 * d is the same bits in both directions.
 *
 * Row of left descriptor i, over C(i) = { j : ok(i, j) and d(i, j) < +inf } (a NaN distance drops out): best and second are
 * the two smallest under lexicographic (d, j).  |C(i)| = 0: best = second = -1, both distances +inf.  |C(i)| = 1:
 * second = -1, dist_second = +inf.  accept = dist_best / dist_second < 0.8f in IEEE float division: 0 for an empty row
 * (inf / inf is NaN), 1 for a single candidate, no special case.  The record is popsift_hip_match.
 *
 * Pairs: the rule of popsift_hip_match_pairs, word for word, on these rows.  Condition 1 becomes "best >= 0"; in condition
 * 4, B is the guided search the other way round: for right descriptor j the nearest under (d, i') among { i' : ok(i', j) }.
 * Pairs in ascending l; *n_pairs, cap, ERR_TOO_SMALL and "cap = 0 with pairs = NULL asks for the count" as there; the same
 * bytes on every run.  popsift_hip_match_set_path does not apply: nothing is screened, every distance is exact.
 *
 * popsift_hip_match_guided returns the rows (parity hook and API): it reads model, M and max_err only, and still rejects
 * invalid other fields.  out has l's descriptor count entries.
 *
 * popsift_hip_devfeatures_from_host_points builds a set of n features and n descriptors from host memory, for callers who
 * bring keypoints and descriptors from elsewhere: feature i sits at (xy[2i], xy[2i+1]) with sigma = 0, num_ori = 1,
 * orientation[0] = 0, its desc[0] points to descriptor i, and the map is i -> i.  Errors as
 * popsift_hip_devfeatures_from_host, plus xy NULL with n > 0.  pair_points, match_sets and match_pairs work on such a set
 * like on any other.
 *
 * ERR_INVALID, before any GPU call: a NULL set, opts, or out / n_pairs; pairs NULL with cap > 0; an unknown model; max_err
 * not finite or <= 0; a non-finite entry of M; ratio negative, NaN or infinite; max_dist2 NaN; cross_check other than 0 / 1;
 * reserved != 0.  ERR_INVALID also when a map entry of either set names no feature (sets of
 * popsift_hip_devfeatures_from_host have -1 everywhere): as in popsift_hip_pair_points this is found on the device, when both
 * sets hold descriptors, and nothing is written then.  Empty l or r: OK; the rows of an empty r are the empty row above;
 * 0 pairs.
 *
 * All scratch belongs to l and is grow-only; one guided call at a time per left set; r is only read and may be the left set
 * of another thread's call.  Sets on different GPUs: what is needed of r is copied to l's GPU once per call.  One download
 * brings the count and the pairs (or the rows).
 *
 * The kernel (match_guided.hip): a wave owns POPSIFT_HIP_GUIDED_ROWS left rows and walks the right positions
 * POPSIFT_HIP_GUIDED_STEP at a time; the pairs that pass ok() wait in a queue of POPSIFT_HIP_GUIDED_QUEUE entries for their
 * distances (stated here for the tests of their edges; results do not depend on them).
 */
enum { POPSIFT_HIP_GUIDE_HOMOGRAPHY = 0, POPSIFT_HIP_GUIDE_EPIPOLAR = 1 };
#define POPSIFT_HIP_GUIDED_ROWS 64
#define POPSIFT_HIP_GUIDED_STEP 256
#define POPSIFT_HIP_GUIDED_QUEUE 512
typedef struct popsift_hip_guided_opts {   /* 64 bytes */
    int32_t model;        /* POPSIFT_HIP_GUIDE_*                                                  */
    float   M[9];         /* row major: right ~ M * left, or [x' y' 1] M [x y 1]^T = 0            */
    float   max_err;      /* px: transfer error in the right image / Sampson distance             */
    float   ratio;        /* as popsift_hip_match_opts                                            */
    float   max_dist2;
    int32_t cross_check;
    int32_t reserved[2];  /* must be 0 */
} popsift_hip_guided_opts;
void popsift_hip_default_guided_opts(popsift_hip_guided_opts* opts); /* {HOMOGRAPHY, identity, 2.0f, 0.8f, INFINITY, 0, {0, 0}} */
int  popsift_hip_match_guided(const popsift_hip_devfeatures* l, const popsift_hip_devfeatures* r,
                              const popsift_hip_guided_opts* opts, popsift_hip_match* out);
int  popsift_hip_match_pairs_guided(const popsift_hip_devfeatures* l, const popsift_hip_devfeatures* r,
                                    const popsift_hip_guided_opts* opts, popsift_hip_pair* pairs, size_t cap, int* n_pairs);
int  popsift_hip_devfeatures_from_host_points(int device, const float* desc, const float* xy, int n,
                                              popsift_hip_devfeatures** out);

int popsift_hip_get_report(const popsift_hip_ctx* ctx, popsift_hip_report* rep);
/* profile != 0: bracket every blur-level launch with HIP events (serialises the
 * octave streams; used by bench.py for the roofline object only). */
int popsift_hip_set_profile(popsift_hip_ctx* ctx, int profile); /* 0 off, 1 blur launches, 2 stages */

/* Debug / parity hooks (replace Octave::download_and_save_array,
 * sift_octave.cu:110-187).  kind: 0 = Gaussian plane, 1 = DoG plane. */
int popsift_hip_octave_dims(const popsift_hip_ctx* ctx, int octave, int* w, int* h);
int popsift_hip_download_plane(popsift_hip_ctx* ctx, int octave, int kind, int level, float* out);
/* Overwrite a plane (stage isolation in tests), then re-run later stages.  kind = 1 needs params.store_dog = 1
 * (POPSIFT_HIP_ERR_STATE otherwise: the consumers form DoG values from the Gaussian planes). */
int popsift_hip_upload_plane(popsift_hip_ctx* ctx, int octave, int kind, int level, const float* in);
/* Initial extrema of the last image, all octaves, in list order (params.feature_order). */
int popsift_hip_download_extrema(popsift_hip_ctx* ctx, popsift_hip_extremum* out, size_t cap, int* n);
/* Re-run extrema + orientation + descriptors on the planes currently in memory. */
int popsift_hip_rerun_keypoint_stages(popsift_hip_ctx* ctx);
/* Test switches of one context (no environment variables are read by this library).  Set them before the first
 * submit: DET_QCAP = candidate-queue entries the fast detection pass may use (small values force strips into the
 * slow pass); CAND_CAP / OHIST_CAP = initial capacity of the candidate buffer / initial number of extrema the orientation
 * stage serves in one pass (small values exercise the grow-and-rerun path of popsift_hip_wait); FAIL_ALLOC = n: the n-th device allocation
 * of this context from now on fails with POPSIFT_HIP_ERR_OOM (0 = off); DESC_ROWS = patch rows the loop descriptor
 * walks per pass (4 .. 96, default 96: small values make ordinary patches take the several passes that otherwise only
 * the largest patches take; results do not depend on it); DESC_LIST = list positions (samples of the patch's rows laid
 * end to end) the loop descriptor walks per pass, clamped to 64 .. the capacity of its row-end bit table (3456, the
 * default: patches of the coarsest levels have up to 5200 and take two passes; a pass that fills up ends inside a row
 * and the next one takes the rest of that row; results do not depend on it);
 * KP_WAVES = waves per image in the launches of
 * the orientation and descriptor kernels (a multiple of 32; default 8 per wave slot of the device; the orientation
 * kernel, whose waves take 16 keypoints at a time, launches an eighth of them, at least 8; results do not
 * depend on it; tools/kp_waves_sweep.sh: 8192 .. 131072 within 1.5 %); BLUR_PATH = which kernels build the pyramid's
 * plane-to-plane levels: 0 by plane size (default), 1 the one-tile-per-workgroup kernels only, 2 the strip-march kernels
 * wherever they apply, also on small planes (results do not depend on it: every path is bit-identical; the tests run
 * their small images through 2); BLUR_SEG = rows per segment of the march kernels (a multiple of 32; 0 = chosen from the
 * plane and the batch); BLUR_TILE_H = rows per tile of the one-tile-per-workgroup kernels: 0 by plane size (default: 64
 * from about 4.2 Mpx on, else 32), 32 or 64 for every plane, anything else is POPSIFT_HIP_ERR_INVALID (results do not
 * depend on it: every height is bit-identical; the tests run their small images through 64); PYR_TAIL = 0: the smallest octaves -- from the first whose plane fits one workgroup's LDS -- are
 * built by one launch (default), 1: by level launches like the others (results do not depend on it); DIRECT_PATH (Gauss
 * mode vlfeat-direct only) = 0: octave 0's levels by one fused launch (default), 1: by one level-0 launch per level
 * (results do not depend on it); SCALE_PATH (ScaleDirect only) = 0: level 0 of every octave by one launch and each
 * level of every octave by one launch (default), 1: one level-0 launch per octave and the default mode's level launches
 * per octave (results do not depend on it); DESC_CAP = initial capacity of the descriptor buffer, in descriptors (0 = the default,
 * 2 * max_extrema: small values exercise the grow-and-rerun path of popsift_hip_wait for descriptors); ORDER_COARSE
 * (POPSIFT_HIP_ORDER_RASTER only) = b in 0 .. 15, default 0: the ordering pass buckets the records by iy >> b instead of
 * by iy before it ranks each bucket by the whole tuple, so a bucket is a band of 2^b pixel rows, all levels, and with 15
 * the whole octave (results do not depend on it: the rank is taken under the whole tuple; the tests run the ranking
 * loop over long buckets with it). */
enum { POPSIFT_HIP_DEBUG_DET_QCAP = 1, POPSIFT_HIP_DEBUG_CAND_CAP = 2, POPSIFT_HIP_DEBUG_OHIST_CAP = 3,
       POPSIFT_HIP_DEBUG_FAIL_ALLOC = 4, POPSIFT_HIP_DEBUG_DESC_ROWS = 5, /* 6: retired, never reused */
       POPSIFT_HIP_DEBUG_KP_WAVES = 7, POPSIFT_HIP_DEBUG_BLUR_PATH = 8, POPSIFT_HIP_DEBUG_BLUR_SEG = 9,
       POPSIFT_HIP_DEBUG_PYR_TAIL = 10, POPSIFT_HIP_DEBUG_DIRECT_PATH = 11,
       POPSIFT_HIP_DEBUG_DESC_CAP = 12, POPSIFT_HIP_DEBUG_SCALE_PATH = 13, POPSIFT_HIP_DEBUG_ORDER_COARSE = 14,
       POPSIFT_HIP_DEBUG_DESC_LIST = 15, POPSIFT_HIP_DEBUG_BLUR_TILE_H = 16 };
int popsift_hip_debug_set(popsift_hip_ctx* ctx, int what, int value);

#ifdef __cplusplus
}
#endif
#endif /* POPSIFT_HIP_H */
