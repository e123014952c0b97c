/* kernels.h -- host-callable launchers of the HIP kernels (internal). */
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sift_types.h"

namespace popsift_hip {

struct Taps {
    float g[PS_GA];
};

/* One level launch; the planes are given as float offsets from the arena of the image's slot (sift_types.h, Slot): the
 * same arguments serve every image of a batch, the kernel adds its slot's arena (blockIdx.y). */
struct BlurArgs {
    int64_t src_off; /* plane l-1 (MODE 0)                     */
    int64_t dst_off; /* plane l                                */
    int64_t dog_off; /* DoG plane l-1 (MODE 0), < 0: not stored */
    int     w, h, pitch;
    int     tiles_x, tiles_y;
    /* MODE 1 (u8) / 2 (f32): the input image is Slot::input */
    int     in_w, in_h, in_pitch;
    float   shift;
    int     fast2x; /* level 0 only: the plane is the input stretched by exactly 2 with source coordinate X / 2 (2: u8 rows on 4-byte boundaries) */
    Taps    taps;
    /* level L-3 only: level 0 of the next octave = every second pixel of this plane (get_by_2_pick_every_second,
     * s_pyramid_build.cu:50-71), written by the same launch; < 0 otherwise */
    int64_t next0_off;
    int     next_pitch;
    /* level 0 only (the first launch of an image): words of the slot's Counters this launch clears, so that the image needs
     * no separate fill launch before detection; 0 otherwise */
    int     zero_words;
    /* march kernels (blur_march.hip) only: rows per segment, a multiple of 32; tiles_y = segments per strip */
    int     seg_rows;
};

/* how launch_blur picks the kernel of a plane-to-plane level launch (popsift_hip_debug_set BLUR_PATH / BLUR_SEG), and the
 * rows per tile of every launch that would take them from blur_tile_h (BLUR_TILE_H) */
struct BlurTune {
    int path;     /* 0: by plane size, 1: tile kernels only (pyramid.hip), 2: march kernels wherever they apply */
    int seg_rows; /* 0: chosen from the plane and the batch, else rows per segment (rounded to a multiple of 32) */
    int tile_h;   /* 0: blur_tile_h(w, h), else 32 or 64 rows for every plane */
};

int        blur_tile_w();
int        blur_tile_h(int w, int h); /* 32 or 64 rows, by plane size */
hipError_t launch_blur(const BlurArgs& a, const BatchDesc& bd, int nb, int mode, int span, int tile_h, hipStream_t s,
                       BlurTune tune = BlurTune{0, 0, 0});
/* blur_march.hip: level l >= 1 of a large plane, strips of 128 columns marched down 32 rows a step */
bool       blur_march_supported(const BlurArgs& a, int halo);
int        blur_march_seg_rows(int w, int h, int nb, int want_wgs);
hipError_t launch_blur_march(BlurArgs a, const BatchDesc& bd, int nb, int halo, int seg_rows, hipStream_t s);
/* two plane-to-plane level launches with 32-row tiles in one (small octaves) */
hipError_t launch_blur_duo(const BlurArgs& a, int span_a, const BlurArgs& b, int span_b, const BatchDesc& bd, int nb, hipStream_t s);

/* pyr_tail.hip: every octave from `first_oct` on in one launch, one workgroup per image (planes in LDS) */
#define PYR_TAIL_PAD 16             /* LDS border = the largest halo the tail takes */
#define PYR_TAIL_PLANE_FLOATS 17408 /* one LDS plane buffer incl. its border (two of them + the next octave's level 0: 154 KB) */
#define PYR_TAIL_MAX_L 10           /* Gaussian planes per octave (levels + 3) */
#define PYR_TAIL_MAX_PX 4096        /* pixels of the first plane the tail takes */
struct TailArgs {
    int     n_oct, first_oct, L;
    int     halo[PYR_TAIL_MAX_L];                     /* span - 1 of level l (the tap loops are rolled: no HALO instances) */
    float   g[PYR_TAIL_MAX_L][PYR_TAIL_PAD + 1];      /* taps of level l, zero beyond its span */
    int     w[PS_MAX_OCT], h[PS_MAX_OCT], pitch[PS_MAX_OCT];
    int64_t data_off[PS_MAX_OCT], plane_stride[PS_MAX_OCT]; /* floats from the arena base / between planes */
};
bool       pyr_tail_fits(int w, int h);
hipError_t launch_pyr_tail(const TailArgs& a, const BatchDesc& bd, int nb, hipStream_t s);

/* pyr_direct.hip: octave 0 of the vlfeat-direct Gauss mode (every level blurred straight from the input image), all
 * L Gaussian planes (+ the L-1 DoG planes) in one launch */
struct DirectArgs {
    int64_t      dst_off;      /* plane 0 of octave 0; plane l at dst_off + l * plane_stride */
    int64_t      dog_off;      /* DoG plane 0 of octave 0, < 0: not stored */
    int64_t      plane_stride; /* floats */
    int64_t      next0_off;    /* level 0 of octave 1 = every second pixel of level L-3, < 0: no octave 1 */
    const float* taps;         /* L x PS_GA abs_o0 taps, zero beyond each level's span (device memory of the context) */
    int          w, h, pitch, next_pitch;
    int          tiles_x, tiles_y;
    int          in_w, in_h, in_pitch;
    float        shift;
    int          L;
    int          halo[PS_MAX_PLANES]; /* span - 1 of level l */
    int          zero_words;          /* words of the slot's Counters the launch clears */
};
int        pyr_direct_tile_h();
hipError_t launch_pyr_direct(const DirectArgs& a, const BatchDesc& bd, int nb, int is_f32, hipStream_t s);
/* the per-level path of the same mode (popsift_hip_debug_set DIRECT_PATH 1): octave 1's level 0 and the DoG planes */
hipError_t launch_pick_every_second(int64_t src_off, int w, int h, int pitch, int64_t dst_off, int nw, int nh, int npitch,
                                    const BatchDesc& bd, int nb, hipStream_t s);
hipError_t launch_dog_batch(int64_t lower_off, int64_t upper_off, int64_t dog_off, int64_t n, const BatchDesc& bd, int nb,
                            hipStream_t s);

/* pyramid.hip, the ScaleDirect scaling mode (every octave's level 0 straight from the input image): */
/* level 0 of every octave of the batch in one launch, horizontal taps dd[o] (d_dd: PS_MAX_OCT x PS_GA floats of the
 * context), vertical taps vt (inc[0]); base: the input image, octave 0's shift / fast2x, zero_words, taps ignored */
hipError_t launch_pyr_level0_octaves(const BlurArgs& base, const Taps& vt, const float* d_dd, const PyrDesc* d_pd,
                                     const PyrDesc& pd, const BatchDesc& bd, int nb, int halo, int is_f32, hipStream_t s);
/* level `level` >= 1 of every octave of the batch in one launch (base: the taps inc[level]; DoG when stored) */
hipError_t launch_blur_octaves(const BlurArgs& base, int level, const PyrDesc* d_pd, const PyrDesc& pd, const BatchDesc& bd,
                               int nb, int halo, hipStream_t s);
/* level 0 of one octave with separate vertical taps (the yardstick path, popsift_hip_debug_set SCALE_PATH 1) */
hipError_t launch_blur_level0_sep(const BlurArgs& a, const Taps& vt, const BatchDesc& bd, int nb, int halo, int is_f32,
                                  hipStream_t s);
int        scale_tile_h(); /* rows of the tiles of the three launches above */

/* extrema.hip */
hipError_t launch_dog_plane(float* dog, const float* upper, const float* lower, size_t n, hipStream_t s); /* debug / test downloads */
int        extrema_units(int w, int h); /* wave-sized work units of the detection kernel */
/* Every launcher below takes the slot table `bd` (passed to the kernels by value) and the number of images nb = gridDim.y. */
/* mid: event recorded between detection and refinement (stage timing), or null; ma: the masks of the batch
 * (popsift_hip_submit_batch_masked), or null when no image has one */
hipError_t launch_extrema(const PyrDesc& pd, const PyrDesc* d_pd, const BatchDesc& bd, int nb, const SiftConsts& sc, int cand_cap,
                          bool filtered, hipStream_t s, hipEvent_t mid, const MaskArgs* ma);

/* keypoint.hip */
/* k_orientation: histograms, peaks, the Ext record of EVERY extremum of the lists and one partial sum per group of
 * scan_chunk() / scan_partials_per_chunk() extrema; hist_cap: extrema from that list position on get no orientation;
 * blocks: the launch size of the one-entry-per-wave keypoint kernels, in waves (the launch takes its share of it) */
hipError_t launch_orientation(const PyrDesc* d_pd, const BatchDesc& bd, int nb, const SiftConsts& sc, bool filtered, int hist_cap,
                              int blocks, hipStream_t s);
int        scan_chunk(); /* extrema per k_scan_apply workgroup */
int        scan_partials_per_chunk(); /* partial sums k_orientation leaves per scan_chunk() extrema */
hipError_t launch_descriptors(const PyrDesc* d_pd, const BatchDesc& bd, int nb, const SiftConsts& sc, int desc_cap, int blocks,
                              hipStream_t s);

/* desc_modes.hip: the descriptor kernel of desc_mode GRID, NOTILE, IGRID or ILOOP (launch_descriptors calls it for those) */
hipError_t launch_desc_modes(const PyrDesc* d_pd, const BatchDesc& bd, int nb, const SiftConsts& sc, int desc_cap, int blocks,
                             hipStream_t s);

/* k_scan_apply: the lists' Ext records and group partial sums are there (k_orientation, or k_frame_place for given angles) */
hipError_t launch_scan_apply(const PyrDesc* d_pd, const BatchDesc& bd, int nb, const SiftConsts& sc, int n_chunks, int desc_cap,
                             hipStream_t s);

/* describe.hip: caller-supplied frames (popsift_hip_describe_batch).  n_max: the most frames of an image of the batch.
 * frame_count + frame_place resolve each frame to (octave, level) and partition the frames stably by octave into the
 * InitExt lists (ext_ct, perm / inv; with `given` also the Ext records and k_orientation's partial sums); frame_out, after
 * the descriptor kernel, moves the feature records to caller order and rewrites the descriptor -> feature map. */
constexpr int FRAME_CHUNK = 256;
int        frame_chunks(int n_max);
hipError_t launch_frame_count(const PyrDesc* d_pd, const FrameBatch& fb, int nb, const SiftConsts& sc, int given, int n_max,
                              hipStream_t s);
hipError_t launch_frame_place(const PyrDesc* d_pd, const BatchDesc& bd, const FrameBatch& fb, int nb, const SiftConsts& sc,
                              int given, int n_max, hipStream_t s);
hipError_t launch_frame_out(const BatchDesc& bd, const FrameBatch& fb, int nb, int desc_cap, int n_max, hipStream_t s);

/* filter.hip: grid filter between refinement and orientation (s_filtergrid.cu:109-322) */
bool       filter_supported(int n_oct, int max_extrema, int grid_size);
size_t     filter_hist_bytes(int grid_size);
hipError_t launch_filter(int n_oct, const SiftConsts& sc, const BatchDesc& bd, int nb, hipStream_t s);

/* strongest.hip: the keep-strongest pass between refinement and orientation, the rule of include/popsift_hip.h: the lists
 * of `sb` (counts ext_ct, capped by max_extrema) thinned to the `keep` >= 1 largest responses per image, stably, into the
 * second lists; ext_ct becomes the survivors'.  strongest_chunks: chunk offsets a slot needs per octave */
int        strongest_chunks(int max_extrema);
hipError_t launch_strongest(const PyrDesc& pd, const PyrDesc* d_pd, const SiftConsts& sc, int keep, const StrongBatch& sb, int nb,
                            hipStream_t s);

/* order.hip: the per-octave extrema lists of `ob` (counts ext_ct, capped by max_extrema) into raster order, the rule of
 * include/popsift_hip.h.  order_rows: row counters a slot needs for this pyramid; coarse: ORDER_COARSE, 0 .. 15 */
size_t     order_rows(const PyrDesc& pd);
hipError_t launch_order(const PyrDesc& pd, const SiftConsts& sc, int coarse, const OrderBatch& ob, int nb, hipStream_t s);

/* The matchers.  A sweep's n_split comes from splits() (top2.h) with the sweep's shape: rows per workgroup, searched rows
 * per tile and the workgroups to aim at; `partial` holds partial_bytes(l_len, n_split, record) bytes. */
constexpr int M_LT = 32, M_RT = 64, M_GROUPS = 2048;    /* match.hip; >= 8 workgroups per CU; records: Top2<float> */
constexpr int S_LB = 128, S_RB = 128, S_GROUPS = 1024;  /* match_mfma.hip; >= 2 resident workgroups per CU x 2 rounds */
constexpr int U_LB = 128, U_RB = 128, U_GROUPS = 1024;  /* match_u8.hip; as S_*; records: Top2<int> */
constexpr size_t S_CAND_BYTES = 32;                     /* match_mfma.hip's record */
/* match.hip: brute-force 2-NN (features.cu:157-300) */
hipError_t launch_match(const float* ldesc, int l_len, const float* rdesc, int r_len, int n_split, void* partial,
                        popsift_hip_match* out, const int* rows, const int* n_rows, int first_row, int row_end,
                        hipStream_t s);
/* match_mfma.hip: matrix-core screening + exact re-rank of the survivors */
hipError_t launch_norms(const float* desc, int n, float* out, hipStream_t s);
hipError_t launch_match_screen(const float* ldesc, int l_len, const float* rdesc, int r_len, const float* lnorm,
                               const float* rnorm, int n_split, void* partial, popsift_hip_match* out, int* redo_list,
                               int* redo_count, hipStream_t s);
/* match_pairs.hip: 2-NN rows -> pair list.  fwd: the forward sweep's rows; a row without a candidate (best < 0, the guided
 * matcher's) yields no pair.  back: the reverse sweep's rows (null without the cross-check): of the flagged right
 * descriptors in the order of `list`, found through rank; or, with rank == null, one row per right descriptor.  counts:
 * pair_count_blocks(n) ints of scratch for a compaction over n elements.  l_len and r_len >= 1. */
int        pair_count_blocks(int n);
hipError_t launch_pair_targets(const popsift_hip_match* fwd, int l_len, int r_len, float ratio, float max_dist2, int* flags,
                               int* counts, int* list, int* rank, int* n_list, hipStream_t s);
hipError_t launch_pair_emit(const popsift_hip_match* fwd, int l_len, float ratio, float max_dist2,
                            const popsift_hip_match* back, const int* rank, int* counts, popsift_hip_pair* pairs, int* n_pairs,
                            hipStream_t s);
/* the rows of a list into a contiguous buffer, for T = float and T = uint8_t (descriptors of 128 T, 16-byte aligned) */
template <class T>
hipError_t launch_gather_rows(const T* desc, const int* list, int n, T* out, hipStream_t s);
/* match_u8.hip: exact integer 2-NN of byte descriptors (128 bytes each, 16-byte aligned) on the i8 matrix instructions.
 * Norms are |x - 128|^2 as int; `out` receives l_len rows whose distances are integers held in floats. */
hipError_t launch_norms_u8(const uint8_t* desc, int n, int* out, hipStream_t s);
hipError_t launch_match_u8(const uint8_t* ldesc, int l_len, const int* lnorm, const uint8_t* rdesc, int r_len,
                           const int* rnorm, int n_split, void* partial, popsift_hip_match* out, hipStream_t s);
/* match_gallery.hip (one byte set against a gallery of byte sets) launches its own kernels -- the grouped k_match_u8 over
 * a work list, its segmented finish and the pair stage -- from its two entry points; of the launchers above it uses
 * launch_norms_u8, launch_gather_rows and launch_match_u8 (the reverse sweep of the cross-check), U_LB / U_RB / U_GROUPS. */
/* match_links.hip (any list of member pairs of one gallery) likewise launches its own kernels -- k_match_gallery with a left
 * side per work item, a finish and a pair stage that find a row's link in a table -- and uses launch_norms_u8 and
 * launch_gather_rows (the reverse sweep of the cross-check), U_LB / U_RB / U_GROUPS. */
/* Feature records (72-byte popsift::Feature layout) with device descriptor pointers for a cloned set */
hipError_t launch_clone_features(const popsift_hip_feature* feats, int n_feat, float* desc_base, void* out, hipStream_t s);

/* desc_bytes.hip: n_desc descriptors (128 floats each, 16-byte aligned) -> 128 bytes each, the rule of
 * include/popsift_hip.h (popsift_hip_fetch_item_u8) */
hipError_t launch_desc_bytes(const float* desc, int n_desc, uint8_t* out, hipStream_t s);

}  // namespace popsift_hip
