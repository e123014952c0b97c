"""The images of tests/test_gpu_blur_paths.py and, restated on the host, which instance of the tile kernels a launch takes.

No GPU and no library here: plain Python.  tile_instance() says what launch_blur (popsift_amd/csrc/pyramid.hip) does with a
launch it hands to the tile kernels, level0_fast2x() what input_args (ctx.hip) sets for the level that samples the input
image.  tests/test_blur_cases.py holds the case list below to every 64-row instance with them, so that the list cannot
silently stop reaching one; a change of the dispatch is made here and there."""

# (name, parameters, (seed, width, height) of popsift_amd.synth.synth); store_dog is the library's alone, the oracle keeps
# its DoG planes always (oracle_kw)
CASES = [
    ("default_400x300", dict(), (61, 400, 300)),
    ("width_not_multiple_of_128_333x257", dict(), (62, 333, 257)),
    ("one_strip_60x200", dict(), (63, 60, 200)),
    ("tall_9x300", dict(), (42, 9, 300)),
    ("thin_300x9", dict(), (25, 300, 9)),
    ("tiny_17x13", dict(), (20, 17, 13)),
    ("no_upscale_257x129", dict(upscale_factor=0.0), (41, 257, 129)),
    ("levels5_sigma1p3", dict(levels=5, sigma=1.3), (64, 260, 200)),
    ("levels2_sigma2", dict(levels=2, sigma=2.0), (65, 220, 170)),
    ("levels6_sigma1", dict(levels=6, sigma=1.0), (66, 200, 260)),
    ("opencv_gauss", dict(sift_mode=1, gauss_mode=3), (67, 300, 220)),
    ("float_input", dict(), (68, 280, 210)),
    ("deep_octaves_40x24", dict(octaves=7), (40, 40, 24)),            # planes shrink to 2 x 1: all but octave 0 in the tail
    ("tail_from_a_plane_that_just_fits_256x176", dict(upscale_factor=0.0), (69, 256, 176)),  # octave 1 = 128 x 88
    # -- for the 64-row tiles (BLUR_TILE_H = 64): the instances and edges the cases above do not reach --
    ("levels2_sigma1p8", dict(levels=2, sigma=1.8), (71, 230, 170)),  # halos 6 8 11 15 21: H = 22, and 16 by halo 15
    ("initial_blur4_sigma2", dict(initial_blur=4.0, sigma=2.0), (72, 160, 120)),      # level 0: halo 30 from u8, 256 lanes
    ("initial_blur4_sigma2_f32", dict(initial_blur=4.0, sigma=2.0), (72, 160, 120)),  # ... and from f32
    # level 0: halo 19 (H = 22) without the exact-2x paths (OpenCV's shift)
    ("initial_blur2p5_sigma2_opencv", dict(initial_blur=2.5, sigma=2.0, sift_mode=1, gauss_mode=3), (73, 150, 110)),
    # stored DoG: H = 13 takes 256 lanes, not lp13; planes 666 / 333 / 167 / 84 / 42 wide: next0 stores at odd widths
    ("store_dog_default", dict(store_dog=1), (74, 333, 257)),
    ("store_dog_levels2_sigma2", dict(store_dog=1, levels=2, sigma=2.0), (75, 220, 170)),  # stored DoG at H = 13, 16 and 30
    # Last tiles of one pixel column and of one, two and three rows (the 4-row blocks of a lane mask the rest).  Twice the
    # input has an even number of rows, so 64 k + 1 rows in octave 0 itself need upscale_factor = 0:
    # 257 x 193 -> octave 0 = 514 x 386 (2 columns, 6 * 64 + 2 rows), octave 1 = 257 x 193 (1 column, 3 * 64 + 1 rows, its
    # level 0 written by octave 0's next0 stores), octave 2 = 129 x 97 (1 column, 64 + 33 rows)
    ("rows_193_after_upscale", dict(), (76, 257, 193)),
    # 257 x 193, not upscaled -> octave 0 = 257 x 193: level 0 from the input too; octave 1 = 129 x 97
    ("rows_193_no_upscale", dict(upscale_factor=0.0), (77, 257, 193)),
    # 257 x 195, not upscaled -> octave 0 = 257 x 195 (1 column, 3 * 64 + 3 rows), octave 1 = 129 x 98
    ("rows_195_no_upscale", dict(upscale_factor=0.0), (78, 257, 195)),
]
F32_CASES = ("float_input", "initial_blur4_sigma2_f32")  # submitted as float32 in [0, 1)

BUCKETS = (4, 5, 6, 7, 8, 10, 13, 16, 22, 30)  # the HALO instances (PS_CASE lists of pyramid.hip)


def oracle_kw(kw):
    """a case's parameters without those only the library has"""
    return {k: v for k, v in kw.items() if k != "store_dog"}


def tile_instance(mode, tile_h, halo, store_dog):
    """launch_blur's choice for a launch that goes to the tile kernels: (kernel family, HALO bucket, lanes per workgroup).
    mode 0: plane to plane, 1: level 0 from a u8 image, 2: from an f32 image; halo = span - 1; store_dog: the launch also
    writes a DoG plane (mode 0 with params.store_dog).  At 32 rows the planes of at most 256 tiles per launch leave for
    k_blur_small and k_blur_duo by their size, which is not restated here."""
    if mode not in (0, 1, 2) or tile_h not in (32, 64) or not 0 <= halo <= 30:
        raise ValueError((mode, tile_h, halo))
    bucket = next(b for b in BUCKETS if halo <= b)
    if tile_h == 64:
        if mode == 0 and not store_dog and 10 < halo <= 13:
            return ("k_blur_tile64_lp", 13, 512)
        return ("k_blur_tile", bucket, 512 if halo <= 10 else 256)
    return ("k_blur_tile", bucket, 256)


def level0_fast2x(kw, width, is_f32):
    """input_args' fast2x for a host image of `width` pixels per row: 0 the general bilinear path, 1 the exact 2x upscale,
    2 the same from a u8 image whose rows start on 4-byte boundaries (a host image is uploaded with pitch = width)"""
    up = kw.get("upscale_factor", 1.0)
    shift = 0.5 * 2.0 ** up if kw.get("sift_mode", 0) in (0, 2) else 0.5  # input_shift: PopSift and VLFeat sampling
    if not (up == 1.0 and shift == 1.0):
        return 0
    return 2 if not is_f32 and width % 4 == 0 else 1


def case_instances(name, kw, spec, spans, tile_h):
    """every tile launch of a case's octave 0 (the other octaves repeat levels 1 ..): a list of
    (mode, store_dog, fast2x or None, tile_instance) from the spans of the case's Gauss table, level 0 first"""
    is_f32 = name in F32_CASES
    store = bool(kw.get("store_dog", 0))
    out = [(2 if is_f32 else 1, False, level0_fast2x(kw, spec[1], is_f32), tile_instance(2 if is_f32 else 1, tile_h, spans[0] - 1, False))]
    for s in spans[1:]:
        out.append((0, store, None, tile_instance(0, tile_h, s - 1, store)))
    return out
