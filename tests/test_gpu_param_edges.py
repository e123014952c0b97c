"""The edges of the parameter range popsift_hip_ctx_create accepts, against the oracle.

The rest of the GPU suite stays inside levels 2 .. 6, sigma 1 .. 2 and upscale -1 .. +1 (the window fuzz_cases draws
from by default).  What only the rest of the accepted range reaches:
  - k_detect at LEVELS 7, 8 and 9 (36 of launch_detect's 96 instances: 3 sift modes x fast / slow pass x DoG on the fly
    or stored), the heaviest code of the library (238 .. 256 VGPRs);
  - k_pyr_tail at its largest L (PYR_TAIL_MAX_L = 10, levels 7), and above it (levels 8, 9: L = 11, 12) the plan without
    the tail, whose smallest octaves go through level launches (and k_blur_duo, but not under BLUR_PATH = 2);
  - filters of one and two taps past the centre (sigma < 1), which go through the HALO-4 tile and march instances and the
    tail's rolled tap loop;
  - level 0's sigma through fabsf (sigma0 < initial_blur * 2^upscale: sigma < 1 at upscale +1);
  - the level-0 bilinear reads at upscale +2 / -2 (sampling shift 2.0 / 0.125);
  - sides of 32767 pixels, where k_detect's candidate packing x | (y << 16) comes within 2^18 of the sign bit, and the
    ERR_INVALID one pixel further.
Bars as everywhere: Gaussian and DoG planes bit-exact, the extremum set bit-exact, orientations and descriptors by
util.feature_parity (grid descriptors in the oracle's frame).  Every failure names the case, octave and level."""
import os

import numpy as np
import pytest

import fuzz_cases
import planted as P
from popsift_amd.synth import synth
from test_gpu_count_edges import check as planted_check
from util import bits, feature_parity, sorted_features

pytestmark = pytest.mark.gpu

DET_QCAP, BLUR_PATH, BLUR_SEG, PYR_TAIL = 1, 8, 9, 10
THREADS = min(os.cpu_count() or 4, 16)

# (name, popsift_hip_debug_set switches): the default plan, the tile kernels without the tail, the march kernels in
# 32-row segments (with BLUR_PATH = 2 no level is paired into k_blur_duo either)
BLUR_SETTINGS = [("default", ()), ("tiles, no tail", ((BLUR_PATH, 1), (PYR_TAIL, 1))),
                 ("march, 32-row segments", ((BLUR_PATH, 2), (BLUR_SEG, 32)))]

OPENCV = dict(sift_mode=1, gauss_mode=3)

RANGE_CASES = [
    ("levels7", dict(levels=7), (31, 240, 180)),                     # L = 10: the tail at PYR_TAIL_MAX_L
    ("levels8", dict(levels=8), (32, 240, 180)),                     # L = 11: no tail
    ("levels9", dict(levels=9), (33, 240, 180)),                     # L = 12, the largest
    ("levels9_opencv", dict(levels=9, **OPENCV), (34, 240, 180)),
    ("levels9_vlfeat", dict(levels=9, sift_mode=2), (35, 240, 180)),
    ("levels9_sigma2", dict(levels=9, sigma=2.0), (36, 240, 180)),
    ("levels9_sigma0p5", dict(levels=9, sigma=0.5), (37, 200, 150)),  # spans of 2 taps: halo 1
    ("sigma0p6", dict(sigma=0.6), (38, 200, 150)),                   # halo 2; level 0 through fabsf
    ("levels0", dict(levels=0), (39, 200, 150)),                     # clamped to 2
    ("levels1", dict(levels=1), (40, 200, 150)),
    ("upscale+2", dict(upscale_factor=2.0), (41, 100, 80)),          # level-0 shift 2.0
    ("upscale-2", dict(upscale_factor=-2.0), (42, 640, 480)),        # level-0 shift 0.125
    ("levels7_odd_333x257", dict(levels=7), (43, 333, 257)),
    ("levels9_odd_333x257", dict(levels=9), (44, 333, 257)),
    ("levels7_tiny_17x13", dict(levels=7), (45, 17, 13)),
    ("levels9_tiny_17x13", dict(levels=9), (46, 17, 13)),
]


def n_planes(kw):
    return max(2, kw.get("levels", 3)) + 3


def oracle_run(O, kw, img):
    return O.Oracle(O.default_params(**kw), threads=THREADS).run(img)


def device_run(hip, kw, img, debug=()):
    ctx = hip.Context(hip.default_params(**kw))
    for what, value in debug:
        ctx.debug_set(what, value)
    ctx.submit(img)
    ctx.wait()
    return ctx


def check_planes(orc, ctx, L, what):
    """every Gaussian and DoG plane of every octave, bit for bit"""
    assert ctx.report().num_octaves == orc.num_octaves, "%s: %d octaves, oracle %d" % (
        what, ctx.report().num_octaves, orc.num_octaves)
    for o in range(orc.num_octaves):
        assert tuple(ctx.octave_dims(o)) == tuple(orc.octave_dims(o)), "%s: octave %d dims" % (what, o)
        for kind, n, name in ((0, L, "gauss"), (1, L - 1, "dog")):
            for l in range(n):
                a, b = orc.plane(o, kind, l), ctx.plane(o, kind, l)
                bad = bits(a) != bits(b)
                assert not bad.any(), "%s: octave %d %s level %d: %d values differ, max %g" % (
                    what, o, name, l, int(bad.sum()), float(np.nanmax(np.abs(a - b))))


def ext_key(e):
    return sorted(zip(e["octave"].tolist(), e["lpos"].tolist(), bits(e["xpos"]).tolist(), bits(e["ypos"]).tolist()))


def check_extrema(want, ctx, what):
    """the extremum set bit for bit; `want` is an oracle or the extrema of another run"""
    eo = want.extrema() if hasattr(want, "extrema") else want
    eh = ctx.extrema()
    if ext_key(eo) != ext_key(eh):
        n = max(int(eo["octave"].max()) + 1 if len(eo) else 0, int(eh["octave"].max()) + 1 if len(eh) else 0)
        rows = []
        for o in range(n):
            a, b = set(ext_key(eo[eo["octave"] == o])), set(ext_key(eh[eh["octave"] == o]))
            if a != b:
                lv = sorted({k[1] for k in a ^ b})
                rows.append("octave %d: %d vs %d, %d only in the reference, %d only on the device, at levels %s" % (
                    o, len(a), len(b), len(a - b), len(b - a), lv))
        raise AssertionError("%s: extrema differ\n    %s" % (what, "\n    ".join(rows)))


def canon(feats, desc):
    f, d = sorted_features(feats, desc)
    return (f["debug_octave"].copy(), bits(f["xpos"]), bits(f["ypos"]), bits(f["sigma"]), f["num_ori"].copy(),
            bits(f["orientation"]), bits(d))


def same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def check_features(orc, ctx, kw, what):
    fh, dh = ctx.fetch()
    ok, msg, _ = feature_parity(orc, fh, dh, grid_mode=kw.get("desc_mode") == 2)
    assert ok, "%s: %s" % (what, msg)
    return canon(fh, dh)


# 1. oracle parity over the range, under three blur plans ---------------------------------------------------------

@pytest.mark.parametrize("name,kw,spec", RANGE_CASES, ids=[c[0] for c in RANGE_CASES])
def test_range_edges_against_the_oracle(oracle_mod, gpu_hip, name, kw, spec):
    img = synth(*spec)
    L = n_planes(kw)
    orc = oracle_run(oracle_mod, kw, img)
    first = None
    for setting, debug in BLUR_SETTINGS:
        what = "%s [%s]" % (name, setting)
        ctx = device_run(gpu_hip, kw, img, debug)
        if setting == "default" and L == 10:
            # the default plan builds the smallest octaves with ONE k_pyr_tail launch at L = PYR_TAIL_MAX_L (enqueue_pyramid:
            # every span of 2 .. PYR_TAIL_PAD + 1 taps; the kernel trace of this file shows the launch)
            _, span, _ = ctx.gauss_table()
            assert len(span) == 10 and span[1:].min() >= 2 and span[1:].max() <= 17, (what, span)
        check_planes(orc, ctx, L, what)
        check_extrema(orc, ctx, what)
        if first is None:
            first = check_features(orc, ctx, kw, what)
        else:
            fh, dh = ctx.fetch()
            assert same(canon(fh, dh), first), "%s: features differ from the default plan's" % what
        ctx.close()


def test_levels_below_two_are_levels_two(gpu_hip):
    img = synth(39, 200, 150)
    res = []
    for levels in (0, 1, 2):
        ctx = device_run(gpu_hip, dict(levels=levels), img)
        res.append((canon(*ctx.fetch()), ctx.plane(1, 0, 4).copy(), ctx.plane(2, 1, 3).copy()))
        ctx.close()
    for k in (1, 2):
        assert same(res[0][0], res[k][0]) and np.array_equal(bits(res[0][1]), bits(res[k][1])) and \
            np.array_equal(bits(res[0][2]), bits(res[k][2])), "levels %d" % (k - 1)


# 2. every LEVELS 7 .. 9 instance of launch_detect --------------------------------------------------------------------

@pytest.mark.parametrize("sift_mode", [0, 1, 2])
@pytest.mark.parametrize("levels", [7, 8, 9])
def test_detection_instances(oracle_mod, gpu_hip, levels, sift_mode):
    """fast and slow pass (DET_QCAP = 4 sends strips into the slow pass), DoG on the fly and stored (store_dog = 1: the
    FLY = false instances and the non-fly k_refine): the same extrema as the oracle and bit-identical results"""
    kw = dict(levels=levels, sift_mode=sift_mode, **(dict(gauss_mode=3) if sift_mode == 1 else {}))
    img = synth(50 + levels, 240, 180)
    orc = oracle_run(oracle_mod, kw, img)
    base = None
    for store_dog in (0, 1):
        for qcap in (None, 4):
            what = "levels %d sift_mode %d store_dog %d %s" % (levels, sift_mode, store_dog,
                                                                "slow pass" if qcap else "fast pass")
            ctx = device_run(gpu_hip, dict(kw, store_dog=store_dog), img, () if qcap is None else ((DET_QCAP, qcap),))
            check_extrema(orc, ctx, what)
            if base is None:
                check_planes(orc, ctx, levels + 3, what)
                base = check_features(orc, ctx, kw, what)
            else:
                if store_dog and qcap is None:
                    check_planes(orc, ctx, levels + 3, what)
                assert same(canon(*ctx.fetch()), base), "%s: features differ from the fast pass on the fly" % what
            ctx.close()


# 3. descriptor modes at levels 9 ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("desc_mode", [0, 1, 2, 3, 4])
def test_descriptor_modes_at_levels_9(oracle_mod, gpu_hip, desc_mode):
    """loop, iloop, grid, igrid, notile: the refined lpos of this image reach L - 1 = 11"""
    kw = dict(levels=9, desc_mode=desc_mode, norm_mode=desc_mode % 2)
    img = synth(5, 200, 150)
    orc = oracle_run(oracle_mod, kw, img)
    assert orc.extrema()["lpos"].max() == 11
    ctx = device_run(gpu_hip, kw, img)
    check_extrema(orc, ctx, "desc_mode %d" % desc_mode)
    check_features(orc, ctx, kw, "desc_mode %d" % desc_mode)
    ctx.close()


# 4. a 1080p batch at levels 9 ----------------------------------------------------------------------------------------

def test_batch_at_levels_9_1080p(oracle_mod, gpu_hip):
    """two 1080p images in one submit: nb >= 2 and >= 12 Mpx per launch, so launch_blur takes the march kernels by itself;
    every item equals its own single submit (features, orientations, descriptors, two planes), a single submit the oracle"""
    kw = dict(levels=9)
    imgs = [synth(100 + k, 1920, 1080) for k in range(2)]
    want, planes = [], []
    single = gpu_hip.Context(gpu_hip.default_params(**kw))
    for k, im in enumerate(imgs):
        single.submit(im).wait()
        if k == 0:
            orc = oracle_run(oracle_mod, kw, im)
            check_extrema(orc, single, "1080p levels 9 single")
            for o, kind, l in ((0, 0, 11), (0, 1, 10), (3, 0, 7), (orc.num_octaves - 1, 1, 5)):
                assert np.array_equal(bits(single.plane(o, kind, l)), bits(orc.plane(o, kind, l))), \
                    "1080p levels 9 single: octave %d kind %d level %d" % (o, kind, l)
            fh, dh = single.fetch()
            ok, msg, _ = feature_parity(orc, fh, dh)
            assert ok, "1080p levels 9 single: " + msg
            orc.close()
        want.append(canon(*single.fetch()))
        planes.append((single.plane(0, 0, 11).copy(), single.plane(1, 1, 9).copy()))
    single.close()
    ctx = gpu_hip.Context(gpu_hip.default_params(**kw))
    ctx.submit_batch(imgs)
    assert len(ctx.wait_batch()) == 2
    for k in range(2):
        assert same(canon(*ctx.fetch_item(k)), want[k]), "batch item %d" % k
    # the debug download reads slot 0
    assert np.array_equal(bits(ctx.plane(0, 0, 11)), bits(planes[0][0])), "batch item 0: octave 0 gauss level 11"
    assert np.array_equal(bits(ctx.plane(1, 1, 9)), bits(planes[0][1])), "batch item 0: octave 1 dog level 9"
    ctx.close()


# 8. the side-length limit ----------------------------------------------------------------------------------------------

SIDE_CASES = [
    ("32767x16_upscale0", dict(upscale_factor=0.0), (32767, 16)),
    ("16x32767_upscale0_opencv", dict(upscale_factor=0.0, **OPENCV), (16, 32767)),   # 6 usable columns
    ("16383x12_upscale1", dict(), (16383, 12)),                                        # octave 0: 32766 x 24
    ("12x16383_upscale1", dict(), (12, 16383)),                                        # octave 0: 24 x 32766 rows
]


@pytest.mark.parametrize("name,kw,shape", SIDE_CASES, ids=[c[0] for c in SIDE_CASES])
def test_longest_side_against_the_oracle(oracle_mod, gpu_hip, name, kw, shape):
    w, h = shape
    img = synth(60 + len(name), w, h)
    orc = oracle_run(oracle_mod, kw, img)
    assert max(orc.octave_dims(0)) >= 32766 and orc.ext_counts()[0] > 0, (name, orc.octave_dims(0), orc.ext_counts())
    ctx = device_run(gpu_hip, kw, img)
    check_planes(orc, ctx, n_planes(kw), name)
    check_extrema(orc, ctx, name)
    e = ctx.extrema()
    long_axis = "ypos" if h > w else "xpos"
    assert e[e["octave"] == 0][long_axis].max() > 32000, name   # candidates packed near the top of 16 bits
    check_features(orc, ctx, kw, name)
    ctx.close()


@pytest.mark.parametrize("kw,shape", [(dict(upscale_factor=0.0), (32768, 16)), (dict(upscale_factor=0.0), (16, 32768)),
                                      (dict(), (16384, 12)), (dict(), (12, 16384))],
                         ids=["32768x16_upscale0", "16x32768_upscale0", "16384x12_upscale1", "12x16384_upscale1"])
def test_side_beyond_the_limit_is_refused_and_the_context_recovers(gpu_hip, kw, shape):
    """a scaled side of 32768 is ERR_INVALID from the submit; the same context then gives a valid image what a fresh
    context gives, bit for bit"""
    w, h = shape
    ctx = gpu_hip.Context(gpu_hip.default_params(**kw))
    with pytest.raises(gpu_hip.PopsiftHipError) as err:
        ctx.submit(synth(3, w, h))
    assert err.value.status == gpu_hip.ERR_INVALID, str(err.value)
    img = synth(4, 300, 200)
    ctx.submit(img).wait()
    got = (canon(*ctx.fetch()), ctx.plane(0, 0, 3).copy(), ctx.plane(2, 1, 2).copy(), ctx.report().num_octaves)
    ctx.close()
    fresh = device_run(gpu_hip, kw, img)
    want = (canon(*fresh.fetch()), fresh.plane(0, 0, 3).copy(), fresh.plane(2, 1, 2).copy(), fresh.report().num_octaves)
    fresh.close()
    assert got[3] == want[3] and len(want[0][0]) > 0
    assert same(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(bits(got[2]), bits(want[2]))


# 9. a fixed-seed slice of the wide fuzz draws ----------------------------------------------------------------------------

def test_thirty_wide_random_configurations(oracle_mod, gpu_hip):
    """fuzz_cases.random_case(wide=True): levels 0 .. 9, sigma 0.4 .. 2, upscale -2 .. 2, every sift mode; every third case
    through the march kernels in 32-row segments"""
    rng = np.random.default_rng(20261015)
    failures = []
    for case in range(30):
        kw, img = fuzz_cases.random_case(rng, case, max_w=240, max_h=180, wide=True)
        debug = ((BLUR_PATH, 2), (BLUR_SEG, 32)) if case % 3 == 2 else ()
        ok, msg = fuzz_cases.check_case(oracle_mod, gpu_hip, kw, img, threads=THREADS, debug=debug)
        if not ok:
            failures.append((case, img.shape, kw, debug, msg))
    assert not failures, failures


# 10. planted counts at levels 9 ------------------------------------------------------------------------------------------

PW = PH = 480
POCT = 4


@pytest.mark.parametrize("sift_mode", [0, 1, 2])
@pytest.mark.parametrize("layout", [{0: 300, 1: 100, 2: 40, 3: 12}, {0: 257, 2: 9}, {3: 20}],
                         ids=lambda r: "-".join("%d:%d" % kv for kv in sorted(r.items())))
def test_planted_counts_at_levels_9(oracle_mod, gpu_hip, layout, sift_mode):
    """bumps on every search level 1 .. 9, centres from zc = 0.7 to 9.3: exact per-octave counts, parity with the oracle
    on the same planes (tests/test_gpu_count_edges.py's check), and the slow detection pass gives the same result"""
    kw = dict(levels=9, sift_mode=sift_mode)
    dims = P.octave_dims(oracle_mod, PW, PH, POCT, **kw)
    pl = P.Planted(dims, layout, seed=len(layout) + 3 * sift_mode, sift_mode=sift_mode, levels=9, pin_z=True)
    assert pl.counts == [layout.get(o, 0) for o in range(POCT)]
    orc = oracle_mod.Oracle(oracle_mod.default_params(**P.params_kw(POCT, **kw)), threads=4)
    orc.run(np.zeros((PH, PW), np.uint8), keypoints=False)
    pl.load_oracle(orc)
    res = []
    for debug in ((), ((DET_QCAP, 4),)):
        ctx = gpu_hip.Context(gpu_hip.default_params(store_dog=1, **P.params_kw(POCT, **kw)))
        for what, value in debug:
            ctx.debug_set(what, value)
        ctx.submit(np.zeros((PH, PW), np.uint8)).wait()
        pl.upload(ctx)
        ctx.rerun_keypoint_stages()
        res.append(planted_check(orc, ctx, pl))
        if layout.get(0, 0) >= 100:
            lv = set(ctx.extrema()["lpos"].tolist())
            assert lv == set(range(1, 10)), lv
        ctx.close()
    assert same(res[0], res[1]), "slow detection pass"
