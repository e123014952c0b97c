"""Every way the library can build a Gaussian plane gives the oracle's plane, bit for bit.

The pyramid's plane-to-plane levels have two sets of kernels: one tile per workgroup (pyramid.hip) and the strip march
(blur_march.hip) that the large planes take.  Which one a launch uses depends on the plane's size and on the batch -- a
matter of speed only; the smallest octaves are built by one launch of one workgroup per image (pyr_tail.hip) or, with
PYR_TAIL = 1, by level launches like the others.  The debug switch BLUR_PATH forces either (1 = tiles only, 2 = march wherever it applies), BLUR_SEG
the rows per segment of the march, so the small images the oracle finishes in seconds reach the march kernels too:
strips cut by the plane's border, segments of one and several steps, a last step of fewer than 32 rows, planes of fewer
rows than the filter is long, every HALO instance (spans of levels 2 .. 6 at sigma 1 .. 2, opencv spans).  The tile kernels
come with 32 and with 64 rows per tile, 64 from about 4.2 Mpx on; BLUR_TILE_H forces either, so the same small images
reach every 64-row instance as well (tests/blur_cases.py has the list and says which instance a launch takes)."""
import numpy as np
import pytest

from blur_cases import CASES, F32_CASES, oracle_kw
from popsift_amd.synth import synth
from util import bits, sorted_features

pytestmark = pytest.mark.gpu

BLUR_PATH, BLUR_SEG, PYR_TAIL, BLUR_TILE_H = 8, 9, 10, 16


def planes(ctx, n_oct, L):
    return [[ctx.plane(o, 0, l) for l in range(L)] for o in range(n_oct)]


# (blur path, rows per march segment, PYR_TAIL: 1 = no tail launch, BLUR_TILE_H: 0 = by plane size).  With tile height 64
# and no tail every octave down to the smallest plane goes through the 64-row tile kernels; forced 32 equals by-size on
# these planes (none yields 512 tiles of 64 rows)
COMBOS = ((1, 0, 1, 0), (1, 0, 0, 0), (2, 0, 0, 0), (2, 32, 1, 0), (2, 64, 0, 0), (2, 96, 0, 0),
          (1, 0, 1, 64), (1, 0, 0, 64), (1, 0, 1, 32))


@pytest.mark.parametrize("name,kw,spec", CASES, ids=[c[0] for c in CASES])
def test_march_and_tile_kernels_give_the_oracles_planes(oracle_mod, gpu_hip, name, kw, spec):
    img = synth(*spec)
    if name in F32_CASES:
        img = img.astype(np.float32) / 256.0
    L = max(2, kw.get("levels", 3)) + 3
    orc = oracle_mod.Oracle(oracle_mod.default_params(**oracle_kw(kw)), threads=8).run(img)
    want = [[orc.plane(o, 0, l) for l in range(L)] for o in range(orc.num_octaves)]
    # with store_dog = 1 the level launches write the DoG planes themselves: compared too
    want_dog = [[orc.plane(o, 1, l) for l in range(L - 1)] for o in range(orc.num_octaves)] if kw.get("store_dog") else None
    for path, seg, tail, tile_h in COMBOS:
        ctx = gpu_hip.Context(gpu_hip.default_params(**kw))
        ctx.debug_set(BLUR_PATH, path)
        ctx.debug_set(BLUR_SEG, seg)
        ctx.debug_set(PYR_TAIL, tail)
        ctx.debug_set(BLUR_TILE_H, tile_h)
        ctx.submit(img)
        ctx.wait()
        assert ctx.report().num_octaves == orc.num_octaves
        got = planes(ctx, orc.num_octaves, L)
        for o in range(orc.num_octaves):
            for l in range(L):
                a, b = want[o][l], got[o][l]
                assert np.array_equal(bits(a), bits(b)), "path %d seg %d tail %d tile_h %d octave %d level %d: %d values differ, max %g" % (
                    path, seg, tail, tile_h, o, l, int((bits(a) != bits(b)).sum()), float(np.abs(a - b).max()))
            for l in range(L - 1 if want_dog else 0):
                a, b = want_dog[o][l], ctx.plane(o, 1, l)
                assert np.array_equal(bits(a), bits(b)), "path %d seg %d tail %d tile_h %d octave %d DoG %d: %d values differ, max %g" % (
                    path, seg, tail, tile_h, o, l, int((bits(a) != bits(b)).sum()), float(np.abs(a - b).max()))
        ctx.close()


def _canon(feats, desc):
    f, d = sorted_features(feats, desc)
    return (bits(f["xpos"]), bits(f["ypos"]), bits(f["sigma"]), f["num_ori"].copy(), bits(f["orientation"]), bits(d))


def test_march_in_a_batch(gpu_hip):
    """blockIdx.y = image: every image of a batch through the march kernels equals its own single submit through the
    tile kernels (features, orientations and descriptors bit for bit)."""
    imgs = [synth(70 + k, 384, 288) for k in range(3)]
    want = []
    for im in imgs:
        ctx = gpu_hip.Context()
        ctx.debug_set(BLUR_PATH, 1)
        want.append(_canon(*ctx.submit(im).fetch()))
        ctx.close()
    ctx = gpu_hip.Context()
    ctx.debug_set(BLUR_PATH, 2)
    ctx.debug_set(BLUR_SEG, 64)
    ctx.submit_batch(imgs)
    ctx.wait_batch()
    for k in range(3):
        got = _canon(*ctx.fetch_item(k))
        assert all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(got, want[k])), "image %d" % k
    ctx.close()


@pytest.mark.parametrize("store_dog", [0, 1])
def test_64_row_tiles_in_a_batch(gpu_hip, store_dog):
    """blockIdx.y = image under the 64-row tile kernels (BLUR_TILE_H = 64, no tail launch): every image of a batch equals
    its own single submit through the 32-row tiles (features, orientations and descriptors bit for bit; two planes of
    slot 0, which the debug download reads), with the DoG planes formed on the fly and stored."""
    imgs = [synth(70 + k, 384, 288) for k in range(3)]
    want, want_planes = [], None
    for im in imgs:
        ctx = gpu_hip.Context(gpu_hip.default_params(store_dog=store_dog))
        ctx.debug_set(BLUR_PATH, 1)
        ctx.debug_set(BLUR_TILE_H, 32)
        want.append(_canon(*ctx.submit(im).fetch()))
        if want_planes is None:
            want_planes = (ctx.plane(0, 0, 5), ctx.plane(1, 0, 2))
        ctx.close()
    ctx = gpu_hip.Context(gpu_hip.default_params(store_dog=store_dog))
    ctx.debug_set(BLUR_PATH, 1)
    ctx.debug_set(BLUR_TILE_H, 64)
    ctx.debug_set(PYR_TAIL, 1)
    ctx.submit_batch(imgs)
    ctx.wait_batch()
    for k in range(3):
        got = _canon(*ctx.fetch_item(k))
        assert len(want[k][0]) > 50
        assert all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(got, want[k])), "image %d" % k
    assert np.array_equal(bits(ctx.plane(0, 0, 5)), bits(want_planes[0])) and np.array_equal(bits(ctx.plane(1, 0, 2)), bits(want_planes[1]))
    ctx.close()


def test_tile_height_switch_arguments(gpu_hip):
    """BLUR_TILE_H takes 0, 32 and 64 only, and a context that had 64 and went back to 0 gives the default's bytes"""
    img = synth(61, 400, 300)
    dflt = gpu_hip.Context()
    want = _canon(*dflt.submit(img).fetch())
    want_plane = dflt.plane(0, 0, 5)
    dflt.close()
    ctx = gpu_hip.Context()
    for bad in (48, 1, -32, 128):
        with pytest.raises(gpu_hip.PopsiftHipError) as e:
            ctx.debug_set(BLUR_TILE_H, bad)
        assert e.value.status == gpu_hip.ERR_INVALID, bad
    assert len(want[0]) > 50
    for tile_h in (64, 0):  # one image through the 64-row tiles, then the same context by plane size again
        ctx.debug_set(BLUR_TILE_H, tile_h)
        got = _canon(*ctx.submit(img).fetch())
        assert all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(got, want)), tile_h
        assert np.array_equal(bits(ctx.plane(0, 0, 5)), bits(want_plane)), tile_h
    ctx.close()


def test_the_batch_path_of_the_timed_loop_at_full_size(gpu_hip):
    """Four 1080p images in one submit: 4 x 8.3 Mpx per level launch of octave 0, so launch_blur takes the march kernels by
    itself (no debug switch: the path of bench.py's timed loop, equal segments of 224 rows) -- every image equals its own single
    submit, which the tile kernels build (features, orientations, descriptors and two planes bit for bit)."""
    imgs = [synth(100 + k, 1920, 1080) for k in range(4)]
    want, planes = [], []
    single = gpu_hip.Context()
    for im in imgs:
        want.append(_canon(*single.submit(im).fetch()))
        planes.append((single.plane(0, 0, 5).copy(), single.plane(1, 0, 2).copy()))
    single.close()
    ctx = gpu_hip.Context()
    ctx.submit_batch(imgs)
    assert len(ctx.wait_batch()) == 4
    for k in range(4):
        got = _canon(*ctx.fetch_item(k))
        assert all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(got, want[k])), "image %d" % k
    # the planes of image 0 of the batch (the debug download reads slot 0)
    assert np.array_equal(bits(ctx.plane(0, 0, 5)), bits(planes[0][0])) and np.array_equal(bits(ctx.plane(1, 0, 2)), bits(planes[0][1]))
    ctx.close()
