"""The vlfeat-direct Gauss mode (Config::VLFeat_Relative_All) on the device: octave 0's levels straight from the input
image (pyr_direct.hip), octaves >= 1 incrementally.  Every plane is compared bit for bit with the CPU restatement
tests/gauss_direct_ref.c; the keypoint stages on the direct pyramid with the oracle's."""
import os
import subprocess

import numpy as np
import pytest

from gauss_direct import Ref
from popsift_amd.synth import synth
from util import bits, feature_parity, sorted_features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "popsift_amd", "popsift-demo")
DIRECT = 2  # POPSIFT_HIP_GAUSS_VLFEAT_RELATIVE_ALL


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return Ref(tmp_path_factory.mktemp("gauss_direct_ref"))


def _ctx(hip, path=0, **kw):
    ctx = hip.Context(hip.default_params(gauss_mode=DIRECT, **kw))
    ctx.debug_set(hip.DEBUG_DIRECT_PATH, path)
    return ctx


def _canon(feats, desc):
    """bit patterns of the results in canonical order (the device's compaction order is arbitrary)"""
    f, d = sorted_features(feats, desc)
    return (bits(f["xpos"]), bits(f["ypos"]), bits(f["sigma"]), f["num_ori"].copy(), bits(f["orientation"]), bits(d))


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def _check_pyramid(ctx, ref, img, params, what):
    n_oct = ctx.report().num_octaves
    dims = [ctx.octave_dims(o) for o in range(n_oct)]
    want = ref.pyramid(img, params, dims, direct=1)
    L = len(want[0])
    for o in range(n_oct):
        for l in range(L):
            assert np.array_equal(bits(ctx.plane(o, 0, l)), bits(want[o][l])), (what, "gauss", o, l)
        for l in range(L - 1):
            assert np.array_equal(bits(ctx.plane(o, 1, l)), bits(want[o][l + 1] - want[o][l])), (what, "dog", o, l)
    return want


CASES = [
    ("default_200x150", dict(), (200, 150), "u8"),
    ("upscale0_203x151", dict(upscale_factor=0.0), (203, 151), "u8"),
    ("upscale-1_320x240", dict(upscale_factor=-1.0), (320, 240), "u8"),
    ("opencv_sift_mode_190x140", dict(sift_mode=1), (190, 140), "u8"),
    ("halo30_levels2_sigma2_160x120", dict(levels=2, sigma=2.0), (160, 120), "u8"),
    ("levels5_150x110", dict(levels=5), (150, 110), "u8"),
    ("no_initial_blur_170x130", dict(assume_initial_blur=0), (170, 130), "u8"),
    ("store_dog_200x150", dict(store_dog=1), (200, 150), "u8"),
    ("f32_180x140", dict(), (180, 140), "f32"),
    ("pitched_odd_151x97", dict(), (151, 97), "pitched"),
    ("tiny_17x13", dict(), (17, 13), "u8"),
    ("thin_300x9", dict(), (300, 9), "u8"),
    ("thin_9x300", dict(), (9, 300), "u8"),
    ("levels7_200x150", dict(levels=7), (200, 150), "u8"),                # L = 10
    ("levels9_180x140", dict(levels=9), (180, 140), "u8"),                # L = 12, the largest the library takes
    ("sigma0p5_190x150", dict(sigma=0.5), (190, 150), "u8"),              # abs_o0 level 3 has sigma 0: a one-tap filter
    ("levels9_sigma0p5_odd_161x117", dict(levels=9, sigma=0.5), (161, 117), "u8"),
]
EDGE_CASES = [c for c in CASES if c[0].startswith(("levels7_", "levels9_", "sigma0p5_"))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,shape,kind", CASES, ids=[c[0] for c in CASES])
def test_planes_bit_identical_to_restatement(gpu_hip, ref, name, kw, shape, kind):
    w, h = shape
    img = synth(90 + len(name), w, h)
    ctx = _ctx(gpu_hip, **kw)
    if kind == "f32":
        img = img.astype(np.float32) / 255.0
        ctx.submit(img)
    elif kind == "pitched":
        padded = np.full((h, w + 13), 201, np.uint8)
        padded[:, :w] = img
        assert gpu_hip.lib().popsift_hip_submit_u8(ctx._h, padded.ctypes.data, w, h, w + 13) == gpu_hip.OK
    else:
        ctx.submit(img)
    ctx.wait()
    want = _check_pyramid(ctx, ref, img, ctx.params, name)
    # the context's abs_o0 table is the restatement's
    f, span, sig = ctx.gauss_table(abs0=True)
    t = ref.tables(ctx.params)
    assert np.array_equal(bits(f), bits(t["abs0"][0])) and np.array_equal(span, t["abs0"][1])
    assert np.array_equal(bits(sig), bits(t["abs0"][2]))
    # the incremental table stays what get_gauss_table (--print-gauss-tables) reports
    assert np.array_equal(bits(ctx.gauss_table()[0]), bits(t["inc"][0]))
    if name == "halo30_levels2_sigma2_160x120":
        assert span.max() == 31
    # octave 0 level 0 is the default mode's
    if kind == "u8":
        d = gpu_hip.Context(gpu_hip.default_params(**kw)).submit(img)
        d.wait()
        assert np.array_equal(bits(d.plane(0, 0, 0)), bits(want[0][0]))
        assert not np.array_equal(d.plane(0, 0, 2), want[0][2])
        d.close()
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,shape,kind", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_per_level_path_at_the_range_edges(gpu_hip, ref, name, kw, shape, kind):
    """DIRECT_PATH = 1 (one level-0 launch per level of octave 0) at L = 10 and 12 and at sigma 0.5: the restatement's
    planes too, and the fused launch's results bit for bit; the per-level path again with 64-row tiles (BLUR_TILE_H)"""
    img = synth(90 + len(name), *shape)
    res = []
    for path, tile_h in ((0, 0), (1, 0), (1, 64)):
        ctx = _ctx(gpu_hip, path=path, **kw)
        ctx.debug_set(gpu_hip.DEBUG_BLUR_TILE_H, tile_h)
        ctx.submit(img)
        ctx.wait()
        _check_pyramid(ctx, ref, img, ctx.params, "%s DIRECT_PATH %d tile_h %d" % (name, path, tile_h))
        res.append(_canon(*ctx.fetch()))
        ctx.close()
    assert _same(res[0], res[1]) and _same(res[0], res[2]), name


@pytest.mark.gpu
def test_planes_1080p(gpu_hip, ref):
    img = synth(7, 1920, 1080)
    ctx = _ctx(gpu_hip).submit(img)
    ctx.wait()
    _check_pyramid(ctx, ref, img, ctx.params, "1080p")
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kw,shape", [(dict(), (1920, 1080)), (dict(store_dog=1, levels=2, sigma=2.0), (333, 257)),
                                      (dict(upscale_factor=0.0, sift_mode=1), (401, 299))])
def test_fused_equals_per_level_path(gpu_hip, kw, shape):
    img = synth(11, *shape)
    res = []
    for path in (0, 1):
        ctx = _ctx(gpu_hip, path, **kw).submit(img)
        res_f = _canon(*ctx.fetch())
        L = len(ctx.gauss_table()[1])
        planes = [ctx.plane(o, k, l) for o in range(ctx.report().num_octaves) for k in (0, 1) for l in range(L - k)]
        res.append((res_f, planes))
        ctx.close()
    (fa, pa), (fb, pb) = res
    assert len(pa) == len(pb) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(pa, pb))
    assert len(fa[0]) > 50 and _same(fa, fb)
    with pytest.raises(gpu_hip.PopsiftHipError):
        _ctx(gpu_hip, 2)


@pytest.mark.gpu
def test_batch_equals_one_by_one(gpu_hip):
    imgs = [synth(200 + k, 640, 480) for k in range(7)]
    imgs.append(np.ascontiguousarray(imgs[0][::-1, ::-1]))
    for path in (0, 1):
        ctx = _ctx(gpu_hip, path)
        single = [_canon(*ctx.submit(im).fetch()) for im in imgs]
        ctx.submit_batch(imgs)
        assert len(ctx.wait_batch()) == len(imgs)
        for k, want in enumerate(single):
            assert len(want[0]) > 50 and _same(_canon(*ctx.fetch_item(k)), want), (path, k)
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kw,shape", [(dict(), (320, 240)), (dict(levels=2, sigma=2.0), (300, 220)),
                                      (dict(upscale_factor=0.0, sift_mode=1), (400, 300))])
def test_keypoint_stages_on_direct_pyramid(gpu_hip, oracle_mod, kw, shape):
    """the oracle's keypoint stages on the device's direct pyramid give the device's features under the ordinary bars"""
    O = oracle_mod
    img = synth(31, *shape)
    ctx = _ctx(gpu_hip, **kw).submit(img)
    fh, dh = ctx.fetch()
    orc = O.Oracle(O.default_params(**kw), threads=8).run(img, keypoints=False)   # gauss_mode 0: the oracle's only mode
    assert orc.num_octaves == ctx.report().num_octaves
    L = len(ctx.gauss_table()[1])
    for o in range(orc.num_octaves):
        for l in range(L):
            orc.plane(o, 0, l, copy=False)[:] = ctx.plane(o, 0, l)
        for l in range(L - 1):
            orc.plane(o, 1, l, copy=False)[:] = ctx.plane(o, 1, l)
    orc.run_keypoint_stages()
    ok, msg, st = feature_parity(orc, fh, dh)
    assert ok, msg
    assert len(fh) > 20
    ctx.close()


def _counts(stderr):
    lines = [l for l in stderr.splitlines() if l.startswith("Number of feature")]
    return [(int(l.split(":")[1].split()[0]), int(l.rsplit(":", 1)[1])) for l in lines]


@pytest.mark.gpu
def test_demo_vlfeat_direct(gpu_hip, tmp_path):
    img = synth(77, 240, 180)
    p = str(tmp_path / "img.pgm")
    with open(p, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())
    feats, desc = _ctx(gpu_hip).submit(img).fetch()
    r = subprocess.run([DEMO, "--gauss-mode", "vlfeat-direct", "-i", p], capture_output=True, text=True, timeout=300,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert _counts(r.stderr) == [(len(feats), len(desc))]
    rows = np.loadtxt(str(tmp_path / "output-features.txt"), ndmin=2)
    assert rows.shape == (len(desc), 133)
    # and the modes that stay unsupported still fail loudly
    r = subprocess.run([DEMO, "--gauss-mode", "fixed9", "-i", p], capture_output=True, text=True, timeout=300,
                       cwd=str(tmp_path))
    assert r.returncode != 0 and "'vlfeat-direct'" in r.stderr + r.stdout
