"""The ScaleDirect scaling mode (Config::ScaleDirect) on the device: every octave's level 0 straight from the input
image in one launch, then one launch per level for all octaves (pyramid.hip).  Every plane is compared bit for bit with
the CPU restatement tests/scale_direct_ref.c; the keypoint and describe stages on the device's planes with the
oracle's; the C++ layer through popsift-demo --direct-scaling."""
import os
import subprocess

import numpy as np
import pytest

from popsift_amd.synth import synth
from scale_direct import Ref
from util import bits, feature_parity, sorted_features

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "popsift_amd", "popsift-demo")
THREADS = min(os.cpu_count() or 4, 16)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return Ref(tmp_path_factory.mktemp("scale_direct_ref"))


def _ctx(hip, path=0, **kw):
    ctx = hip.Context(hip.default_params(scale_direct=hip.SCALE_DIRECT, **kw))
    ctx.debug_set(hip.DEBUG_SCALE_PATH, path)
    return ctx


def _canon(feats, desc):
    """bit patterns of the results in canonical order (the device's compaction order is arbitrary)"""
    f, d = sorted_features(feats, desc)
    return (bits(f["xpos"]), bits(f["ypos"]), bits(f["sigma"]), f["num_ori"].copy(), bits(f["orientation"]), bits(d))


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def _planes(ctx):
    L = len(ctx.gauss_table()[1])
    return [ctx.plane(o, k, l) for o in range(ctx.report().num_octaves) for k in (0, 1) for l in range(L - k)]


def _check_pyramid(ctx, ref, img, params, what):
    n_oct = ctx.report().num_octaves
    dims = [ctx.octave_dims(o) for o in range(n_oct)]
    want = ref.pyramid(img, params, dims, scale_direct=1)
    L = len(want[0])
    for o in range(n_oct):
        for l in range(L):
            assert np.array_equal(bits(ctx.plane(o, 0, l)), bits(want[o][l])), (what, "gauss", o, l)
        for l in range(L - 1):
            assert np.array_equal(bits(ctx.plane(o, 1, l)), bits(want[o][l + 1] - want[o][l])), (what, "dog", o, l)
    return want


def _submit(hip, ctx, img, kind):
    h, w = img.shape
    if kind == "f32":
        img = img.astype(np.float32) / 255.0
        ctx.submit(img)
    elif kind == "pitched":
        padded = np.full((h, w + 13), 201, np.uint8)
        padded[:, :w] = img
        assert hip.lib().popsift_hip_submit_u8(ctx._h, padded.ctypes.data, w, h, w + 13) == hip.OK
    else:
        ctx.submit(img)
    ctx.wait()
    return img


CASES = [
    ("default_200x150", dict(), (200, 150), "u8"),
    ("f32_180x140", dict(), (180, 140), "f32"),
    ("pitched_odd_151x97", dict(), (151, 97), "pitched"),
    ("upscale0_203x151", dict(upscale_factor=0.0), (203, 151), "u8"),
    ("upscale-1_320x240", dict(upscale_factor=-1.0), (320, 240), "u8"),
    ("opencv_sift_mode_190x140", dict(sift_mode=1), (190, 140), "u8"),
    ("gauss_vlfeat_direct_200x150", dict(gauss_mode=2), (200, 150), "u8"),
    ("gauss_opencv_210x160", dict(gauss_mode=3, sift_mode=1), (210, 160), "u8"),
    ("levels2_sigma2_160x120", dict(levels=2, sigma=2.0), (160, 120), "u8"),
    ("levels9_180x140", dict(levels=9), (180, 140), "u8"),
    ("no_initial_blur_170x130", dict(assume_initial_blur=0), (170, 130), "u8"),
    # a large assumed blur widens inc[0] (and dd[0]): level-0 halos 9 .. 30, beyond the common 5 .. 8
    ("initial_blur1p3_180x130", dict(initial_blur=1.3), (180, 130), "u8"),
    ("initial_blur1p5_f32_170x120", dict(initial_blur=1.5), (170, 120), "f32"),
    ("initial_blur0p7_upscale2_90x70", dict(initial_blur=0.7, upscale_factor=2.0), (90, 70), "u8"),
    ("initial_blur2p5_sigma2_opencv_150x110", dict(initial_blur=2.5, sigma=2.0, gauss_mode=3, sift_mode=1), (150, 110), "u8"),
    ("initial_blur4_sigma2_160x120", dict(initial_blur=4.0, sigma=2.0), (160, 120), "u8"),
    ("store_dog_200x150", dict(store_dog=1), (200, 150), "u8"),
    ("store_dog_f32_upscale0_161x117", dict(store_dog=1, upscale_factor=0.0), (161, 117), "f32"),
    ("tiny_17x13", dict(), (17, 13), "u8"),
    ("thin_300x9", dict(), (300, 9), "u8"),
    ("thin_9x300", dict(), (9, 300), "u8"),
]


@pytest.mark.parametrize("name,kw,shape,kind", CASES, ids=[c[0] for c in CASES])
def test_planes_bit_identical_to_restatement(gpu_hip, ref, name, kw, shape, kind):
    hip = gpu_hip
    img = synth(90 + len(name), *shape)
    ctx = _ctx(hip, **kw)
    img = _submit(hip, ctx, img, kind)
    want = _check_pyramid(ctx, ref, img, ctx.params, name)
    # the context's dd table is the restatement's, one row per octave
    n_oct = ctx.report().num_octaves
    f, span, sig = ctx.gauss_table(dd=True)
    t = ref.tables(ctx.params)
    assert len(span) == n_oct
    assert np.array_equal(bits(f), bits(t["dd"][0][:n_oct])) and np.array_equal(span, t["dd"][1][:n_oct])
    assert np.array_equal(bits(sig), bits(t["dd"][2][:n_oct]))
    assert np.array_equal(bits(ctx.gauss_table()[0]), bits(t["inc"][0]))
    if name.startswith("initial_blur"):
        assert max(span.max(), t["inc"][1][0]) - 1 > 8, name  # a level-0 halo beyond 8
    if name.startswith("initial_blur4_"):
        assert max(span.max(), t["inc"][1][0]) == 31  # the widest filter the tables hold: halo 30
    # octave 0 is the default mode's, every level; the octaves after it are not (ScaleDirect with Gauss mode 2 is mode
    # 0's pyramid, the default scaling mode with Gauss mode 2 is not)
    d = hip.Context(hip.default_params(**dict(kw, gauss_mode=0) if kw.get("gauss_mode") == 2 else kw))
    _submit(hip, d, synth(90 + len(name), *shape), kind)
    L = len(want[0])
    for l in range(L):
        assert np.array_equal(bits(d.plane(0, 0, l)), bits(want[0][l])), (name, l)
    if n_oct >= 2:
        assert not np.array_equal(d.plane(1, 0, 0), want[1][0])
    d.close()
    ctx.close()


@pytest.mark.parametrize("shape,n_oct", [((1920, 1080), 9), ((3840, 2160), 10)])
def test_planes_large(gpu_hip, ref, shape, n_oct):
    img = synth(7, *shape)
    ctx = _ctx(gpu_hip).submit(img)
    ctx.wait()
    assert ctx.report().num_octaves == n_oct
    _check_pyramid(ctx, ref, img, ctx.params, "%dx%d" % shape)
    ctx.close()


@pytest.mark.parametrize("kw,shape", [(dict(), (1920, 1080)), (dict(store_dog=1, levels=2, sigma=2.0), (333, 257)),
                                      (dict(upscale_factor=0.0, sift_mode=1, gauss_mode=3), (401, 299)),
                                      (dict(levels=9, upscale_factor=-1.0), (640, 480)),
                                      (dict(initial_blur=1.5), (500, 380)), (dict(initial_blur=4.0, sigma=2.0), (300, 200))])
def test_fused_equals_yardstick_path(gpu_hip, kw, shape):
    img = synth(11, *shape)
    res = []
    # the yardstick's level launches of the stored-DoG and the wide-filter rows again with 64-row tiles (BLUR_TILE_H)
    again_64 = bool(kw.get("store_dog")) or kw.get("initial_blur") == 4.0
    for path, tile_h in ((0, 0), (1, 0)) + (((1, 64),) if again_64 else ()):
        ctx = _ctx(gpu_hip, path, **kw)
        ctx.debug_set(gpu_hip.DEBUG_BLUR_TILE_H, tile_h)
        ctx.submit(img)
        res.append((_canon(*ctx.fetch()), _planes(ctx)))
        ctx.close()
    (fa, pa), (fb, pb) = res[:2]
    for fc, pc in res[2:]:
        assert len(pa) == len(pc) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(pa, pc)), "tile_h 64"
        assert _same(fa, fc), "tile_h 64"
    assert len(pa) == len(pb) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(pa, pb))
    # (an assumed blur of 4 leaves few or no extrema: the planes carry that case)
    assert (len(fa[0]) > 50 or kw.get("initial_blur", 0.5) > 2) and _same(fa, fb)
    ctx = gpu_hip.Context(gpu_hip.default_params(scale_direct=gpu_hip.SCALE_DIRECT))
    with pytest.raises(gpu_hip.PopsiftHipError):
        ctx.debug_set(gpu_hip.DEBUG_SCALE_PATH, 2)
    ctx.close()


def test_vlfeat_direct_gauss_mode_equals_vlfeat(gpu_hip):
    """ScaleDirect comes before the vlfeat-direct branch (s_pyramid_build.cu:499-516): with Gauss mode 2 the pyramid and
    the features are mode 0's bit for bit"""
    img = synth(12, 400, 300)
    res = []
    for gm in (0, 2):
        ctx = _ctx(gpu_hip, gauss_mode=gm).submit(img)
        res.append((_canon(*ctx.fetch()), _planes(ctx)))
        ctx.close()
    (fa, pa), (fb, pb) = res
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(pa, pb))
    assert len(fa[0]) > 50 and _same(fa, fb)


def test_batch_of_16_equals_one_by_one(gpu_hip):
    imgs = [synth(200 + k, 640, 480) for k in range(14)]
    imgs.append(np.ascontiguousarray(imgs[0][::-1, ::-1]))
    imgs.append(np.full((480, 640), 128, np.uint8))  # featureless
    for path in (0, 1):
        ctx = _ctx(gpu_hip, path)
        single = [_canon(*ctx.submit(im).fetch()) for im in imgs]
        ctx.submit_batch(imgs)
        assert len(ctx.wait_batch()) == 16
        for k, want in enumerate(single):
            assert _same(_canon(*ctx.fetch_item(k)), want), (path, k)
            assert k == 15 or len(want[0]) > 50
        ctx.close()


def _inject(orc, ctx, L):
    for o in range(orc.num_octaves):
        for l in range(L):
            orc.plane(o, 0, l, copy=False)[:] = ctx.plane(o, 0, l)
        for l in range(L - 1):
            orc.plane(o, 1, l, copy=False)[:] = ctx.plane(o, 1, l)


@pytest.mark.parametrize("kw,shape", [(dict(), (320, 240)), (dict(levels=2, sigma=2.0), (300, 220)),
                                      (dict(upscale_factor=0.0, sift_mode=1, gauss_mode=3), (400, 300))])
def test_keypoint_stages_on_scale_direct_pyramid(gpu_hip, oracle_mod, kw, shape):
    """the oracle's keypoint stages on the device's ScaleDirect pyramid give the device's features under the ordinary
    bars"""
    O = oracle_mod
    img = synth(31, *shape)
    ctx = _ctx(gpu_hip, **kw).submit(img)
    fh, dh = ctx.fetch()
    orc = O.Oracle(O.default_params(**kw), threads=THREADS).run(img, keypoints=False)
    assert orc.num_octaves == ctx.report().num_octaves
    _inject(orc, ctx, len(ctx.gauss_table()[1]))
    orc.run_keypoint_stages()
    ok, msg, st = feature_parity(orc, fh, dh)
    assert ok, msg
    assert len(fh) > 20
    ctx.close()


def test_describe_on_scale_direct_pyramid(gpu_hip, oracle_mod):
    """popsift_hip_describe_batch builds its pyramid through the same branch; with computed orientations the oracle's
    orientation and descriptor stages on the device's planes and the resolved frames agree under the ordinary bars"""
    hip, O = gpu_hip, oracle_mod
    w, h = 320, 240
    img = synth(11, w, h)
    rng = np.random.default_rng(3)
    n = 3000
    fr = np.zeros(n, hip.FRAME_DTYPE)
    fr["xpos"], fr["ypos"] = rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)
    fr["sigma"] = np.exp2(rng.uniform(-1.0, 5.0, n))
    fr["octave"], fr["level"] = -1, -1
    ctx = _ctx(hip)
    df, dd = ctx.describe(img, fr, "compute")
    e = ctx.extrema()
    valid = np.zeros(n, bool)
    valid[e["cell"]] = True
    assert valid.sum() > 1000 and ctx.report().ext_total == len(e)
    assert ((df["debug_octave"] >= 0) == valid).all()
    # the frames describe the ScaleDirect planes: the same frames on a default-mode context give other descriptors
    dflt = hip.Context(hip.default_params())
    _, dd0 = dflt.describe(img, fr, "compute")
    dflt.close()
    assert not (len(dd0) == len(dd) and np.array_equal(dd0, dd))
    orc = O.Oracle(O.default_params(), threads=THREADS).run(img, keypoints=False)
    _inject(orc, ctx, len(ctx.gauss_table()[1]))
    orc.run_from_extrema(e)
    ok, msg, _ = feature_parity(orc, df[valid], dd)
    assert ok, msg
    ctx.close()


def _counts(stderr):
    lines = [l for l in stderr.splitlines() if l.startswith("Number of feature")]
    return [(int(l.split(":")[1].split()[0]), int(l.rsplit(":", 1)[1])) for l in lines]


@pytest.mark.parametrize("args,kw", [([], dict()), (["--gauss-mode", "opencv"], dict(gauss_mode=3))])
def test_demo_direct_scaling(gpu_hip, tmp_path, args, kw):
    """Config::ScaleDirect through the C++ layer (PopSift::configure / to_params): popsift-demo --direct-scaling"""
    img = synth(77, 240, 180)
    p = str(tmp_path / "img.pgm")
    with open(p, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())
    ctx, dctx = _ctx(gpu_hip, **kw), gpu_hip.Context(gpu_hip.default_params(**kw))
    feats, desc = ctx.submit(img).fetch()
    dflt, _ = dctx.submit(img).fetch()
    ctx.close()
    dctx.close()
    r = subprocess.run([DEMO, "--direct-scaling", *args, "-i", p], capture_output=True, text=True, timeout=300,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert _counts(r.stderr) == [(len(feats), len(desc))]
    assert len(feats) != len(dflt) or not np.array_equal(np.sort(feats["xpos"]), np.sort(dflt["xpos"]))
    rows = np.loadtxt(str(tmp_path / "output-features.txt"), ndmin=2)
    assert rows.shape == (len(desc), 133)


def test_match_program_direct_scaling(gpu_hip, tmp_path):
    """popsift-match --direct-scaling: both images extracted in ScaleDirect mode (the C ABI's counts), one line per left
    descriptor"""
    a = synth(95, 240, 180)
    b = np.roll(a, (2, 4), axis=(0, 1))
    pa, pb = str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm")
    for path, im in ((pa, a), (pb, b)):
        with open(path, "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (im.shape[1], im.shape[0]))
            f.write(im.tobytes())
    r = subprocess.run([os.path.join(ROOT, "popsift_amd", "popsift-match"), "--direct-scaling", "-l", pa, "--right=" + pb],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    ctx = _ctx(gpu_hip)
    fa, da = ctx.submit(a).fetch()
    fb, db = ctx.submit(b).fetch()
    ctx.close()
    lines = r.stdout.splitlines()
    assert lines[1:5] == ["Number of features:    %d" % len(fa), "Number of descriptors: %d" % len(da),
                          "Number of features:    %d" % len(fb), "Number of descriptors: %d" % len(db)]
    assert len(lines) - 5 == len(da) and all(l.startswith(("accept", "reject")) for l in lines[5:])
