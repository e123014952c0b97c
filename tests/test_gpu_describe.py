"""Describe caller-supplied keypoints on the device (popsift_hip_describe_batch): round trips against extraction bit for
bit, the octave / level rule against its numpy restatement (tests/describe_rule.py), oracle parity on random frames,
invalid frames, caller order, limits, re-runs, batches, interleaving with extraction and matching."""
import os

import numpy as np
import pytest

from describe_rule import SIGMA_MAX, resolve
from popsift_amd.synth import synth
from util import bits, feature_parity, sorted_features

pytestmark = pytest.mark.gpu

THREADS = min(os.cpu_count() or 4, 16)


def _img(seed, w, h, f32=False):
    im = synth(seed, w, h)
    return (im.astype(np.float32) / 256.0).astype(np.float32) if f32 else im


def _extract(hip, img, **kw):
    ctx = hip.Context(hip.default_params(**kw))
    feats, desc = ctx.submit(img).fetch()
    ext = ctx.extrema()
    ctx.close()
    return feats, desc, ext


def _frames(hip, feats, ext, given, hints=True, dims=None):
    """one frame per feature (compute) or per (feature, orientation) (given); src = (feature, orientation) of each.
    dims: skip extrema outside [0, w_o - 1] x [0, h_o - 1] (OpenCV mode's refinement does not clip its positions)"""
    rows, src = [], []
    for g, f in enumerate(feats):
        if dims is not None:
            w, h = dims[ext[g]["octave"]]
            if not (0 <= ext[g]["xpos"] <= w - 1 and 0 <= ext[g]["ypos"] <= h - 1):
                continue
        for k in range(int(f["num_ori"]) if given else 1):
            rows.append((f["xpos"], f["ypos"], f["sigma"], f["orientation"][k] if given else 0.0,
                         f["debug_octave"] if hints else -1, ext[g]["lpos"] if hints else -1))
            src.append((g, k))
    return np.array(rows, hip.FRAME_DTYPE), src


ROUND_TRIP = [
    dict(),
    dict(desc_mode=1), dict(desc_mode=2), dict(desc_mode=3), dict(desc_mode=4),
    dict(norm_mode=1),
    dict(sift_mode=1), dict(sift_mode=2, desc_mode=4),
    dict(upscale_factor=0.0), dict(upscale_factor=-1.0, desc_mode=2),
    dict(levels=9), dict(levels=9, sigma=2.0),    # 12 Gaussian planes: level hints and derived lpos up to L - 1 = 11
]


@pytest.mark.parametrize("kw", ROUND_TRIP + [dict(f32=True), dict(odd=True)], ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()) or "default")
def test_round_trip_given_and_computed(gpu_hip, kw):
    hip = gpu_hip
    kw = dict(kw)
    f32, odd = kw.pop("f32", False), kw.pop("odd", False)
    big = kw.get("upscale_factor") == -1.0  # a downscaled pyramid needs a larger image for as many keypoints
    img = _img(5, 161, 117, f32) if odd else _img(5, 480, 360, f32) if big else _img(5, 200, 150, f32)
    feats, desc, ext = _extract(hip, img, **kw)
    assert len(feats) > 50
    ctx = hip.Context(hip.default_params(**kw))
    ctx.submit(img).wait()
    dims = [ctx.octave_dims(o) for o in range(ctx.report().num_octaves)]
    # given orientation: one descriptor per (feature, orientation), bit for bit the extraction's
    fr, src = _frames(hip, feats, ext, True, dims=dims)
    df, dd = ctx.describe(img, fr, "given")
    assert len(df) == len(fr) and len(dd) == len(fr)
    assert (df["num_ori"] == 1).all() and (df["debug_octave"] == fr["octave"]).all()
    for name in ("xpos", "ypos", "sigma"):
        assert np.array_equal(bits(df[name]), bits(fr[name])), name
    assert np.array_equal(bits(df["orientation"][:, 0]), bits(fr["orientation"]))
    want = np.array([desc[feats[g]["desc_idx"][k]] for g, k in src])
    assert np.array_equal(bits(dd[df["desc_idx"][:, 0]]), bits(want))
    # computed orientation: num_ori, the orientations and the descriptors bit for bit
    fr, src = _frames(hip, feats, ext, False, dims=dims)
    cf, cd = ctx.describe(img, fr, "compute")
    sel = feats[[g for g, _ in src]]
    assert np.array_equal(cf["num_ori"], sel["num_ori"])
    assert np.array_equal(bits(cf["orientation"]), bits(sel["orientation"]))
    for f, g in zip(cf, sel):
        n = int(f["num_ori"])
        assert np.array_equal(bits(cd[f["desc_idx"][:n]]), bits(desc[g["desc_idx"][:n]]))
    assert len(cd) == sel["num_ori"].sum()
    ctx.close()


def _resolved(ctx, n):
    """(octave, lpos) per frame from the resolved extrema (cell = frame index); -1 for invalid frames"""
    e = ctx.extrema()
    o, lp = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    o[e["cell"]], lp[e["cell"]] = e["octave"], e["lpos"]
    assert len(np.unique(e["cell"])) == len(e)
    assert (np.diff(e["octave"]) >= 0).all()
    for oc in np.unique(e["octave"]):
        assert (np.diff(e["cell"][e["octave"] == oc]) > 0).all()  # caller order within an octave
    return o, lp, e


@pytest.mark.parametrize("up", [1.0, 0.0, -1.0])
def test_derived_octave_and_level(gpu_hip, up):
    hip = gpu_hip
    img = _img(7, 240, 180)
    feats, desc, ext = _extract(hip, img, upscale_factor=up)
    ctx = hip.Context(hip.default_params(upscale_factor=up))
    fr, src = _frames(hip, feats, ext, True, hints=False)
    df, dd = ctx.describe(img, fr, "given")
    o, lp, _ = _resolved(ctx, len(fr))
    p = ctx.params
    dims = [ctx.octave_dims(k) for k in range(ctx.report().num_octaves)]
    ro, rl, _, _, rs = resolve(fr, p.sigma, p.levels, int(up), dims, given=True)
    # the numpy rule; a disagreement only where log2 sits within 1e-5 of a .5 boundary, a handful at most
    bad = np.nonzero((o != ro) | ((o >= 0) & (lp != rl)))[0]
    t = np.log2(fr["sigma"].astype(np.float64) / p.sigma) + int(up)
    near = np.minimum(np.abs((t - 0.5 / p.levels) - np.round(t - 0.5 / p.levels)),
                      np.abs(np.abs(p.levels * (t - np.maximum(ro, 0)) - np.floor(p.levels * (t - np.maximum(ro, 0)))) - 0.5))
    assert len(bad) <= 5 and (near[bad] < 1e-5 * p.levels).all(), (bad, near[bad])
    # frames that resolve as extraction placed them round-trip bit for bit
    same = [i for i, (g, k) in enumerate(src) if o[i] == feats[g]["debug_octave"] and lp[i] == ext[g]["lpos"]]
    assert len(same) > len(src) // 2
    for i in same:
        g, k = src[i]
        assert np.array_equal(bits(dd[df[i]["desc_idx"][0]]), bits(desc[feats[g]["desc_idx"][k]]))
    ctx.close()


def _random_frames(hip, rng, n, w, h, up, sigma0=1.6, n_oct=5):
    fr = np.zeros(n, hip.FRAME_DTYPE)
    fr["xpos"] = rng.uniform(0, w - 1, n)
    fr["ypos"] = rng.uniform(0, h - 1, n)
    # log-uniform sigma past both ends of the octave range
    fr["sigma"] = np.exp2(rng.uniform(np.log2(sigma0) - up - 2, np.log2(sigma0) - up + n_oct + 1, n))
    fr["orientation"] = rng.uniform(-np.pi, np.pi, n)
    fr["octave"], fr["level"] = -1, -1
    # on the border
    k = n // 10
    fr["xpos"][:k] = rng.choice([0.0, w - 1.0], k)
    fr["ypos"][k:2 * k] = rng.choice([0.0, h - 1.0], k)
    return fr


@pytest.mark.parametrize("given", [False, True])
def test_oracle_parity_on_random_frames(gpu_hip, oracle_mod, given):
    hip, O = gpu_hip, oracle_mod
    img = _img(11, 320, 240)
    rng = np.random.default_rng(3 + given)
    fr = _random_frames(hip, rng, 3000, 320, 240, 1)
    ctx = hip.Context(hip.default_params())
    df, dd = ctx.describe(img, fr, "given" if given else "compute")
    o, lp, e = _resolved(ctx, len(fr))
    valid = o >= 0
    assert valid.sum() > 1000 and (~valid).sum() > 100
    assert ctx.report().ext_total == valid.sum() == len(e)
    orc = O.Oracle(O.default_params(), threads=THREADS).run(img, keypoints=False).run_from_extrema(e)
    if not given:
        ok, msg, _ = feature_parity(orc, df[valid], dd)
        assert ok, msg
    else:
        fo, _ = orc.fetch()
        assert len(fo) == len(e)
        ori = np.zeros((len(fo), 4), np.float32)
        ori[:, 0] = fr["orientation"][e["cell"]]
        fo, do = orc.redo_descriptors(ori).fetch()
        bad, n = 0, 0
        for j in range(len(fo)):
            if fo[j]["num_ori"] < 1:
                continue
            a, b = do[fo[j]["desc_idx"][0]], dd[df[e["cell"][j]]["desc_idx"][0]]
            n += 1
            if np.linalg.norm(a - b) > 1e-3 * max(np.linalg.norm(a), 1e-20):
                bad += 1
        assert n > 1000 and bad <= max(1, n // 5000), (bad, n)
    ctx.close()


def _invalid_case(hip):
    """valid frames with one of every invalid class between them; -> (frames, which are invalid)"""
    up = 1
    fr = np.zeros(24, hip.FRAME_DTYPE)
    fr["xpos"] = np.linspace(20, 180, 24)
    fr["ypos"] = np.linspace(15, 130, 24)
    fr["sigma"], fr["orientation"], fr["octave"], fr["level"] = 2.0, 0.5, -1, -1
    bad = {1: ("xpos", np.nan), 3: ("ypos", np.inf), 5: ("sigma", np.nan), 7: ("sigma", 0.0), 9: ("sigma", -1.0),
           11: ("xpos", -0.25), 13: ("ypos", 400.0), 15: ("octave", 9), 17: ("octave", -2), 19: ("level", 6),
           21: ("level", -3), 23: ("orientation", np.nan)}
    for i, (k, v) in bad.items():
        fr[k][i] = v
    fr["octave"][22], fr["sigma"][22] = 0, np.ldexp(SIGMA_MAX, -up)                                   # at the cap: valid
    fr["octave"][20], fr["sigma"][20] = 0, np.nextafter(np.ldexp(SIGMA_MAX, -up), np.float32(1e9))   # one ulp beyond
    inval = sorted(list(bad) + [20])
    return fr, inval


def test_invalid_frames_order_and_determinism(gpu_hip):
    hip = gpu_hip
    img = _img(13, 200, 150)
    fr, inval = _invalid_case(hip)
    ctx = hip.Context(hip.default_params())
    for mode in ("given", "compute"):
        df, dd = ctx.describe(img, fr, mode)
        assert len(df) == len(fr)
        bad = [i for i in range(len(fr)) if df[i]["num_ori"] == 0]
        expect = [i for i in inval if not (mode == "compute" and i == 23)]
        assert bad == expect, (mode, bad)
        for i in expect:
            f = df[i]
            assert f["debug_octave"] == -1 and (f["desc_idx"] == -1).all()
            for k in ("xpos", "ypos", "sigma"):
                assert bits(f[k]) == bits(fr[k][i])
        # the neighbours are what they are without the invalid frames
        ok = np.array([i for i in range(len(fr)) if i not in expect])
        gf, gd = ctx.describe(img, fr[ok], mode)
        assert np.array_equal(gf["num_ori"], df["num_ori"][ok])
        for a, b in zip(gf, df[ok]):
            n = int(a["num_ori"])
            assert np.array_equal(bits(gd[a["desc_idx"][:n]]), bits(dd[b["desc_idx"][:n]]))
        assert df[22]["num_ori"] >= 1
    # a shuffled list gives permuted features with equal descriptors; two runs are byte-identical
    rng = np.random.default_rng(1)
    fr = _random_frames(hip, rng, 2000, 200, 150, 1)
    for mode in ("given", "compute"):
        a = ctx.describe(img, fr, mode)
        b = ctx.describe(img, fr, mode)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        p = rng.permutation(len(fr))
        sf, sd = ctx.describe(img, fr[p], mode)
        f0 = a[0][p]
        assert np.array_equal(sf["num_ori"], f0["num_ori"])
        assert np.array_equal(bits(sf["orientation"]), bits(f0["orientation"]))
        for x, y in zip(sf, f0):
            n = int(x["num_ori"])
            assert np.array_equal(bits(sd[x["desc_idx"][:n]]), bits(a[1][y["desc_idx"][:n]]))
    ctx.close()


def test_limits_caps_and_rerun(gpu_hip):
    hip = gpu_hip
    img = _img(17, 200, 150)
    cap = 600
    rng = np.random.default_rng(5)
    fr = _random_frames(hip, rng, cap + 1, 200, 150, 1)
    ctx = hip.Context(hip.default_params(max_extrema=cap))
    for mode in ("given", "compute"):
        ref = ctx.describe(img, fr[:cap], mode)
        assert len(ref[0]) == cap
        with pytest.raises(hip.PopsiftHipError) as ei:
            ctx.describe(img, fr, mode)
        assert ei.value.status == hip.ERR_INVALID
        again = ctx.describe(img, fr[:cap], mode)
        assert again[0].tobytes() == ref[0].tobytes() and again[1].tobytes() == ref[1].tobytes()
        # rerun_keypoint_stages after a describe re-runs the describe stages
        ctx.rerun_keypoint_stages()
        again = ctx.fetch()
        assert again[0].tobytes() == ref[0].tobytes() and again[1].tobytes() == ref[1].tobytes()
        # tiny histogram / descriptor buffers: grow and re-run, same bytes
        tiny = hip.Context(hip.default_params(max_extrema=cap))
        tiny.debug_set(hip.DEBUG_OHIST_CAP, 7).debug_set(hip.DEBUG_DESC_CAP, 5)
        got = tiny.describe(img, fr[:cap], mode)
        assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()
        tiny.close()
    empty = ctx.describe(img, fr[:0], "compute")
    assert len(empty[0]) == 0 and len(empty[1]) == 0 and ctx.report().ext_total == 0
    ctx.close()


def test_batch_equals_single_describes(gpu_hip):
    hip = gpu_hip
    rng = np.random.default_rng(9)
    imgs = [_img(30 + k, 160, 120) for k in range(16)]
    counts = [0, 1, 63, 64, 65, 300, 0, 777, 5, 256, 257, 1000, 2, 511, 129, 40]
    lists = [_random_frames(hip, rng, n, 160, 120, 1) for n in counts]
    for mode in ("given", "compute"):
        ctx = hip.Context(hip.default_params())
        got = ctx.describe_batch(imgs, lists, mode)
        one = hip.Context(hip.default_params())
        for k in range(16):
            f, d = one.describe(imgs[k], lists[k], mode)
            assert len(got[k][0]) == counts[k]
            assert got[k][0].tobytes() == f.tobytes() and got[k][1].tobytes() == d.tobytes(), (mode, k)
        ctx.close()
        one.close()


def test_interleaving_and_matching(gpu_hip):
    hip = gpu_hip
    img_a, img_b = _img(41, 200, 150), _img(42, 240, 160)
    fresh = lambda f: f(hip.Context(hip.default_params()))
    ea = fresh(lambda c: c.submit(img_a).fetch())
    eb = fresh(lambda c: c.submit(img_b).fetch())
    feats, desc, ext = _extract(hip, img_a)
    fr, src = _frames(hip, feats, ext, True)
    da = fresh(lambda c: c.describe(img_b, fr[:500], "given"))
    ctx = hip.Context(hip.default_params())
    # an extraction's list order is its refinement's arrival order: extractions are compared as sorted sets
    def canon(r):
        f, d = sorted_features(*r)
        return tuple(f[k].tobytes() for k in ("debug_octave", "xpos", "ypos", "sigma", "num_ori", "orientation")) + (d.tobytes(),)
    for step, (want, run, key) in enumerate(((ea, lambda: ctx.submit(img_a).fetch(), canon),
                                             (da, lambda: ctx.describe(img_b, fr[:500], "given"), None),
                                             (eb, lambda: ctx.submit(img_b).fetch(), canon),
                                             (da, lambda: ctx.describe(img_b, fr[:500], "given"), None))):
        got = run()
        if key:
            assert key(got) == key(want), step
        else:
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), step
    # matching: a given-orientation describe of the extraction's own keypoints finds every descriptor's source at 0
    ctx.submit(img_a)
    lset = ctx.clone_results()
    df, dd = ctx.describe(img_a, fr, "given")
    rset = ctx.clone_results()
    _, nf, nd = rset.info()
    assert (nf, nd) == (len(fr), len(fr))
    m = rset.match(lset)
    rdesc, rev = rset.download()
    ldesc, _ = lset.download()
    assert (m["dist_best"] == 0).all()
    assert np.array_equal(bits(ldesc[m["best"]]), bits(rdesc))  # the source (or an identical copy of it)
    assert np.array_equal(bits(rdesc), bits(dd))
    # the reverse map names caller-order feature indices
    assert np.array_equal(rev[df["desc_idx"][:, 0]], np.arange(len(fr)))
    lset.close()
    rset.close()
    ctx.close()
