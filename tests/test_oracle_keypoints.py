"""Keypoint stages of the oracle: analytic and invariance known-answer tests
(SURVEY.md 8(c) items 3-5).  These pin behaviour; they cannot pin bit patterns
(parity unpinned: the reference ships no goldens and cannot be built here)."""
import numpy as np
import pytest

from popsift_amd.synth import gaussian_blob, synth


@pytest.mark.parametrize("std,x0,y0", [(3.0, 40.3, 33.7), (5.0, 61.5, 48.25), (8.0, 70.0, 64.0)])
def test_gaussian_blob_is_found_at_its_centre(oracle_mod, std, x0, y0):
    O = oracle_mod
    img = gaussian_blob(140, 128, x0, y0, std)
    feats, desc = O.Oracle().run(img).fetch()
    assert len(feats) >= 1
    d = np.hypot(feats["xpos"] - x0, feats["ypos"] - y0)
    i = int(np.argmin(d))
    assert d[i] < 0.15
    # DoG between sigma and k*sigma responds most to a blob of std ~ sigma*sqrt(k): the reported
    # sigma sits a little below the blob's std (k = 2^(1/3))
    assert 0.78 * std < feats["sigma"][i] < 1.05 * std
    assert 1 <= feats["num_ori"][i] <= 4


def test_dark_blob_is_found_too(oracle_mod):
    O = oracle_mod
    img = gaussian_blob(128, 128, 64.0, 64.0, 4.0, amp=-60.0, bg=180.0)
    feats, _ = O.Oracle().run(img).fetch()
    assert np.min(np.hypot(feats["xpos"] - 64, feats["ypos"] - 64)) < 0.15


def test_descriptor_invariants(oracle_mod):
    O = oracle_mod
    img = synth(8, 200, 150)
    for norm_mode, multi in ((0, 0), (1, 0), (0, 9)):
        feats, desc = O.Oracle(O.default_params(norm_mode=norm_mode, norm_multi=multi)).run(img).fetch()
        assert len(feats) > 100 and len(desc) >= len(feats)
        assert np.all(desc >= 0.0)
        n2 = (desc.astype(np.float64) ** 2).sum(1)
        np.testing.assert_allclose(n2, 4.0 ** multi, rtol=2e-4)
        if norm_mode == 1:
            assert desc.max() <= 0.2 / 0.2 and desc.max() < 0.6  # clipped at 0.2*|v| before renorm
        assert feats["num_ori"].min() >= 1 and feats["num_ori"].max() <= 4
        for f in feats:
            k = int(f["num_ori"])
            assert np.all(f["desc_idx"][:k] >= 0) and np.all(f["desc_idx"][k:] == -1)
            assert np.all(f["orientation"][:k] >= -np.pi - 1e-6) and np.all(f["orientation"][:k] < np.pi + 1e-6)
        # descriptors are laid out feature by feature (s_orientation.cu:303-345)
        idx = np.concatenate([f["desc_idx"][:int(f["num_ori"])] for f in feats])
        assert np.array_equal(idx, np.arange(len(desc)))
        assert np.all(np.diff(feats["debug_octave"]) >= 0)


def test_rotation_by_90_degrees_is_covariant(oracle_mod):
    """Rotating the input by 90 degrees maps keypoints accordingly.  Not exact: the H-then-V
    rounding order is not rotation symmetric and the reference rejects offsets >= +1.5 but not
    <= -1.5 (s_extrema.cu:455-460), so a few threshold-edge keypoints differ."""
    O = oracle_mod
    img = synth(9, 128, 128)
    rot = np.ascontiguousarray(np.rot90(img, k=-1))      # clockwise: (x, y) -> (H-1-y, x)
    fa, da = O.Oracle(O.default_params(upscale_factor=0.0)).run(img).fetch()
    fb, db = O.Oracle(O.default_params(upscale_factor=0.0)).run(rot).fetch()
    assert abs(len(fa) - len(fb)) <= max(3, len(fa) // 50)
    H = img.shape[0]
    pts_b = np.stack([fb["xpos"], fb["ypos"], fb["sigma"]], 1)
    hit0 = n0 = hit = 0
    for f in fa:
        want = np.array([H - 1 - f["ypos"], f["xpos"], f["sigma"]])
        d = np.abs(pts_b - want).max(1).min()
        if f["debug_octave"] == 0:
            # octave 0: only rounding order differs -> essentially exact
            n0 += 1
            hit0 += d < 1e-3
        # octaves >= 1 sample every second pixel (s_pyramid_build.cu:50-71): x -> H-1-y maps the
        # even sampling grid onto the odd one, so positions agree only to a fraction of a pixel
        hit += d < 0.25 * 2.0 ** f["debug_octave"]
    assert n0 > 30 and hit0 >= 0.97 * n0
    assert hit >= 0.95 * len(fa)


def test_orientation_follows_image_rotation(oracle_mod):
    """For octave-0 keypoints matched across a 90-degree clockwise rotation, gradient angles
    turn by +90 degrees (y points down) and the descriptor is unchanged up to rounding."""
    O = oracle_mod
    img = synth(9, 128, 128)
    rot = np.ascontiguousarray(np.rot90(img, k=-1))
    fa, da = O.Oracle(O.default_params(upscale_factor=0.0)).run(img).fetch()
    fb, db = O.Oracle(O.default_params(upscale_factor=0.0)).run(rot).fetch()
    H = img.shape[0]
    checked = 0
    for f in fa[fa["debug_octave"] == 0]:
        d = np.hypot(fb["xpos"] - (H - 1 - f["ypos"]), fb["ypos"] - f["xpos"])
        j = int(np.argmin(d))
        if d[j] > 1e-3 or fb["num_ori"][j] != f["num_ori"]:
            continue
        for k in range(int(f["num_ori"])):
            want = f["orientation"][k] + np.pi / 2
            got = fb["orientation"][j][: fb["num_ori"][j]]
            err = np.abs(((got - want + np.pi) % (2 * np.pi)) - np.pi)
            q = int(np.argmin(err))
            assert err[q] < 2e-3
            a, b = da[f["desc_idx"][k]], db[fb["desc_idx"][j][q]]
            assert np.linalg.norm(a - b) < 2e-2 * np.linalg.norm(a)
            checked += 1
    assert checked > 30


def test_contrast_threshold_and_edge_rejection(oracle_mod):
    O = oracle_mod
    img = synth(10, 160, 120)
    n_default = O.Oracle().run(img).counts()[0]
    n_strict = O.Oracle(O.default_params(threshold=0.12)).run(img).counts()[0]
    n_edge = O.Oracle(O.default_params(edge_limit=2.0)).run(img).counts()[0]
    assert 0 < n_strict < n_default
    assert n_edge < n_default


def test_straight_edge_yields_no_keypoints(oracle_mod):
    O = oracle_mod
    img = np.zeros((96, 96), np.uint8)
    img[:, 48:] = 200          # a step edge: extrema along it fail the edge test / are not strict
    assert O.Oracle().run(img).counts()[0] == 0


def test_sift_modes_differ_but_overlap(oracle_mod):
    O = oracle_mod
    img = synth(12, 160, 120)
    sets = {}
    for mode in (0, 1, 2):
        f, _ = O.Oracle(O.default_params(sift_mode=mode)).run(img).fetch()
        sets[mode] = f
        assert len(f) > 50
    # OpenCV mode ignores a 5-pixel border (s_extrema.cu:331-335) on every octave
    e = O.Oracle(O.default_params(sift_mode=1)).run(img).extrema()
    assert e["xpos"].min() >= 4.4 and e["ypos"].min() >= 4.4


def test_max_extrema_caps_each_octave(oracle_mod):
    O = oracle_mod
    img = synth(13, 160, 120)
    o = O.Oracle(O.default_params(max_extrema=50)).run(img)
    assert max(o.ext_counts()) == 50
    assert o.counts()[0] == sum(o.ext_counts())


def test_grid_descriptor_mode(oracle_mod):
    """DescMode Grid (s_desc_grid.cu): same keypoints and orientations as Loop, a descriptor sampled
    on a fixed 16x16 grid per cell -- close to the Loop descriptor, normalised the same way."""
    O = oracle_mod
    img = synth(8, 200, 150)
    fa, da = O.Oracle(O.default_params()).run(img).fetch()
    fb, db = O.Oracle(O.default_params(desc_mode=2)).run(img).fetch()
    assert np.array_equal(fa, fb)                     # descriptors do not feed back into keypoints
    assert db.shape == da.shape and np.all(db >= 0)
    np.testing.assert_allclose((db.astype(np.float64) ** 2).sum(1), 1.0, rtol=2e-4)
    cos = np.sum(da * db, axis=1)                     # both RootSift-normalised: unit vectors
    assert np.median(cos) > 0.98 and cos.min() > 0.6
    assert not np.allclose(da, db)


def test_notile_descriptor_mode(oracle_mod):
    """DescMode NoTile (s_desc_notile.cu): 40x40 interpolated sample grid in the rotated frame."""
    O = oracle_mod
    img = synth(8, 200, 150)
    fa, da = O.Oracle(O.default_params()).run(img).fetch()
    fb, db = O.Oracle(O.default_params(desc_mode=4)).run(img).fetch()
    assert np.array_equal(fa, fb)
    assert db.shape == da.shape and np.all(db >= 0)
    np.testing.assert_allclose((db.astype(np.float64) ** 2).sum(1), 1.0, rtol=2e-4)
    cos = np.sum(da * db, axis=1)
    assert np.median(cos) > 0.995 and cos.min() > 0.6
    assert not np.allclose(da, db)


def test_interpolated_descriptor_modes(oracle_mod):
    """DescMode IGrid (s_desc_igrid.cu) evaluates NoTile's point lattice cell by cell: same numbers up to the
    summation order.  DescMode ILoop (s_desc_iloop.cu) is the loop descriptor's weighting on a fixed 32 x 32
    lattice per cell with the interpolated gradient: close to Loop, not equal."""
    O = oracle_mod
    img = synth(9, 180, 140)
    res = {m: O.Oracle(O.default_params(desc_mode=m)).run(img).fetch() for m in (0, 1, 3, 4)}
    for m in (1, 3, 4):
        assert np.array_equal(res[0][0], res[m][0])                       # keypoints do not depend on the mode
        np.testing.assert_allclose((res[m][1].astype(np.float64) ** 2).sum(1), 1.0, rtol=2e-4)
    rel = lambda a, b: np.linalg.norm(a - b, axis=1) / np.linalg.norm(a, axis=1)
    assert rel(res[4][1], res[3][1]).max() < 1e-5
    r = rel(res[0][1], res[1][1])
    cos = np.sum(res[0][1] * res[1][1], axis=1)
    assert 1e-4 < np.median(r) < 0.05 and np.median(cos) > 0.999 and cos.min() > 0.6


# ---- the keypoint stages on a given extremum list (oracle_keypoint_stages_from): what the capped-run checks stand on ----

FROM_CONFIGS = [dict(desc_mode=0), dict(desc_mode=2), dict(desc_mode=4), dict(sift_mode=1, desc_mode=0, norm_mode=1),
                dict(desc_mode=0, max_extrema=200)]


@pytest.mark.parametrize("kw", FROM_CONFIGS, ids=["loop", "grid", "notile", "opencv", "loop-capped"])
def test_keypoint_stages_from_own_extrema_are_bit_identical(oracle_mod, kw):
    """The oracle's own extrema fed into a pyramid-only oracle: the same features and descriptors, bit for bit."""
    O = oracle_mod
    img = synth(8, 200, 150)
    full = O.Oracle(O.default_params(**kw), threads=4).run(img)
    fa, da = full.fetch()
    ext = full.extrema()
    assert len(ext) > 100
    if "max_extrema" in kw:
        assert max(full.ext_counts()) == kw["max_extrema"]
    fresh = O.Oracle(O.default_params(**kw), threads=4).run(img, keypoints=False)
    assert fresh.counts() == (0, 0)
    fb, db = fresh.run_from_extrema(ext).fetch()
    assert fresh.ext_counts() == full.ext_counts()
    assert np.array_equal(fa.view(np.uint8), fb.view(np.uint8))
    assert np.array_equal(da.view(np.uint32), db.view(np.uint32))
    assert np.array_equal(fresh.extrema().view(np.uint8), ext.view(np.uint8))


@pytest.mark.parametrize("desc_mode", [0, 2])
def test_keypoint_stages_from_a_shuffled_subset(oracle_mod, desc_mode):
    """A subset shuffled within each octave (arrival order): every keypoint keeps its own orientations and
    descriptors, bit for bit, and the features come out in the order of the list."""
    O = oracle_mod
    img = synth(9, 180, 140)
    p = O.default_params(desc_mode=desc_mode)
    full = O.Oracle(p, threads=4).run(img)
    fa, da = full.fetch()
    ext = full.extrema()
    rng = np.random.default_rng(5)
    pick = np.sort(rng.choice(len(ext), size=len(ext) * 3 // 5, replace=False))
    pick = np.concatenate([rng.permutation(pick[ext["octave"][pick] == o]) for o in range(full.num_octaves)])
    assert np.all(np.diff(ext["octave"][pick]) >= 0) and not np.all(np.diff(pick) > 0)
    sub = O.Oracle(p, threads=4).run(img, keypoints=False).run_from_extrema(ext[pick])
    fb, db = sub.fetch()
    assert len(fb) == len(pick)
    assert sub.ext_counts() == np.bincount(ext["octave"][pick], minlength=full.num_octaves).tolist()
    for i, j in enumerate(pick):
        a, b = fa[j], fb[i]
        for f in ("debug_octave", "xpos", "ypos", "sigma", "num_ori"):
            assert a[f] == b[f], (i, j, f)
        n = int(a["num_ori"])
        assert np.array_equal(a["orientation"][:n].view(np.uint32), b["orientation"][:n].view(np.uint32)), (i, j)
        assert np.array_equal(da[a["desc_idx"][:n]].view(np.uint32), db[b["desc_idx"][:n]].view(np.uint32)), (i, j)
    # descriptors are laid out feature by feature in the list's order (s_orientation.cu:303-345)
    idx = np.concatenate([f["desc_idx"][:int(f["num_ori"])] for f in fb])
    assert np.array_equal(idx, np.arange(len(db)))


def test_keypoint_stages_from_rejects_malformed_lists(oracle_mod):
    O = oracle_mod
    img = synth(8, 200, 150)
    p = O.default_params(max_extrema=120)
    full = O.Oracle(O.default_params(), threads=4).run(img)
    ext = full.extrema()
    n_oct = full.num_octaves
    o0 = ext[ext["octave"] == 0]
    assert len(o0) > 120
    ok = ext[np.concatenate([np.nonzero(ext["octave"] == o)[0][:120] for o in range(n_oct)])]

    cases = {}
    e = ok.copy(); e["octave"][-1] = n_oct; cases["octave past the last"] = e
    e = ok.copy(); e["octave"][0] = -1; cases["negative octave"] = e
    cases["not grouped by ascending octave"] = ok[::-1].copy()
    cases["more than max_extrema in an octave"] = np.concatenate([o0[:121], ok[ok["octave"] > 0]])
    e = ok.copy(); e["xpos"][3] = full.octave_dims(0)[0]; cases["x outside the plane"] = e
    e = ok.copy(); e["ypos"][3] = -0.5; cases["y outside the plane"] = e
    e = ok.copy(); e["xpos"][3] = np.nan; cases["NaN position"] = e
    e = ok.copy(); e["sigma"][3] = 0.0; cases["zero sigma"] = e
    e = ok.copy(); e["sigma"][3] = np.inf; cases["infinite sigma"] = e
    orc = O.Oracle(p, threads=4).run(img, keypoints=False)
    for what, e in cases.items():
        with pytest.raises(ValueError):
            orc.run_from_extrema(e)
        assert orc.counts() == (0, 0), what          # rejected: nothing computed, nothing replaced
    with pytest.raises(TypeError):
        orc.run_from_extrema(np.zeros(3, O.FEATURE_DTYPE))
    with pytest.raises(ValueError):                  # no planes yet
        O.Oracle(p).run_from_extrema(ok[:5])
    # the well-formed list is accepted, and a rejected one after it leaves its results in place
    orc.run_from_extrema(ok)
    before = orc.fetch()
    with pytest.raises(ValueError):
        orc.run_from_extrema(cases["not grouped by ascending octave"])
    after = orc.fetch()
    assert np.array_equal(before[0].view(np.uint8), after[0].view(np.uint8))
    assert np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
    # an empty list: no features
    assert orc.run_from_extrema(ok[:0]).counts() == (0, 0)


def test_capped_parity_passes_a_capped_oracle_run_and_catches_defects(oracle_mod):
    """util.capped_parity on a capped oracle run (raster-order survivors) standing in for a batch item, then on
    copies with the defects it exists to catch: each must raise, naming what is wrong."""
    from util import capped_parity
    O = oracle_mod
    img = synth(21, 200, 150)
    cap = 150
    full = O.Oracle(O.default_params(max_extrema=100000), threads=4).run(img)
    capped = O.Oracle(O.default_params(max_extrema=cap), threads=4).run(img)
    counts = full.ext_counts()
    assert counts[0] > cap and counts[1] < cap
    assert capped.ext_counts() == [min(c, cap) for c in counts]
    fc, dc = capped.fetch()
    pyr = lambda: O.Oracle(O.default_params(max_extrema=cap), threads=4).run(img, keypoints=False)
    capped_parity(full.extrema(), cap, (fc, dc), 1.0, orc=pyr(), full_dev=full.fetch())

    def expect(msg, f, d):
        with pytest.raises(AssertionError, match=msg):
            capped_parity(full.extrema(), cap, (f, d), 1.0, orc=pyr(), full_dev=full.fetch())

    i = int(np.nonzero(fc["debug_octave"] == 0)[0][-1])
    f = fc.copy(); f["sigma"][i] = np.nextafter(f["sigma"][i], np.float32(0)); expect("not uncapped extrema", f, dc)
    expect("per-octave counts", fc[np.arange(len(fc)) != i], dc)                     # one survivor short
    f = fc.copy(); f[i] = f[i - 1]; expect("repeated", f, dc)                          # a survivor twice
    f = fc.copy(); f["debug_octave"][i] = 1; expect("per-octave counts", f, dc)       # in the next octave's region
    d = dc.copy(); d[fc["desc_idx"][i][0]] *= 1.0001
    with pytest.raises(AssertionError, match="not bit-identical"):
        capped_parity(full.extrema(), cap, (fc, d), 1.0, full_dev=full.fetch())
    f = fc.copy(); f["orientation"][i][0] = np.nextafter(f["orientation"][i][0], np.float32(9))
    with pytest.raises(AssertionError, match="not bit-identical"):
        capped_parity(full.extrema(), cap, (f, dc), 1.0, full_dev=full.fetch())
    d = dc.copy(); d[fc["desc_idx"][i][0]] = np.roll(d[fc["desc_idx"][i][0]], 8)   # another keypoint's frame, in effect
    expect("oracle", fc, d)


class _OracleAsContext:
    """The three calls capped_parity makes on a device Context, answered by a capped oracle run."""

    def __init__(self, O, orc):
        self._o, self._O = orc, O
        self.ext_ct = orc.ext_counts() + [0] * (O.MAX_OCTAVES - orc.num_octaves)
        self.num_octaves, self.ext_total = orc.num_octaves, orc.counts()[0]

    def fetch(self):
        return self._o.fetch()

    def extrema(self):
        return self._o.extrema()

    def report(self):
        return self


def test_capped_parity_on_a_context(oracle_mod):
    """The Context form of util.capped_parity (report counts, extrema() identity with lpos, features against the list)."""
    from util import capped_parity
    O = oracle_mod
    img = synth(22, 200, 150)
    cap = 97
    full = O.Oracle(O.default_params(), threads=4).run(img)
    capped = O.Oracle(O.default_params(max_extrema=cap), threads=4).run(img)
    assert full.ext_counts()[0] > cap
    pyr = lambda: O.Oracle(O.default_params(max_extrema=cap), threads=4).run(img, keypoints=False)
    stub = _OracleAsContext(O, capped)
    capped_parity(full.extrema(), cap, stub, 1.0, orc=pyr(), full_dev=full.fetch())
    stub.ext_ct[0] -= 1
    with pytest.raises(AssertionError, match="report"):
        capped_parity(full.extrema(), cap, stub, 1.0)
    stub = _OracleAsContext(O, capped)
    e = capped.extrema()
    e["lpos"][5] += 1
    stub.extrema = lambda: e
    with pytest.raises(AssertionError, match="extrema\\(\\) entries"):
        capped_parity(full.extrema(), cap, stub, 1.0)
