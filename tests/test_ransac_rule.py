"""The verifier's rule on the CPU (tests/ransac_ref.c): the sampler's contract, the planted scene the GPU tests rely on
-- checked here against an independent float64 computation -- and one scene per step of the rule whose result changes when
that step is broken."""
import os
import re

import numpy as np
import pytest

import ransac_rule as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return R.Ref(tmp_path_factory.mktemp("ransac_ref"))


@pytest.mark.parametrize("model", [R.HOMOGRAPHY, R.AFFINE])
def test_sampler(ref, model):
    m = R.SAMPLE_SIZE[model]
    for n in (m, 5, 64, 1000, 1 << 24):
        s, valid = ref.samples(7, n, model, 500)
        ok = valid == 1
        assert ok.sum() > 400
        assert ((s[ok][:, :m] >= 0) & (s[ok][:, :m] < n)).all() and (s[:, m:] == -1).all()
        assert all(len(set(row[:m])) == m for row in s[ok])
        for row in s[~ok]:                      # found slots, then -1 from the failed slot on
            k = list(row).index(-1)
            assert 0 < k < m and (row[k:] == -1).all() and len(set(row[:k])) == k
        other, _ = ref.samples(8, n, model, 500)
        assert (other != s).any()
        if n > 64:
            assert len(np.unique(s[ok][:, 0])) > 300  # spread over the range, not stuck
    # n = m: a permutation of 0 .. m-1, or invalid
    s, valid = ref.samples(3, m, model, 300)
    assert 0 < (valid == 0).sum() < 150
    assert all(sorted(row[:m]) == list(range(m)) for row in s[valid == 1])


def test_samples_do_not_depend_on_the_points(ref):
    a, b = R.planted(200, 1)[0], R.all_outliers(200)
    for model in (R.HOMOGRAPHY, R.AFFINE):
        sa = ref.ransac(a, model, 100, 0.5, 11)["samples"]
        assert np.array_equal(sa, ref.ransac(b, model, 100, 0.5, 11)["samples"])
        assert np.array_equal(sa, ref.samples(11, 200, model, 100)[0])


def float64_mask(pts, sample, model, max_err):
    """an independent statement of what the winner's sample implies: numpy.linalg.solve on the sample's pairs in float64,
    projection and distance in float64 -> (inlier mask, distances)"""
    p = pts.astype(np.float64)
    x, y, u, v = p[sample].T
    if model == R.AFFINE:
        A = np.c_[x, y, np.ones(3)]
        Hm = np.vstack([np.linalg.solve(A, u), np.linalg.solve(A, v), [0, 0, 1]])
    else:
        A = np.zeros((8, 8))
        A[0::2] = np.c_[x, y, np.ones(4), np.zeros((4, 3)), -u * x, -u * y]
        A[1::2] = np.c_[np.zeros((4, 3)), x, y, np.ones(4), -v * x, -v * y]
        b = np.zeros(8)
        b[0::2], b[1::2] = u, v
        Hm = np.append(np.linalg.solve(A, b), 1.0).reshape(3, 3)
    d = np.hypot(*(R.project(Hm, p[:, :2]) - p[:, 2:]).T)
    return d <= max_err, d


@pytest.mark.parametrize("model", [R.HOMOGRAPHY, R.AFFINE])
def test_planted_scene(ref, model):
    """n = 1000, 60 % inliers, max_err = 0.5, T = 1000: the winner's mask is the planted one, and the float64 check agrees
    with margins of 1e-3 px on one side and 20 px on the other -- nothing here is tuned."""
    pts, inl, _ = R.planted(1000, 1, model)
    assert inl.sum() == 600
    out = ref.ransac(pts, model, 1000, 0.5, 5)
    res = out["result"]
    assert res["hypothesis"] >= 0 and res["n_inliers"] == 600 and res["n_valid"] > 900
    assert np.array_equal(out["mask"], inl)
    t = int(res["hypothesis"])
    assert out["counts"][t] == 600 == out["counts"].max() and t == np.flatnonzero(out["counts"] == 600)[0]
    assert out["models"][t].tobytes() == res["H"].tobytes()
    sample = out["samples"][t][:R.SAMPLE_SIZE[model]]
    assert inl[sample].all()
    mask64, d = float64_mask(pts, sample, model, 0.5)
    assert np.array_equal(mask64, inl.astype(bool))
    assert d[inl == 1].max() < 1e-3 and d[inl == 0].min() > 20.0 - 1e-3


def test_tie_break_has_teeth(ref):
    pts = R.planted(1000, 1)[0]
    a = ref.ransac(pts, R.HOMOGRAPHY, 1000, 0.5, 5)
    b = ref.ransac(pts, R.HOMOGRAPHY, 1000, 0.5, 5, variant=R.TIE_TO_HIGHEST)
    top = np.flatnonzero(a["counts"] == a["counts"].max())
    assert len(top) > 10
    assert a["result"]["hypothesis"] == top[0] and b["result"]["hypothesis"] == top[-1]
    assert a["result"]["H"].tobytes() != b["result"]["H"].tobytes()


def test_w_test_has_teeth(ref):
    """the horizon scene: pairs behind the winner's horizon satisfy e <= lim and are inliers only without `w > 0`"""
    pts = R.horizon(600)
    a = ref.ransac(pts, R.HOMOGRAPHY, 200, 0.5, 9)
    b = ref.ransac(pts, R.HOMOGRAPHY, 200, 0.5, 9, variant=R.NO_W_TEST)
    front = pts[:, 0] > 300.0
    assert 0.3 < front.mean() < 0.9
    assert np.array_equal(a["mask"], front.astype(np.uint8)) and a["result"]["n_inliers"] == front.sum()
    assert b["mask"].all() and b["result"]["n_inliers"] == len(pts)


def test_nan_pair(ref):
    for model in (R.HOMOGRAPHY, R.AFFINE):
        n = 300
        pts = R.with_nan(n, 4, model)
        clean, inl, _ = R.planted(n, 4, model)
        out = ref.ransac(pts, model, 400, 0.5, 2)
        want = inl.copy()
        want[[n // 3, n // 2]] = 0                       # a NaN fails both tests, whatever the pair was
        assert np.array_equal(out["mask"], want)
        # a sample that holds one of the two pairs has no model; every other hypothesis is untouched by them
        bad = np.isin(out["samples"], [n // 3, n // 2]).any(axis=1)
        assert bad.any() and (out["counts"][bad] == -1).all() and not out["models"][bad].any()
        assert (out["counts"][~bad] >= 0).sum() > 300
        # the bounding box skips them: the other models are those of the clean scene
        assert out["models"][~bad].tobytes() == ref.ransac(clean, model, 400, 0.5, 2)["models"][~bad].tobytes()


def test_degenerate_sets(ref):
    for model in (R.HOMOGRAPHY, R.AFFINE):
        m = R.SAMPLE_SIZE[model]
        out = ref.ransac(R.identical(50), model, 200, 0.5, 1)
        assert (out["counts"] == -1).all() and not out["models"].any() and not out["mask"].any()
        res = out["result"]
        assert (res["hypothesis"], res["n_inliers"], res["n_valid"]) == (-1, 0, 0) and not res["H"].any()
        # fewer pairs than a sample
        for n in range(m):
            out = ref.ransac(R.planted(8, 1, model)[0][:n], model, 10, 0.5, 1)
            assert out["result"]["hypothesis"] == -1 and (out["counts"] == -1).all() and (out["samples"] == -1).all()
        # exactly a sample: the model passes through its own pairs
        pts = R.planted(8, 1, model)[0][:m]
        out = ref.ransac(pts, model, 50, 0.5, 1)
        assert out["result"]["n_inliers"] == m and out["mask"].all()


def test_binding_mirrors_the_header(hip):
    """the structures and the two kernel-shape constants of the verifier as a C compiler sees them"""
    import ctypes as C
    txt = open(os.path.join(ROOT, "include", "popsift_hip.h")).read()
    assert int(re.search(r"#define POPSIFT_HIP_RANSAC_CHUNK (\d+)", txt).group(1)) == hip.RANSAC_CHUNK
    assert int(re.search(r"#define POPSIFT_HIP_RANSAC_HYP_BLOCK (\d+)", txt).group(1)) == hip.RANSAC_HYP_BLOCK
    assert hip.RANSAC_RESULT_DTYPE == R.RESULT_DTYPE and hip.RANSAC_RESULT_DTYPE.itemsize == 52
    assert C.sizeof(hip.RansacOpts) == 24
    o = hip.ransac_opts()
    assert (o.model, o.hypotheses, o.max_err, o.seed, tuple(o.reserved)) == (0, 2048, 2.0, 0, (0, 0))


def test_invalid_arguments_are_rejected_without_a_gpu(hip):
    """every ERR_INVALID case of popsift_hip_ransac / _trace / _pair_points; none of them reaches a GPU call, so they hold
    on a machine without one (the verifier pointer is never dereferenced before the checks pass)"""
    import ctypes as C
    lib = hip.lib()
    pts = R.planted(16)[0]
    res = np.zeros(1, hip.RANSAC_RESULT_DTYPE)
    fake = C.c_void_p(pts.ctypes.data)               # a non-NULL "verifier": the argument checks come first
    call = lambda v, p, n, o, r: lib.popsift_hip_ransac(v, p, n, C.byref(o) if o is not None else None, r, None)
    good = hip.ransac_opts(hypotheses=8, max_err=1.0)
    assert call(None, pts.ctypes.data, 16, good, res.ctypes.data) == hip.ERR_INVALID
    assert call(fake, pts.ctypes.data, 16, None, res.ctypes.data) == hip.ERR_INVALID
    assert call(fake, pts.ctypes.data, 16, good, None) == hip.ERR_INVALID
    assert call(fake, None, 16, good, res.ctypes.data) == hip.ERR_INVALID
    assert call(fake, pts.ctypes.data, -1, good, res.ctypes.data) == hip.ERR_INVALID
    assert call(fake, pts.ctypes.data, (1 << 24) + 1, good, res.ctypes.data) == hip.ERR_INVALID
    for kw in (dict(model=2), dict(model=-1), dict(hypotheses=0), dict(hypotheses=65537), dict(max_err=0.0),
               dict(max_err=-1.0), dict(max_err=float("nan")), dict(max_err=float("inf"))):
        assert call(fake, pts.ctypes.data, 16, hip.ransac_opts(**{**dict(hypotheses=8, max_err=1.0), **kw}),
                    res.ctypes.data) == hip.ERR_INVALID, kw
    for k in (0, 1):
        o = hip.ransac_opts(hypotheses=8, max_err=1.0)
        o.reserved[k] = 1
        assert call(fake, pts.ctypes.data, 16, o, res.ctypes.data) == hip.ERR_INVALID
        assert lib.popsift_hip_ransac_trace(fake, pts.ctypes.data, 16, C.byref(o), None, None, None) == hip.ERR_INVALID
    assert lib.popsift_hip_ransac_trace(None, pts.ctypes.data, 16, C.byref(good), None, None, None) == hip.ERR_INVALID
    # fewer pairs than a sample: answered on the host
    assert call(fake, pts.ctypes.data, 3, good, res.ctypes.data) == hip.OK
    assert (res[0]["hypothesis"], res[0]["n_inliers"], res[0]["n_valid"]) == (-1, 0, 0)
    assert call(fake, None, 0, good, res.ctypes.data) == hip.OK and res[0]["hypothesis"] == -1
    assert lib.popsift_hip_verifier_create(0, None) == hip.ERR_INVALID
    assert lib.popsift_hip_verifier_free(None) == hip.OK
    assert lib.popsift_hip_pair_points(None, None, None, 0, None) == hip.ERR_INVALID
