"""The epipolar verifier's rule on the CPU (tests/epipolar_ref.c): the two-view scene the GPU tests rely on -- checked here
against an independent float64 SVD 8-point --, one scene per step of the rule that depends on the step, and the interface
of popsift_hip_epipolar as far as it needs no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import epipolar_rule as E
import ransac_rule as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return E.Ref(tmp_path_factory.mktemp("epipolar_ref"))


@pytest.fixture(scope="module")
def two_view(ref):
    """the scene and the rule's answer, computed once: n = 1000, 60 % inliers, max_err 0.5, T = 1500, seed 0"""
    pts, inl, F = E.two_view(1000, 1)
    out = ref.epipolar(pts, 1500, 0.5, 0)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return pts, inl, F, out


def test_sampler(ref):
    """step 1 of the sibling with m = 8: same hash, same draws (the first 4 slots of a sample are the sibling's sample)"""
    sibling = R.Ref(os.path.dirname(ref.lib._name))
    for n in (8, 9, 64, 1000, 1 << 24):
        s, valid = ref.samples(7, n, 500)
        ok = valid == 1
        assert ((s[ok] >= 0) & (s[ok] < n)).all() and all(len(set(row)) == 8 for row in s[ok])
        for row in s[~ok]:                      # found slots, then -1 from the failed slot on
            k = list(row).index(-1)
            assert 0 < k < 8 and (row[k:] == -1).all() and len(set(row[:k])) == k
        s4, v4 = sibling.samples(7, n, R.HOMOGRAPHY, 500)
        assert np.array_equal(s[v4 == 1][:, :4], s4[v4 == 1]) and (valid <= v4).all()
        if n >= 64:
            assert ok.sum() > 400
    s, valid = ref.samples(3, 8, 2000)          # n = m: a permutation of 0 .. 7, or invalid
    assert 0 < (valid == 1).sum() and all(sorted(row) == list(range(8)) for row in s[valid == 1])


def svd_eight_point(pts8):
    """the textbook float64 8-point algorithm: Hartley normalisation (centroid, mean distance sqrt 2), the right singular
    vector of the smallest singular value, rank-2 truncation by a second SVD, denormalisation"""
    p = np.asarray(pts8, np.float64)

    def hartley(xy):
        c = xy.mean(0)
        s = np.sqrt(2.0) / np.hypot(*(xy - c).T).mean()
        return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1]])
    Tl, Tr = hartley(p[:, :2]), hartley(p[:, 2:])
    l = np.c_[p[:, :2], np.ones(8)] @ Tl.T
    r = np.c_[p[:, 2:], np.ones(8)] @ Tr.T
    A = np.stack([r[:, i] * l[:, j] for i in range(3) for j in range(3)], 1)
    Fn = np.linalg.svd(A)[2][-1].reshape(3, 3)
    U, S, Vt = np.linalg.svd(Fn)
    return Tr.T @ (U @ np.diag([S[0], S[1], 0.0]) @ Vt) @ Tl


def test_two_view_scene(two_view):
    """The winner's mask is the planted mask, and the textbook SVD 8-point on the winner's sample agrees.  Reference figures
    (seed 0): winner t = 266 with 600 of 600 and no extras; Sampson distances of the planted inliers at most 1.3e-4 px under
    the rule's F and 1.3e-4 px under the SVD's; of the outliers at least 15.59 px under both.  The bounds are the specification's:
    1e-3 px and 10 px (a 20 px perpendicular offset is about 20 / sqrt(2) px of Sampson distance)."""
    pts, inl, _, out = two_view
    res = out["result"]
    assert inl.sum() == 600
    assert res["hypothesis"] >= 0 and res["n_inliers"] == 600 and res["n_valid"] > 1400
    assert np.array_equal(out["mask"], inl)
    t = int(res["hypothesis"])
    assert out["counts"][t] == 600 == out["counts"].max() and t == np.flatnonzero(out["counts"] == 600)[0]
    assert out["models"][t].tobytes() == res["H"].tobytes()
    assert np.abs(res["H"]).max() == 1.0 == res["H"][np.argmax(np.abs(res["H"]))]   # scaled: the largest entry is exactly 1
    sample = out["samples"][t]
    assert inl[sample].all()
    for name, F in (("rule", res["H"]), ("svd", svd_eight_point(pts[sample]))):
        d = E.sampson(F, pts)
        print(name, "inliers max %.3g px, outliers min %.4g px" % (d[inl == 1].max(), d[inl == 0].min()))
        assert d[inl == 1].max() < 1e-3 and d[inl == 0].min() > 10.0, name


def rel_det(F):
    F = np.asarray(F, np.float64).reshape(3, 3)
    return abs(np.linalg.det(F)) / np.linalg.norm(F) ** 3


def rounding_bound(F):
    """what rounding the nine entries of an exactly singular matrix to float32 can do to |det| / ||F||^3, to first order:
    2^-24 * sum |F_ij * cofactor_ij| / ||F||^3"""
    F = np.asarray(F, np.float64).reshape(3, 3)
    s = sum(abs(F[i, j] * np.linalg.det(np.delete(np.delete(F, i, 0), j, 1))) for i in range(3) for j in range(3))
    return 2.0 ** -24 * s / np.linalg.norm(F) ** 3


def test_rank2_step_has_teeth(ref, two_view):
    """|det F| / ||F||^3 of the winner, in float64 from its nine floats.  Reference figures (seed 0, winner t = 266 with and
    without the step): 1.2e-17 with the rank-2 step, 1.1e-15 without it.  Both are far below the specified 1e-6 because F is in
    pixel units (its entries span 1e-6 .. 1, so every product in det is at most about 1e-12 of ||F||^3) and because the
    planted inliers are exact, so that even the unprojected solution is singular up to the float32 rounding of its sample's
    points.  What separates the two is therefore stated relative to what float32 rounding of the nine entries alone can
    give (rounding_bound, 5.6e-17 here): the rule's value lies within it -- its float64 matrix is singular to about 1e-16 of
    that -- and the value without the step (20 times the bound) cannot come from rounding; 4 x leaves room for the
    second-order terms the bound ignores and a factor 5 to the figure."""
    pts, _, _, out = two_view
    broken = ref.epipolar(pts, 1500, 0.5, 0, variant=E.NO_RANK2)
    F, G = out["result"]["H"], broken["result"]["H"]
    print("with the step %.3g (bound %.3g), without %.3g (bound %.3g)" % (rel_det(F), rounding_bound(F), rel_det(G), rounding_bound(G)))
    assert out["result"]["hypothesis"] >= 0 and broken["result"]["hypothesis"] >= 0
    assert rel_det(F) <= 1e-6
    assert rel_det(F) <= rounding_bound(F)
    assert rel_det(G) > 4.0 * rounding_bound(G) and rel_det(G) > 4.0 * rel_det(F)
    # every valid hypothesis, not only the winner: the projected models are singular within rounding
    ok = out["counts"] >= 0
    worst = max(rel_det(m) / rounding_bound(m) for m in out["models"][ok])
    print("largest det / bound over %d hypotheses: %.3g" % (ok.sum(), worst))
    assert worst <= 1.0


def test_g_test_has_teeth(ref):
    """identical pairs: no hypothesis has a model.  Every hypothesis is scored all the same, with the all-zero model it
    stores: r = g = 0, so without `g > 0` each would add all n pairs to its count of -1 and the first would win."""
    n = 50
    pts = E.identical(n)
    a = ref.epipolar(pts, 200, 0.5, 1)
    assert (a["counts"] == -1).all() and not a["models"].any() and not a["mask"].any()
    res = a["result"]
    assert (res["hypothesis"], res["n_inliers"], res["n_valid"]) == (-1, 0, 0) and not res["H"].any()
    b = ref.epipolar(pts, 200, 0.5, 1, variant=E.NO_G_TEST)
    assert (b["counts"] == n - 1).all() and not b["models"].any() and b["mask"].all()
    res = b["result"]
    assert (res["hypothesis"], res["n_inliers"], res["n_valid"]) == (0, n - 1, 200) and not res["H"].any()
    # a scene with models: a pair at the origin of both images, where most terms vanish, still has g > 0
    pts = E.two_view(300, 2)[0]
    pts[7] = 0.0
    a, b = ref.epipolar(pts, 300, 0.5, 4), ref.epipolar(pts, 300, 0.5, 4, variant=E.NO_G_TEST)
    assert (a["counts"] >= 0).all() and np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["mask"], b["mask"])


def test_complete_pivoting_on_a_sideways_translation(ref):
    """x' = x + disparity, y' = y: F = [[0, 0, 0], [0, 0, -1], [0, 1, 0]] up to sign, F22 = 0.  The rule finds every pair in
    every hypothesis and returns |F22| below 1e-9 (reference: 3.4e-13 at n = 300; the unknown is 0 up to the float64 solve's
    rounding, about 1e-16 times the conditioning of a sample).
    The specification expected the variant that fixes the last unknown to 1 (partial pivoting, column 8 as the right-hand side) to
    miss pairs here.  It does not: in float64 its last pivot is not 0 but about 1e-17, the solution is about 1e16 times the
    null vector plus a particular solution of size 1, and after the scaling of step 5 that is the same F (reference: 300 of
    300 in every hypothesis, |F22| 1.7e-12).  So what is asserted of the variant is what holds: it takes another path -- its
    models differ from the rule's as bytes -- and it is no better.  The rule's own requirement, every pair found with
    F22 = 0, is asserted in full."""
    n = 300
    pts = E.translation(n)
    a = ref.epipolar(pts, 500, 0.5, 0)
    b = ref.epipolar(pts, 500, 0.5, 0, variant=E.LAST_UNKNOWN_FIXED)
    assert a["result"]["n_inliers"] == n and a["mask"].all() and (a["counts"] == n).all()
    F = a["result"]["H"].astype(np.float64)
    print("rule F", F, "variant F", b["result"]["H"])
    assert abs(F[8]) < 1e-9 and np.abs(F[[0, 1, 2, 3, 4, 6]]).max() < 1e-9 and abs(abs(F[5]) - 1) < 1e-6 and abs(F[5] + F[7]) < 1e-6
    assert E.sampson(F, pts).max() < 1e-3
    assert (a["models"].view(np.uint32) != b["models"].view(np.uint32)).any(1).mean() > 0.9
    assert b["result"]["n_inliers"] <= n


def test_tie_break_has_teeth(ref, two_view):
    pts, _, _, a = two_view
    b = ref.epipolar(pts, 1500, 0.5, 0, variant=E.TIE_TO_HIGHEST)
    top = np.flatnonzero(a["counts"] == a["counts"].max())
    assert len(top) > 5
    assert a["result"]["hypothesis"] == top[0] and b["result"]["hypothesis"] == top[-1]
    assert a["result"]["H"].tobytes() != b["result"]["H"].tobytes()


def test_nan_pair(ref):
    n = 300
    pts = E.with_nan(n)
    clean, inl, _ = E.two_view(n, 4)
    out = ref.epipolar(pts, 2000, 0.5, 2)
    want = inl.copy()
    want[[n // 3, n // 2]] = 0                       # a NaN fails both tests, whatever the pair was
    assert np.array_equal(out["mask"], want)
    # a sample that holds one of the two pairs has no model; every other hypothesis is untouched by them
    bad = np.isin(out["samples"], [n // 3, n // 2]).any(axis=1)
    assert bad.any() and (out["counts"][bad] == -1).all() and not out["models"][bad].any()
    assert (out["counts"][~bad] >= 0).all()
    # the bounding box skips them: the other models are those of the clean scene
    assert out["models"][~bad].tobytes() == ref.epipolar(clean, 2000, 0.5, 2)["models"][~bad].tobytes()


def test_degenerate_sets(ref):
    for n in range(8):                               # fewer pairs than a sample
        out = ref.epipolar(E.two_view(8, 1)[0][:n], 10, 0.5, 1)
        assert out["result"]["hypothesis"] == -1 and (out["counts"] == -1).all() and (out["samples"] == -1).all()
    # exactly a sample: the model passes through its own pairs
    pts = E.two_view(8, 1, 1.0)[0]
    out = ref.epipolar(pts, 400, 0.5, 1)
    assert out["result"]["n_inliers"] == 8 and out["mask"].all()
    # planar and collinear pairs: degenerate, the reference is the definition; it still returns a model all pairs fit
    for name in ("planar", "collinear"):
        out = ref.epipolar(E.scene(name, 200), 100, 0.5, 1)
        assert out["result"]["n_inliers"] == 200


def test_binding_mirrors_the_header(hip):
    txt = open(os.path.join(ROOT, "include", "popsift_hip.h")).read()
    assert int(re.search(r"#define POPSIFT_HIP_EPIPOLAR_SAMPLE (\d+)", txt).group(1)) == hip.EPIPOLAR_SAMPLE == E.SAMPLE == 8
    assert C.sizeof(hip.EpipolarOpts) == 24
    o = hip.epipolar_opts()
    assert (o.hypotheses, o.max_err, o.seed, tuple(o.reserved)) == (2048, 2.0, 0, (0, 0, 0))
    o = hip.epipolar_opts(hypotheses=7, max_err=0.25, seed=0xffffffff)
    assert (o.hypotheses, o.max_err, o.seed) == (7, 0.25, 0xffffffff)
    # the sibling's options are untouched: a numeric model 2 still passes through, to be refused
    assert hip.ransac_opts(model=2).model == 2 and "epipolar" not in hip.MODELS


def test_invalid_arguments_are_rejected_without_a_gpu(hip):
    """every ERR_INVALID case of popsift_hip_epipolar / _trace; none of them reaches a GPU call, so they hold on a machine
    without one (the verifier pointer is never dereferenced before the checks pass)"""
    lib = hip.lib()
    pts = E.two_view(16)[0]
    res = np.zeros(1, hip.RANSAC_RESULT_DTYPE)
    fake = C.c_void_p(pts.ctypes.data)               # a non-NULL "verifier": the argument checks come first
    call = lambda v, p, n, o, r: lib.popsift_hip_epipolar(v, p, n, C.byref(o) if o is not None else None, r, None)
    trace = lambda v, p, n, o: lib.popsift_hip_epipolar_trace(v, p, n, C.byref(o) if o is not None else None, None, None, None)
    good = hip.epipolar_opts(hypotheses=8, max_err=1.0)
    assert call(None, pts.ctypes.data, 16, good, res.ctypes.data) == hip.ERR_INVALID
    assert call(fake, pts.ctypes.data, 16, None, res.ctypes.data) == hip.ERR_INVALID
    assert call(fake, pts.ctypes.data, 16, good, None) == hip.ERR_INVALID
    assert call(fake, None, 16, good, res.ctypes.data) == hip.ERR_INVALID
    assert call(fake, pts.ctypes.data, -1, good, res.ctypes.data) == hip.ERR_INVALID
    assert call(fake, pts.ctypes.data, (1 << 24) + 1, good, res.ctypes.data) == hip.ERR_INVALID
    assert trace(None, pts.ctypes.data, 16, good) == hip.ERR_INVALID
    assert trace(fake, pts.ctypes.data, 16, None) == hip.ERR_INVALID
    assert trace(fake, None, 16, good) == hip.ERR_INVALID
    assert trace(fake, pts.ctypes.data, -1, good) == hip.ERR_INVALID
    assert trace(fake, pts.ctypes.data, (1 << 24) + 1, good) == hip.ERR_INVALID
    for kw in (dict(hypotheses=0), dict(hypotheses=-1), dict(hypotheses=65537), dict(max_err=0.0), dict(max_err=-1.0),
               dict(max_err=float("nan")), dict(max_err=float("inf"))):
        o = hip.epipolar_opts(**{**dict(hypotheses=8, max_err=1.0), **kw})
        assert call(fake, pts.ctypes.data, 16, o, res.ctypes.data) == hip.ERR_INVALID, kw
        assert trace(fake, pts.ctypes.data, 16, o) == hip.ERR_INVALID, kw
    for k in (0, 1, 2):
        o = hip.epipolar_opts(hypotheses=8, max_err=1.0)
        o.reserved[k] = 1
        assert call(fake, pts.ctypes.data, 16, o, res.ctypes.data) == hip.ERR_INVALID
        assert trace(fake, pts.ctypes.data, 16, o) == hip.ERR_INVALID
    # fewer pairs than a sample: answered on the host
    for n in (7, 4, 1):
        res[0]["hypothesis"] = 5
        assert call(fake, pts.ctypes.data, n, good, res.ctypes.data) == hip.OK
        assert (res[0]["hypothesis"], res[0]["n_inliers"], res[0]["n_valid"]) == (-1, 0, 0) and not res[0]["H"].any()
    assert call(fake, None, 0, good, res.ctypes.data) == hip.OK and res[0]["hypothesis"] == -1
    s, m, c = np.zeros((8, 8), np.int32), np.ones((8, 9), np.float32), np.zeros(8, np.int32)
    assert lib.popsift_hip_epipolar_trace(fake, pts.ctypes.data, 7, C.byref(good), s.ctypes.data, m.ctypes.data,
                                          c.ctypes.data) == hip.OK
    assert (s == -1).all() and not m.any() and (c == -1).all()
    mask = np.ones(7, np.uint8)
    assert lib.popsift_hip_epipolar(fake, pts.ctypes.data, 7, C.byref(good), res.ctypes.data, mask.ctypes.data) == hip.OK
    assert not mask.any()
    # popsift_hip_ransac does not know the new model: 2 stays refused
    o = hip.ransac_opts(model=2, hypotheses=8, max_err=1.0)
    assert lib.popsift_hip_ransac(fake, pts.ctypes.data, 16, C.byref(o), res.ctypes.data, None) == hip.ERR_INVALID
