"""popsift_hip_epipolar on the GPU, byte for byte against the CPU restatement of its rule (tests/epipolar_ref.c): the trace
(samples, models, counts), the result record and the mask, at the sizes where the kernels change behaviour; the scratch it
shares with popsift_hip_ransac; and a rolled image pair end to end."""
import ctypes as C

import numpy as np
import pytest

import epipolar_rule as E
from popsift_amd import _capi
from popsift_amd.synth import synth

pytestmark = pytest.mark.gpu

CHUNK, HYP = _capi.RANSAC_CHUNK, _capi.RANSAC_HYP_BLOCK
# (n, T, scene): exactly a sample and one more; around a wave and a workgroup; one below / at / one above the scoring kernel's
# pair chunk; three chunks with a partial last one; T = 1, around a wave, one above the hypothesis block, several blocks
CASES = [(8, 1, "two_view"), (9, 63, "two_view"), (63, HYP + 1, "outliers"), (64, 257, "nan"), (65, 1000, "two_view"),
         (255, 64, "collinear"), (256, HYP + 1, "planar"), (257, 63, "identical"), (1000, 1000, "two_view"),
         (CHUNK - 1, HYP + 1, "translation"), (CHUNK, 64, "outliers"), (CHUNK + 1, 257, "nan"),
         (2 * CHUNK + 452, HYP + 1, "two_view")]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return E.Ref(tmp_path_factory.mktemp("epipolar_ref"))


@pytest.fixture(scope="module")
def verifier(gpu_hip):
    v = gpu_hip.Verifier()
    yield v
    v.close()


def same(v, ref, pts, T, max_err, seed):
    """trace, result record and mask of the verifier against the reference, as bytes; returns the reference's output"""
    want = ref.epipolar(pts, T, max_err, seed)
    samples, models, counts = v.epipolar_trace(pts, T, max_err, seed)
    assert samples.shape == (T, 8) and samples.tobytes() == want["samples"].tobytes()
    differ = np.flatnonzero((models.view(np.uint32) != want["models"].view(np.uint32)).any(1))
    assert models.tobytes() == want["models"].tobytes(), (differ[:8], models[differ[:2]], want["models"][differ[:2]])
    assert counts.tobytes() == want["counts"].tobytes(), np.flatnonzero(counts != want["counts"])[:8]
    res, mask = v.epipolar(pts, T, max_err, seed)
    assert res.tobytes() == want["result"].tobytes(), (res, want["result"])
    assert mask.tobytes() == want["mask"].tobytes()
    return want


@pytest.mark.parametrize("n,T,name", CASES)
def test_trace_result_and_mask_equal_the_rule(verifier, ref, n, T, name):
    pts = E.scene(name, n)
    assert pts.shape == (n, 4)
    want = same(verifier, ref, pts, T, 0.5, 1234 + n)
    if name == "two_view" and n >= 63 and T >= 1000:
        assert want["result"]["n_inliers"] == E.two_view(n, 1)[1].sum()      # the scene is found, not only agreed on
    if name == "identical":
        assert want["result"]["hypothesis"] == -1 and want["result"]["n_valid"] == 0


def test_other_options(verifier, ref):
    """other limits, down to one no pair can meet by more than rounding, and seeds at the ends of their range"""
    pts = E.two_view(700, 3)[0]
    for max_err in (3.0, 0.01, 1e-6):
        for seed in (0, 0xffffffff):
            same(verifier, ref, pts, 130, max_err, seed)


def test_largest_hypothesis_count(verifier, ref):
    """T = 65536, the upper end of the range, on few pairs"""
    same(verifier, ref, E.two_view(100, 8)[0], 65536, 0.5, 3)


def test_small_inputs_null_mask_and_errors(gpu_hip, verifier):
    hip, lib = gpu_hip, gpu_hip.lib()
    pts = E.two_view(64)[0]
    for n in range(8):
        res, mask = verifier.epipolar(pts[:n], 16, 0.5, 1)
        assert (res["hypothesis"], res["n_inliers"], res["n_valid"]) == (-1, 0, 0) and not res["H"].any()
        assert len(mask) == n and not mask.any()
        s, mo, c = verifier.epipolar_trace(pts[:n], 16, 0.5, 1)
        assert s.shape == (16, 8) and (s == -1).all() and not mo.any() and (c == -1).all()
    # inlier = NULL: the record alone, equal to the one that comes with a mask
    with_mask, _ = verifier.epipolar(pts, 256, 0.5, 1)
    alone, none = verifier.epipolar(pts, 256, 0.5, 1, want_mask=False)
    assert none is None and alone.tobytes() == with_mask.tobytes() and alone["hypothesis"] >= 0
    # every ERR_INVALID case, on a real verifier
    res = np.zeros(1, hip.RANSAC_RESULT_DTYPE)
    call = lambda v, p, n, o, r: lib.popsift_hip_epipolar(v, p, n, C.byref(o) if o is not None else None, r, None)
    good = hip.epipolar_opts(hypotheses=8, max_err=1.0)
    h = verifier._h
    assert call(h, pts.ctypes.data, 64, good, res.ctypes.data) == hip.OK
    assert call(None, pts.ctypes.data, 64, good, res.ctypes.data) == hip.ERR_INVALID
    assert call(h, pts.ctypes.data, 64, None, res.ctypes.data) == hip.ERR_INVALID
    assert call(h, pts.ctypes.data, 64, good, None) == hip.ERR_INVALID
    assert call(h, None, 64, good, res.ctypes.data) == hip.ERR_INVALID
    assert call(h, pts.ctypes.data, -1, good, res.ctypes.data) == hip.ERR_INVALID
    assert call(h, pts.ctypes.data, (1 << 24) + 1, good, res.ctypes.data) == hip.ERR_INVALID
    for kw in (dict(hypotheses=0), dict(hypotheses=65537), dict(max_err=0.0), dict(max_err=-1.0), dict(max_err=float("nan")),
               dict(max_err=float("inf"))):
        o = hip.epipolar_opts(**{**dict(hypotheses=8, max_err=1.0), **kw})
        assert call(h, pts.ctypes.data, 64, o, res.ctypes.data) == hip.ERR_INVALID, kw
    for k in range(3):
        o = hip.epipolar_opts(hypotheses=8, max_err=1.0)
        o.reserved[k] = 5
        assert call(h, pts.ctypes.data, 64, o, res.ctypes.data) == hip.ERR_INVALID
        assert lib.popsift_hip_epipolar_trace(h, pts.ctypes.data, 64, C.byref(o), None, None, None) == hip.ERR_INVALID
    assert lib.popsift_hip_epipolar_trace(h, pts.ctypes.data, 64, C.byref(good), None, None, None) == hip.OK  # all three NULL
    assert call(h, pts.ctypes.data, 64, good, res.ctypes.data) == hip.OK                                      # and it still works


def test_scratch_shared_with_the_homography(gpu_hip, ref):
    """a sample is 4 ints for popsift_hip_ransac and 8 for popsift_hip_epipolar, in the same grow-only scratch: calls of both
    kinds alternate on one verifier and each returns what a fresh verifier returns"""
    small, big = E.two_view(300, 5)[0], E.two_view(5000, 6)[0]
    raw = lambda out: [x.tobytes() for x in out]
    used = gpu_hip.Verifier()
    h_first = raw(used.ransac(small, "homography", 100, 0.5, 2)) + raw(used.trace(small, "homography", 100, 0.5, 2))
    big_trace = used.epipolar_trace(big, 3000, 0.5, 1)
    h_again = raw(used.ransac(small, "homography", 100, 0.5, 2)) + raw(used.trace(small, "homography", 100, 0.5, 2))
    e_small = raw(used.epipolar(small, 100, 0.5, 2)) + raw(used.epipolar_trace(small, 100, 0.5, 2))
    fresh = gpu_hip.Verifier()
    e_fresh = raw(fresh.epipolar(small, 100, 0.5, 2)) + raw(fresh.epipolar_trace(small, 100, 0.5, 2))
    fresh.close()
    fresh = gpu_hip.Verifier()
    h_fresh = raw(fresh.ransac(small, "homography", 100, 0.5, 2)) + raw(fresh.trace(small, "homography", 100, 0.5, 2))
    assert h_again == h_first == h_fresh
    assert e_small == e_fresh
    want = ref.epipolar(small, 100, 0.5, 2)
    assert e_small == [want["result"].tobytes(), want["mask"].tobytes(), want["samples"].tobytes(), want["models"].tobytes(),
                       want["counts"].tobytes()]
    want = ref.epipolar(big, 3000, 0.5, 1)
    assert raw(big_trace) == [want["samples"].tobytes(), want["models"].tobytes(), want["counts"].tobytes()]
    assert want["result"]["n_inliers"] == E.two_view(5000, 6)[1].sum()
    used.close()
    fresh.close()


SHIFT = (8, 16)   # rows, columns: the rolled pair of tests/test_gpu_ransac.py


def test_a_shifted_image_pair(gpu_hip, verifier):
    """Extract, match with cross-check, gather the points, verify at 0.5 px.  A pure image shift is degenerate for a
    fundamental matrix (every F = [e]x with e on the line at infinity towards the shift, and more, fits), so nothing is
    asserted about F itself: every pair displaced by exactly the roll is an inlier of whatever F wins.  A pair the roll
    wraps around the border may lie on its epipolar line as well; nothing is asserted about those."""
    hip = gpu_hip
    a = synth(95, 96, 72)
    b = np.roll(a, SHIFT, axis=(0, 1))
    A, B = hip.Context().submit(a).clone_results(), hip.Context().submit(b).clone_results()
    pairs = A.match_pairs(B, cross_check=True)
    pts = A.pair_points(B, pairs)
    # displaced by the roll: x and x + 16 round to float32 separately, each within 2^-18 px in a 96 px image
    rolled = (np.abs(pts[:, 2] - pts[:, 0] - SHIFT[1]) < 1e-4) & (np.abs(pts[:, 3] - pts[:, 1] - SHIFT[0]) < 1e-4)
    assert rolled.sum() >= 8 and rolled.sum() > len(pairs) // 2
    res, mask = verifier.epipolar(pts, max_err=0.5, seed=1)
    assert res["hypothesis"] >= 0
    assert mask[rolled].all() and res["n_inliers"] >= rolled.sum() and res["n_inliers"] == mask.sum()
