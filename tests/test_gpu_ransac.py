"""popsift_hip_ransac on the GPU, byte for byte against the CPU restatement of its rule (tests/ransac_ref.c): the trace
(samples, models, counts), the result record and the mask, at the sizes where the kernels change behaviour; and
popsift_hip_pair_points against the numpy gather."""
import ctypes as C

import numpy as np
import pytest

import ransac_rule as R
from popsift_amd import _capi
from popsift_amd.synth import synth

pytestmark = pytest.mark.gpu

CHUNK, HYP = _capi.RANSAC_CHUNK, _capi.RANSAC_HYP_BLOCK
# (n, T, scene): the small sizes around a wave and a workgroup, one below / at / one above the scoring kernel's pair chunk,
# three chunks with a partial last one; T around a wave, one above the hypothesis block, several blocks
CASES = [(3, 1, "planted"), (4, 63, "planted"), (5, 64, "outliers"), (63, HYP + 1, "planted"), (64, 257, "nan"),
         (65, 1000, "planted"), (255, 64, "collinear"), (256, HYP + 1, "horizon"), (257, 63, "identical"),
         (1000, 1000, "planted"), (CHUNK - 1, HYP + 1, "planted"), (CHUNK, 64, "outliers"), (CHUNK + 1, 257, "nan"),
         (2 * CHUNK + 452, HYP + 1, "horizon")]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return R.Ref(tmp_path_factory.mktemp("ransac_ref"))


@pytest.fixture(scope="module")
def verifier(gpu_hip):
    v = gpu_hip.Verifier()
    yield v
    v.close()


def same(v, ref, pts, model, T, max_err, seed):
    """trace, result record and mask of the verifier against the reference, as bytes; returns the reference's output"""
    want = ref.ransac(pts, model, T, max_err, seed)
    samples, models, counts = v.trace(pts, model, T, max_err, seed)
    assert samples.tobytes() == want["samples"].tobytes()
    assert counts.tobytes() == want["counts"].tobytes(), np.flatnonzero(counts != want["counts"])[:8]
    assert models.tobytes() == want["models"].tobytes(), np.flatnonzero((models.view(np.uint32) != want["models"].view(np.uint32)).any(1))[:8]
    res, mask = v.ransac(pts, model, T, max_err, seed)
    assert res.tobytes() == want["result"].tobytes(), (res, want["result"])
    assert mask.tobytes() == want["mask"].tobytes()
    return want


@pytest.mark.parametrize("model", [R.HOMOGRAPHY, R.AFFINE])
@pytest.mark.parametrize("n,T,name", CASES)
def test_trace_result_and_mask_equal_the_rule(verifier, ref, n, T, name, model):
    pts = R.scene(name, n, model)
    assert pts.shape == (n, 4)
    want = same(verifier, ref, pts, model, T, 0.5, 1234 + n)
    if name == "planted" and n >= 63 and T >= 64:
        assert want["result"]["n_inliers"] == R.planted(n, 1, model)[1].sum()      # the scene is found, not only agreed on
    if name == "identical":
        assert want["result"]["hypothesis"] == -1 and want["result"]["n_valid"] == 0


def test_other_options(verifier, ref):
    """another max_err and seeds at the ends of their range"""
    pts = R.planted(700, 3)[0]
    for max_err, seed in ((3.0, 0), (0.01, 0xffffffff), (1e-6, 77)):
        same(verifier, ref, pts, R.HOMOGRAPHY, 130, max_err, seed)
        same(verifier, ref, pts, R.AFFINE, 130, max_err, seed)


def test_repeatable_and_free_of_stale_scratch(gpu_hip, ref):
    small, big = R.planted(300, 5)[0], R.planted(5000, 6)[0]
    used = gpu_hip.Verifier()
    big_res = used.ransac(big, "homography", 3000, 0.5, 1)
    used.trace(big, "affine", 3000, 0.5, 1)
    fresh = gpu_hip.Verifier()
    for model in ("homography", "affine"):
        a = [x.tobytes() for x in used.ransac(small, model, 100, 0.5, 2)]
        assert a == [x.tobytes() for x in used.ransac(small, model, 100, 0.5, 2)]
        assert a == [x.tobytes() for x in fresh.ransac(small, model, 100, 0.5, 2)]
        ta = [x.tobytes() for x in used.trace(small, model, 100, 0.5, 2)]
        assert ta == [x.tobytes() for x in fresh.trace(small, model, 100, 0.5, 2)]
    again = used.ransac(big, "homography", 3000, 0.5, 1)
    assert [x.tobytes() for x in again] == [x.tobytes() for x in big_res]
    want = ref.ransac(big, R.HOMOGRAPHY, 3000, 0.5, 1, trace=False)
    assert again[0].tobytes() == want["result"].tobytes() and again[1].tobytes() == want["mask"].tobytes()
    used.close()
    fresh.close()


def test_small_inputs_null_mask_and_errors(gpu_hip, verifier):
    hip, lib = gpu_hip, gpu_hip.lib()
    pts = R.planted(64)[0]
    for model, m in (("homography", 4), ("affine", 3)):
        for n in range(m):
            res, mask = verifier.ransac(pts[:n], model, 16, 0.5, 1)
            assert (res["hypothesis"], res["n_inliers"], res["n_valid"]) == (-1, 0, 0) and not res["H"].any()
            assert len(mask) == n and not mask.any()
            s, mo, c = verifier.trace(pts[:n], model, 16, 0.5, 1)
            assert (s == -1).all() and not mo.any() and (c == -1).all()
    # inlier = NULL: the record alone, equal to the one that comes with a mask
    with_mask, _ = verifier.ransac(pts, "homography", 64, 0.5, 1)
    alone, none = verifier.ransac(pts, "homography", 64, 0.5, 1, want_mask=False)
    assert none is None and alone.tobytes() == with_mask.tobytes() and alone["hypothesis"] >= 0
    # every ERR_INVALID case, on a real verifier
    res = np.zeros(1, hip.RANSAC_RESULT_DTYPE)
    call = lambda v, p, n, o, r: lib.popsift_hip_ransac(v, p, n, C.byref(o) if o is not None else None, r, None)
    good = hip.ransac_opts(hypotheses=8, max_err=1.0)
    h = verifier._h
    assert call(h, pts.ctypes.data, 64, good, res.ctypes.data) == hip.OK
    assert call(None, pts.ctypes.data, 64, good, res.ctypes.data) == hip.ERR_INVALID
    assert call(h, pts.ctypes.data, 64, None, res.ctypes.data) == hip.ERR_INVALID
    assert call(h, pts.ctypes.data, 64, good, None) == hip.ERR_INVALID
    assert call(h, None, 64, good, res.ctypes.data) == hip.ERR_INVALID
    assert call(h, pts.ctypes.data, -1, good, res.ctypes.data) == hip.ERR_INVALID
    assert call(h, pts.ctypes.data, (1 << 24) + 1, good, res.ctypes.data) == hip.ERR_INVALID
    for kw in (dict(model=2), dict(hypotheses=0), dict(hypotheses=65537), dict(max_err=0.0), dict(max_err=float("nan")),
               dict(max_err=float("inf"))):
        o = hip.ransac_opts(**{**dict(hypotheses=8, max_err=1.0), **kw})
        assert call(h, pts.ctypes.data, 64, o, res.ctypes.data) == hip.ERR_INVALID, kw
    o = hip.ransac_opts(hypotheses=8, max_err=1.0)
    o.reserved[1] = 5
    assert call(h, pts.ctypes.data, 64, o, res.ctypes.data) == hip.ERR_INVALID
    with pytest.raises(hip.PopsiftHipError) as e:
        hip.Verifier(device=hip.device_count())
    assert e.value.status == hip.ERR_INVALID


def test_largest_hypothesis_count(verifier, ref):
    """T = 65536, the upper end of the range, on few pairs"""
    same(verifier, ref, R.planted(100, 8)[0], R.AFFINE, 65536, 0.5, 3)


SHIFT = (8, 16)   # rows, columns: a multiple of 8 keeps every octave's sampling grid aligned, so the shift is exact


def test_pair_points_and_a_shifted_image_pair(gpu_hip, verifier):
    hip = gpu_hip
    a = synth(95, 96, 72)
    b = np.roll(a, SHIFT, axis=(0, 1))
    ca, cb = hip.Context().submit(a), hip.Context().submit(b)
    fa, _ = ca.fetch()
    fb, _ = cb.fetch()
    A, B = ca.clone_results(), cb.clone_results()
    pairs = A.match_pairs(B, cross_check=True)
    assert len(pairs) >= 8
    pts = A.pair_points(B, pairs)
    ra, rb = A.download()[1], B.download()[1]
    want = np.stack([fa["xpos"][ra[pairs["l"]]], fa["ypos"][ra[pairs["l"]]],
                     fb["xpos"][rb[pairs["r"]]], fb["ypos"][rb[pairs["r"]]]], 1).astype(np.float32)
    assert pts.dtype == np.float32 and pts.tobytes() == want.tobytes()
    assert A.pair_points(B, pairs[:0]).shape == (0, 4)
    assert A.pair_points(B, pairs[::-1]).tobytes() == want[::-1].tobytes()      # any order, repeats allowed
    # a pair index outside its set; a descriptor without a feature behind it
    for field, value in (("l", A.info()[2]), ("r", B.info()[2]), ("l", -1), ("r", -1)):
        bad = pairs.copy()
        bad[field][len(bad) // 2] = value
        with pytest.raises(hip.PopsiftHipError) as e:
            A.pair_points(B, bad)
        assert e.value.status == hip.ERR_INVALID
    bare = hip.DevFeatures.from_host(B.download()[0])
    with pytest.raises(hip.PopsiftHipError) as e:
        A.pair_points(bare, pairs)
    assert e.value.status == hip.ERR_INVALID
    assert A.pair_points(B, pairs).tobytes() == want.tobytes()                  # and the set still works afterwards
    # The shift comes back as the affine model's translation.  np.roll is a CYCLIC shift: a feature that leaves the image on
    # the right or at the bottom comes back on the other side, a whole image width or height away from where the
    # translation puts it.  Every other cross-checked pair is an inlier at 0.5 px, and none of those.
    res, mask = verifier.ransac(pts, "affine", 256, 0.5, 1)
    Hm = res["H"].reshape(3, 3)
    assert res["hypothesis"] >= 0
    assert abs(Hm[0, 2] - SHIFT[1]) < 0.5 and abs(Hm[1, 2] - SHIFT[0]) < 0.5
    assert np.abs(Hm[:2, :2] - np.eye(2)).max() < 0.02
    wrapped = (pts[:, 0] + SHIFT[1] >= a.shape[1]) | (pts[:, 1] + SHIFT[0] >= a.shape[0])
    assert 0 < wrapped.sum() < len(pairs) // 4
    assert mask[~wrapped].all() and not mask[wrapped].any() and res["n_inliers"] == (~wrapped).sum()
