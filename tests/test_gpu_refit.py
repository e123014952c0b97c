"""popsift_hip_refit on the GPU, byte for byte against the CPU restatement of its rule (tests/refit_ref.c): the trace (sums,
candidates, counts, accepted flags), the result record and the mask, for the three kinds of model at the sizes where the
kernels change behaviour; the scratch it shares with popsift_hip_ransac and popsift_hip_epipolar; and every refusal."""
import ctypes as C

import numpy as np
import pytest

import epipolar_rule as E
import ransac_rule as R
import refit_rule as F
from popsift_amd import _capi

pytestmark = pytest.mark.gpu

CHUNK = _capi.REFIT_CHUNK
SCENES = {F.HOMOGRAPHY: ["noisy", "exact", "nan", "horizon", "collinear", "identical", "rough"],
          F.AFFINE: ["noisy", "exact", "nan", "horizon", "collinear", "identical", "rough"],
          F.EPIPOLAR: ["noisy", "exact", "nan", "translation", "planar", "collinear", "identical", "rough"]}


def sizes(kind):
    """exactly a sample and one more; around a wave, a workgroup's lanes and the accumulating kernel's chunk; chunks with a
    partial last one; 69 chunks: the solving kernel's tree over the chunk sums crosses a wave; 258 chunks: more than one
    chunk sum per lane, the tree's levels below the lanes run through memory"""
    m = F.SAMPLE_SIZE[kind]
    return [m, m + 1, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 452, 5 * CHUNK + 1, 70001,
            257 * CHUNK + 1000]


CASES = [(kind, n, SCENES[kind][i % len(SCENES[kind])], (1, 4, 16)[i % 3])
         for kind in F.KINDS for i, n in enumerate(sizes(kind))]
# every scene of every kind once at a size where the scene is what it says, and the larger sizes on noise as well
CASES += [(kind, 1000, name, 4) for kind in F.KINDS for name in SCENES[kind]]
CASES += [(kind, 70001, "rough", 16) for kind in F.KINDS] + [(F.HOMOGRAPHY, 513 * CHUNK + 7, "noisy", 2)]


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp("refit_ref")
    return F.Ref(d), R.Ref(d), E.Ref(d)


@pytest.fixture(scope="module")
def verifier(gpu_hip):
    v = gpu_hip.Verifier()
    yield v
    v.close()


def raw(out):
    return [np.asarray(x).tobytes() for x in out]


def same(v, ref, pts, kind, M, max_err, rounds):
    """trace, result record and mask of the verifier against the reference, as bytes; returns the reference's output"""
    want = ref.refit(pts, kind, M, max_err, rounds)
    res, mask, sums, models, counts, accepted = v.refit_trace(pts, kind, M, max_err, rounds)
    assert counts.tobytes() == want["counts"].tobytes(), (counts, want["counts"])
    differ = np.argwhere(sums.view(np.uint64) != want["sums"].view(np.uint64))
    assert sums.tobytes() == want["sums"].tobytes(), (differ[:8], [(sums[tuple(i)], want["sums"][tuple(i)]) for i in differ[:4]])
    assert models.tobytes() == want["models"].tobytes(), (models, want["models"])
    assert accepted.tobytes() == want["accepted"].tobytes(), (accepted, want["accepted"])
    assert res.tobytes() == want["result"].tobytes(), (res, want["result"])
    assert mask.tobytes() == want["mask"].tobytes()
    plain, plain_mask = v.refit(pts, kind, M, max_err, rounds)
    assert plain.tobytes() == res.tobytes() and plain_mask.tobytes() == mask.tobytes()
    return want


@pytest.mark.parametrize("kind,n,name,rounds", CASES)
def test_trace_result_and_mask_equal_the_rule(verifier, refs, kind, n, name, rounds):
    ref, rr, er = refs
    pts, M = F.start_model(name, n, kind, rr, er, 2.0)
    assert pts.shape == (n, 4)
    want = same(verifier, ref, pts, kind, M, 2.0, rounds)["result"]
    assert want["n_inliers"] >= want["n_start"]
    if name == "noisy" and n >= 1000:                  # the scene is refitted, not only agreed on
        assert want["rounds"] >= 1 and want["n_inliers"] >= 0.55 * n
    if name == "rough" and n >= 1000:                  # and more than one round is accepted
        assert want["rounds"] >= 2
    if name == "identical" and kind != F.EPIPOLAR:
        assert want["stop"] == F.NO_FIT and want["n_start"] == n


@pytest.mark.parametrize("kind", F.KINDS)
def test_sparse_chunks(verifier, refs, kind):
    """three chunks: the second adds nothing but +0.0, the third two terms at its two ends"""
    ref = refs[0]
    pts, inl, _ = F.sparse_chunks(kind)
    want = same(verifier, ref, pts, kind, F.planted_model("noisy", len(pts), kind), 2.0, 4)
    assert want["mask"].tobytes() == inl.tobytes() and want["result"]["rounds"] >= 1
    assert not want["mask"][CHUNK:2 * CHUNK].any() and list(np.flatnonzero(want["mask"][2 * CHUNK:])) == [0, CHUNK - 1]


def test_other_limits(verifier, refs):
    """limits from generous down to one hardly a pair can meet"""
    ref, rr, er = refs
    for kind in F.KINDS:
        pts, M = F.start_model("noisy", 700, kind, rr, er, 2.0)
        for max_err in (5.0, 0.5, 0.05, 1e-6):
            same(verifier, ref, pts, kind, M, max_err, 3)


def test_repeat_and_shared_scratch(gpu_hip, refs):
    """the same call twice and on a fresh verifier; ransac -> refit -> epipolar -> refit on one verifier against fresh ones"""
    ref, rr, er = refs
    small, big = F.noisy_planted(300, 5)[0], F.noisy_two_view(5000, 6)[0]
    used = gpu_hip.Verifier()
    h = used.ransac(small, "homography", 100, 2.0, 2)
    h_fit = raw(used.refit_trace(small, "homography", h[0]["H"], 2.0, 4))
    assert raw(used.refit_trace(small, "homography", h[0]["H"], 2.0, 4)) == h_fit
    e = used.epipolar(big, 3000, 2.0, 1)
    e_fit = raw(used.refit_trace(big, "epipolar", e[0]["H"], 2.0, 16))
    h_again = used.ransac(small, "homography", 100, 2.0, 2)
    e_small = raw(used.epipolar(small, 100, 2.0, 2))
    a_fit = raw(used.refit_trace(small, "affine", h[0]["H"], 2.0, 2))
    assert raw(used.refit_trace(small, "homography", h[0]["H"], 2.0, 4)) == h_fit
    used.close()

    def fresh(call):
        v = gpu_hip.Verifier()
        out = raw(call(v))
        v.close()
        return out
    assert raw(h) == raw(h_again) == fresh(lambda v: v.ransac(small, "homography", 100, 2.0, 2))
    assert raw(e) == fresh(lambda v: v.epipolar(big, 3000, 2.0, 1))
    assert e_small == fresh(lambda v: v.epipolar(small, 100, 2.0, 2))
    assert h_fit == fresh(lambda v: v.refit_trace(small, "homography", h[0]["H"], 2.0, 4))
    assert e_fit == fresh(lambda v: v.refit_trace(big, "epipolar", e[0]["H"], 2.0, 16))
    assert a_fit == fresh(lambda v: v.refit_trace(small, "affine", h[0]["H"], 2.0, 2))
    want = ref.refit(big, F.EPIPOLAR, e[0]["H"], 2.0, 16)
    assert e_fit == raw([want[k] for k in ("result", "mask", "sums", "models", "counts", "accepted")])
    assert h[0].tobytes() == rr.ransac(small, R.HOMOGRAPHY, 100, 2.0, 2)["result"].tobytes()
    assert e[0].tobytes() == er.epipolar(big, 3000, 2.0, 1, trace=False)["result"].tobytes()


def test_small_inputs_null_mask_and_errors(gpu_hip, verifier):
    hip, lib = gpu_hip, gpu_hip.lib()
    pts = F.noisy_planted(64)[0]
    M = F.planted_model("noisy", 64, F.HOMOGRAPHY)
    for kind in F.KINDS:
        for n in range(F.SAMPLE_SIZE[kind]):      # answered on the host
            res, mask, sums, models, counts, accepted = verifier.refit_trace(pts[:n], kind, M, 2.0, 3)
            assert (res["n_inliers"], res["n_start"], res["rounds"], res["stop"]) == (0, 0, 0, F.NO_SUPPORT)
            assert res["M"].tobytes() == M.tobytes() and len(mask) == n and not mask.any()
            assert not sums.any() and not models.any() and (counts == -1).all() and not accepted.any()
    # inlier = NULL: the record alone, equal to the one that comes with a mask
    with_mask, _ = verifier.refit(pts, "homography", M, 2.0, 4)
    alone, none = verifier.refit(pts, "homography", M, 2.0, 4, want_mask=False)
    assert none is None and alone.tobytes() == with_mask.tobytes() and alone["n_inliers"] > 30
    # every ERR_INVALID case, on a real verifier
    res = np.zeros(1, hip.REFIT_RESULT_DTYPE)
    call = lambda v, p, n, o, r: lib.popsift_hip_refit(v, p, n, C.byref(o) if o is not None else None, r, None)
    good = hip.refit_opts("homography", M, 2.0, 4)
    h = verifier._h
    assert call(h, pts.ctypes.data, 64, good, res.ctypes.data) == hip.OK
    assert call(None, pts.ctypes.data, 64, good, res.ctypes.data) == hip.ERR_INVALID
    assert call(h, pts.ctypes.data, 64, None, res.ctypes.data) == hip.ERR_INVALID
    assert call(h, pts.ctypes.data, 64, good, None) == hip.ERR_INVALID
    assert call(h, None, 64, good, res.ctypes.data) == hip.ERR_INVALID
    assert call(h, pts.ctypes.data, -1, good, res.ctypes.data) == hip.ERR_INVALID
    assert call(h, pts.ctypes.data, (1 << 24) + 1, good, res.ctypes.data) == hip.ERR_INVALID
    for kw in (dict(model=-1), dict(model=3), dict(rounds=0), dict(rounds=17), dict(max_err=0.0), dict(max_err=-1.0),
               dict(max_err=float("nan")), dict(max_err=float("inf"))):
        o = hip.refit_opts(**{**dict(model="homography", M=M, max_err=2.0, rounds=4), **kw})
        assert call(h, pts.ctypes.data, 64, o, res.ctypes.data) == hip.ERR_INVALID, kw
    for k in range(9):
        for bad in (float("nan"), float("inf"), -float("inf")):
            o = hip.refit_opts("homography", M, 2.0, 4)
            o.M[k] = bad
            assert call(h, pts.ctypes.data, 64, o, res.ctypes.data) == hip.ERR_INVALID, (k, bad)
    for k in range(4):
        o = hip.refit_opts("homography", M, 2.0, 4)
        o.reserved[k] = 5
        assert call(h, pts.ctypes.data, 64, o, res.ctypes.data) == hip.ERR_INVALID
        assert lib.popsift_hip_refit_trace(h, pts.ctypes.data, 64, C.byref(o), res.ctypes.data, None, None, None, None,
                                           None) == hip.ERR_INVALID
    assert lib.popsift_hip_refit_trace(h, pts.ctypes.data, 64, C.byref(good), res.ctypes.data, None, None, None, None,
                                       None) == hip.OK                       # all four NULL
    assert call(h, pts.ctypes.data, 64, good, res.ctypes.data) == hip.OK   # and it still works
    assert res[0].tobytes() == with_mask.tobytes()


def test_defaults(gpu_hip):
    o = gpu_hip.refit_opts()
    assert (o.model, o.rounds, o.max_err, list(o.M), list(o.reserved)) == (0, 4, 2.0, [1, 0, 0, 0, 1, 0, 0, 0, 1], [0] * 4)
    assert (gpu_hip.REFIT_CHUNK, gpu_hip.REFIT_MAX_ROUNDS, gpu_hip.REFIT_SLOTS) == (1024, 16, 45)
