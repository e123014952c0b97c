"""popsift_hip_ransac_many on the GPU, byte for byte against the CPU restatements of the per-list rules (tests/ransac_ref.c,
tests/epipolar_ref.c) applied list by list: the records, the masks and the full trace; the groups, the per-list GPU calls,
stale scratch, small inputs and every ERR_INVALID case."""
import ctypes as C

import numpy as np
import pytest

import epipolar_rule as E
import ransac_rule as R
from popsift_amd import _capi

pytestmark = pytest.mark.gpu

HOMOGRAPHY, AFFINE, EPIPOLAR = _capi.REFIT_HOMOGRAPHY, _capi.REFIT_AFFINE, _capi.REFIT_EPIPOLAR
KINDS = [HOMOGRAPHY, AFFINE, EPIPOLAR]
SAMPLE = {HOMOGRAPHY: 4, AFFINE: 3, EPIPOLAR: 8}
SEG = _capi.RANSAC_MANY_SEGMENT
assert SEG == 256   # SEG - 1, SEG and SEG + 1 are among the lengths below
# One call per kind holds lists of these lengths in this order: the short ones pack together at unaligned flat offsets,
# 255 / 256 / 257 straddle the scoring kernel's segment, 1023 / 1024 / 1025 the per-list kernel's chunk, 2500 takes ten
# segments.  The scene of each list: "planted" is the kind's scene with a planted model (a homography, an affine map, two
# views of a 3-D scene with 80 % inliers -- with 60 % an 8-pair sample is clean in 1.7 % of draws)
TRANSFER_LISTS = [(0, "planted"), (1, "outliers"), (2, "identical"), (3, "planted"), (4, "planted"), (5, "collinear"),
                  (7, "nan"), (8, "horizon"), (9, "planted"), (63, "planted"), (64, "nan"), (65, "planted"),
                  (255, "collinear"), (256, "planted"), (257, "horizon"), (1000, "planted"), (1023, "identical"),
                  (1024, "planted"), (1025, "nan"), (2500, "planted")]
EPIPOLAR_LISTS = [(0, "planted"), (1, "outliers"), (2, "identical"), (3, "planted"), (4, "translation"), (5, "collinear"),
                  (7, "planted"), (8, "translation"), (9, "nan"), (63, "planted"), (64, "nan"), (65, "planted"),
                  (255, "translation"), (256, "planted"), (257, "planar"), (1000, "planted"), (1023, "identical"),
                  (1024, "planted"), (1025, "collinear"), (2500, "planted")]
assert [n for n, _ in TRANSFER_LISTS] == [n for n, _ in EPIPOLAR_LISTS] == \
    [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024, 1025, 2500]
TS = [1, 63, 64, 65, 257]
MAX_ERR, SEED = 0.5, 20261
EPI_SHARE = 0.8


def scene(kind, name, n):
    """-> (pts (n, 4), planted inlier count or None)"""
    if kind == EPIPOLAR:
        if name == "planted":
            pts, inl, _ = E.two_view(n, 1, EPI_SHARE)
            return pts, int(inl.sum())
        return E.scene(name, n), None
    if name == "planted":
        pts, inl, _ = R.planted(n, 1, kind)
        return pts, int(inl.sum())
    return R.scene(name, n, kind), None


def csr(lists):
    offsets = np.zeros(len(lists) + 1, np.int32)
    offsets[1:] = np.cumsum([len(p) for p in lists])
    flat = np.concatenate([p.reshape(-1, 4) for p in lists]).astype(np.float32) if lists else np.zeros((0, 4), np.float32)
    return flat, offsets


class Rule:
    """the two references behind one call, by kind"""

    def __init__(self, tmp):
        self.r, self.e = R.Ref(tmp), E.Ref(tmp)

    def __call__(self, kind, pts, T, max_err, seed):
        if kind == EPIPOLAR:
            return self.e.epipolar(pts, T, max_err, seed)
        return self.r.ransac(pts, kind, T, max_err, seed)


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    return Rule(tmp_path_factory.mktemp("many_ref"))


@pytest.fixture(scope="module")
def verifier(gpu_hip):
    v = gpu_hip.Verifier()
    yield v
    v.close()


@pytest.fixture(scope="module")
def edge(rule):
    """per kind: the lists, their planted counts, the flat points and offsets, and per T the reference's output per list
    (computed once, shared, never modified)"""
    out = {}
    for kind in KINDS:
        made = [scene(kind, name, n) for n, name in (EPIPOLAR_LISTS if kind == EPIPOLAR else TRANSFER_LISTS)]
        lists, planted = [p for p, _ in made], [c for _, c in made]
        flat, offsets = csr(lists)
        want = {T: [rule(kind, p, T, MAX_ERR, SEED) for p in lists] for T in TS}
        out[kind] = dict(lists=lists, planted=planted, flat=flat, offsets=offsets, want=want)
    return out


def many_bytes(v, flat, offsets, kind, T, max_err=MAX_ERR, seed=SEED):
    """everything one (call, trace) pair returns"""
    res, mask = v.ransac_many(flat, offsets, kind, T, max_err, seed)
    samples, models, counts = v.ransac_many_trace(flat, offsets, kind, T, max_err, seed)
    return res, mask, samples, models, counts


def assert_equal_the_rule(got, offsets, want):
    res, mask, samples, models, counts = got
    assert len(res) == len(want) and len(mask) == offsets[-1]
    for m, w in enumerate(want):
        a, b = offsets[m], offsets[m + 1]
        assert res[m].tobytes() == w["result"].tobytes(), (m, res[m], w["result"])
        assert mask[a:b].tobytes() == w["mask"].tobytes(), (m, np.flatnonzero(mask[a:b] != w["mask"])[:8])
        assert samples[m].tobytes() == w["samples"].tobytes(), m
        assert counts[m].tobytes() == w["counts"].tobytes(), (m, np.flatnonzero(counts[m] != w["counts"])[:8])
        assert models[m].tobytes() == w["models"].tobytes(), m


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("kind", KINDS)
def test_edge_lists_equal_the_rule(verifier, edge, kind, T):
    e = edge[kind]
    assert_equal_the_rule(many_bytes(verifier, e["flat"], e["offsets"], kind, T), e["offsets"], e["want"][T])
    for m, w in enumerate(e["want"][T]):
        n = len(e["lists"][m])
        if n < SAMPLE[kind]:     # the rule for a list shorter than a sample, spelled out
            r = w["result"]
            assert (r["hypothesis"], r["n_inliers"], r["n_valid"]) == (-1, 0, 0) and not r["H"].any() and not w["mask"].any()
            assert (w["samples"] == -1).all() and not w["models"].any() and (w["counts"] == -1).all()
        if T == max(TS) and e["planted"][m] is not None and n >= 63:
            assert w["result"]["n_inliers"] == e["planted"][m], (m, n)      # found, not only agreed on


@pytest.mark.parametrize("kind", KINDS)
def test_groups_do_not_change_the_bytes(gpu_hip, edge, kind):
    e, T = edge[kind], 65
    v = gpu_hip.Verifier()
    default = [x.tobytes() for x in many_bytes(v, e["flat"], e["offsets"], kind, T)]
    # every list a group of its own; a boundary after every third list, the first ones between short lists; fewer
    # records than one list's T (a group is still one whole list); one record
    for records in (T, 3 * T, 3 * T + T // 2, T - 1, 1):
        v.set_group(records)
        assert [x.tobytes() for x in many_bytes(v, e["flat"], e["offsets"], kind, T)] == default, records
    v.set_group(0)
    assert [x.tobytes() for x in many_bytes(v, e["flat"], e["offsets"], kind, T)] == default
    assert gpu_hip.lib().popsift_hip_verifier_debug_set_group(v._h, -1) == gpu_hip.ERR_INVALID
    assert gpu_hip.lib().popsift_hip_verifier_debug_set_group(None, 1) == gpu_hip.ERR_INVALID
    v.close()


@pytest.mark.parametrize("kind", KINDS)
def test_equal_to_the_per_list_gpu_calls(verifier, edge, kind):
    e = edge[kind]
    lists = [e["lists"][i] for i in (11, 14, 19)]       # 65, 257 and 2500 pairs
    flat, offsets = csr(lists)
    res, mask = verifier.ransac_many(flat, offsets, kind, 300, 1.0, 7)
    for m, p in enumerate(lists):
        if kind == EPIPOLAR:
            r, k = verifier.epipolar(p, 300, 1.0, 7)
        else:
            r, k = verifier.ransac(p, kind, 300, 1.0, 7)
        assert res[m].tobytes() == r.tobytes() and mask[offsets[m]:offsets[m + 1]].tobytes() == k.tobytes(), m


def test_free_of_stale_scratch(gpu_hip, edge):
    """a large many-call, a per-list ransac, a refit, a small many-call on one verifier: each the bytes of a fresh one"""
    big, small = edge[EPIPOLAR], edge[HOMOGRAPHY]
    sl, so = csr(small["lists"][2:9])
    one = R.planted(700, 3)[0]
    steps = [lambda v: many_bytes(v, big["flat"], big["offsets"], EPIPOLAR, 257),
             lambda v: v.ransac(one, "homography", 130, 0.5, 1),
             lambda v: v.refit(one, "homography", R.pixel_homography(), 0.5, 3),
             lambda v: many_bytes(v, sl, so, HOMOGRAPHY, 63),
             lambda v: v.ransac_many(sl, so, AFFINE, 1, 0.5, 2)]
    used = gpu_hip.Verifier()
    for k, step in enumerate(steps):
        fresh = gpu_hip.Verifier()
        assert [x.tobytes() for x in step(used)] == [x.tobytes() for x in step(fresh)], k
        fresh.close()
    used.close()


def test_small_inputs_null_mask_and_errors(gpu_hip, verifier, edge):
    hip, lib = gpu_hip, gpu_hip.lib()
    e = edge[HOMOGRAPHY]
    flat, offsets = e["flat"], e["offsets"]
    nl = len(offsets) - 1
    # inlier = NULL: the records alone, equal to those that come with the masks
    with_mask, _ = verifier.ransac_many(flat, offsets, HOMOGRAPHY, 64, 0.5, 1)
    alone, none = verifier.ransac_many(flat, offsets, HOMOGRAPHY, 64, 0.5, 1, want_mask=False)
    assert none is None and alone.tobytes() == with_mask.tobytes() and (alone["hypothesis"] >= 0).any()
    # all lists empty
    for kind in KINDS:
        res, mask = verifier.ransac_many(np.zeros((0, 4), np.float32), np.zeros(6, np.int32), kind, 16, 0.5, 1)
        assert len(res) == 5 and len(mask) == 0 and (res["hypothesis"] == -1).all() and not res["H"].any()
        assert not res["n_inliers"].any() and not res["n_valid"].any() and not res["reserved"].any()
        s, mo, c = verifier.ransac_many_trace(np.zeros((0, 4), np.float32), np.zeros(6, np.int32), kind, 16, 0.5, 1)
        assert s.shape == (5, 16, 8 if kind == EPIPOLAR else 4) and (s == -1).all() and not mo.any() and (c == -1).all()

    res = np.full(nl, 7, hip.RANSAC_RESULT_DTYPE)
    good = hip.ransac_many_opts(hypotheses=8, max_err=1.0)
    h, p, o = verifier._h, flat.ctypes.data, offsets.ctypes.data

    def call(v, pts, off, n_lists, opts, r):
        return lib.popsift_hip_ransac_many(v, pts, off, n_lists, C.byref(opts) if opts is not None else None, r, None)

    # no list: accepted, nothing written
    zero = np.zeros(1, np.int32)
    before = res.tobytes()
    assert call(h, None, zero.ctypes.data, 0, good, res.ctypes.data) == hip.OK and res.tobytes() == before
    assert call(h, None, zero.ctypes.data, 0, good, None) == hip.ERR_INVALID
    assert call(h, p, o, nl, good, res.ctypes.data) == hip.OK
    # every ERR_INVALID case, on a real verifier
    assert call(None, p, o, nl, good, res.ctypes.data) == hip.ERR_INVALID
    assert call(h, p, o, nl, None, res.ctypes.data) == hip.ERR_INVALID
    assert call(h, p, None, nl, good, res.ctypes.data) == hip.ERR_INVALID
    assert call(h, p, o, nl, good, None) == hip.ERR_INVALID
    assert call(h, None, o, nl, good, res.ctypes.data) == hip.ERR_INVALID
    assert call(h, p, o, -1, good, res.ctypes.data) == hip.ERR_INVALID
    assert call(h, p, o, (1 << 20) + 1, good, res.ctypes.data) == hip.ERR_INVALID
    for bad in ([1, 5], [0, 5, 4], [0, -1], [0, (1 << 24) + 1]):
        off = np.array(bad, np.int32)
        assert call(h, p, off.ctypes.data, len(bad) - 1, good, res.ctypes.data) == hip.ERR_INVALID, bad
    for kw in (dict(kind=3), dict(kind=-1), dict(hypotheses=0), dict(hypotheses=65537), dict(max_err=0.0), dict(max_err=-1.0),
               dict(max_err=float("nan")), dict(max_err=float("inf"))):
        opts = hip.ransac_many_opts(**{**dict(hypotheses=8, max_err=1.0), **kw})
        assert call(h, p, o, nl, opts, res.ctypes.data) == hip.ERR_INVALID, kw
    for k in range(4):
        opts = hip.ransac_many_opts(hypotheses=8, max_err=1.0)
        opts.reserved[k] = 1
        assert call(h, p, o, nl, opts, res.ctypes.data) == hip.ERR_INVALID, k
    # the trace does not need res
    s = np.zeros((nl, 8, 4), np.int32)
    assert lib.popsift_hip_ransac_many_trace(h, p, o, nl, C.byref(good), None, None, s.ctypes.data, None, None) == hip.OK
    assert lib.popsift_hip_ransac_many_trace(h, p, None, nl, C.byref(good), None, None, s.ctypes.data, None, None) == hip.ERR_INVALID
