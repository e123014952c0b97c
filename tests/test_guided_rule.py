"""The guided matcher without a GPU: the CPU rule the GPU tests compare with (tests/guided_ref.c) tied to the references
that exist -- the oracle's matcher for the distances and the rows, the two verifier references for the candidate test --,
proof that the shared scenes exercise what they are meant to, and the argument checks of the C ABI (made before any GPU
call)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import epipolar_rule
import guided_rule as G
import match_pairs_rule
import ransac_rule
from guided_rule import guided_ref  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("nl,nr", [(300, 257), (64, 2)])
def test_with_every_pair_a_candidate_the_rows_are_the_oracles(oracle_mod, guided_ref, nl, nr):
    l, r = match_pairs_rule.planted(nl, nr)
    rng = np.random.default_rng(3)
    lxy, rxy = rng.random((nl, 2)) * 700, rng.random((nr, 2)) * 700
    rows, ncand = guided_ref.rows(G.HOMOGRAPHY, G.IDENTITY, G.ALL_PASS_ERR, l, lxy, r, rxy)
    assert (ncand == nr).all()
    want = oracle_mod.match(l, r)
    assert rows.tobytes() == want.tobytes()
    back, _ = guided_ref.rows(G.HOMOGRAPHY, G.IDENTITY, G.ALL_PASS_ERR, l, lxy, r, rxy, back=True)
    assert back.tobytes() == oracle_mod.match(r, l).tobytes()
    # d is the same bits both ways
    assert guided_ref.dist(l[3], r[1]).tobytes() == guided_ref.dist(r[1], l[3]).tobytes() == \
        oracle_mod.match(l[3:4], r[1:2])["dist_best"].tobytes()
    for o in match_pairs_rule.OPTION_SETS:
        got = guided_ref.pairs(rows, back, **o)
        assert got.tobytes() == match_pairs_rule.expected_pairs(want, back, **o).tobytes(), o


@pytest.mark.parametrize("model", [ransac_rule.HOMOGRAPHY, ransac_rule.AFFINE])
def test_the_candidate_test_is_the_ransac_references_mask(guided_ref, tmp_path, model):
    rr = ransac_rule.Ref(tmp_path)
    for pts in (ransac_rule.planted(500, 1, model)[0], ransac_rule.with_nan(400, 4, model), ransac_rule.horizon(400)):
        for max_err in (0.5, 2.0):
            out = rr.ransac(pts, model, 300, max_err, 5, trace=False)
            assert out["result"]["hypothesis"] >= 0 and 0 < out["mask"].sum() < len(pts)
            mask = guided_ref.ok_pairs(G.HOMOGRAPHY, out["result"]["H"], max_err, pts)
            assert mask.tobytes() == out["mask"].tobytes()


def test_the_candidate_test_is_the_epipolar_references_mask(guided_ref, tmp_path):
    er = epipolar_rule.Ref(tmp_path)
    for pts in (epipolar_rule.two_view(500, 1)[0], epipolar_rule.with_nan(400), epipolar_rule.translation(300)):
        for max_err in (0.5, 2.0):
            out = er.epipolar(pts, 400, max_err, 5, trace=False)
            assert out["result"]["hypothesis"] >= 0 and out["mask"].sum() > 8
            mask = guided_ref.ok_pairs(G.EPIPOLAR, out["result"]["H"], max_err, pts)
            assert mask.tobytes() == out["mask"].tobytes()
    # an all-zero model (a verifier without a winner) makes nobody a candidate
    assert guided_ref.ok_pairs(G.EPIPOLAR, np.zeros(9), 2.0, epipolar_rule.two_view(50, 1)[0]).sum() == 0


@pytest.mark.parametrize("nl,nr", [(64, 64), (65, 257), (200, 1000), (1000, 1000)])
def test_the_shared_scene_has_empty_single_and_crowded_rows(guided_ref, nl, nr):
    s, Hm = G.scene(nl, nr)
    e = G.Expected(guided_ref, G.HOMOGRAPHY, Hm, 2.0, s)
    shares = [(e.ncand == 0).mean(), (e.ncand == 1).mean(), (e.ncand >= 2).mean()]
    assert min(shares) >= 0.15, shares
    # the planted point pairs carry near-copy descriptors: most rows with a candidate are accepted pairs
    assert len(e.pairs()) >= 0.5 * (e.ncand >= 1).sum()
    # a tight and a wide band change the candidate sets
    tight = G.Expected(guided_ref, G.HOMOGRAPHY, Hm, 0.5, s).ncand
    wide = G.Expected(guided_ref, G.HOMOGRAPHY, Hm, 50.0, s).ncand
    assert (tight <= e.ncand).all() and (e.ncand <= wide).all() and tight.sum() < e.ncand.sum() < wide.sum()
    assert wide.max() >= 5
    # the epipolar band of the same points is not empty either
    assert G.Expected(guided_ref, G.EPIPOLAR, G.scene_F(), 2.0, s).ncand.sum() > nl // 4


def test_the_rule_is_not_match_then_filter(oracle_mod, guided_ref):
    s, M, max_err = G.planted_cases()
    e = G.Expected(guided_ref, G.HOMOGRAPHY, M, max_err, s)
    U, UB = oracle_mod.match(s["l"], s["r"]), oracle_mod.match(s["r"], s["l"])
    ok = lambda i, j: guided_ref.ok(G.HOMOGRAPHY, M, max_err, *s["lxy"][i], *s["rxy"][j])
    # the unguided best fails the geometry, the guided row still has a best
    rescued = [i for i in range(len(U)) if not ok(i, U["best"][i]) and e.F["best"][i] >= 0]
    assert len(rescued) >= 5 and set(range(6)) <= set(rescued)
    assert [e.F["best"][i] for i in range(6)] == [110 + i for i in range(6)]
    # duplicates that tie: the lower index is no candidate, the higher one wins
    assert s["r"][20].tobytes() == s["r"][40].tobytes() and U["best"][10] == 20 and U["second"][10] == 40
    assert not ok(10, 20) and ok(10, 40) and e.F["best"][10] == 40 and e.F["dist_best"][10] == U["dist_best"][10]
    # the cross-check removes (12, 50) because the search the other way round has two candidates, and nothing else does
    assert e.F["best"][12] == 50 and e.F["best"][13] == 50 and e.ncand[12] == 1 and e.B["best"][50] == 13 and e.B["second"][50] == 12
    for o in match_pairs_rule.OPTION_SETS:
        p = e.pairs(**o)
        if o.get("max_dist2") is None:                   # (12, 50) are unrelated descriptors: the cap would remove them too
            assert (12 in p["l"]) == (not o.get("cross_check")), o
        assert 13 in p["l"] or o.get("max_dist2") is not None
    # ... and keeps (15, 60), which the unguided reverse search would drop: its nearest left descriptor is no candidate
    assert UB["best"][60] == 16 and not ok(16, 60) and e.B["best"][60] == 15
    assert 15 in e.pairs(ratio=0.0, cross_check=True)["l"]
    unguided = match_pairs_rule.expected_pairs(U, UB, ratio=0.0, cross_check=True)
    assert 15 not in unguided["l"]
    # filtering the unguided pairs afterwards finds fewer than the guided search
    filtered = [p for p in match_pairs_rule.expected_pairs(U, UB, ratio=0.0) if ok(p["l"], p["r"])]
    assert len(filtered) < len(e.pairs(ratio=0.0))


def test_empty_and_single_candidate_rows(guided_ref):
    s, M, max_err = G.planted_cases()
    e = G.Expected(guided_ref, G.HOMOGRAPHY, M, max_err, s)
    empty = np.flatnonzero(e.ncand == 0)
    assert len(empty) > 40
    row = e.F[empty[0]]
    assert (row["best"], row["second"], row["accept"]) == (-1, -1, 0) and np.isposinf(row["dist_best"]) and np.isposinf(row["dist_second"])
    one = e.F[12]
    assert (one["second"], one["accept"]) == (-1, 1) and np.isposinf(one["dist_second"]) and np.isfinite(one["dist_best"])
    # with the ratio test off an empty row passes conditions 2 and 3: condition 1, best >= 0, keeps it out
    assert not np.isin(empty, e.pairs(ratio=0.0)["l"]).any()


def test_struct_layout_and_defaults(hip, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "popsift_hip.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu %d %d %d\n", sizeof(popsift_hip_guided_opts), offsetof(popsift_hip_guided_opts, M),
           offsetof(popsift_hip_guided_opts, max_err), offsetof(popsift_hip_guided_opts, cross_check),
           offsetof(popsift_hip_guided_opts, reserved), POPSIFT_HIP_GUIDED_ROWS, POPSIFT_HIP_GUIDED_STEP,
           POPSIFT_HIP_GUIDED_QUEUE);
    return 0;
}
""")
    exe = str(tmp_path / "layout.bin")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = list(map(int, subprocess.check_output([exe], text=True).split()))
    assert got == [C.sizeof(hip.GuidedOpts), hip.GuidedOpts.M.offset, hip.GuidedOpts.max_err.offset,
                   hip.GuidedOpts.cross_check.offset, hip.GuidedOpts.reserved.offset, hip.GUIDED_ROWS, hip.GUIDED_STEP,
                   hip.GUIDED_QUEUE]
    assert got[:5] == [64, 4, 40, 52, 56]
    o = hip.GuidedOpts()
    C.memset(C.byref(o), 0x55, C.sizeof(o))
    hip.lib().popsift_hip_default_guided_opts(C.byref(o))
    assert (o.model, list(o.M), o.max_err, o.ratio, o.max_dist2, o.cross_check, list(o.reserved)) == \
        (hip.GUIDE_HOMOGRAPHY, [1, 0, 0, 0, 1, 0, 0, 0, 1], 2.0, np.float32(0.8), np.inf, 0, [0, 0])
    hip.lib().popsift_hip_default_guided_opts(None)                # tolerated
    assert hip.MATCH_DTYPE == G.MATCH_DTYPE


def test_invalid_arguments_are_rejected_without_a_gpu(hip):
    """Every ERR_INVALID case of the header's three calls.  The arguments are checked before a set is looked at, so two
    blocks of zeros stand in for sets (as sets they would be empty: nothing reaches a GPU even where a check is missing)."""
    lib = hip.lib()
    l, r = C.create_string_buffer(512), C.create_string_buffer(512)
    pairs, rows = np.zeros(4, hip.PAIR_DTYPE), np.zeros(4, hip.MATCH_DTYPE)
    n = C.c_int(-1)
    nan, inf = float("nan"), float("inf")

    def call_pairs(o, l=l, r=r, pairs=pairs.ctypes.data, cap=4, n_pairs=C.byref(n)):
        return lib.popsift_hip_match_pairs_guided(l, r, C.byref(o) if o is not None else None, pairs, cap, n_pairs)

    def call_rows(o, l=l, r=r, out=rows.ctypes.data):
        return lib.popsift_hip_match_guided(l, r, C.byref(o) if o is not None else None, out)

    def opts(M=None, **kw):
        o = hip.guided_opts(M=M)
        for k, v in kw.items():
            if k == "reserved":
                o.reserved[v] = 1
            else:
                setattr(o, k, v)
        return o

    for call in (call_pairs, call_rows):
        assert call(opts(), l=None) == hip.ERR_INVALID
        assert call(opts(), r=None) == hip.ERR_INVALID
        assert call(None) == hip.ERR_INVALID
        bad_M = [np.where(np.arange(9) == k, v, np.eye(3).reshape(9)) for k in (0, 4, 8) for v in (nan, inf, -inf)]
        for kw in [dict(model=2), dict(model=-1), dict(max_err=0.0), dict(max_err=-1.0), dict(max_err=nan), dict(max_err=inf),
                   dict(ratio=-0.1), dict(ratio=nan), dict(ratio=inf), dict(max_dist2=nan), dict(cross_check=2),
                   dict(cross_check=-1), dict(reserved=0), dict(reserved=1)] + [dict(M=m) for m in bad_M]:
            assert call(opts(**kw)) == hip.ERR_INVALID, kw
    assert call_pairs(opts(), n_pairs=None) == hip.ERR_INVALID
    assert call_pairs(opts(), pairs=None) == hip.ERR_INVALID       # cap > 0 without a buffer
    assert call_rows(opts(), out=None) == hip.ERR_INVALID
    assert n.value == -1                                            # a rejected call writes nothing
    # accepted: the edges of the ranges, both models; empty sets give 0 pairs
    for kw in (dict(), dict(model=hip.GUIDE_EPIPOLAR), dict(ratio=0.0), dict(max_dist2=0.0), dict(max_dist2=-1.0),
               dict(cross_check=1), dict(max_err=1e-30), dict(max_err=3e38), dict(M=np.zeros(9)), dict(ratio=1e30, max_dist2=inf)):
        n.value = -1
        assert call_pairs(opts(**kw)) == hip.OK and n.value == 0, kw
        assert call_rows(opts(**kw)) == hip.OK, kw
    n.value = -1
    assert call_pairs(opts(), pairs=None, cap=0) == hip.OK and n.value == 0
    # the points constructor: argument errors come before the device is looked for
    h = C.c_void_p()
    xy, desc = np.zeros((2, 2), np.float32), np.zeros((2, 128), np.float32)
    f = lib.popsift_hip_devfeatures_from_host_points
    assert f(0, desc.ctypes.data, xy.ctypes.data, 2, None) == hip.ERR_INVALID
    assert f(0, desc.ctypes.data, xy.ctypes.data, -1, C.byref(h)) == hip.ERR_INVALID
    assert f(0, None, xy.ctypes.data, 2, C.byref(h)) == hip.ERR_INVALID
    assert f(0, desc.ctypes.data, None, 2, C.byref(h)) == hip.ERR_INVALID
    assert h.value is None
    if hip.device_count() == 0:
        assert f(0, desc.ctypes.data, xy.ctypes.data, 2, C.byref(h)) == hip.ERR_NO_DEVICE


def test_the_reference_is_clean_under_the_sanitizers(tmp_path):
    """tests/san/guided_san_main.c: a stand-alone program around guided_ref.c, built with and without
    -fsanitize=address,undefined; a report ends it (-fno-sanitize-recover), and both builds print the same checksum."""
    src = os.path.join(ROOT, "tests", "san", "guided_san_main.c")
    out = []
    for name, flags in (("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), ("plain", ["-O2"])):
        exe = str(tmp_path / ("guided_" + name))
        subprocess.check_call(["gcc", "-ffp-contract=off", *flags, src, "-o", exe, "-lm"])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("guided_san ok: "), r.stdout + r.stderr
        out.append(r.stdout)
    assert out[0] == out[1]
