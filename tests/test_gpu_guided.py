"""popsift_hip_match_guided / popsift_hip_match_pairs_guided on the GPU against the CPU rule (tests/guided_ref.c through
tests/guided_rule.py), byte for byte: every size at which the kernel takes another path (its rows per workgroup, positions
per step and queue entries, include/popsift_hip.h), both models, tight and wide bands, the option sets of the pair rule."""
import ctypes as C
import functools

import numpy as np
import pytest

import guided_rule as G
import ransac_rule
from guided_rule import guided_ref  # noqa: F401  (fixture)
from match_pairs_rule import OPTION_SETS
from popsift_amd.synth import synth

pytestmark = pytest.mark.gpu

MODELS = {"homography": G.HOMOGRAPHY, "epipolar": G.EPIPOLAR}


@functools.lru_cache(maxsize=None)
def shared_scene(nl, nr):
    return G.scene(nl, nr)


def upload(hip, s):
    return hip.DevFeatures.from_host_points(s["l"], s["lxy"]), hip.DevFeatures.from_host_points(s["r"], s["rxy"])


def check(hip, ref, s, model, M, max_err, option_sets=OPTION_SETS, sets=None):
    """rows and pairs of the scene against the rule; -> the rule's answers"""
    L, R = sets or upload(hip, s)
    e = G.Expected(ref, MODELS[model], M, max_err, s)
    rows = L.match_guided(R, model, M, max_err)
    bad = np.flatnonzero(rows != e.F)
    assert rows.tobytes() == e.F.tobytes(), (model, max_err, len(s["l"]), len(s["r"]), bad[:5], rows[bad[:3]], e.F[bad[:3]])
    for o in option_sets:
        got = L.match_pairs_guided(R, model, M, max_err, **o)
        want = e.pairs(**o)
        assert got.tobytes() == want.tobytes(), (model, max_err, len(s["l"]), len(s["r"]), o, len(got), len(want))
    return e


def sizes(hip):
    """1, K - 1, K, K + 1, 2K + 1 rows against as many positions for the kernel's stated sizes, the queue's among the
    positions, and the two larger scenes"""
    edge = lambda k: [1, k - 1, k, k + 1, 2 * k + 1]
    out = [(nl, nr) for nl in edge(hip.GUIDED_ROWS) for nr in edge(hip.GUIDED_STEP)]
    out += [(nl, nr) for nl in (1, hip.GUIDED_ROWS + 1) for nr in edge(hip.GUIDED_QUEUE)[1:]]
    return out + [(200, 1000), (1000, 1000)]


@pytest.mark.parametrize("max_err", [0.5, 2.0, 50.0])
@pytest.mark.parametrize("model", ["homography", "epipolar"])
def test_rows_and_pairs_equal_the_rule(gpu_hip, guided_ref, model, max_err):
    seen = 0
    for nl, nr in sizes(gpu_hip):
        s, Hm = shared_scene(nl, nr)
        # the edge sizes with the first and the last option set, the two larger scenes with all five
        big = nl >= 200
        e = check(gpu_hip, guided_ref, s, model, Hm if model == "homography" else G.scene_F(), max_err,
                  OPTION_SETS if big else (OPTION_SETS[0], OPTION_SETS[-1]))
        seen += int((e.ncand >= 2).sum())
        if big and model == "epipolar":                  # a camera moved sideways: F22 = 0, the band runs along (10, 5)
            check(gpu_hip, guided_ref, s, model, G.translation_F(10, 5), max_err)
    assert seen > (100 if max_err >= 2 else 10), seen      # rows with two or more candidates, over all sizes


@pytest.mark.parametrize("nl,nr", [(300, 257), (64, 2), (129, 513)])
def test_with_every_pair_a_candidate_the_rows_are_the_matchers(gpu_hip, nl, nr):
    hip = gpu_hip
    s, _ = shared_scene(nl, nr)
    L, R = upload(hip, s)
    hip.lib().popsift_hip_match_set_path(hip.MATCH_EXACT)
    try:
        want = L.match(R)
        assert L.match_guided(R, "homography", G.IDENTITY, G.ALL_PASS_ERR).tobytes() == want.tobytes()
        for o in OPTION_SETS:
            got = L.match_pairs_guided(R, "homography", G.IDENTITY, G.ALL_PASS_ERR, **o)
            assert got.tobytes() == L.match_pairs(R, **o).tobytes(), o
    finally:
        hip.lib().popsift_hip_match_set_path(hip.MATCH_AUTO)
    # a set with positions serves the other calls like any other
    pairs = L.match_pairs(R, ratio=0.0)
    pts = L.pair_points(R, pairs)
    assert pts.tobytes() == np.c_[s["lxy"][pairs["l"]], s["rxy"][pairs["r"]]].astype(np.float32).tobytes()
    assert L.info() == (0, nl, nl) and np.array_equal(L.download()[1], np.arange(nl))
    assert L.download()[0].tobytes() == s["l"].tobytes()


def test_the_threshold_is_closed_and_the_horizon_is_respected(gpu_hip, guided_ref):
    hip = gpu_hip
    rng = np.random.default_rng(11)
    # integer positions under a pure translation: a right point 3 px and 4 px off its image has e = 25 exactly
    n = 70
    lxy = np.c_[20.0 + 10.0 * np.arange(n), 300.0 - 3.0 * np.arange(n)].astype(np.float32)
    rxy = (lxy + [7.0, -2.0] + [3.0, 4.0]).astype(np.float32)
    s = dict(l=rng.random((n, 128), np.float32), lxy=lxy, r=rng.random((n, 128), np.float32), rxy=rxy)
    M = G.translation_H(7, -2)
    at = check(hip, guided_ref, s, "homography", M, 5.0)
    assert (at.ncand == 1).all() and np.array_equal(at.F["best"], np.arange(n))
    below = check(hip, guided_ref, s, "homography", M, np.nextafter(np.float32(5), np.float32(0)))
    assert (below.ncand == 0).all() and (below.F["best"] == -1).all() and len(below.pairs(ratio=0.0)) == 0
    # a homography whose horizon (x = 300) runs through the image: the points beyond it have w < 0 and no candidates,
    # although their images are exactly where the right points are
    Hm = np.array([[1.0, 0.02, 3.0], [0.01, 1.0, -2.0], [-1.0 / 300.0, 0.0, 1.0]])
    left = (rng.random((200, 2)) * [G.W - 1, G.H - 1]).astype(np.float32)
    left = left[np.abs(left[:, 0] - 300.0) > 30.0]
    s = dict(l=rng.random((len(left), 128), np.float32), lxy=left, r=rng.random((len(left), 128), np.float32),
             rxy=ransac_rule.project(Hm, left).astype(np.float32))
    e = check(hip, guided_ref, s, "homography", Hm.astype(np.float32), 2.0)
    near, beyond = left[:, 0] < 300.0, left[:, 0] > 300.0
    assert near.sum() > 30 and beyond.sum() > 30
    assert (e.ncand[near] >= 1).all() and (e.ncand[beyond] == 0).all() and (e.F["best"][beyond] == -1).all()


@pytest.mark.parametrize("model", ["homography", "epipolar"])
def test_points_and_descriptors_that_are_not_numbers(gpu_hip, guided_ref, model):
    s, Hm = shared_scene(65, 257)
    s = {k: v.copy() for k, v in s.items()}
    M = Hm if model == "homography" else G.scene_F()
    clean = G.Expected(guided_ref, MODELS[model], M, 2.0, s)
    rows = np.flatnonzero(clean.ncand >= 1)
    cols = np.unique(clean.F["best"][rows])
    assert len(rows) >= 8 and len(cols) >= 8
    nan, inf = np.float32("nan"), np.float32("inf")
    lbad, rbad = rows[:4], cols[:4]
    s["lxy"][lbad[0]] = [nan, 5.0]
    s["lxy"][lbad[1], 1] = inf
    s["lxy"][lbad[2], 0] = -inf
    s["lxy"][lbad[3]] = [nan, nan]
    s["rxy"][rbad[0], 1] = nan
    s["rxy"][rbad[1], 0] = inf
    s["rxy"][rbad[2]] = [-inf, inf]
    s["rxy"][rbad[3], 0] = nan
    s["lxy"][rows[4]] = [np.float32(-0.0), np.float32(-0.0)]               # -0.0: an ordinary number, the origin
    s["rxy"][cols[4]] = ransac_rule.project(Hm, [[0.0, 0.0]])[0]
    s["rxy"][cols[7], 0] = np.float32(-0.0)
    s["l"][rows[5], 17] = nan                       # every distance of this row is NaN: candidates, but an empty row
    s["r"][cols[5], 99] = nan                       # a candidate that can never win
    s["r"][cols[6], 3] = inf                        # a distance of +inf: no candidate either
    e = check(gpu_hip, guided_ref, s, model, M, 2.0)
    # a NaN fails every comparison.  An infinite LEFT coordinate under a projective H makes w and lim infinite, and
    # e <= lim can then hold (the header says so): those two rows are held to the rule's bytes only
    sure = lbad[[0, 3]] if model == "homography" else lbad
    assert (e.ncand[sure] == 0).all() and (e.F["best"][sure] == -1).all()
    assert not np.isin(e.F["best"], rbad).any() and not np.isin(e.F["second"], rbad).any() and (e.B["best"][rbad] == -1).all()
    assert model != "homography" or e.ncand[rows[4]] >= 1
    assert e.ncand[rows[5]] >= 1 and e.F["best"][rows[5]] == -1 and not e.F["accept"][rows[5]]
    assert not np.isin(e.F["best"], cols[5:7]).any() and not np.isin(e.F["second"], cols[5:7]).any()
    assert np.isfinite(e.F["dist_best"][e.F["best"] >= 0]).all()


def test_dense_rows_overflow_the_queue_many_times(gpu_hip, guided_ref):
    """All right points at one position and every left point within max_err of its image: every pair is a candidate, a
    wave queues 64 x 256 pairs per step into 512 entries.  Exact duplicates at both ends of r: ties go to the lower index."""
    hip = gpu_hip
    rng = np.random.default_rng(21)
    nl, nr = hip.GUIDED_ROWS + 6, 3000
    l = rng.random((nl, 128), np.float32)
    r = rng.random((nr, 128), np.float32)
    r[0] = l[5] + rng.normal(0, 0.01, 128).astype(np.float32)
    r[nr - 1] = r[0]
    r[1] = l[nl - 1] + rng.normal(0, 0.01, 128).astype(np.float32)
    r[nr - 2] = r[1]
    lxy = (np.array([400.0, 300.0]) + rng.random((nl, 2)) - 0.5).astype(np.float32)
    rxy = np.tile(np.array([[410.0, 305.0]], np.float32), (nr, 1))
    s = dict(l=l, lxy=lxy, r=r, rxy=rxy)
    e = check(hip, guided_ref, s, "homography", G.translation_H(10, 5), 2.0)
    assert (e.ncand == nr).all()
    assert (e.F["best"][5], e.F["second"][5]) == (0, nr - 1) and (e.F["best"][nl - 1], e.F["second"][nl - 1]) == (1, nr - 2)
    assert e.F["dist_best"][5] == e.F["dist_second"][5] and not e.F["accept"][5]
    check(hip, guided_ref, s, "epipolar", G.translation_F(10, 5), 2.0, (OPTION_SETS[3],))


def test_the_planted_cases(gpu_hip, guided_ref):
    s, M, max_err = G.planted_cases()
    e = check(gpu_hip, guided_ref, s, "homography", M, max_err)
    assert e.F["best"][10] == 40 and e.B["best"][50] == 13 and e.B["best"][60] == 15   # tests/test_guided_rule.py says why
    L, R = upload(gpu_hip, s)
    unguided = L.match(R)
    assert unguided["best"][10] == 20 and [unguided["best"][i] for i in range(6)] == [100 + i for i in range(6)]
    got = L.match_guided(R, "homography", M, max_err)
    assert [got["best"][i] for i in range(6)] == [110 + i for i in range(6)]
    with_cc = L.match_pairs_guided(R, "homography", M, max_err, ratio=0.0, cross_check=True)
    without = L.match_pairs_guided(R, "homography", M, max_err, ratio=0.0)
    assert 12 in without["l"] and 12 not in with_cc["l"] and 13 in with_cc["l"] and 15 in with_cc["l"]


def test_cap_count_empty_sets_and_sets_without_positions(gpu_hip, guided_ref):
    hip = gpu_hip
    lib = hip.lib()
    s, Hm = shared_scene(200, 1000)
    L, R = upload(hip, s)
    e = G.Expected(guided_ref, G.HOMOGRAPHY, Hm, 2.0, s)
    want = e.pairs(cross_check=True)
    total = len(want)
    assert total > 20
    o = hip.guided_opts("homography", Hm, 2.0, cross_check=True)
    n = C.c_int(-1)
    assert lib.popsift_hip_match_pairs_guided(L._h, R._h, C.byref(o), None, 0, C.byref(n)) == hip.ERR_TOO_SMALL and n.value == total
    for cap in (1, total - 1, total, total + 1):
        buf = np.zeros(cap + 1, hip.PAIR_DTYPE)
        buf["l"] = -7
        n.value = -1
        rc = lib.popsift_hip_match_pairs_guided(L._h, R._h, C.byref(o), buf.ctypes.data, cap, C.byref(n))
        assert rc == (hip.ERR_TOO_SMALL if cap < total else hip.OK) and n.value == total
        k = min(cap, total)
        assert buf[:k].tobytes() == want[:k].tobytes() and (buf["l"][k:] == -7).all()
    # two calls, the same bytes; and after the matchers that share the left set's scratch
    a = L.match_pairs_guided(R, "homography", Hm, 2.0, cross_check=True)
    L.match(R), L.match_pairs(R, cross_check=True)
    b = L.match_pairs_guided(R, "homography", Hm, 2.0, cross_check=True)
    assert a.tobytes() == b.tobytes() == want.tobytes()
    assert L.match_guided(R, "homography", Hm, 2.0).tobytes() == L.match_guided(R, "homography", Hm, 2.0).tobytes()
    # empty sets
    E = hip.DevFeatures.from_host_points(np.zeros((0, 128), np.float32), np.zeros((0, 2), np.float32))
    assert E.info() == (0, 0, 0)
    rows = L.match_guided(E, "homography", Hm, 2.0)
    assert (rows["best"] == -1).all() and (rows["second"] == -1).all() and not rows["accept"].any()
    assert np.isposinf(rows["dist_best"]).all() and np.isposinf(rows["dist_second"]).all()
    assert len(E.match_guided(R, "homography", Hm, 2.0)) == 0
    assert len(L.match_pairs_guided(E, "homography", Hm, 2.0, ratio=0.0)) == 0
    assert len(E.match_pairs_guided(R, "homography", Hm, 2.0, ratio=0.0)) == 0
    # a set without positions, on either side: ERR_INVALID, nothing written, and the left set still works afterwards
    bare_r, bare_l = hip.DevFeatures.from_host(s["r"]), hip.DevFeatures.from_host(s["l"])
    for l_set, r_set in ((L, bare_r), (bare_l, R)):
        buf = np.zeros(200, hip.PAIR_DTYPE)
        buf["l"] = -7
        n.value = -1
        assert lib.popsift_hip_match_pairs_guided(l_set._h, r_set._h, C.byref(o), buf.ctypes.data, 200, C.byref(n)) == hip.ERR_INVALID
        assert n.value == -1 and (buf["l"] == -7).all()
        out = np.zeros(200, hip.MATCH_DTYPE)
        out["best"] = -7
        assert lib.popsift_hip_match_guided(l_set._h, r_set._h, C.byref(o), out.ctypes.data) == hip.ERR_INVALID
        assert (out["best"] == -7).all()
    assert L.match_pairs_guided(R, "homography", Hm, 2.0, cross_check=True).tobytes() == want.tobytes()
    assert bare_l.match(bare_r).tobytes() == L.match(R).tobytes()


def test_an_image_pair_through_the_whole_chain(gpu_hip, guided_ref):
    """match_pairs -> pair_points -> RANSAC -> match_pairs_guided under the winner: every verified pair comes back."""
    hip = gpu_hip
    a = synth(95, 96, 72)
    b = np.roll(a, (8, 16), axis=(0, 1))
    ca, cb = hip.Context().submit(a), hip.Context().submit(b)
    fa, fb = ca.fetch()[0], cb.fetch()[0]
    A, B = ca.clone_results(), cb.clone_results()
    pairs = A.match_pairs(B, cross_check=True)
    pts = A.pair_points(B, pairs)
    v = hip.Verifier()
    res, mask = v.ransac(pts, "affine", 256, 0.5, 1)
    v.close()
    assert res["hypothesis"] >= 0 and mask.sum() >= 8
    guided = A.match_pairs_guided(B, "affine", res["H"], 0.5, cross_check=True)
    counts = "unguided %d, verified %d, guided %d" % (len(pairs), mask.sum(), len(guided))
    # the theorem: a verified pair's r is the global nearest and a candidate, the guided second is no nearer than the global
    # one, and the same holds the other way round
    verified = pairs[mask == 1]
    at = np.searchsorted(guided["l"], verified["l"])
    assert (at < len(guided)).all() and np.array_equal(guided["l"][at], verified["l"]), counts
    assert np.array_equal(guided["r"][at], verified["r"]), counts
    assert guided["dist_best"][at].tobytes() == verified["dist_best"].tobytes(), counts
    assert (guided["dist_second"][at] >= verified["dist_second"]).all(), counts
    # every guided pair is a candidate under the rule
    ra, rb = A.download()[1], B.download()[1]
    gp = np.stack([fa["xpos"][ra[guided["l"]]], fa["ypos"][ra[guided["l"]]],
                   fb["xpos"][rb[guided["r"]]], fb["ypos"][rb[guided["r"]]]], 1).astype(np.float32)
    assert guided_ref.ok_pairs(G.HOMOGRAPHY, res["H"], 0.5, gp).all(), counts
    assert A.pair_points(B, guided).tobytes() == gp.tobytes()
    # and the whole answer is the rule's on the downloaded sets
    s = dict(l=A.download()[0], lxy=np.c_[fa["xpos"][ra], fa["ypos"][ra]], r=B.download()[0], rxy=np.c_[fb["xpos"][rb], fb["ypos"][rb]])
    e = G.Expected(guided_ref, G.HOMOGRAPHY, res["H"], 0.5, s)
    assert guided.tobytes() == e.pairs(cross_check=True).tobytes(), counts
    print(counts)


def test_sets_on_two_gpus(gpu_hip, guided_ref):
    hip = gpu_hip
    if hip.device_count() < 2:
        pytest.skip("one GPU")
    s, Hm = shared_scene(200, 1000)
    L, R = upload(hip, s)
    far = hip.DevFeatures.from_host_points(s["r"], s["rxy"], device=1)
    for model, M in (("homography", Hm), ("epipolar", G.scene_F())):
        assert L.match_guided(far, model, M, 2.0).tobytes() == L.match_guided(R, model, M, 2.0).tobytes()
        for o in OPTION_SETS:
            assert L.match_pairs_guided(far, model, M, 2.0, **o).tobytes() == L.match_pairs_guided(R, model, M, 2.0, **o).tobytes()
    check(hip, guided_ref, s, "homography", Hm, 2.0, sets=(L, far))
