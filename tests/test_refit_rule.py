"""The refit's rule on the CPU (tests/refit_ref.c): its pairwise tree against a plain recursion, what a refit does to a noisy
planted scene -- checked against independent float64 least squares --, one scene per step of the rule whose result changes
when that step is broken, and one scene per reason to stop."""
import numpy as np
import pytest

import epipolar_rule as E
import ransac_rule as R
import refit_rule as F


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp("refit_ref")
    return F.Ref(d), R.Ref(d), E.Ref(d)


@pytest.mark.parametrize("kind", F.KINDS)
def test_the_sums_are_the_pairwise_tree(refs, kind):
    """rule 3b restated as a recursion over numpy float64 rows: equal to the traced sums of round 0 as bytes"""
    ref, m = refs[0], F.SAMPLE_SIZE[kind]
    for n in (m, 5, 64, 1000, 1025):
        if n < m:
            continue
        pts = (E.two_view(n, 1, 1.0) if kind == F.EPIPOLAR else R.planted(n, 1, kind, 1.0))[0]
        if n >= 64:
            pts[::3, 2] += 50.0                   # every third pair is no inlier: its leaf is +0.0
        M = F.planted_model("exact", n, kind)
        inl = ref.mask(pts, kind, M, 2.0)
        moved = (np.arange(n) % 3 == 0) & (n >= 64)
        assert inl[~moved].all() and inl[moved].sum() <= moved.sum() // 10   # moved along its epipolar line: still an inlier
        terms = np.where(inl.astype(bool)[:, None], ref.terms(pts, kind), 0.0)
        assert not (np.signbit(terms) & (terms == 0.0)).any()
        got = ref.refit(pts, kind, M, 2.0, 1)
        assert got["counts"][0] >= 0 and got["result"]["n_start"] == inl.sum()
        assert got["sums"][0].tobytes() == F.root(terms).tobytes()
        unused = sorted(set(range(F.SLOTS)) - set(F.USED_SLOTS[kind]))
        assert not got["sums"][0][unused].any() and got["sums"][0][F.USED_SLOTS[kind]].all()


def started(refs, kind, n=1000, seed=1, sigma=0.3):
    """the noisy planted scene and the winner of the kind's RANSAC reference on it (500 hypotheses, max_err 2)"""
    ref, rr, er = refs
    if kind == F.EPIPOLAR:
        pts, inl, Hm = F.noisy_two_view(n, seed, sigma)
        win = er.epipolar(pts, 2000, 2.0, 1, trace=False)["result"]
    else:
        pts, inl, Hm = F.noisy_planted(n, seed, kind, sigma)
        win = rr.ransac(pts, kind, 500, 2.0, 1, trace=False)["result"]
    assert win["hypothesis"] >= 0
    return pts, inl.astype(bool), Hm, win


# The largest distance (px) between the images of the final inliers under the refitted float32 model and under
# numpy.linalg.lstsq's float64 model of the same pairs, measured once on the reference: 5.99e-06 px for the homography,
# 2.56e-05 px for the affine map (float32 rounding of nine coefficients at coordinates <= 800 px predicts 1e-4).  Asserted
# at 4 x the measured value.
LSTSQ_BOUND = {F.HOMOGRAPHY: 4 * 5.99e-06, F.AFFINE: 4 * 2.56e-05}


@pytest.mark.parametrize("kind", [F.HOMOGRAPHY, F.AFFINE])
def test_noisy_planted_map(refs, kind):
    pts, inl, Hm, win = started(refs, kind)
    got = refs[0].refit(pts, kind, win["H"], 2.0, 4)
    res = got["result"]
    assert res["n_start"] == win["n_inliers"] and res["n_inliers"] >= res["n_start"] and res["rounds"] >= 1
    assert res["n_inliers"] == got["mask"].sum()
    truth = R.project(Hm, pts[inl, :2])
    off = lambda M: F.rms(np.hypot(*(R.project(np.asarray(M, np.float64).reshape(3, 3), pts[inl, :2]) - truth).T))
    print("rms to the planted map: start %.4f px, refitted %.4f px" % (off(win["H"]), off(res["M"])))
    assert off(res["M"]) < off(win["H"])
    assert off(res["M"]) < 0.1 < off(win["H"])             # 0.3 px of noise on 600 pairs against noise on 3 or 4
    final = pts[got["mask"].astype(bool)]
    lsq = F.lstsq_model(pts, got["mask"], kind)
    d = np.hypot(*(R.project(lsq, final[:, :2]) - R.project(res["M"].astype(np.float64).reshape(3, 3), final[:, :2])).T).max()
    print("largest distance to numpy.linalg.lstsq on the final mask: %.3g px" % d)
    assert d <= LSTSQ_BOUND[kind]


@pytest.mark.parametrize("name", ["two_view", "translation"])
def test_noisy_epipolar(refs, name):
    """against the float64 eigenvector solution of the same normal matrix, by Sampson rms over the planted inliers: equal to
    three digits (the gauge -- the coefficient the pivoting leaves over fixed to 1 -- costs nothing), F22 = 0 included"""
    ref, rr, er = refs
    if name == "two_view":
        pts, inl, _, win = started(refs, F.EPIPOLAR)
    else:
        inl = np.ones(1000, bool)
        pts = F.noisy(E.translation(1000), inl, 0.3)
        win = er.epipolar(pts, 2000, 2.0, 1, trace=False)["result"]
    got = ref.refit(pts, F.EPIPOLAR, win["H"], 2.0, 4)
    res = got["result"]
    assert res["n_inliers"] >= res["n_start"] == win["n_inliers"] and res["rounds"] >= 1
    mine, start = F.rms(E.sampson(res["M"], pts[inl])), F.rms(E.sampson(win["H"], pts[inl]))
    eig = F.rms(E.sampson(F.eigen_F(pts, got["mask"]), pts[inl]))
    print("Sampson rms: start %.4f px, refitted %.4f px, eigenvector %.4f px" % (start, mine, eig))
    assert mine < start and abs(mine - eig) <= 1e-3 * eig
    assert np.abs(res["M"]).max() == 1.0


@pytest.mark.parametrize("kind", F.KINDS)
def test_exact_scene(refs, kind):
    """no noise: the mask stays the planted mask and the count does not drop"""
    ref, rr, er = refs
    if kind == F.EPIPOLAR:
        pts, inl, _ = E.two_view(1000, 1)
        win = er.epipolar(pts, 2000, 0.5, 1, trace=False)["result"]
    else:
        pts, inl, _ = R.planted(1000, 1, kind)
        win = rr.ransac(pts, kind, 500, 0.5, 1, trace=False)["result"]
    assert win["n_inliers"] == inl.sum()
    got = ref.refit(pts, kind, win["H"], 0.5, 4)
    assert got["mask"].tobytes() == inl.tobytes() and got["result"]["n_inliers"] == inl.sum() == got["result"]["n_start"]


# ---- one scene per step whose result changes when the step is broken

def test_sums_over_the_inliers_only(refs):
    pts, inl, Hm, win = started(refs, F.HOMOGRAPHY)
    good, bad = (refs[0].refit(pts, F.HOMOGRAPHY, win["H"], 2.0, 4, v) for v in (0, F.ALL_PAIRS))
    assert good["result"]["n_inliers"] >= 600 and bad["result"]["stop"] == F.NOT_BETTER and bad["counts"][0] < 100
    assert bad["sums"][0][5] == 1000.0 and good["sums"][0][5] == float(win["n_inliers"])    # slot 5 counts the pairs


def test_tree_not_left_to_right(refs):
    pts, inl, Hm, win = started(refs, F.HOMOGRAPHY)
    good, bad = (refs[0].refit(pts, F.HOMOGRAPHY, win["H"], 2.0, 1, v) for v in (0, F.LEFT_TO_RIGHT))
    assert good["sums"].tobytes() != bad["sums"].tobytes()
    assert np.allclose(good["sums"], bad["sums"], rtol=1e-12, atol=1e-12)                   # the same sums, another order


def test_a_lower_count_is_not_accepted(refs):
    """1 px of noise on the affine scene: the fourth candidate holds 520 pairs after 522 (seed pinned by a search over the
    reference); the rule keeps the 522"""
    pts, inl, Hm = F.noisy_planted(1000, 1, F.AFFINE, 1.0)
    win = refs[1].ransac(pts[:2000], F.AFFINE, 300, 2.0, 5, trace=False)["result"]
    good, bad = (refs[0].refit(pts, F.AFFINE, win["H"], 2.0, 4, v) for v in (0, F.ACCEPT_LOWER))
    assert list(good["counts"]) == list(bad["counts"]) and good["counts"][3] < good["counts"][2]
    assert (good["result"]["stop"], good["result"]["rounds"], good["result"]["n_inliers"]) == (F.NOT_BETTER, 3, good["counts"][2])
    assert list(good["accepted"]) == [1, 1, 1, 0] and list(bad["accepted"]) == [1, 1, 1, 1]
    assert bad["result"]["n_inliers"] == good["counts"][3] and bad["result"]["M"].tobytes() == good["models"][3].tobytes()
    assert good["result"]["M"].tobytes() == good["models"][2].tobytes()


def test_w_positive_on_the_horizon(refs):
    """the pairs beyond the horizon meet e <= lim with w < 0: without `w > 0` they are counted and enter the sums"""
    pts = R.horizon(1000)
    win = refs[1].ransac(pts, F.HOMOGRAPHY, 300, 0.5, 1, trace=False)["result"]
    good, bad = (refs[0].refit(pts, F.HOMOGRAPHY, win["H"], 0.5, 2, v) for v in (0, F.NO_W_TEST))
    side = pts[:, 0] > 300.0
    assert 0 < good["result"]["n_start"] < len(pts) and bad["result"]["n_start"] == len(pts)
    assert good["mask"].astype(bool).tolist() in (side.tolist(), (~side).tolist())
    assert good["sums"][0].tobytes() != bad["sums"][0].tobytes()


@pytest.mark.parametrize("kind", F.KINDS)
def test_pairs_that_are_not_finite_stay_out(refs, kind):
    ref, rr, er = refs
    pts, M = F.start_model("nan", 1000, kind, rr, er, 2.0)
    good, bad = (ref.refit(pts, kind, M, 2.0, 2, v) for v in (0, F.NON_FINITE_ENTERS))
    assert np.isfinite(good["sums"]).all() and good["result"]["stop"] == F.CONVERGED and good["result"]["rounds"] == 1
    assert not good["mask"][[1000 // 3, 1000 // 2]].any()
    assert not np.isfinite(bad["sums"][0]).all() and bad["result"]["stop"] == F.NO_FIT and bad["counts"][0] == -1
    assert bad["result"]["M"].tobytes() == np.asarray(M, np.float32).tobytes()


# ---- one scene per reason to stop

@pytest.mark.parametrize("kind", F.KINDS)
def test_stop_no_support(refs, kind):
    ref = refs[0]
    pts = F.scene("noisy", 500, kind)
    got = ref.refit(pts, kind, np.zeros(9), 2.0, 4)                      # a zero M: w = 0, g = 0
    assert (got["result"]["stop"], got["result"]["n_start"], got["result"]["rounds"]) == (F.NO_SUPPORT, 0, 0)
    assert not got["mask"].any() and not got["result"]["M"].any() and (got["counts"] == -1).all() and not got["sums"].any()
    if kind != F.EPIPOLAR:                                               # outliers only, and a map they do not follow
        got = ref.refit(R.all_outliers(500), kind, F.planted_model("noisy", 500, kind), 2.0, 4)
        assert got["result"]["stop"] == F.NO_SUPPORT and got["result"]["n_inliers"] == got["result"]["n_start"] < 3
    for n in range(F.SAMPLE_SIZE[kind]):                                 # fewer pairs than a sample
        got = ref.refit(pts[:n], kind, F.IDENTITY, 2.0, 4)
        assert got["result"]["stop"] == F.NO_SUPPORT and got["result"]["M"].tobytes() == F.IDENTITY.tobytes()


def test_stop_no_fit(refs):
    """a normal matrix with a pivot of exactly 0: identical pairs; left points on one image row.  The collinear scene of
    ransac_rule is a line only up to float32 rounding: its system is ill conditioned, not singular, the rule has no
    conditioning threshold, and what the fit returns there keeps every pair within the limit."""
    ref = refs[0]
    shift = np.array([1, 0, 20, 0, 1, 10, 0, 0, 1], np.float32)
    for kind in (F.HOMOGRAPHY, F.AFFINE):
        got = ref.refit(R.identical(300), kind, shift, 2.0, 4)
        assert (got["result"]["stop"], got["result"]["n_start"], got["result"]["rounds"]) == (F.NO_FIT, 300, 0)
        assert got["result"]["M"].tobytes() == shift.tobytes() and got["mask"].all() and got["counts"][0] == -1
        assert got["sums"][0][5] == 300.0 and not got["models"].any()
    Hm = R.pixel_homography().astype(np.float32).reshape(9)
    got = ref.refit(F.collinear_row(300), F.HOMOGRAPHY, Hm, 2.0, 4)
    assert (got["result"]["stop"], got["result"]["n_start"]) == (F.NO_FIT, 300) and got["result"]["M"].tobytes() == Hm.tobytes()
    got = ref.refit(R.collinear(300), F.HOMOGRAPHY, Hm, 2.0, 4)
    assert got["result"]["stop"] in (F.CONVERGED, F.NOT_BETTER) and got["result"]["n_inliers"] == 300
    got = ref.refit(R.identical(300), F.EPIPOLAR, [0, 0, 0, 0, 0, -1, 0, 1, 10], 2.0, 4)    # y' = y + 10: every pair
    assert (got["result"]["stop"], got["result"]["n_start"]) == (F.NO_FIT, 300)


def test_stop_converged_not_better_and_rounds(refs):
    pts, inl, Hm, win = started(refs, F.HOMOGRAPHY)
    got = refs[0].refit(pts, F.HOMOGRAPHY, win["H"], 2.0, 16)
    assert (got["result"]["stop"], got["result"]["rounds"]) == (F.CONVERGED, 1)
    assert list(got["accepted"][:3]) == [1, 0, 0] and got["models"][1].tobytes() == got["models"][0].tobytes()
    assert (got["counts"][2:] == -1).all() and not got["sums"][2:].any()                   # rounds that did not run
    got = refs[0].refit(pts, F.HOMOGRAPHY, win["H"], 2.0, 1)
    assert (got["result"]["stop"], got["result"]["rounds"]) == (F.ROUNDS, 1)
    again = refs[0].refit(pts, F.HOMOGRAPHY, got["result"]["M"], 2.0, 1)                    # a fitted model comes back unchanged
    assert again["result"]["stop"] == F.CONVERGED and again["result"]["M"].tobytes() == got["result"]["M"].tobytes()
    # NOT_BETTER: test_a_lower_count_is_not_accepted
