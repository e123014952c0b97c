"""The oracle's extremum search against the float64 rule of tests/extrema_rule.py on the planted cases of
tests/extrema_cases.py: every candidate has one right answer with a margin of 1e-4 or more, so
the two must agree candidate by candidate; the census proves that every branch was taken, and every broken variant of
the rule changes the expected set, so a kernel with that defect fails tests/test_gpu_extrema_rule.py."""
import numpy as np
import pytest

import extrema_cases as X
import extrema_rule as R

from extrema_cases import MODES, MODE_ID, POS_BAR, SETS, SET_ID, SIGMA_BAR, oracle_on

_worst = {}


@pytest.mark.parametrize("cset", SETS, ids=SET_ID)
def test_oracle_equals_rule(oracle_mod, cset):
    cs = X.case_set(*cset)
    orc = oracle_on(oracle_mod, cs)
    got = orc.extrema()
    bad, worst, worst_s = X.match(cs.extrema, got)
    print("%s: %d extrema, largest distance %.3e px, sigma %.3e" % (SET_ID(cset), len(got), worst, worst_s))
    _worst[cset] = worst
    assert not bad, "\n".join(bad[:20])
    assert orc.ext_counts() == cs.counts
    assert worst <= POS_BAR and worst_s <= SIGMA_BAR, (worst, worst_s)
    # the same order as well: octave, level, row, column
    assert np.array_equal(got["lpos"], cs.extrema["lpos"]) and np.array_equal(got["cell"], cs.extrema["cell"])
    assert np.abs(got["xpos"] - cs.extrema["xn"]).max(initial=0) <= POS_BAR


def test_the_bar_is_the_measured_one(oracle_mod):
    """the bar is four times the largest distance measured over all case sets (figures the parametrised test above left,
    or measured here): MEASURED_PX is that distance rounded up in its third digit, no more"""
    worst = 0.0
    for cset in SETS:
        if cset not in _worst:
            cs = X.case_set(*cset)
            _worst[cset] = X.match(cs.extrema, oracle_on(oracle_mod, cs).extrema())[1]
        worst = max(worst, _worst[cset])
    print("largest oracle-to-rule distance %.4e px" % worst)
    assert POS_BAR == 4 * X.MEASURED_PX
    assert 0.99 * X.MEASURED_PX <= worst <= X.MEASURED_PX


@pytest.mark.parametrize("mode", MODES, ids=MODE_ID)
def test_no_thin_case_and_the_cap(mode):
    thin, cands = 0, 0
    for kind in X.KINDS:
        cs = X.case_set(mode, kind)
        assert cs.min_margin() >= R.THIN, (kind, cs.min_margin())
        thin += cs.thin_cands[0]
        cands += cs.thin_cands[1]
        # no directed site lost its case: on the final planes its need still holds
        found = {}
        for o, t in enumerate(cs.trace):
            for f in t:
                found.setdefault(int(cs.site_id[o][f[1], f[0]]), []).append(f)
        for i, s in enumerate(cs.sites):
            if s.need is not None:
                assert s.need(s, found.get(i, [])), (kind, s.family, s.octave, s.cx, s.cy, s.level)
            if s.family == "first_equal":    # |v| == first_thr as float32 values: the comparison >= decides at equality
                assert abs(cs.dog[s.octave][s.level, s.cy, s.cx]) == np.float32(cs.C.first_thr)
    print("%s: %d of %d candidates of the random family were thin (%.2f %%)" % (R.MODE_NAMES[mode], thin, cands, 100.0 * thin / cands))
    assert cands > 1000 and thin <= 0.03 * cands


@pytest.mark.parametrize("mode", MODES, ids=MODE_ID)
def test_census(mode):
    tot = {}
    for kind in X.KINDS:
        for k, v in X.case_set(mode, kind).tag_counts().items():
            tot[k] = tot.get(k, 0) + v
    print(R.MODE_NAMES[mode], sorted(tot.items()))
    short = {t: tot.get(t, 0) for t in X.CENSUS[mode] if tot.get(t, 0) < X.CENSUS_MIN}
    assert not short, short


def test_other_level_counts_reach_the_top_plane():
    for lv in (2, 9):
        assert X.case_set(R.POPSIFT, "top", lv).tag_counts().get("top_accept", 0) >= X.CENSUS_MIN
        for mode in MODES:
            assert X.case_set(mode, "top", lv).min_margin() >= R.THIN


# where each broken variant is caught: (mode, kind) of a case set whose expected extrema it changes
CAUGHT = {
    "nonstrict_26": [(m, k) for m in MODES for k in ("ties_max", "ties_min")],
    "centre_in_own_plane": [(m, "seams") for m in MODES],
    "gt_at_0.6": [(R.POPSIFT, "variants"), (R.VLFEAT, "variants")],
    "no_x_guard": [(R.POPSIFT, "variants"), (R.VLFEAT, "variants")],
    "no_z_guard": [(R.POPSIFT, "variants")],
    "no_top_clamp": [(R.POPSIFT, "variants"), (R.POPSIFT, "guards")],
    "two_sided_1.5": [(R.VLFEAT, "variants")],
    "det_lt_0": [(m, "variants") for m in MODES],
    "singular_rejects": [(m, "directed") for m in MODES],
    "opencv_fifth_accepts": [(R.OPENCV, "variants")],
    "opencv_level_bound": [(R.OPENCV, "variants")],
}


def _differs(a, b):
    if len(a) != len(b):
        return True
    key = lambda e: sorted(zip(e["octave"].tolist(), e["lpos"].tolist(), e["cell"].tolist(), np.round(e["xn"], 2).tolist(),
                               np.round(e["yn"], 2).tolist()))
    return key(a) != key(b)


@pytest.mark.parametrize("variant", sorted(CAUGHT))
def test_every_broken_variant_changes_the_expected_set(variant):
    assert variant in R.VARIANTS
    for mode, kind in CAUGHT[variant]:
        cs = X.case_set(mode, kind)
        assert _differs(cs.extrema, cs.expected(variant)), (variant, R.MODE_NAMES[mode], kind)


def test_the_equal_step_is_decided_in_float32():
    """the step_equal family: the offset on the landing pixel is 0.6f to the bit in the reference's float32 solve, 0.6 in
    float64 (2.4e-8 below); the rule takes the float32 comparison there and nowhere else"""
    assert set(CAUGHT) == set(R.VARIANTS)
    for DDx, Dx in ((-5.0, -3.0), (-10.0, -6.0), (-2.5, -1.5), (-1.25, -0.75)):
        d = R._solve3_f32(((DDx, 0.0, 0.0), (0.0, -2.0, 0.0), (0.0, 0.0, -2.0)), (-Dx, 0.0, 0.0))
        assert d[0] == np.float32(-0.6) and d[1] == 0 and d[2] == 0
        assert -Dx / DDx > -R.H6             # float64 alone would not step
    for mode in (R.POPSIFT, R.VLFEAT):
        cs = X.case_set(mode, "variants")
        n = sum("step_equal" in f[4] and f[5] >= R.THIN for t in cs.trace for f in t)
        assert n >= X.CENSUS_MIN


@pytest.mark.parametrize("cset", SETS, ids=SET_ID)
def test_gauss_route_subtracts_back_bit_for_bit(cset):
    cs = X.case_set(*cset)
    for o in range(len(cs.dims)):
        g = cs.gauss[o]
        assert g.dtype == np.float32 and len(g) == cs.levels + 3
        back = g[1:] - g[:-1]
        assert back.dtype == np.float32
        assert np.array_equal(back.view(np.uint32), cs.dog[o].view(np.uint32))
        on_grid = cs.dog[o].astype(np.float64) * X.Q
        off = on_grid != np.round(on_grid)
        assert np.abs(cs.dog[o]).max() <= X.VMAX
        # off the grid: nothing but the first_equal family's two values per site
        assert off.sum() <= 2 * sum(s.family == "first_equal" for s in cs.sites)
