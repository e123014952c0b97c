"""tests/filter_rule.py against the oracle, without a GPU: on bare (cell, scale) keys over a table of grids, count patterns,
filter_max values and modes; on every planted case of tests/filter_cases.py through the oracle's pipeline; and against
its own doctored variants.  Every case asserts from the rule alone what it is there for, so it cannot go vacuous."""
import numpy as np
import pytest

import filter_cases as C
import filter_rule as F
import order_rule as R

MODES = [0, 1, 2]


# ------------------------------------------------------------------------------------------------- bare keys

def _pattern(name, n, rng):
    """per-cell member counts of n cells"""
    if name == "random":
        return rng.integers(0, 40, n)
    if name == "equal":
        return np.full(n, 7)
    if name == "one_holds_all":
        c = np.zeros(n, np.int64)
        c[rng.integers(n)] = 300
        return c
    if name == "mostly_empty":
        return np.where(rng.random(n) < 0.8, 0, rng.integers(1, 30, n))
    if name == "ones_and_a_huge":
        c = np.ones(n, np.int64)
        c[rng.integers(n)] = 500
        return c
    if name == "0..2":
        return rng.integers(0, 3, n)
    raise KeyError(name)


PATTERNS = ["random", "equal", "one_holds_all", "mostly_empty", "ones_and_a_huge", "0..2"]


def _keys(counts, ties, rng):
    cell = np.repeat(np.arange(len(counts)), counts).astype(np.int32)
    if ties:
        scale = rng.integers(1, 6, len(cell)).astype(np.float32) * np.float32(1.25)      # five values: large tie groups
    else:
        scale = rng.permutation(len(cell)).astype(np.float32) + np.float32(1.0)
    p = rng.permutation(len(cell))
    return cell[p], scale[p]


def _fmax_values(total, rng, few):
    if total <= 1:
        return []
    if total <= 40 and not few:
        return list(range(1, total))
    pick = {1, 2, total // 10, total // 3, total // 2, total - 2, total - 1} | set(rng.integers(1, total, 2 if few else 6).tolist())
    return sorted(v for v in pick if 1 <= v < total)


@pytest.mark.parametrize("grid", [1, 2, 3, 5, 16, 63, 64])
def test_rule_equals_the_oracle_on_bare_keys(oracle_mod, grid):
    rng = np.random.default_rng(100 + grid)
    n = grid * grid
    few = n >= 3969                       # the 3969- and 4096-cell grids: a handful of cases each
    done = 0
    for k, name in enumerate(PATTERNS):
        for ties in (False, True):
            if few and (k + ties) % 2:
                continue
            counts = _pattern(name, n, rng)
            if counts.sum() == 0:
                counts[0] = 3
            cell, scale = _keys(counts, ties, rng)
            for fmax in _fmax_values(len(cell), rng, few):
                for mode in MODES:
                    keep_o, lim_o = oracle_mod.filter_grid_keys(cell, scale, grid, fmax, mode)
                    keep_r, lim_r = F.select(cell, scale, n, fmax, mode)
                    assert lim_r == lim_o, (name, ties, fmax, mode, lim_r, lim_o)
                    assert np.array_equal(keep_r, keep_o), (name, ties, fmax, mode)
                    done += 1
    assert done >= (30 if few else 100)


def test_rule_gives_the_known_answers():
    """the hand-worked answers of tests/test_oracle_filter.py"""
    rng = np.random.default_rng(0)
    cell, scale = _keys([10, 20, 30, 40], False, rng)
    for mode in MODES:
        keep, lim = F.select(cell, scale, 4, 60, mode)
        assert lim == 17 and [int(keep[cell == c].sum()) for c in range(4)] == [10, 17, 17, 17]
    cell, scale = _keys([50, 0, 50, 0], False, rng)
    keep, lim = F.select(cell, scale, 4, 70, 1)
    assert lim == 35 and keep.sum() == 70
    keep, lim = F.select(cell, scale, 4, 71, 1)                  # (100 - 71) // 2 = 14: the reference overshoots
    assert lim == 36 and keep.sum() == 72
    keep, lim = F.select(np.zeros(6, np.int32), np.full(6, 2, np.float32), 1, 3, 1)
    assert lim == 3 and keep.tolist() == [True] * 3 + [False] * 3          # equal scales: the earlier one wins
    assert F.active(500, 551) and not F.active(500, 550) and not F.active(0, 10) and not F.active(-1, 10)


def test_leaving_empty_cells_out_consistently_is_the_same_rule():
    """zeros come first in the ascending counts, add nothing to the prefix and shift i and n alike: dropping them and
    taking n = the number of non-empty cells is the rule again (the doctored variant keeps n and differs)"""
    rng = np.random.default_rng(5)
    for _ in range(200):
        counts = np.where(rng.random(64) < 0.6, 0, rng.integers(1, 50, 64))
        total = int(counts.sum())
        if total < 3:
            continue
        fmax = int(rng.integers(1, total))
        assert F.limit(counts, fmax, total) == F.limit(counts[counts > 0], fmax, total)


# ------------------------------------------------------------------------------------------------- planted cases

def _premises(case, pl, unf, mode):
    """what the case is there for, from the rule alone"""
    n = case.grid ** 2
    s = R.sort(unf)
    lim, keep, act = F.apply(s, case.grid, case.fmax, mode)
    counts = np.bincount(s["cell"], minlength=n)
    assert act, "the filter is not active"
    assert (counts > lim).any(), "the limit binds in no cell"
    assert np.array_equal(F.recompute_cells(unf, pl.dims, case.grid), unf["cell"])
    if "tie" in case.tags:
        inside = [g for g in F.straddled(s, case.grid, case.fmax, mode) if g[2] - g[1] + 1 >= 3 and g[1] < g[3] - 1 < g[2]]
        assert inside, "no cell's limit-th member lies strictly inside a tie group of three or more"
    if "whole_cell" in case.tags:
        m = s["cell"] == 4
        assert len(set(F.scale_of(s[m]).tolist())) == 1 and m.sum() > lim >= 2
    if "keep_all" in case.tags:
        assert ((counts > 0) & (counts <= lim)).any() and (counts > lim).any()
    if "seams" in case.tags:
        assert lim > 1 and all((counts == v).any() for v in (1, lim - 1, lim, lim + 1))
    if case.name == "limit_one":
        assert lim == 1
    if case.name == "all_equal":
        assert len(set(counts.tolist())) == 1 and F.over_count(counts, case.fmax) == n
    if case.name == "one_holds_all":
        assert F.over_count(counts, case.fmax) == 1 and sorted(counts.tolist())[:-1] == [1] * (n - 1)
        assert counts.max() == pl.counts[0]
    if case.name == "mostly_empty":
        assert (counts == 0).sum() > n * 0.9
    if case.name == "grid64":
        assert (counts == 0).sum() > 1000 and counts.max() == 3
    if case.name == "fmax_below_cells":
        assert case.fmax < n
    if "overshoot" in case.tags:
        assert keep.sum() >= 5 * case.fmax, "kept %d of filter_max %d" % (keep.sum(), case.fmax)
    if "empty_octave" in case.tags:
        assert pl.counts[1] == 0 and pl.counts[0] == int(case.name.split("_")[1])
        assert F.octave_counts(unf, C.OCT) == pl.counts
    if "boundary" in case.tags:
        near = {-1: 0, 1: 0}
        for o, (w, h) in enumerate(pl.dims):
            e = unf[unf["octave"] == o]
            for v, size in ((e["xpos"].astype(np.float64), w), (e["ypos"].astype(np.float64), h)):
                t = v * case.grid / size
                d = (t - np.round(t)) * size / case.grid          # signed distance to the nearest cell boundary, pixels
                inner = (np.round(t) > 0) & (np.round(t) < case.grid) & (np.abs(d) < 2e-3)
                near[-1] += int((inner & (d < 0)).sum())
                near[1] += int((inner & (d >= 0)).sum())
        assert near[-1] + near[1] >= 12 and min(near.values()) >= 4, near
    if case.sift_mode == 1:
        assert case.levels == 5 and set(unf["lpos"].tolist()) == {1, 2, 3, 4, 5}
        for o, (w, h) in enumerate(pl.dims):
            e = unf[unf["octave"] == o]
            assert e["xpos"].min() > 4.5 and e["xpos"].max() < w - 5.5
    return lim, int(keep.sum())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", C.NAMES)
def test_planted_case_through_the_oracle_pipeline(oracle_mod, name, mode):
    """the oracle's filtered extrema are the rule applied to the oracle's own unfiltered list in the oracle's own order:
    the pipeline hook, the 10 % test, the limit and the selection"""
    case = C.BY_NAME[name]
    pl = case.planted(oracle_mod)
    unf = case.unfiltered(oracle_mod)
    assert F.octave_counts(unf, C.OCT) == pl.counts
    _premises(case, pl, unf, mode)
    lim, keep, act = F.apply(unf, case.grid, case.fmax, mode)
    orc = case.oracle(oracle_mod, mode)
    got = orc.extrema()
    assert got.tobytes() == unf[keep].tobytes()
    assert orc.ext_counts() == F.octave_counts(unf[keep], C.OCT)
    F.check_properties(unf, got, case.grid, case.fmax, mode)


# ------------------------------------------------------------------------------------------------- doctored rules

DOCTORED = {                                          # the case and mode on which each mistake must show
    "later_wins": ("whole_cell_tie", 1),
    "float_division": ("limit_seams", 2),
    "strict_threshold": ("tie_grid3", 1),
    "no_empty_cells": ("mostly_empty", 1),
}


@pytest.mark.parametrize("doctor", F.DOCTORS)
def test_doctored_rule_changes_a_named_case(oracle_mod, doctor):
    name, mode = DOCTORED[doctor]
    case = C.BY_NAME[name]
    case.planted(oracle_mod)
    unf = case.unfiltered(oracle_mod)
    want, lim, act = F.expected_raster(unf, case.grid, case.fmax, mode)
    got, lim_d, _ = F.expected_raster(unf, case.grid, case.fmax, mode, doctor=doctor)
    assert act and want.tobytes() != got.tobytes()
    if doctor in ("float_division", "no_empty_cells"):
        assert lim_d != lim
    else:
        assert lim_d == lim
    if doctor == "later_wins":
        assert len(got) == len(want)                  # the same counts, other members
    # and the property checker, which knows no list position, tells the count mistakes from the rule
    if doctor != "later_wins":
        with pytest.raises(AssertionError):
            F.check_properties(unf, got, case.grid, case.fmax, mode)


def test_property_checker_accepts_any_tie_break_and_nothing_else(oracle_mod):
    case = C.BY_NAME["tie_grid3"]
    case.planted(oracle_mod)
    unf = case.unfiltered(oracle_mod)
    for mode in MODES:
        for doctor in (None, "later_wins"):
            got, _, _ = F.expected_raster(unf, case.grid, case.fmax, mode, doctor=doctor)
            F.check_properties(unf, got, case.grid, case.fmax, mode)
    # a kept member swapped for a strictly worse one of its cell
    s = R.sort(unf)
    lim, keep, _ = F.apply(s, case.grid, case.fmax, 1)
    sc = F.scale_of(s)
    m = s["cell"] == 0
    best = np.flatnonzero(m & keep)[np.argmax(sc[m & keep])]
    worst = np.flatnonzero(m & ~keep)[np.argmin(sc[m & ~keep])]
    keep[best], keep[worst] = False, True
    with pytest.raises(AssertionError):
        F.check_properties(unf, s[keep], case.grid, case.fmax, 1)
