"""The grid filter (filter.hip; Pyramid::extrema_filter_grid of the reference) restated in NumPy: integers, plus the few
float32 steps the reference has, each named.  Input is a list of extremum records (EXTREMUM_DTYPE of popsift_amd/_capi.py
or oracle/oracle.py) IN THE ORDER THE FILTER SEES IT, the grid size, filter_max and the mode (0 RANDOM: scale ignored,
1 largest scale first, 2 smallest scale first).

  active   filter_max > 0 and int(filter_max * 1.1) < total            (the double constant 1.1)
  limit    c = the n = grid^2 per-cell counts ascending, EMPTY CELLS INCLUDED; prefix = cumsum(c)
           sumup[i] = c[i] * (n - 1 - i) + prefix[i];   ct = #(sumup > filter_max);   ct == 0: no limit
           tail = the sum of the ct largest counts
           limit = ceil( float32(tail) / float32(ct)  -  float32( (total - filter_max) // ct ) )     INTEGER division
  select   scale = float32(sigma) * float32(2 ** octave); every cell keeps its first min(count, limit) members in the
           order (scale descending / ascending / ignored, then list position ascending)
  cell     int( floor(ypos / (float32(h) / grid)) * grid + floor(xpos / (float32(w) / grid)) ), all in float32, with
           (w, h) the record's octave's size (extrema.hip, sift_octave.cu:39-40)

Under POPSIFT_HIP_ORDER_RASTER the list the filter sees is order_rule.sort of the unfiltered list and its output is
ordered again: expected_raster().  In arrival order the members of a tie group that straddles a cell's limit are
undefined by design; check_properties() states what holds all the same.

The doctored variants (`doctor=`) are the mistakes a kernel could make; tests/test_filter_rule.py shows that each of them
changes the result of a named case, i.e. that the cases can tell them from the rule."""
import numpy as np

import order_rule as R

NO_LIMIT = 0x7fffffff
RANDOM, LARGEST_FIRST, SMALLEST_FIRST = 0, 1, 2
DOCTORS = ("later_wins", "float_division", "strict_threshold", "no_empty_cells")


def active(filter_max, total):
    return filter_max > 0 and int(filter_max * 1.1) < total


def limit(counts, filter_max, total, doctor=None):
    """counts: the members of each of the n cells (zeros included) -> the per-cell limit, NO_LIMIT when no cell is cut"""
    c = np.sort(np.asarray(counts, np.int64))
    n = len(c)
    if doctor == "no_empty_cells":
        # the non-empty counts alone at positions 0 .. m - 1 of the n: every factor n - 1 - i too large by the number of
        # empty cells.  (Leaving them out AND taking n = m is the same arithmetic as the rule: the zeros come first,
        # add nothing to the prefix and shift i and n alike; test_filter_rule.py states that identity.)
        c = c[c > 0]
    m = len(c)
    sumup = c * (n - 1 - np.arange(m)) + np.cumsum(c)
    ct = int((sumup > filter_max).sum())
    if ct == 0:
        return NO_LIMIT
    tail = int(c[m - ct:].sum())
    tailaverage = np.float32(tail) / np.float32(ct)
    assert total >= filter_max                      # // and C's truncating division agree
    if doctor == "float_division":
        cut = np.float32(total - filter_max) / np.float32(ct)
    else:
        cut = np.float32((total - filter_max) // ct)
    return int(np.ceil(np.float32(tailaverage - cut)))


def over_count(counts, filter_max):
    """ct of the limit: the number of ascending positions whose sumup exceeds filter_max (n: every cell is cut alike)"""
    c = np.sort(np.asarray(counts, np.int64))
    n = len(c)
    return int((c * (n - 1 - np.arange(n)) + np.cumsum(c) > filter_max).sum())


def scale_of(ext):
    return ext["sigma"].astype(np.float32) * np.exp2(ext["octave"].astype(np.float64)).astype(np.float32)


def ranks(cell, scale, mode, doctor=None):
    """the rank (0 = first) of every record inside its cell, in the order (scale by mode, list position)"""
    cell = np.asarray(cell, np.int64)
    scale = np.asarray(scale, np.float32).astype(np.float64)
    pos = np.arange(len(cell), dtype=np.int64)
    primary = {RANDOM: np.zeros(len(cell)), LARGEST_FIRST: -scale, SMALLEST_FIRST: scale}[mode]
    order = np.lexsort((-pos if doctor == "later_wins" else pos, primary, cell))
    sc = cell[order]
    first = np.ones(len(cell), bool)
    first[1:] = sc[1:] != sc[:-1]
    start = np.maximum.accumulate(np.where(first, np.arange(len(cell)), 0))
    rank = np.empty(len(cell), np.int64)
    rank[order] = np.arange(len(cell)) - start
    return rank


def select(cell, scale, n_cells, filter_max, mode, doctor=None):
    """the filter on bare (cell, scale) keys in list order, unconditionally (no 10 % test) -> (keep mask, limit)"""
    cell = np.asarray(cell, np.int64)
    assert len(cell) == 0 or (cell.min() >= 0 and cell.max() < n_cells)
    counts = np.bincount(cell, minlength=n_cells)
    lim = limit(counts, filter_max, len(cell), doctor)
    rank = ranks(cell, scale, mode, doctor)
    if doctor == "strict_threshold":                # `>` for `>=`: a cut cell loses its limit-th member too
        cut = counts[cell] > lim
        return rank < np.where(cut, lim - 1, lim), lim
    return rank < lim, lim


def apply(ext, grid, filter_max, mode, doctor=None):
    """-> (limit, keep mask over ext, active)"""
    if not active(filter_max, len(ext)):
        return NO_LIMIT, np.ones(len(ext), bool), False
    keep, lim = select(ext["cell"], scale_of(ext), grid * grid, filter_max, mode, doctor)
    return lim, keep, True


def expected_raster(unfiltered, grid, filter_max, mode, doctor=None):
    """the list a RASTER context returns for the unfiltered list `unfiltered` (any order) -> (records, limit, active)"""
    s = R.sort(unfiltered)
    lim, keep, act = apply(s, grid, filter_max, mode, doctor)
    return R.sort(s[keep]), lim, act


def octave_counts(ext, n_oct):
    return np.bincount(ext["octave"], minlength=n_oct)[:n_oct].tolist()


def cell_of(xpos, ypos, w, h, grid):
    """the cell of a refined position (octave units) in a w x h octave, float32 as extrema.hip writes it"""
    g = np.float32(grid)
    wdiv, hdiv = np.float32(w) / g, np.float32(h) / g
    x, y = np.asarray(xpos, np.float32), np.asarray(ypos, np.float32)
    v = np.floor(y / hdiv).astype(np.float32) * g + np.floor(x / wdiv).astype(np.float32)
    return v.astype(np.float32).astype(np.int32)


def recompute_cells(ext, dims, grid):
    out = np.zeros(len(ext), np.int32)
    for o, (w, h) in enumerate(dims):
        m = ext["octave"] == o
        out[m] = cell_of(ext["xpos"][m], ext["ypos"][m], w, h, grid)
    return out


def straddled(ext, grid, filter_max, mode):
    """[(cell, first rank, last rank, limit)] of the tie groups that straddle their cell's limit: the limit-th member
    (rank limit - 1) and the first dropped one (rank limit) share a scale -- in RANDOM mode every cut cell is one group"""
    lim, keep, act = apply(ext, grid, filter_max, mode)
    if not act or lim == NO_LIMIT:
        return []
    cell, scale = np.asarray(ext["cell"], np.int64), scale_of(ext)
    rank = ranks(cell, scale, mode)
    key = np.zeros(len(ext), np.float32) if mode == RANDOM else scale
    out = []
    for c in np.flatnonzero(np.bincount(cell, minlength=grid * grid) > lim):
        m = cell == c
        k = key[m][np.argsort(rank[m])]
        if lim >= 1 and k[lim - 1] == k[lim]:
            same = np.flatnonzero(k == k[lim])
            out.append((int(c), int(same[0]), int(same[-1]), lim))
    return out


def check_properties(unfiltered, kept, grid, filter_max, mode):
    """what every correct filter leaves of `unfiltered`, in whatever order it saw the list (raises AssertionError):
    kept is a subset; every cell holds min(count, limit); in a cell no dropped member is better than a kept one; every
    member strictly better than the cell's threshold scale (its limit-th best) is kept"""
    n = grid * grid
    rec = lambda e: [r.tobytes() for r in e]
    full, got = rec(unfiltered), rec(kept)
    assert len(set(full)) == len(full), "the unfiltered list holds a record twice"
    assert len(set(got)) == len(got), "a record was kept twice"
    assert set(got) <= set(full), "%d kept records are not in the unfiltered list" % len(set(got) - set(full))
    counts = np.bincount(unfiltered["cell"], minlength=n)
    act = active(filter_max, len(unfiltered))
    lim = limit(counts, filter_max, len(unfiltered)) if act else NO_LIMIT
    want = np.minimum(counts, lim)
    have = np.bincount(kept["cell"], minlength=n)
    bad = np.flatnonzero(want != have)
    assert not len(bad), "cells %s: kept %s, the rule keeps %s (limit %d)" % (bad[:8], have[bad][:8], want[bad][:8], lim)
    if mode == RANDOM or lim == NO_LIMIT:
        return lim
    sign = -1.0 if mode == LARGEST_FIRST else 1.0          # ascending in `sign * scale` = best first
    gotset = set(got)
    inset = np.array([b in gotset for b in full], bool)
    key = sign * scale_of(unfiltered).astype(np.float64)
    for c in np.flatnonzero(counts > lim):
        m = unfiltered["cell"] == c
        k, kin = key[m], inset[m]
        if lim == 0:
            continue
        thr = np.sort(k)[lim - 1]
        assert k[kin].max() <= k[~kin].min(), "cell %d: a dropped member is better than a kept one" % c
        assert kin[k < thr].all(), "cell %d: a member strictly better than the threshold scale was dropped" % c
    return lim
