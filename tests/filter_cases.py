"""The planted cases of the grid-filter tests (tests/test_filter_rule.py on the oracle, tests/test_gpu_filter_rule.py on
the device): per-cell populations and scale tie groups on a 480 x 480 image of 4 octaves (480, 240, 120, 60), built
with planted.Planted.from_tables.  A case names the grid, filter_max, the parameters, and what it is there for
(`tie`: a tie group must straddle a limit in the scale modes; `keep_all`: a cell is kept whole while another is cut)."""
import numpy as np

import filter_rule as F
import planted as P

W = H = 480
OCT = 4
SEP = 9           # bumps are at least this far apart (Chebyshev): supports of radius 3.5 plus the 3 x 3 test


def _offsets(rng, n, triples, levels):
    """(z, off): distinct random offsets, or `triples` shared (dx, dy, dz) triples: members of one (triple, level) tie"""
    z = 1 + rng.integers(0, levels, n)
    if triples is None:
        return z, rng.uniform(0.05, 0.3, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    t = rng.uniform(0.05, 0.3, (triples, 3)) * rng.choice([-1.0, 1.0], (triples, 3))
    return z, t[rng.integers(0, triples, n)]


def _table(rng, sites, triples, levels):
    z, off = _offsets(rng, len(sites), triples, levels)
    return P.bump_table(sites["x"], sites["y"], z, off, rng.choice([-1, 1], len(sites)))


def per_cell(dims, grid, want, rng, triples=None, sift_mode=0, levels=P.LEVELS):
    """want = {octave: {cell: n}}: n bumps on `inside` sites of the cell (exact counts, wherever the centres fall);
    {octave: n}: n sites of the whole lattice, counts as they come"""
    tables = {}
    for o, spec in want.items():
        cs = P.cell_sites(*dims[o], grid, sift_mode)
        if isinstance(spec, dict):
            pick = []
            for c, n in spec.items():
                at = np.flatnonzero((cs["cell"] == c) & cs["inside"])
                if n > len(at):
                    raise ValueError("octave %d cell %d: %d wanted, %d sites inside" % (o, c, n, len(at)))
                pick.append(rng.permutation(at)[:n])
            sites = cs[np.concatenate(pick)] if pick else cs[:0]
        else:
            sites = cs[rng.permutation(len(cs))[:spec]]
        tables[o] = _table(rng, sites, triples, levels)
    return tables


class Case:
    def __init__(self, name, grid, fmax, build, tags=(), seed=0, **kw):
        self.name, self.grid, self._fmax, self.build, self.tags, self.seed, self.kw = name, grid, fmax, build, set(tags), seed, kw
        self._pl = self._unf = None
        self.fmax = None if callable(fmax) else fmax

    @property
    def sift_mode(self):
        return self.kw.get("sift_mode", 0)

    @property
    def levels(self):
        return self.kw.get("levels", P.LEVELS)

    def params(self, mode=None, filtered=True):
        """the params_kw of the case; filtered=False: the same grid (the cell field), the filter off"""
        kw = dict(filter_grid_size=self.grid, **self.kw)
        if filtered:
            kw.update(filter_max_extrema=self.fmax, filter_sorting=mode)
        return P.params_kw(OCT, **kw)

    def dims(self, O):
        return P.octave_dims(O, W, H, OCT, **self.kw)

    def planted(self, O):
        if self._pl is None:
            dims = self.dims(O)
            rng = np.random.default_rng(1000 + self.seed)
            self._pl = P.Planted.from_tables(dims, self.build(dims, self, rng), seed=self.seed, levels=self.levels)
            if callable(self._fmax):
                self.fmax = self._fmax(self._pl)
        return self._pl

    def oracle(self, O, mode=None, filtered=True):
        pl = self.planted(O)
        orc = O.Oracle(O.default_params(**self.params(mode, filtered)), threads=4)
        orc.run(np.zeros((H, W), np.uint8), keypoints=False)
        pl.load_oracle(orc)
        return orc

    def unfiltered(self, O):
        """the oracle's unfiltered list, in the oracle's order (never modified)"""
        if self._unf is None:
            self._unf = self.oracle(O, filtered=False).extrema()
            self._unf.setflags(write=False)
        return self._unf


def _search_fmax(counts, total, ok):
    """the smallest filter_max that passes the 10 % test and whose limit satisfies ok(limit)"""
    for fmax in range(1, total):
        if F.active(fmax, total) and ok(F.limit(counts, fmax, total)):
            return fmax
    raise ValueError("no filter_max gives the wanted limit")


def _b_tie_grid3(dims, case, rng):
    o0 = rng.integers(40, 71, 9)
    return per_cell(dims, 3, {0: dict(enumerate(o0)), 1: {c: 20 for c in range(9)}, 2: {c: 6 for c in range(9)},
                              3: {c: 2 for c in range(9)}}, rng, triples=4)


def _b_whole_cell_tie(dims, case, rng):
    other = {c: int(n) for c, n in enumerate(rng.integers(20, 41, 9)) if c != 4}
    t = per_cell(dims, 3, {0: other, 1: {c: 8 for c in range(9) if c != 4}}, rng)
    cs = P.cell_sites(*dims[0], 3)
    at = rng.permutation(np.flatnonzero((cs["cell"] == 4) & cs["inside"]))[:50]
    one = P.bump_table(cs["x"][at], cs["y"][at], np.full(50, 2), np.tile([[0.21, -0.13, 0.17]], (50, 1)), rng.choice([-1, 1], 50))
    t[0] = np.concatenate([t[0], one])
    return t


def _b_distinct_grid2(dims, case, rng):
    return per_cell(dims, 2, {0: dict(enumerate([300, 120, 40, 210])), 1: dict(enumerate([50, 90, 10, 30])), 2: 60, 3: 20}, rng)


def _b_limit_one(dims, case, rng):
    return per_cell(dims, 3, {0: dict(enumerate([5, 6, 7, 8, 9, 7, 7, 7, 7]))}, rng, triples=2)


SEAM_COUNTS = [1, 12, 13, 14, 30, 31, 32, 33, 34]


def _b_limit_seams(dims, case, rng):
    return per_cell(dims, 3, {0: dict(enumerate(SEAM_COUNTS))}, rng)


def _b_all_equal(dims, case, rng):
    return per_cell(dims, 4, {0: {c: 30 for c in range(16)}, 1: {c: 10 for c in range(16)}}, rng, triples=4)


def _b_one_holds_all(dims, case, rng):
    return per_cell(dims, 3, {0: {0: 200}, 1: {c: 1 for c in range(1, 9)}}, rng)


def _b_mostly_empty(dims, case, rng):
    """12 of 256 cells are occupied, two of them above the limit: the ten small ones stay under filter_max only because
    the 244 empty cells take the first places of the ascending counts"""
    cs = P.cell_sites(*dims[0], 16)
    room = [c for c in rng.permutation(256) if ((cs["cell"] == c) & cs["inside"]).sum() >= 8][:12]
    return per_cell(dims, 16, {0: {int(c): (8 if k < 2 else 2) for k, c in enumerate(room)}}, rng, triples=3)


def _b_scatter(counts, triples=None):
    def build(dims, case, rng):
        return per_cell(dims, case.grid, dict(counts), rng, triples=triples, sift_mode=case.sift_mode, levels=case.levels)
    return build


def _b_boundaries(dims, case, rng):
    """bump centres within 1e-3 px of a vertical or horizontal cell boundary, on both sides, plus lattice bumps away from
    them that make the filter bind"""
    g = case.grid
    tables = {}
    for o in (0, 1):
        w, h = dims[o]
        rows = []
        for k in range(1, g):
            b = k * w / g                        # w == h
            p = int(round(b))
            if abs(b - p) > 0.29:
                continue
            for side in (-1e-3, 1e-3):
                rows.append(("v", p, b - p + side))
                rows.append(("h", p, b - p + side))
        xs, ys, off = [], [], []
        free_v = iter(range(14, h - 14, 2 * SEP))
        free_h = iter(range(14 + SEP, w - 14, 2 * SEP))
        for kind, p, d in rows:
            q = next(free_v if kind == "v" else free_h)
            x, y, dx, dy = (p, q, d, 0.11) if kind == "v" else (q, p, -0.07, d)
            if all(max(abs(x - a), abs(y - c)) >= SEP for a, c in zip(xs, ys)):
                xs.append(x), ys.append(y), off.append((dx, dy, rng.uniform(-0.3, 0.3)))
        n_b = len(xs)
        for s in rng.permutation(P.lattice(w, h)):
            if len(xs) >= n_b + (400 if o == 0 else 100):
                break
            if all(max(abs(s[0] - a), abs(s[1] - c)) >= SEP for a, c in zip(xs[:n_b], ys[:n_b])):
                xs.append(int(s[0])), ys.append(int(s[1]))
                off.append(tuple(rng.uniform(0.05, 0.3, 3) * rng.choice([-1.0, 1.0], 3)))
        tables[o] = P.bump_table(xs, ys, 1 + rng.integers(0, 3, len(xs)), off, rng.choice([-1, 1], len(xs)))
    return tables


def _seam_fmax(pl):
    counts = np.array(SEAM_COUNTS)
    return _search_fmax(counts, int(counts.sum()), lambda lim: lim == 13)


CASES = [
    Case("tie_grid3", 3, 400, _b_tie_grid3, tags=("tie",), seed=1),
    Case("whole_cell_tie", 3, 200, _b_whole_cell_tie, tags=("tie", "whole_cell"), seed=2),
    Case("distinct_grid2", 2, 500, _b_distinct_grid2, tags=("keep_all",), seed=3),
    Case("limit_one", 3, 9, _b_limit_one, tags=(), seed=4),
    Case("limit_seams", 3, _seam_fmax, _b_limit_seams, tags=("keep_all", "seams"), seed=5),
    Case("all_equal", 4, 300, _b_all_equal, tags=("tie",), seed=6),
    Case("one_holds_all", 3, 100, _b_one_holds_all, tags=("keep_all",), seed=7),
    Case("mostly_empty", 16, 30, _b_mostly_empty, tags=("keep_all",), seed=8),
    Case("grid5", 5, 500, _b_scatter({0: 1200, 1: 300, 2: 80, 3: 20}), tags=(), seed=9),
    Case("grid7_ties", 7, 600, _b_scatter({0: 1200, 1: 300, 2: 80, 3: 20}, triples=4), tags=("tie",), seed=10),
    Case("grid63_overshoot", 63, lambda pl: pl.total // 10, _b_scatter({0: 2304, 1: 576, 2: 144, 3: 36}), tags=("overshoot",), seed=11),
    Case("grid64", 64, 1500, _b_scatter({0: 2000, 1: 500, 2: 144, 3: 35}, triples=4), tags=("keep_all",), seed=12),
    Case("fmax_below_cells", 16, 100, _b_scatter({0: 1200, 1: 300}), tags=(), seed=13),
    Case("compact_2047", 2, 1000, _b_scatter({0: 2047, 2: 100, 3: 20}), tags=("empty_octave",), seed=14),
    Case("compact_2048", 2, 1000, _b_scatter({0: 2048, 2: 100, 3: 20}, triples=4), tags=("empty_octave", "tie"), seed=15),
    Case("compact_2049", 2, 1000, _b_scatter({0: 2049, 2: 100, 3: 20}), tags=("empty_octave",), seed=16),
    Case("boundaries_grid7", 7, 300, _b_boundaries, tags=("boundary",), seed=17),
    Case("boundaries_grid9", 9, 300, _b_boundaries, tags=("boundary",), seed=18),
    Case("opencv_levels5", 3, 400, _b_scatter({0: 900, 1: 250, 2: 60, 3: 10}, triples=4), tags=("tie",), seed=19, sift_mode=1, levels=5),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
