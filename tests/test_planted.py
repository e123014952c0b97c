"""The contract of tests/planted.py, checked on the oracle without a GPU: the keypoint stages run on the planted planes
find EXACTLY the requested number of extrema in every octave, each at its planted centre and level."""
import hashlib

import numpy as np
import pytest

import planted as P

W, H, OCT = 480, 480, 4


def _run(O, request, seed=0, sift_mode=0, w=W, h=H, octaves=OCT, pin_z=False, **kw):
    dims = P.octave_dims(O, w, h, octaves, sift_mode=sift_mode, **kw)
    pl = P.Planted(dims, request, seed=seed, sift_mode=sift_mode, levels=kw.get("levels", P.LEVELS), pin_z=pin_z)
    orc = O.Oracle(O.default_params(**P.params_kw(octaves, sift_mode=sift_mode, **kw)), threads=4)
    orc.run(np.zeros((h, w), np.uint8), keypoints=False)
    pl.load_oracle(orc)
    return pl, orc


def _check(pl, orc):
    assert orc.ext_counts() == pl.counts
    e = orc.extrema()
    for o, bt in enumerate(pl.bumps):
        eo = e[e["octave"] == o]
        assert len(eo) == len(bt)
        if not len(eo):
            continue
        # each extremum at its own bump's centre (one to one), on the bump's search level
        d = np.hypot(eo["xpos"][:, None] - bt["xc"][None, :], eo["ypos"][:, None] - bt["yc"][None, :])
        j = d.argmin(1)
        assert len(set(j.tolist())) == len(bt), "octave %d: two extrema at one bump" % o
        assert d[np.arange(len(eo)), j].max() <= 2e-3, "octave %d: found and planted centres differ" % o
        assert np.array_equal(eo["lpos"], bt["z"][j]), "octave %d: lpos differs from the planted level" % o
        zc = bt["zc"][j]
        assert np.allclose(eo["sigma"], 1.6 * 2.0 ** (zc / pl.levels), rtol=1e-5), o


@pytest.mark.parametrize("sift_mode", [0, 1, 2])
@pytest.mark.parametrize("request_", [{}, {0: 1}, {0: 63, 1: 2}, {0: 255, 1: 3}, {0: 40, 2: 40}, {1: 10, 2: 10, 3: 5},
                                      {3: 20}, {0: 2049}, {0: 1000, 1: 500, 2: 120, 3: 20}],
                         ids=lambda r: "-".join("%d:%d" % kv for kv in sorted(r.items())) or "empty")
def test_oracle_finds_exactly_the_planted_extrema(oracle_mod, sift_mode, request_):
    pl, orc = _run(oracle_mod, request_, seed=len(request_) + sift_mode, sift_mode=sift_mode)
    _check(pl, orc)


def test_planted_regions_and_sub_queues(oracle_mod):
    """bumps confined to one detection sub-queue's cell land there, and only there"""
    dims = P.octave_dims(oracle_mod, W, H, OCT)
    w, h = dims[0]
    rect = P.subq_rect(w, h, 9)
    n = P.capacity(w, h, rect=rect)
    assert n >= 20
    pl, orc = _run(oracle_mod, {0: (n, rect)})
    _check(pl, orc)
    x0, y0, x1, y1 = rect
    bt = pl.bumps[0]
    assert ((bt["x"] >= x0) & (bt["x"] < x1) & (bt["y"] >= y0) & (bt["y"] < y1)).all()
    # every pixel of the octave belongs to exactly one sub-queue cell
    cover = np.zeros((h, w), np.int32)
    for q in range(P.DET_SUBQ):
        a, b, c, d = P.subq_rect(w, h, q)
        cover[b:d, a:c] += 1
    assert (cover[1:h - 1, 1:w - 1] == 1).all()
    yy, xx = np.mgrid[0:h, 0:w]
    q = np.full((h, w), -1)
    q[1:h - 1, 1:w - 1] = P.subq_of(w, h, xx, yy)[1:h - 1, 1:w - 1]
    for k in range(P.DET_SUBQ):
        a, b, c, d = P.subq_rect(w, h, k)
        inner = q[max(b, 1):min(d, h - 1), max(a, 1):min(c, w - 1)]
        assert inner.size and (inner == k).all(), k


def test_planted_geometry_covers_the_edges(oracle_mod):
    """the first / last detectable rows and columns, both ends of the search range, minima and maxima, the smallest
    octave, and orientations of more than one peak: the cases where clipping and indexing go wrong"""
    for mode in (0, 1):
        pl, orc = _run(oracle_mod, {0: 300, 1: 100, 2: 40, 3: 12}, seed=5, sift_mode=mode)
        _check(pl, orc)
        b = P.border(mode)
        for o, bt in enumerate(pl.bumps):
            w, h = pl.dims[o]
            assert (bt["x"] == b).any() and (bt["x"] == w - 1 - b).any(), o
            assert (bt["y"] == b).any() and (bt["y"] == h - 1 - b).any(), o
            assert set(bt["z"]) == {1, 2, 3}, o
            assert set(bt["sign"]) == {-1, 1}, o
        f, _ = orc.fetch()
        assert (f["num_ori"] > 1).sum() >= 5
    # the orientations are not mirror-symmetric: no two peaks of one keypoint tie (a set comparison is not needed)
    for r in f[f["num_ori"] > 1]:
        v = r["orientation"][:r["num_ori"]]
        assert len(set(v.tolist())) == len(v)


def test_request_beyond_the_lattice_is_refused(oracle_mod):
    dims = P.octave_dims(oracle_mod, 64, 64, 2)
    with pytest.raises(ValueError):
        P.Planted(dims, {1: P.capacity(*dims[1]) + 1})


def _digest(pl):
    h = hashlib.sha256()
    for o in range(len(pl.dims)):
        h.update(pl.bumps[o].tobytes())
        for p in pl.dog[o] + pl.gauss[o]:
            h.update(p.tobytes())
    return h.hexdigest()[:16]


def test_default_levels_generate_the_same_planes():
    """levels became a parameter of Planted: its default (3) draws and writes exactly what the generator did before,
    so the planted cases of tests/test_gpu_count_edges.py are the ones they were (digests of bumps and planes)"""
    assert _digest(P.Planted([(120, 90), (60, 45), (30, 22)], {0: 40, 1: (10, (0, 0, 40, 40)), 2: 3}, seed=5)) == \
        "40855fb0a8573ebb"
    assert _digest(P.Planted([(100, 80), (50, 40)], {0: 30, 1: 8}, seed=1, sift_mode=1, minima=False)) == "baa3a62b1667e03d"
    assert _digest(P.Planted([(100, 80), (50, 40)], {0: 30, 1: 8}, seed=1, sift_mode=1, minima=False, levels=3)) == \
        "baa3a62b1667e03d"


@pytest.mark.parametrize("sift_mode", [0, 1, 2])
def test_oracle_finds_exactly_the_planted_extrema_at_levels_9(oracle_mod, sift_mode):
    """nine search levels (12 Gaussian planes): bumps on every level 1 .. 9, centres down to zc = 0.7 and up to 9.3"""
    pl, orc = _run(oracle_mod, {0: 300, 1: 100, 2: 40, 3: 12}, seed=9 + sift_mode, sift_mode=sift_mode, levels=9, pin_z=True)
    _check(pl, orc)
    for o, bt in enumerate(pl.bumps):
        assert len(pl.dog[o]) == 11 and len(pl.gauss[o]) == 12
        assert set(bt["z"]) == set(range(1, 10)), o
        assert np.isclose(bt["zc"].min(), 0.7) and np.isclose(bt["zc"].max(), 9.3), o


def test_tables_give_the_requested_cells_and_tie_groups(oracle_mod):
    """Planted.from_tables: bumps on `inside` sites of chosen grid cells with 4 shared offset triples per octave -- the
    oracle finds exactly the requested number in every cell and exactly triples x levels distinct sigma bit patterns"""
    O = oracle_mod
    grid, triples = 3, 4
    dims = P.octave_dims(O, W, H, OCT)
    rng = np.random.default_rng(77)
    want = {0: [40, 0, 25, 31, 60, 1, 17, 0, 33], 1: [12, 9, 0, 20, 15, 12, 0, 3, 14], 2: [3, 4, 5, 0, 6, 3, 4, 5, 3]}
    tables = {}
    for o, counts in want.items():
        cs = P.cell_sites(*dims[o], grid)
        assert len(cs) == P.capacity(*dims[o]) and cs["inside"].sum() > 0.8 * len(cs)
        off = rng.uniform(0.05, 0.3, (triples, 3)) * rng.choice([-1.0, 1.0], (triples, 3))
        at = np.concatenate([rng.permutation(np.flatnonzero((cs["cell"] == c) & cs["inside"]))[:n] for c, n in enumerate(counts)])
        k = np.arange(len(at)) % triples
        tables[o] = P.bump_table(cs["x"][at], cs["y"][at], 1 + (np.arange(len(at)) // triples) % P.LEVELS, off[k],
                                 rng.choice([-1, 1], len(at)))
    pl = P.Planted.from_tables(dims, tables, seed=3)
    assert pl.counts == [sum(want[0]), sum(want[1]), sum(want[2]), 0]
    orc = O.Oracle(O.default_params(filter_grid_size=grid, **P.params_kw(OCT)), threads=4)
    orc.run(np.zeros((H, W), np.uint8), keypoints=False)
    pl.load_oracle(orc)
    _check(pl, orc)
    e = orc.extrema()
    for o, counts in want.items():
        eo = e[e["octave"] == o]
        assert np.bincount(eo["cell"], minlength=grid * grid).tolist() == counts, o
        assert len(set(eo["sigma"].view(np.uint32).tolist())) == triples * P.LEVELS, o
    with pytest.raises(ValueError):
        P.Planted.from_tables(dims, {0: P.bump_table([5, 5], [9, 9], [1, 2], np.zeros((2, 3)))})
    with pytest.raises(ValueError):
        P.Planted.from_tables(dims, {3: P.bump_table([dims[3][0] - 1], [9], [1], np.zeros((1, 3)))})
