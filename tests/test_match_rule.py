"""The oracle's matcher (oracle_match) held to the float64 rule of tests/match_rule.py on the case sets built against
the screening path, both ways round, with no row left out -- and the case sets held to what they claim to be."""
import numpy as np
import pytest

import match_rule as MR
from match_rule import RULE_CASES, case, dist64, violations


@pytest.fixture(scope="module")
def D_of():
    """dist64 of a case, computed once and shared: the reverse direction is its transpose"""
    memo = {}

    def get(name, size):
        if (name, size) not in memo:
            memo[(name, size)] = dist64(*case(name, *size), min_term=True)
        return memo[(name, size)]
    return get


@pytest.mark.parametrize("name,size", RULE_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_oracle_rows_satisfy_the_float64_rule(oracle_mod, D_of, name, size):
    """several_tiles_per_split is planted(16385, 3073), the issue's own size: the oracle takes 1.2 s for it with 16
    threads on an 8-core host (0.4 s the other way round), well inside the 15 s it was given: the size is not shrunk."""
    l, r = case(name, *size)
    D, min_term = D_of(name, size)
    assert min_term >= MR.MIN_TERM, "the case underflows: the rule's bounds do not apply"
    F, B = oracle_mod.match(l, r, threads=16), oracle_mod.match(r, l, threads=16)
    assert violations(l, r, F, D) == []
    assert violations(r, l, B, np.ascontiguousarray(D.T)) == []


@pytest.mark.parametrize("nl,K", MR.ALL_UNDECIDABLE_SIZES)
def test_all_undecidable_is_what_it_claims(oracle_mod, nl, K):
    l, r = case("all_undecidable", nl, K)
    assert len(r) == 4 * K and len(np.unique(r, axis=0)) == K
    F = oracle_mod.match(l, r)
    first, second = MR.duplicate_ranks(r)
    assert np.array_equal(F["best"], first[F["best"]]) and np.array_equal(F["second"], second[F["best"]])
    assert np.array_equal(F["dist_best"], F["dist_second"]) and np.all(F["dist_best"] > 0)


def test_mostly_undecidable_is_what_it_claims(oracle_mod):
    l, r, n_und = MR.mostly_undecidable()
    assert (len(l), len(r), n_und) == (3000, 1200, 1500)
    F = oracle_mod.match(l, r)
    first, second = MR.duplicate_ranks(r)
    even, odd = F[0::2], F[1::2]
    assert np.all(second[even["best"]] == even["second"]) and np.array_equal(even["dist_best"], even["dist_second"])
    assert np.all(second[odd["best"]] == -1) and np.all(second[odd["second"]] == -1)     # unique rows
    # far from the margin on both sides: the third nearest of an odd row is a random row, at about 128 / 6
    D = dist64(l[1::2], r)
    third = np.partition(D, 2, axis=1)[:, 2]
    assert np.all(third > 10.0) and np.all(odd["dist_second"] < 0.2)


@pytest.mark.parametrize("size", [(300, 400), (3, 2)])
def test_non_finite_is_what_it_claims(oracle_mod, size):
    l, r = case("non_finite", *size)
    F, B = oracle_mod.match(l, r), oracle_mod.match(r, l)
    if size == (3, 2):
        assert F.tolist() == [MR.EMPTY_ROW] * 3 and B.tolist() == [MR.EMPTY_ROW] * 2
        return
    assert np.isnan(l).any(1).sum() == 6 and np.isnan(r).any(1).sum() == 5
    assert np.isposinf(r).any(1).sum() == 6 and np.isneginf(r).any(1).sum() == 3 and np.isposinf(l).any(1).sum() == 1
    clean_l = np.setdiff1d(np.arange(len(l)), MR.NF_POISONED_L)
    clean_r = np.setdiff1d(np.arange(len(r)), MR.NF_POISONED_R)
    for rows, clean, poisoned_self, poisoned_other in ((F, clean_l, MR.NF_POISONED_L, MR.NF_POISONED_R),
                                                      (B, clean_r, MR.NF_POISONED_R, MR.NF_POISONED_L)):
        assert not np.isin(rows["best"][clean], poisoned_other).any()
        assert not np.isin(rows["second"][clean], poisoned_other).any()
        assert np.isfinite(rows["dist_second"][clean]).all()
        assert rows[poisoned_self].tolist() == [MR.EMPTY_ROW] * len(poisoned_self)
    # the near-copies are found among the poison
    a, b = MR.NF_COPIES
    assert np.array_equal(F["best"][a:b], np.arange(a, b)) and np.array_equal(B["best"][a:b], np.arange(a, b))


@pytest.mark.parametrize("size", [(64, 96), (300, 400)])
def test_huge_finite_is_what_it_claims(oracle_mod, size):
    l, r = case("huge_finite", *size)
    with np.errstate(over="ignore"):
        assert np.isposinf((l * l).sum(1, dtype=np.float32)).all() and np.isposinf((r * r).sum(1, dtype=np.float32)).all()
    for rows in (oracle_mod.match(l, r), oracle_mod.match(r, l)):
        assert np.isfinite(rows["dist_best"]).all() and np.isfinite(rows["dist_second"]).all()
        assert np.all(rows["dist_best"] > 0)
    F = oracle_mod.match(l, r)
    assert F["best"][2] == 3 and F["best"][5] == 10 and F["accept"][2] == 1
    assert np.isfinite(dist64(l, r)).all()


@pytest.mark.parametrize("size", [(700, 900), (5000, 4000)])
def test_mixed_norms_outsiders_have_the_intended_gaps(size):
    l, r = case("mixed_norms", *size)
    n = MR.N_OUTSIDER_ROWS
    D = dist64(l[:n], r)
    i = np.arange(n)
    best, second, out = D[i, 4 * i], D[i, 4 * i + 1], np.stack([D[i, 4 * i + 2], D[i, 4 * i + 3]], 1)
    assert np.allclose(best, MR.OUT_BEST, atol=1e-6) and np.allclose(second, MR.OUT_SECOND, atol=1e-6)
    gap = out - second[:, None]
    assert np.all(np.abs(gap) <= MR.OUT_GAP + 2e-6) and np.all(gap != 0)
    l64, r64 = l[:n].astype(np.float64), r[:4 * n].astype(np.float64)
    assert np.allclose((l64 ** 2).sum(1), 1, atol=1e-6)
    assert np.allclose((r64 ** 2).sum(1).reshape(n, 4), [1, 1, MR.OUT_NORM2, MR.OUT_NORM2], atol=1e-5)
    # nothing else comes near: the rows at the origin (scale 1e-3) lie at squared distance 1
    D[i[:, None], 4 * i[:, None] + np.arange(4)] = np.inf
    assert D.min() > MR.OUT_SECOND + 0.05
    # and the set spans the scales: squared norms from 1e-5 to 1e8
    n2 = (r.astype(np.float64) ** 2).sum(1)
    assert n2.min() < 1e-4 and n2.max() > 1e7


def test_zeros_and_tiny_is_what_it_claims(oracle_mod):
    l, r = case("zeros_and_tiny", 300, 400)
    F = oracle_mod.match(l, r)
    assert F[:10].tolist() == [(0, 1, 0, 0.0, 0.0)] * 10          # zero against zero: ties at 0, 0 / 0 fails the ratio
    assert F["best"][30] == 20 and F["dist_best"][30] == 0
    tiny = F[300 - MR.N_TINY_L:]
    assert np.all(tiny["dist_second"] < 1.2e-38)                    # denormal or zero distances
    assert F["best"][299] in (0, 399) and F["dist_best"][299] == 0


def test_the_rule_rejects_wrong_rows(oracle_mod):
    l, r = case("mixed_norms", 700, 900)
    D = dist64(l, r)
    F = oracle_mod.match(l, r)
    assert violations(l, r, F, D) == []
    order = np.argsort(D, axis=1, kind="stable")
    i = int(np.flatnonzero(F["dist_second"] > 1.01 * F["dist_best"])[0])          # a row without a tie
    swapped = F.copy()
    swapped[i] = (F["second"][i], F["best"][i], F["accept"][i], F["dist_second"][i], F["dist_best"][i])
    assert {x for x, _ in violations(l, r, swapped, D)} == {i}
    third = F.copy()
    j = int(order[i, 2])
    third["second"][i] = j
    third["dist_second"][i] = np.float32(D[i, j])
    third["accept"][i] = third["dist_best"][i] / third["dist_second"][i] < np.float32(0.8)
    assert violations(l, r, third, D) == [(i, "second is not the second nearest")]
    off = F.copy()
    off["dist_best"][i] *= np.float32(1 + 4e-6)
    off["accept"][i] = off["dist_best"][i] / off["dist_second"][i] < np.float32(0.8)
    assert violations(l, r, off, D) == [(i, "dist_best")]
    # a tie resolved to the higher index
    l, r = case("all_undecidable", 33, 40)
    D = dist64(l, r)
    F = oracle_mod.match(l, r)
    assert violations(l, r, F, D) == []
    copies = np.flatnonzero((r == r[F["best"][4]]).all(1))
    assert len(copies) == 4 and copies[0] == F["best"][4] and copies[1] == F["second"][4]
    high = F.copy()
    high["second"][4] = copies[2]
    assert violations(l, r, high, D) == [(4, "second: an equal row has a lower index")]
    high = F.copy()
    high["best"][4], high["second"][4] = copies[1], copies[0]
    assert violations(l, r, high, D) == [(4, "best: an equal row has a lower index")]
    # a non-candidate named, and a wrong empty record
    l, r = case("non_finite", 300, 400)
    D = dist64(l, r)
    F = oracle_mod.match(l, r)
    bad = F.copy()
    bad["second"][0] = MR.NF_R_NAN[0]
    assert (0, "second is no candidate") in violations(l, r, bad, D)
    bad = F.copy()
    bad[MR.NF_L_NAN[0]] = F[0]
    assert violations(l, r, bad, D) == [(MR.NF_L_NAN[0], "no candidate: not the empty record")]
