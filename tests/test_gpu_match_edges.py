"""popsift_hip_match_sets / popsift_hip_match_pairs on float sets built against the screening path's argument
(tests/match_rule.py): redo lists that fill and cross the exact kernel's workgroups and the two redo launches, norms that
span orders of magnitude, negative components, zero and denormal rows, NaN and Inf elements, norms that overflow while
distances do not; scratch that outlives a call; matching from several host threads.  Every result is held to the oracle
as bytes on every path, and to the float64 rule."""
import threading

import numpy as np
import pytest

import match_rule as MR
from match_pairs_rule import OPTION_SETS, expected_pairs, planted
from match_rule import ORACLE_ONLY_CASES, RULE_CASES, case, dist64, violations
from test_gpu_match import assert_same

pytestmark = pytest.mark.gpu

PAIR_OPTIONS = OPTION_SETS + [dict(cross_check=True)]
# rows the forward screening sweep must hand to the exact kernel (popsift_hip_devfeatures_debug_redo_count), where the
# construction fixes the number: every row of all_undecidable; the rows planted near a quadruple; and, because the
# screening pass decides nothing from norms that are not finite, every row of a sweep whose right set has such a norm
N_REDO = {"all_undecidable": lambda l, r: len(l), "mostly_undecidable": lambda l, r: (len(l) + 1) // 2,
          "huge_finite": lambda l, r: len(l), "non_finite": lambda l, r: len(l)}


@pytest.fixture
def match_path(gpu_hip):
    """popsift_hip_match_set_path for the duration of a test"""
    def set_path(p):
        assert gpu_hip.lib().popsift_hip_match_set_path(p) == 0
    yield set_path
    gpu_hip.lib().popsift_hip_match_set_path(gpu_hip.MATCH_AUTO)


def paths(hip):
    return (("exact", hip.MATCH_EXACT), ("screen", hip.MATCH_SCREEN), ("auto", hip.MATCH_AUTO))


@pytest.mark.parametrize("name,size", RULE_CASES + ORACLE_ONLY_CASES,
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_case_sets_match_the_oracle_and_the_rule_on_every_path(oracle_mod, gpu_hip, match_path, name, size):
    hip = gpu_hip
    l, r = case(name, *size)
    F, B = oracle_mod.match(l, r, threads=16), oracle_mod.match(r, l, threads=16)
    ruled = (name, size) in RULE_CASES
    D = dist64(l, r) if ruled else None
    Dt = np.ascontiguousarray(D.T) if ruled else None
    L, R = hip.DevFeatures.from_host(l), hip.DevFeatures.from_host(r)
    assert L.debug_redo_count() == -1
    seen = set()
    for tag, path in paths(hip):
        match_path(path)
        f, b = L.match(R), R.match(L)
        if path == hip.MATCH_SCREEN and name in N_REDO:
            assert L.debug_redo_count() == N_REDO[name](l, r), tag
        # the rule first: when device and oracle agree on something wrong, or differ, it says what is wrong with a row
        for rows, x, y, d in ((f, l, r, D), (b, r, l, Dt)):
            if ruled and rows.tobytes() not in seen:
                assert violations(x, y, rows, d) == [], tag
                seen.add(rows.tobytes())
        assert_same(F, f)
        assert_same(B, b)
        for opts in PAIR_OPTIONS:
            assert L.match_pairs(R, **opts).tobytes() == expected_pairs(F, B, **opts).tobytes(), (tag, opts)
            assert R.match_pairs(L, **opts).tobytes() == expected_pairs(B, F, **opts).tobytes(), (tag, opts)


def test_rows_without_a_candidate_in_match_pairs(oracle_mod, gpu_hip, match_path):
    """ratio = 0 and max_dist2 = +inf: condition 3 of the header reads dist_best <= max_dist2, and +inf <= +inf holds.  A
    left row without any candidate (a NaN or Inf element) therefore yields the pair (i, 0, +inf, +inf) -- the header's
    wording taken literally -- unless the cross-check removes it: right row 0's nearest left row is another."""
    hip = gpu_hip
    l, r = case("non_finite", 300, 400)
    F, B = oracle_mod.match(l, r), oracle_mod.match(r, l)
    L, R = hip.DevFeatures.from_host(l), hip.DevFeatures.from_host(r)
    for tag, path in paths(hip):
        match_path(path)
        for cross in (False, True):
            opts = dict(ratio=0.0, max_dist2=np.inf, cross_check=cross)
            p = L.match_pairs(R, **opts)
            assert p.tobytes() == expected_pairs(F, B, **opts).tobytes(), (tag, opts)
            assert R.match_pairs(L, **opts).tobytes() == expected_pairs(B, F, **opts).tobytes(), (tag, opts)
            empty = p[np.isin(p["l"], MR.NF_POISONED_L)]
            if cross:
                assert len(empty) == 0
            else:
                assert len(p) == len(l) and empty["l"].tolist() == MR.NF_POISONED_L
                assert np.all(empty["r"] == 0) and np.all(np.isposinf(empty["dist_best"]))
        # any finite cap removes them
        p = L.match_pairs(R, ratio=0.0, max_dist2=3.0e38)
        assert len(p) == len(l) - len(MR.NF_POISONED_L) and not np.isin(p["l"], MR.NF_POISONED_L).any()


def test_scratch_of_a_left_set_across_right_sets_and_paths(oracle_mod, gpu_hip, match_path):
    """One left set against right sets of 3100, 1, 0, 129, 5000 and 160 (all undecidable) rows in turn, the screening and
    the exact path alternating, twice round with the paths exchanged: the candidate buffer (Cand and Top2 records, three
    split counts), the right norms and the redo list are the left set's and only ever grow."""
    hip = gpu_hip
    l = planted(2500, 3100)[0]
    rng = np.random.default_rng(5)
    rights = [planted(2500, 3100)[1], rng.random((1, 128), np.float32), np.zeros((0, 128), np.float32),
              planted(2500, 129)[1], planted(2500, 5000)[1], case("all_undecidable", 31, 40)[1]]
    want = [oracle_mod.match(l, r, threads=16) for r in rights]
    Rs = [hip.DevFeatures.from_host(r) for r in rights]

    def sequence(L):
        out, step = [], 0
        for rnd in range(2):
            for R in Rs:
                screen = (step + rnd) % 2 == 0
                match_path(hip.MATCH_SCREEN if screen else hip.MATCH_EXACT)
                out.append(L.match(R))
                if screen and R is Rs[5]:
                    assert L.debug_redo_count() == len(l)
                step += 1
        return out

    first = sequence(hip.DevFeatures.from_host(l))
    for k, m in enumerate(first):
        assert_same(want[k % len(Rs)], m)
    again = sequence(hip.DevFeatures.from_host(l))
    assert [m.tobytes() for m in again] == [m.tobytes() for m in first]


@pytest.mark.parametrize("path", ["MATCH_SCREEN", "MATCH_EXACT"])
def test_matching_from_several_host_threads(oracle_mod, gpu_hip, match_path, path):
    """Four threads, each with a left set of its own, match against one shared right set while a fifth uses that right
    set as its left set (include/popsift_hip.h: "all scratch belongs to l ... r may be the left set of another thread's
    call").  Every result equals the serial run's bytes."""
    hip = gpu_hip
    match_path(getattr(hip, path))
    ls = [planted(1500 + k, 2100)[0] for k in range(4)]
    r = planted(1500, 2100)[1]
    Ls, R = [hip.DevFeatures.from_host(l) for l in ls], hip.DevFeatures.from_host(r)
    opts = dict(cross_check=True)

    def work(k):
        if k < 4:
            return Ls[k].match(R).tobytes(), Ls[k].match_pairs(R, **opts).tobytes()
        return R.match(Ls[0]).tobytes(), R.match_pairs(Ls[0], **opts).tobytes()

    serial = [work(k) for k in range(5)]
    for k in range(5):
        x, y = (ls[k], r) if k < 4 else (r, ls[0])
        F, B = oracle_mod.match(x, y, threads=16), oracle_mod.match(y, x, threads=16)
        assert serial[k] == (F.tobytes(), expected_pairs(F, B, **opts).tobytes()), k
    got, errors = [[] for _ in range(5)], []

    def run(k):
        try:
            for _ in range(3):
                got[k].append(work(k))
        except Exception as e:          # noqa: BLE001 -- reported below, in the test's thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=run, args=(k,)) for k in range(5)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert errors == []
    for k in range(5):
        assert got[k] == [serial[k]] * 3, k
