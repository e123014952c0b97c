"""popsift_hip_match_pairs without a GPU: the numpy rule the GPU tests compare with (tests/match_pairs_rule.py) against
known answers on the oracle's searches, proof that no filter of the tested option sets is vacuous, and the argument
checks of the C ABI (made before any GPU call)."""
import ctypes as C
import os
import subprocess

import numpy as np

from match_pairs_rule import CAP, OPTION_SETS, PAIR_DTYPE, expected_pairs, keep_masks, planted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def searches(oracle_mod, l, r):
    return oracle_mod.match(l, r), oracle_mod.match(r, l)


def test_default_options_give_the_accepted_rows(oracle_mod):
    l, r = planted(300, 400)
    F, B = searches(oracle_mod, l, r)
    p = expected_pairs(F, B)
    acc = np.flatnonzero(F["accept"] == 1)
    assert len(acc) > 50
    assert np.array_equal(p["l"], acc) and np.array_equal(p["r"], F["best"][acc])
    assert p["dist_best"].tobytes() == F["dist_best"][acc].tobytes()
    assert p["dist_second"].tobytes() == F["dist_second"][acc].tobytes()
    assert p.dtype == PAIR_DTYPE and PAIR_DTYPE.itemsize == 16


def test_cross_check_is_symmetric_without_ties(oracle_mod):
    rng = np.random.default_rng(5)
    l = rng.random((300, 128), np.float32)
    r = rng.random((400, 128), np.float32)
    r[rng.permutation(400)[:100]] = l[rng.permutation(300)[:100]] + rng.normal(0, 0.02, (100, 128)).astype(np.float32)
    F, B = searches(oracle_mod, l, r)
    p = expected_pairs(F, B, ratio=0.0, cross_check=True)
    q = expected_pairs(B, F, ratio=0.0, cross_check=True)          # the swapped call: its l is a right index
    assert 100 <= len(p) < 300
    p = p[np.argsort(p["r"], kind="stable")]
    assert np.array_equal(p["r"], q["l"]) and np.array_equal(p["l"], q["r"])
    assert p["dist_best"].tobytes() == q["dist_best"].tobytes()     # (a - b)^2 = (b - a)^2: the same float both ways
    # every pair is a mutual nearest neighbour, and every mutual nearest neighbour is a pair
    mutual = np.flatnonzero(B["best"][F["best"]] == np.arange(300))
    assert np.array_equal(np.sort(q["r"]), mutual)


def test_of_two_identical_left_rows_the_lower_index_survives(oracle_mod):
    l, r = planted(300, 400)
    F, B = searches(oracle_mod, l, r)
    assert F["best"][50] == 3 and F["best"][200] == 3 and B["best"][3] == 50
    without = expected_pairs(F, B, ratio=0.0)
    with_cc = expected_pairs(F, B, ratio=0.0, cross_check=True)
    assert 50 in without["l"] and 200 in without["l"]
    assert 50 in with_cc["l"] and 200 not in with_cc["l"]
    # duplicates on the right: l[7] points to the lowest of the three copies and passes the cross-check there
    assert F["best"][7] == 1 and F["second"][7] == 200 and 7 in with_cc["l"]
    assert len(np.unique(with_cc["r"])) == len(with_cc)            # a right descriptor has one nearest left one


def test_no_filter_is_vacuous(oracle_mod):
    """On the sets the GPU tests use, each of the three conditions removes a row the other two keep, and together they
    keep some: a kernel that ignored one of them would not pass."""
    for nl, nr in ((300, 400), (2500, 3100), (5000, 4000)):
        l, r = planted(nl, nr)
        F, B = searches(oracle_mod, l, r)
        opts = OPTION_SETS[-1]
        assert opts == dict(ratio=0.8, max_dist2=CAP, cross_check=True)
        k_ratio, k_cap, k_cross = keep_masks(F, B, **opts)
        assert (~k_ratio & k_cap & k_cross).any(), "the ratio test removes nothing of its own"
        assert (k_ratio & ~k_cap & k_cross).any(), "the cap removes nothing of its own"
        assert (k_ratio & k_cap & ~k_cross).any(), "the cross-check removes nothing of its own"
        assert (k_ratio & k_cap & k_cross).sum() >= 10
        assert not k_ratio[7] and k_cap[7] and k_cross[7]
        assert k_ratio[200] and k_cap[200] and not k_cross[200]
        # the tighter ratio differs from the default: row 9's quotient lies between them
        assert 0.6 < F["dist_best"][9] / F["dist_second"][9] < 0.8
        assert len(expected_pairs(F, B, ratio=0.6)) < len(expected_pairs(F, B))
        counts = [len(expected_pairs(F, B, **o)) for o in OPTION_SETS]
        assert len(set(counts)) == len(counts), counts


def test_degenerate_sizes(oracle_mod):
    l = np.ones((5, 128), np.float32)
    e = np.zeros((0, 128), np.float32)
    assert len(expected_pairs(*searches(oracle_mod, l, e), ratio=0.0)) == 0        # no right descriptor: no pair
    assert len(expected_pairs(*searches(oracle_mod, e, l), ratio=0.0)) == 0
    F, B = searches(oracle_mod, l, l[:1])                           # one candidate: second = inf, 0 / inf < 0.8
    assert expected_pairs(F, B)["l"].tolist() == [0, 1, 2, 3, 4]
    assert expected_pairs(F, B, cross_check=True)["l"].tolist() == [0]
    F, B = searches(oracle_mod, l, l)                               # all distances 0: 0 / 0 is NaN and fails
    assert len(expected_pairs(F, B)) == 0 and len(expected_pairs(F, B, ratio=0.0)) == 5


def test_struct_layouts_and_defaults(hip, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "popsift_hip.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu\n", sizeof(popsift_hip_match_opts), sizeof(popsift_hip_pair),
           offsetof(popsift_hip_match_opts, cross_check), offsetof(popsift_hip_pair, r), offsetof(popsift_hip_pair, dist_second));
    return 0;
}
""")
    exe = str(tmp_path / "layout.bin")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = list(map(int, subprocess.check_output([exe], text=True).split()))
    assert got == [C.sizeof(hip.MatchOpts), hip.PAIR_DTYPE.itemsize, hip.MatchOpts.cross_check.offset,
                   hip.PAIR_DTYPE.fields["r"][1], hip.PAIR_DTYPE.fields["dist_second"][1]] == [16, 16, 8, 4, 12]
    assert hip.PAIR_DTYPE == PAIR_DTYPE
    o = hip.MatchOpts(-1.0, -1.0, 7, 7)
    hip.lib().popsift_hip_default_match_opts(C.byref(o))
    assert (o.ratio, o.max_dist2, o.cross_check, o.reserved) == (np.float32(0.8), np.inf, 0, 0)
    hip.lib().popsift_hip_default_match_opts(None)                  # tolerated


def test_invalid_arguments_are_rejected_without_a_gpu(hip):
    """Every ERR_INVALID case of the header.  The arguments are checked before a set is looked at, so two blocks of
    zeros stand in for sets here (as sets they would be empty: nothing reaches a GPU even where a check is missing)."""
    lib = hip.lib()
    l, r = C.create_string_buffer(512), C.create_string_buffer(512)
    out = np.zeros(4, hip.PAIR_DTYPE)
    n = C.c_int(-1)

    def call(opts, l=l, r=r, pairs=out.ctypes.data, cap=4, n_pairs=C.byref(n)):
        return lib.popsift_hip_match_pairs(l, r, C.byref(opts) if opts is not None else None, pairs, cap, n_pairs)

    def opts(**kw):
        o = hip.MatchOpts()
        lib.popsift_hip_default_match_opts(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    assert call(opts(), l=None) == hip.ERR_INVALID
    assert call(opts(), r=None) == hip.ERR_INVALID
    assert call(None) == hip.ERR_INVALID
    assert call(opts(), n_pairs=None) == hip.ERR_INVALID
    assert call(opts(), pairs=None) == hip.ERR_INVALID              # cap > 0 without a buffer
    for kw in (dict(ratio=-0.1), dict(ratio=float("nan")), dict(ratio=float("inf")), dict(max_dist2=float("nan")),
               dict(reserved=1), dict(cross_check=2), dict(cross_check=-1)):
        assert call(opts(**kw)) == hip.ERR_INVALID, kw
    assert n.value == -1                                            # a rejected call writes nothing
    # accepted: the edges of the ranges; empty sets give 0 pairs
    for kw in (dict(), dict(ratio=0.0), dict(ratio=-0.0), dict(max_dist2=0.0), dict(max_dist2=-1.0), dict(cross_check=1),
               dict(ratio=1e30, max_dist2=float("inf"))):
        n.value = -1
        assert call(opts(**kw)) == hip.OK and n.value == 0, kw
    n.value = -1
    assert call(opts(), pairs=None, cap=0) == hip.OK and n.value == 0
