"""popsift_hip_match_pairs on the GPU: byte for byte against the numpy rule (tests/match_pairs_rule.py) applied to the
oracle's forward and reverse searches, for every match path, on both sides of the 4 M-pair switch."""
import ctypes as C

import numpy as np
import pytest

from match_pairs_rule import CAP, OPTION_SETS, expected_pairs, keep_masks, planted
from popsift_amd.synth import synth

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 2), (3, 1), (31, 63), (32, 64), (33, 65), (100, 1000), (700, 129), (2500, 3100),   # test_gpu_match's
         (1, 0), (0, 5), (5000, 4000)]                                                                   # empty; > 4 M pairs


@pytest.fixture
def match_path(gpu_hip):
    """popsift_hip_match_set_path for the duration of a test"""
    def set_path(p):
        assert gpu_hip.lib().popsift_hip_match_set_path(p) == 0
    yield set_path
    gpu_hip.lib().popsift_hip_match_set_path(gpu_hip.MATCH_AUTO)


def raw_pairs(hip, L, R, cap, buf_len=None, null=False, **kw):
    """popsift_hip_match_pairs with a caller-chosen cap: (status, n_pairs, buffer).  The buffer is filled with 0xff
    bytes first, so what the call did not write shows."""
    buf = np.full(cap if buf_len is None else buf_len, -1, np.int32).repeat(4).view(hip.PAIR_DTYPE)
    opts = hip.MatchOpts(kw.get("ratio", 0.8), kw.get("max_dist2", np.inf), 1 if kw.get("cross_check") else 0, 0)
    n = C.c_int(-1)
    rc = hip.lib().popsift_hip_match_pairs(L._h, R._h, C.byref(opts), None if null else buf.ctypes.data, cap, C.byref(n))
    return rc, n.value, buf


@pytest.mark.parametrize("nl,nr", SIZES)
def test_planted_sets_match_the_rule_on_every_path(oracle_mod, gpu_hip, match_path, nl, nr):
    hip = gpu_hip
    l, r = planted(nl, nr)
    F, B = oracle_mod.match(l, r), oracle_mod.match(r, l)
    L, R = hip.DevFeatures.from_host(l), hip.DevFeatures.from_host(r)
    for path in (hip.MATCH_AUTO, hip.MATCH_EXACT, hip.MATCH_SCREEN):
        match_path(path)
        for opts in OPTION_SETS:
            want = expected_pairs(F, B, **opts)
            got = L.match_pairs(R, **opts)
            assert got.dtype == hip.PAIR_DTYPE
            assert got.tobytes() == want.tobytes(), (path, opts, len(got), len(want))
    # default options: the accepted rows of match_sets
    m = L.match(R)
    if nr > 0:
        acc = np.flatnonzero(m["accept"] == 1)
        p = L.match_pairs(R)
        assert np.array_equal(p["l"], acc) and np.array_equal(p["r"], m["best"][acc])


def test_cap_count_and_repeatability(oracle_mod, gpu_hip):
    hip = gpu_hip
    l, r = planted(2500, 3100)
    F, B = oracle_mod.match(l, r), oracle_mod.match(r, l)
    L, R = hip.DevFeatures.from_host(l), hip.DevFeatures.from_host(r)
    before = L.match(R)
    for opts in (OPTION_SETS[0], OPTION_SETS[3], OPTION_SETS[4]):
        want = expected_pairs(F, B, **opts)
        total = len(want)
        assert total > 2
        rc, n, buf = raw_pairs(hip, L, R, total, **opts)                       # cap = total: fits
        assert (rc, n) == (hip.OK, total) and buf.tobytes() == want.tobytes()
        rc, n, buf = raw_pairs(hip, L, R, total - 1, buf_len=total, **opts)     # one short: the count, the first cap pairs
        assert (rc, n) == (hip.ERR_TOO_SMALL, total)
        assert buf[:total - 1].tobytes() == want[:total - 1].tobytes()
        assert buf[total - 1:].tobytes() == b"\xff" * 16                        # nothing past cap
        rc, n, _ = raw_pairs(hip, L, R, 0, null=True, **opts)                   # the count alone
        assert (rc, n) == (hip.ERR_TOO_SMALL, total)
        rc, n, buf = raw_pairs(hip, L, R, len(l), **opts)                       # l_len is always enough
        assert (rc, n) == (hip.OK, total) and buf[:total].tobytes() == want.tobytes()
        assert buf[total:].tobytes() == b"\xff" * 16 * (len(l) - total)
        assert L.match_pairs(R, **opts).tobytes() == L.match_pairs(R, **opts).tobytes()
    after = L.match(R)
    assert before.tobytes() == after.tobytes()
    assert before.tobytes() == F.tobytes()
    # the right set as somebody's left set, and a set against itself
    assert R.match_pairs(L, ratio=0.0, cross_check=True).tobytes() == expected_pairs(B, F, ratio=0.0, cross_check=True).tobytes()
    S = oracle_mod.match(l, l)
    assert L.match_pairs(L, ratio=0.0, cross_check=True).tobytes() == expected_pairs(S, S, ratio=0.0, cross_check=True).tobytes()


def test_screening_margin_cases_with_the_cross_check(oracle_mod, gpu_hip, match_path):
    """The sets of test_screening_margin_cases: exact duplicates and near-ties, in the forward sweep's right set and --
    as the reverse sweep sees them -- among the left rows it ranks."""
    hip = gpu_hip
    rng = np.random.default_rng(7)
    l = rng.random((300, 128), np.float32)
    r = rng.random((900, 128), np.float32)
    r[10:17] = l[5]                                        # seven exact copies of a left row: all distance 0
    r[100:106] = l[6] + 1e-7                               # six near-copies inside the margin
    r[200] = l[7]
    r[201] = l[7] + np.float32(3e-4)                       # best and second a hair apart
    r[300:303] = r[299]                                    # duplicates that are nobody's neighbour
    for scale in (1.0, 512.0):
        ls, rs = (l * scale).astype(np.float32), (r * scale).astype(np.float32)
        F, B = oracle_mod.match(ls, rs), oracle_mod.match(rs, ls)
        L, R = hip.DevFeatures.from_host(ls), hip.DevFeatures.from_host(rs)
        for path in (hip.MATCH_SCREEN, hip.MATCH_EXACT, hip.MATCH_AUTO):
            match_path(path)
            for opts in (dict(ratio=0.0, cross_check=True), dict(cross_check=True),
                         dict(ratio=0.9, max_dist2=19.0 * scale * scale, cross_check=True)):
                assert L.match_pairs(R, **opts).tobytes() == expected_pairs(F, B, **opts).tobytes(), (scale, path, opts)
                assert R.match_pairs(L, **opts).tobytes() == expected_pairs(B, F, **opts).tobytes(), (scale, path, opts)
        p = L.match_pairs(R, ratio=0.0, cross_check=True)
        assert p["r"][p["l"] == 5].tolist() == [10] and p["r"][p["l"] == 7].tolist() == [200]


def test_image_pair(oracle_mod, gpu_hip):
    """The image pair of test_cloned_results_and_image_to_image_matching.  On the CPU oracle's own extraction of this
    pair 3184 of 3409 descriptors are cross-checked pairs and 99.9 % of them land within 1 px of the shift: the bound
    of that test (0.9) holds for the cross-checked set with room."""
    a = synth(90, 320, 240)
    b = np.roll(a, (3, 5), axis=(0, 1))
    ca, cb = gpu_hip.Context().submit(a), gpu_hip.Context().submit(b)
    fa, da = ca.fetch()
    fb, db = cb.fetch()
    A, B = ca.clone_results(), cb.clone_results()
    F, G = oracle_mod.match(da, db), oracle_mod.match(db, da)
    for opts in OPTION_SETS[:2] + [dict(cross_check=True), dict(ratio=0.0, cross_check=True),
                                   dict(max_dist2=float(np.median(F["dist_best"])), cross_check=True)]:
        assert A.match_pairs(B, **opts).tobytes() == expected_pairs(F, G, **opts).tobytes(), opts
    p = A.match_pairs(B, cross_check=True)
    k_ratio, _, k_cross = keep_masks(F, G, cross_check=True)
    assert (k_ratio & ~k_cross).any() and len(p) > 0.3 * len(da)
    ra, rb = A.download()[1], B.download()[1]
    pa = np.stack([fa["xpos"][ra], fa["ypos"][ra]], 1)[p["l"]]
    pb = np.stack([fb["xpos"][rb], fb["ypos"][rb]], 1)[p["r"]]
    ok = np.hypot(pb[:, 0] - pa[:, 0] - 5, pb[:, 1] - pa[:, 1] - 3) < 1.0
    assert ok.mean() > 0.9


def test_full_size_sets(gpu_hip):
    """20 k x 95 k descriptors of two unrelated 1080p images, where the reverse sweep is restricted to a small J.  The
    expected pairs are the rule applied to match_sets both ways (held to the oracle by tests/test_gpu_match.py)."""
    a = gpu_hip.Context().submit(synth(2, 1920, 1080))
    fa, da = a.fetch()
    b = gpu_hip.Context().submit(synth(102, 1920, 1080))
    A, B = gpu_hip.DevFeatures.from_host(da[:20000]), b.clone_results()
    F, G = A.match(B), B.match(A)
    acc = F["dist_best"][F["accept"] == 1]
    assert len(acc) > 2
    cap = float(np.median(acc))
    for opts in (dict(), dict(ratio=0.0, cross_check=True), dict(ratio=0.8, max_dist2=cap, cross_check=True)):
        want = expected_pairs(F, G, **opts)
        got = A.match_pairs(B, **opts)
        assert got.tobytes() == want.tobytes(), (opts, len(got), len(want))
    # and the other way round: 95 k left rows, most of the right set not a target
    want = expected_pairs(G, F, cross_check=True)
    assert B.match_pairs(A, cross_check=True).tobytes() == want.tobytes()


def test_sets_on_two_gpus(oracle_mod, gpu_hip):
    if gpu_hip.device_count() < 2:
        pytest.skip("one GPU")
    l, r = planted(2500, 3100)
    F, B = oracle_mod.match(l, r), oracle_mod.match(r, l)
    L, R = gpu_hip.DevFeatures.from_host(l, device=0), gpu_hip.DevFeatures.from_host(r, device=1)
    for opts in OPTION_SETS:
        assert L.match_pairs(R, **opts).tobytes() == expected_pairs(F, B, **opts).tobytes(), opts
        assert R.match_pairs(L, **opts).tobytes() == expected_pairs(B, F, **opts).tobytes(), opts
