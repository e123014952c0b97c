"""popsift_hip_match_bytes / popsift_hip_match_pairs_bytes on the GPU (match_u8.hip): byte for byte against the numpy rule
(tests/match_bytes_rule.py, pinned to the oracle by tests/test_match_bytes.py) and against the float matcher on the same
values as floats.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from match_bytes_rule import MATCH_DTYPE, match_rows, planted_bytes, position_coded
from match_pairs_rule import OPTION_SETS, expected_pairs, keep_masks
from popsift_amd.synth import synth
from test_gpu_match_pairs import SIZES as PAIR_SIZES
from test_match_bytes import byte_opts

pytestmark = pytest.mark.gpu

SIZES = PAIR_SIZES + [(129, 257), (4097, 130), (30000, 30000)]
BUILDERS = {"planted": planted_bytes, "coded": position_coded}


def raw_pairs(hip, L, R, cap, buf_len=None, null=False, **kw):
    """popsift_hip_match_pairs_bytes with a caller-chosen cap: (status, n_pairs, buffer filled with 0xff bytes first)"""
    buf = np.full(cap if buf_len is None else buf_len, -1, np.int32).repeat(4).view(hip.PAIR_DTYPE)
    opts = hip.MatchOpts(kw.get("ratio", 0.8), kw.get("max_dist2", np.inf), 1 if kw.get("cross_check") else 0, 0)
    n = C.c_int(-1)
    rc = hip.lib().popsift_hip_match_pairs_bytes(L._h, R._h, C.byref(opts), None if null else buf.ctypes.data, cap,
                                                 C.byref(n))
    return rc, n.value, buf


@pytest.mark.parametrize("nl,nr", SIZES)
@pytest.mark.parametrize("builder", sorted(BUILDERS))
def test_rows_and_pairs_equal_the_rule_and_the_float_matcher(gpu_hip, builder, nl, nr):
    hip = gpu_hip
    l, r = BUILDERS[builder](nl, nr)
    L, R = hip.ByteFeatures.from_host(l), hip.ByteFeatures.from_host(r)
    assert L.info() == (0, nl) and R.info() == (0, nr)
    F = match_rows(l, r)
    got = L.match(R)
    assert got.dtype == MATCH_DTYPE
    assert got.tobytes() == F.tobytes(), np.flatnonzero(got != F)[:8]
    # the float matcher on the same values (exact there too: integers below 2^24)
    LF, RF = hip.DevFeatures.from_host(l.astype(np.float32)), hip.DevFeatures.from_host(r.astype(np.float32))
    assert got.tobytes() == LF.match(RF).tobytes()
    B = match_rows(r, l)
    assert R.match(L).tobytes() == B.tobytes()
    for o in map(byte_opts, OPTION_SETS):
        want = expected_pairs(F, B, **o)
        pairs = L.match_pairs(R, **o)
        assert pairs.dtype == hip.PAIR_DTYPE
        assert pairs.tobytes() == want.tobytes(), (o, len(pairs), len(want))
    assert L.match(R).tobytes() == F.tobytes()                     # the rows are untouched by the pair calls
    d, rev = L.download()
    assert np.array_equal(d, l) and (rev == -1).all()


def test_the_cap_has_rows_on_both_sides():
    """the cap of the option sets, in byte units, keeps some rows and removes others in the sets above (CPU, from the rule)"""
    for nl, nr in ((100, 1000), (2500, 3100), (5000, 4000)):
        l, r = planted_bytes(nl, nr)
        F, B = match_rows(l, r), match_rows(r, l)
        _, k_cap, _ = keep_masks(F, B, **byte_opts(OPTION_SETS[2]))
        assert k_cap.any() and (~k_cap).any()


def test_cap_count_and_repeatability(gpu_hip):
    hip = gpu_hip
    l, r = planted_bytes(2500, 3100)
    F, B = match_rows(l, r), match_rows(r, l)
    L, R = hip.ByteFeatures.from_host(l), hip.ByteFeatures.from_host(r)
    before = L.match(R)
    for opts in map(byte_opts, (OPTION_SETS[0], OPTION_SETS[3], OPTION_SETS[4])):
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
    assert before.tobytes() == after.tobytes() == F.tobytes()
    # the right set as somebody's left set, and a set against itself
    assert R.match_pairs(L, ratio=0.0, cross_check=True).tobytes() == expected_pairs(B, F, ratio=0.0, cross_check=True).tobytes()
    S = match_rows(l, l)
    assert L.match(L).tobytes() == S.tobytes()
    assert (S["dist_best"] == 0).all() and S["best"][200] == 50                 # l[200] = l[50]: the lower index
    assert L.match_pairs(L, ratio=0.0, cross_check=True).tobytes() == expected_pairs(S, S, ratio=0.0, cross_check=True).tobytes()


def test_empty_sets_in_every_position(gpu_hip):
    hip = gpu_hip
    l, _ = position_coded(5, 1)
    E, L = hip.ByteFeatures.from_host(np.zeros((0, 128), np.uint8)), hip.ByteFeatures.from_host(l)
    assert E.info() == (0, 0) and E.download()[0].shape == (0, 128)
    assert len(E.match(L)) == 0 and len(E.match(E)) == 0
    want = np.array([(0, 0, 0, np.inf, np.inf)] * 5, MATCH_DTYPE)
    assert L.match(E).tobytes() == want.tobytes()
    # what the float matcher does with an empty right set
    LF, EF = hip.DevFeatures.from_host(l.astype(np.float32)), hip.DevFeatures.from_host(np.zeros((0, 128), np.float32))
    assert LF.match(EF).tobytes() == want.tobytes()
    for a, b in ((E, L), (L, E), (E, E)):
        for o in OPTION_SETS:
            assert len(a.match_pairs(b, **o)) == 0
    out = np.full(5, 7, np.int32).repeat(5).view(MATCH_DTYPE)
    assert hip.lib().popsift_hip_match_bytes(E._h, L._h, out.ctypes.data) == hip.OK
    assert (out.view(np.int32) == 7).all()                                      # an empty left set writes nothing
    assert hip.lib().popsift_hip_match_bytes(L._h, E._h, None) == hip.ERR_INVALID
    h = C.c_void_p()
    assert hip.lib().popsift_hip_bytefeatures_from_host(99, l.ctypes.data, 5, C.byref(h)) == hip.ERR_INVALID   # no such GPU
    # one right descriptor: second = 0, dist_second = inf, accepted (d / inf = 0)
    one = L.match(hip.ByteFeatures.from_host(l[2:3]))
    assert one.tobytes() == match_rows(l, l[2:3]).tobytes()
    assert (one["second"] == 0).all() and np.isinf(one["dist_second"]).all() and (one["accept"] == 1).all()


def test_sets_from_extraction(gpu_hip):
    """clone_results_u8 and from_set: the bytes of the byte fetch calls, the float clone's reverse map, and image-to-image
    matching of such sets against the rule on the downloaded bytes."""
    hip = gpu_hip
    a = synth(90, 320, 240)
    b = np.roll(a, (3, 5), axis=(0, 1))
    sets = []
    for img in (a, b):
        ctx = hip.Context(hip.default_params(norm_multi=9)).submit(img)
        _, fetched = ctx.fetch(fmt="u8")
        fl = ctx.clone_results()
        cl, fs = ctx.clone_results_u8(), hip.ByteFeatures.from_set(fl)
        assert len(fetched) > 500 and fetched.max() > 100
        for s in (cl, fs):
            d, rev = s.download()
            assert s.info() == (0, len(fetched))
            assert np.array_equal(d, fetched) and np.array_equal(d, fl.download_u8())
            assert np.array_equal(rev, fl.download()[1])
        ctx.fetch_begin().result()                                              # the results have left the context
        with pytest.raises(hip.PopsiftHipError) as e:
            ctx.clone_results_u8()
        assert e.value.status == hip.ERR_STATE
        sets.append((cl, fs, fetched))
    (A, A2, da), (B, B2, db) = sets
    F, G = match_rows(da, db), match_rows(db, da)
    assert A.match(B).tobytes() == F.tobytes() == A2.match(B2).tobytes()
    assert (F["accept"] == 1).mean() > 0.3
    for o in OPTION_SETS[:2] + [dict(cross_check=True), dict(ratio=0.0, cross_check=True),
                                dict(max_dist2=float(np.median(F["dist_best"])), cross_check=True)]:
        assert A.match_pairs(B2, **o).tobytes() == expected_pairs(F, G, **o).tobytes(), o
    # a batch: image k's own set
    ctx = hip.Context(hip.default_params(norm_multi=9)).submit_batch([a, b])
    by_row = lambda d: d[np.lexsort(d.T[::-1])]                                # the compaction order varies from run to run
    for k, want in enumerate((da, db)):
        assert np.array_equal(by_row(ctx.clone_results_u8(k).download()[0]), by_row(want))
    with pytest.raises(hip.PopsiftHipError) as e:
        ctx.clone_results_u8(2)
    assert e.value.status == hip.ERR_INVALID


def test_sets_on_two_gpus(gpu_hip):
    if gpu_hip.device_count() < 2:
        pytest.skip("one GPU")
    l, r = planted_bytes(2500, 3100)
    F, B = match_rows(l, r), match_rows(r, l)
    L, R = gpu_hip.ByteFeatures.from_host(l, device=0), gpu_hip.ByteFeatures.from_host(r, device=1)
    assert L.match(R).tobytes() == F.tobytes() and R.match(L).tobytes() == B.tobytes()
    for o in map(byte_opts, OPTION_SETS):
        assert L.match_pairs(R, **o).tobytes() == expected_pairs(F, B, **o).tobytes(), o
        assert R.match_pairs(L, **o).tobytes() == expected_pairs(B, F, **o).tobytes(), o
