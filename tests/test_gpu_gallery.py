"""popsift_hip_match_gallery / popsift_hip_match_pairs_gallery on the GPU (match_gallery.hip): byte for byte against the rule
(tests/gallery_rule.py: the per-pair rules member by member) and against the per-pair calls on the GPU.  Every comparison is
exact."""
import ctypes as C
import functools

import numpy as np
import pytest

from gallery_rule import BUILDERS, SIZES, expected, planted_gallery
from match_bytes_rule import MATCH_DTYPE, match_rows
from match_pairs_rule import OPTION_SETS, expected_pairs
from popsift_amd.synth import synth
from test_match_bytes import byte_opts

pytestmark = pytest.mark.gpu

OPTS = [byte_opts(o) for o in OPTION_SETS]


@functools.lru_cache(maxsize=None)
def case(builder, nl):
    """(l, members, rows, [(pairs, offsets) per option set]) of the rule, computed once and never written to"""
    l, members = BUILDERS[builder](nl, SIZES)
    rows = expected(l, members)[0]
    return l, members, rows, [expected(l, members, **o)[1:] for o in OPTS]


def gallery_of(hip, members, device=0):
    g = hip.Gallery(device)
    for k, r in enumerate(members):
        assert g.add(r) == k
    return g


def per_pair(hip, L, members, **o):
    """what the loop over the per-pair calls returns, in the gallery's form"""
    pairs, offsets = [], [0]
    for r in members:
        pairs.append(L.match_pairs(hip.ByteFeatures.from_host(r), **o))
        offsets.append(offsets[-1] + len(pairs[-1]))
    return np.concatenate(pairs), np.array(offsets, np.int32)


def raw_pairs(hip, L, g, cap, buf_len=None, null=False, **kw):
    """popsift_hip_match_pairs_gallery with a caller-chosen cap: (status, n_pairs, 0xff-filled buffer, offsets)"""
    buf = np.full(cap if buf_len is None else buf_len, -1, np.int32).repeat(4).view(hip.PAIR_DTYPE)
    offsets = np.full(g.info()[1] + 1, -1, np.int32)
    opts = hip.MatchOpts(kw.get("ratio", 0.8), kw.get("max_dist2", np.inf), 1 if kw.get("cross_check") else 0, 0)
    n = C.c_int(-1)
    rc = hip.lib().popsift_hip_match_pairs_gallery(L._h, g._h, C.byref(opts), None if null else buf.ctypes.data, cap,
                                                   offsets.ctypes.data, C.byref(n))
    return rc, n.value, buf, offsets


def check_all(hip, L, g, rows, by_set):
    got = g.match(L)
    assert got.dtype == MATCH_DTYPE and got.shape == rows.shape
    assert got.tobytes() == rows.tobytes(), np.argwhere(got != rows)[:8]
    for o, (pairs, offsets) in zip(OPTS, by_set):
        p, off = g.match_pairs(L, **o)
        assert p.dtype == hip.PAIR_DTYPE and off.dtype == np.int32
        assert off.tobytes() == offsets.tobytes(), (o, off, offsets)
        assert p.tobytes() == pairs.tobytes(), o
        assert np.array_equal(g.counts(L, **o), np.diff(offsets))


@pytest.mark.parametrize("nl", [1, 33, 129, 700])
@pytest.mark.parametrize("builder", sorted(BUILDERS))
def test_rows_and_pairs_equal_the_rule_and_the_per_pair_calls(gpu_hip, builder, nl):
    hip = gpu_hip
    l, members, rows, by_set = case(builder, nl)
    L = hip.ByteFeatures.from_host(l)
    R = hip.ByteFeatures.from_host(members[7])
    before = L.match(R)
    g = gallery_of(hip, members)
    assert g.info() == (0, len(SIZES), sum(SIZES))
    first = 0
    for m, r in enumerate(members):
        assert g.member(m) == (first, len(r))
        assert np.array_equal(g.download(m), r)
        first += len(r)
    check_all(hip, L, g, rows, by_set)
    got = g.match(L)
    for m, r in enumerate(members):                                  # the per-pair call on the GPU, member by member
        assert got[m].tobytes() == L.match(hip.ByteFeatures.from_host(r)).tobytes(), m
    assert L.match(R).tobytes() == before.tobytes() == rows[7].tobytes()   # l's own scratch and rows are untouched


@pytest.mark.parametrize("builder", sorted(BUILDERS))
def test_group_edges_do_not_change_the_bytes(gpu_hip, builder):
    """rows of a group at l_len = 129: every member alone; exactly one member; one member and no room for the next; two
    members; the default"""
    hip = gpu_hip
    l, members, rows, by_set = case(builder, 129)
    L, g = hip.ByteFeatures.from_host(l), gallery_of(hip, members)
    for group_rows in (1, 129, 130, 2 * 129 + 1, 0):
        g.set_group_rows(group_rows)
        check_all(hip, L, g, rows, by_set)
    with pytest.raises(hip.PopsiftHipError) as e:
        g.set_group_rows(-1)
    assert e.value.status == hip.ERR_INVALID


def test_growth_keeps_earlier_members(gpu_hip):
    hip = gpu_hip
    l, members, rows, by_set = case("planted", 129)
    L = hip.ByteFeatures.from_host(l)
    # the first allocation holds 1024 descriptors: the first three members (256) fit, all nine (2029) do not
    assert sum(SIZES[:3]) < 1024 < sum(SIZES)
    g = hip.Gallery()
    for r in members[:3]:
        g.add(hip.ByteFeatures.from_host(r))                          # from a set on the device
    rows3 = g.match(L)
    assert rows3.tobytes() == rows[:3].tobytes()
    pairs3 = [g.match_pairs(L, **o) for o in OPTS]
    for r in members[3:]:
        g.add(r)                                                      # from host bytes
    assert g.info() == (0, len(SIZES), sum(SIZES))
    assert g.match(L).tobytes() == rows.tobytes()
    one_go = gallery_of(hip, [hip.ByteFeatures.from_host(r) for r in members])
    assert one_go.match(L).tobytes() == rows.tobytes()
    for o, (p3, off3), (pairs, offsets) in zip(OPTS, pairs3, by_set):
        p, off = g.match_pairs(L, **o)
        assert np.array_equal(off[:4], off3) and p[:off[3]].tobytes() == p3.tobytes()
        assert np.array_equal(off, offsets) and p.tobytes() == pairs.tobytes()
        q, qoff = one_go.match_pairs(L, **o)
        assert q.tobytes() == p.tobytes() and np.array_equal(qoff, off)
    for m, r in enumerate(members):
        assert np.array_equal(g.download(m), r) and np.array_equal(one_go.download(m), r)


def test_cap_count_and_offsets(gpu_hip):
    hip = gpu_hip
    l, members, rows, by_set = case("planted", 700)
    L, g = hip.ByteFeatures.from_host(l), gallery_of(hip, members)
    n_rows = len(members) * len(l)
    for o, (want, offsets) in zip(OPTS, by_set):
        total = len(want)
        assert total > 2
        rc, n, buf, off = raw_pairs(hip, L, g, total, **o)                       # cap = total: fits
        assert (rc, n) == (hip.OK, total) and buf.tobytes() == want.tobytes() and np.array_equal(off, offsets)
        rc, n, buf, off = raw_pairs(hip, L, g, total - 1, buf_len=total, **o)    # one short: the count, the first cap pairs
        assert (rc, n) == (hip.ERR_TOO_SMALL, total) and np.array_equal(off, offsets)
        assert buf[:total - 1].tobytes() == want[:total - 1].tobytes()
        assert buf[total - 1:].tobytes() == b"\xff" * 16                         # nothing past cap
        rc, n, _, off = raw_pairs(hip, L, g, 0, null=True, **o)                  # the counts alone
        assert (rc, n) == (hip.ERR_TOO_SMALL, total) and np.array_equal(off, offsets)
        rc, n, buf, off = raw_pairs(hip, L, g, n_rows, **o)                      # n_members x l_len is always enough
        assert (rc, n) == (hip.OK, total) and buf[:total].tobytes() == want.tobytes() and np.array_equal(off, offsets)
        assert buf[total:].tobytes() == b"\xff" * 16 * (n_rows - total)
    out = np.full(n_rows, 7, np.int32).repeat(5).view(MATCH_DTYPE)
    assert hip.lib().popsift_hip_match_gallery(L._h, g._h, out.ctypes.data, n_rows - 1) == hip.ERR_TOO_SMALL
    assert (out.view(np.int32) == 7).all()                                       # all or nothing
    assert hip.lib().popsift_hip_match_gallery(L._h, g._h, None, n_rows) == hip.ERR_INVALID
    assert hip.lib().popsift_hip_match_gallery(L._h, g._h, out.ctypes.data, n_rows) == hip.OK
    assert out.tobytes() == rows.tobytes()


@pytest.mark.parametrize("sizes", [[130, 4000, 5000], [5000]])
def test_split_members_equal_the_per_pair_calls(gpu_hip, sizes):
    """Few members: every member's right tiles are split over several workgroups.  The per-pair calls on the GPU are the
    yardstick at this size."""
    hip = gpu_hip
    l, members = planted_gallery(4097, sizes)
    L, g = hip.ByteFeatures.from_host(l), gallery_of(hip, members)
    got = g.match(L)
    for m, r in enumerate(members):
        assert got[m].tobytes() == L.match(hip.ByteFeatures.from_host(r)).tobytes(), m
    for o in OPTS:
        want, offsets = per_pair(hip, L, members, **o)
        assert len(want) > 0
        p, off = g.match_pairs(L, **o)
        assert np.array_equal(off, offsets) and p.tobytes() == want.tobytes(), o


def test_empty_cases(gpu_hip):
    hip = gpu_hip
    l, members, rows, by_set = case("planted", 129)
    L, E = hip.ByteFeatures.from_host(l), hip.ByteFeatures.from_host(np.zeros((0, 128), np.uint8))
    g = gallery_of(hip, members)
    # an empty query
    assert g.match(E).shape == (len(SIZES), 0)
    for o in OPTS:
        p, off = g.match_pairs(E, **o)
        assert len(p) == 0 and (off == 0).all() and len(off) == len(SIZES) + 1
    # a gallery without members
    none = hip.Gallery()
    assert none.info() == (0, 0, 0) and none.match(L).shape == (0, 129)
    p, off = none.match_pairs(L)
    assert len(p) == 0 and off.tolist() == [0]
    # only empty members: one from a set, one from the host
    empties = hip.Gallery()
    assert empties.add(E) == 0 and empties.add(np.zeros((0, 128), np.uint8)) == 1
    assert empties.info() == (0, 2, 0) and empties.member(1) == (0, 0) and empties.download(1).shape == (0, 128)
    want = np.array([(0, 0, 0, np.inf, np.inf)] * 129, MATCH_DTYPE)
    got = empties.match(L)
    assert got[0].tobytes() == got[1].tobytes() == want.tobytes()
    for o in OPTS + [dict(ratio=0.0)]:                               # ratio 0 and no cap: only condition 1 removes the rows
        p, off = empties.match_pairs(L, **o)
        assert len(p) == 0 and off.tolist() == [0, 0, 0]
    # ... and an empty member among others under the same options
    p, off = g.match_pairs(L, ratio=0.0)
    assert np.array_equal(np.diff(off), [129 if n else 0 for n in SIZES])
    # the query as a member, behind an empty one
    own = gallery_of(hip, [members[4], l])
    S = match_rows(l, l)
    got = own.match(L)[1]
    assert got.tobytes() == S.tobytes()
    assert (got["dist_best"] == 0).all() and (got["best"] <= np.arange(129)).all()   # the lowest equal index
    p, off = own.match_pairs(L, ratio=0.0, cross_check=True)
    assert p.tobytes() == expected_pairs(S, S, ratio=0.0, cross_check=True).tobytes() and off[1] == 0


def test_sets_from_extraction(gpu_hip):
    hip = gpu_hip
    a = synth(90, 320, 240)
    imgs = [a, np.roll(a, (3, 5), axis=(0, 1)), synth(17, 320, 240)]
    sets = []
    for img in imgs:
        sets.append(hip.Context(hip.default_params(norm_multi=9)).submit(img).clone_results_u8())
        assert sets[-1].info()[1] > 300
    Q, gallery = sets[0], [sets[2], sets[1]]                         # the unrelated image, then the rolled copy
    g = hip.Gallery()
    for s in gallery:
        g.add(s)
    rows = g.match(Q)
    for m, s in enumerate(gallery):
        assert rows[m].tobytes() == Q.match(s).tobytes()
    for o in OPTION_SETS[:2] + [dict(cross_check=True), dict(ratio=0.0, cross_check=True)]:
        p, off = g.match_pairs(Q, **o)
        want = [Q.match_pairs(s, **o) for s in gallery]
        assert np.array_equal(np.diff(off), [len(w) for w in want])
        assert p.tobytes() == np.concatenate(want).tobytes(), o
        assert off[2] - off[1] > off[1] - off[0]                     # the rolled copy has the most pairs


def test_gallery_and_query_on_two_gpus(gpu_hip):
    if gpu_hip.device_count() < 2:
        pytest.skip("one GPU")
    hip = gpu_hip
    l, members, rows, by_set = case("planted", 129)
    L = hip.ByteFeatures.from_host(l, device=1)
    g = hip.Gallery(0)
    for r in members:
        g.add(hip.ByteFeatures.from_host(r, device=1))
    check_all(hip, L, g, rows, by_set)
