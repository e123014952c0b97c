"""popsift_hip_match_links / popsift_hip_match_pairs_links / popsift_hip_gallery_link_points on the GPU (match_links.hip): byte
for byte against the rule (tests/links_rule.py: the per-pair rules link by link) and against the per-pair calls on the GPU.
Every comparison is exact."""
import ctypes as C
import functools

import numpy as np
import pytest

from gallery_rule import SIZES, planted_gallery
from links_rule import EMPTY, EMPTY_LEFT, EMPTY_RUN, MEMBERS, ORDERED, REPEATED, expected_links, left_rows
from match_bytes_rule import MATCH_DTYPE
from match_pairs_rule import OPTION_SETS
from test_match_bytes import byte_opts

pytestmark = pytest.mark.gpu

OPTS = [byte_opts(o) for o in OPTION_SETS]


@functools.lru_cache(maxsize=None)
def rule(links):
    """(rows, [(pairs, offsets) per option set]) of the rule for a tuple of links, computed once and never written to"""
    rows = expected_links(MEMBERS, links)[0]
    return rows, [expected_links(MEMBERS, links, **o)[1:] for o in OPTS]


def gallery_of(hip, members):
    g = hip.Gallery()
    for k, r in enumerate(members):
        assert g.add(r) == k
    return g


@pytest.fixture(scope="module")
def planted(gpu_hip):
    """the gallery of links_rule.MEMBERS and its members as byte sets for the per-pair calls"""
    g = gallery_of(gpu_hip, MEMBERS)
    yield g, [gpu_hip.ByteFeatures.from_host(r) for r in MEMBERS]
    g.close()


def check_rule(hip, g, links):
    links = tuple(links)
    rows, by_set = rule(links)
    got = g.match_links(links)
    assert got.dtype == MATCH_DTYPE and got.shape == rows.shape
    assert got.tobytes() == rows.tobytes(), np.flatnonzero(got != rows)[:8]
    for o, (pairs, offsets) in zip(OPTS, by_set):
        p, off = g.match_pairs_links(links, **o)
        assert p.dtype == hip.PAIR_DTYPE and off.dtype == np.int32
        assert off.tobytes() == offsets.tobytes(), (o, off, offsets)
        assert p.tobytes() == pairs.tobytes(), o
        assert np.array_equal(g.link_counts(links, **o), np.diff(offsets))


def per_pair(sets, links, **o):
    """what the loop over the per-pair calls returns, in the links' form"""
    rows, pairs, offsets = [np.zeros(0, MATCH_DTYPE)], [], [0]
    for a, b in links:
        rows.append(sets[a].match(sets[b]))
        pairs.append(sets[a].match_pairs(sets[b], **o))
        offsets.append(offsets[-1] + len(pairs[-1]))
    return np.concatenate(rows), np.concatenate(pairs), np.array(offsets, np.int32)


def raw_pairs(hip, g, links, cap, buf_len=None, null=False, **kw):
    """popsift_hip_match_pairs_links with a caller-chosen cap: (status, n_pairs, 0xff-filled buffer, offsets)"""
    links = hip.as_links(links)
    buf = np.full(cap if buf_len is None else buf_len, -1, np.int32).repeat(4).view(hip.PAIR_DTYPE)
    offsets = np.full(len(links) + 1, -1, np.int32)
    opts = hip.MatchOpts(kw.get("ratio", 0.8), kw.get("max_dist2", np.inf), 1 if kw.get("cross_check") else 0, 0)
    n = C.c_int(-1)
    rc = hip.lib().popsift_hip_match_pairs_links(g._h, links.ctypes.data, len(links), C.byref(opts),
                                                 None if null else buf.ctypes.data, cap, offsets.ctypes.data, C.byref(n))
    return rc, n.value, buf, offsets


def test_all_ordered_links_equal_the_rule_and_the_per_pair_calls(gpu_hip, planted):
    hip = gpu_hip
    g, sets = planted
    check_rule(hip, g, ORDERED)
    got = g.match_links(ORDERED)
    for o in OPTS:
        rows, pairs, offsets = per_pair(sets, ORDERED, **o)
        assert got.tobytes() == rows.tobytes()
        p, off = g.match_pairs_links(ORDERED, **o)
        assert off.tobytes() == offsets.tobytes() and p.tobytes() == pairs.tobytes(), o
    assert g.match_pairs_links(ORDERED)[0].tobytes() == g.match_pairs_links(ORDERED)[0].tobytes()


@pytest.mark.parametrize("links", [ORDERED[::-1], REPEATED], ids=["reversed", "repeated"])
def test_order_and_repeats(gpu_hip, planted, links):
    check_rule(gpu_hip, planted[0], links)
    if links is REPEATED:
        p, off = planted[0].match_pairs_links(links, cross_check=True)
        assert off[1] > 0 and p[off[0]:off[1]].tobytes() == p[off[2]:off[3]].tobytes() == p[off[4]:off[5]].tobytes()


@pytest.mark.parametrize("name", sorted(EMPTY_LEFT))
def test_links_with_an_empty_left_member(gpu_hip, planted, name):
    """such a link has no row and so nothing on the device that could write its offset"""
    links = EMPTY_LEFT[name]
    g = planted[0]
    check_rule(gpu_hip, g, links)
    for group_rows in (1, 0):
        g.set_group_rows(group_rows)
        for o in OPTS:
            off = g.match_pairs_links(links, **o)[1]
            assert (np.diff(off) >= 0).all() and off.tobytes() == rule(tuple(links))[1][OPTS.index(o)][1].tobytes()
    rc, n, _, off = raw_pairs(gpu_hip, g, links, 0, null=True)
    assert rc == (gpu_hip.OK if name == "only" else gpu_hip.ERR_TOO_SMALL) and n == off[-1] and (np.diff(off) >= 0).all()


def test_group_edges_do_not_change_the_bytes(gpu_hip, planted):
    """Left rows of EMPTY_RUN: 129, 127, 0, 0, 0, 1000, 257.  Every link with rows alone; exactly the first link; one row
    short of it and one more; the first two links and one row; the first two links exactly, which puts the edge at the run
    of empty-left links (they add no rows, so the run closes the group); the default.  Then the lists that start with, end
    with and consist of such links, every link with rows alone."""
    hip, g = gpu_hip, planted[0]
    first, second = left_rows(EMPTY_RUN)[:2]
    assert left_rows(EMPTY_RUN)[2:5] == [0, 0, 0]
    try:
        for group_rows in (1, first, first - 1, first + 1, first + second + 1, first + second, 0):
            g.set_group_rows(group_rows)
            check_rule(hip, g, EMPTY_RUN)
        for group_rows in (1, 1000, 0):
            g.set_group_rows(group_rows)
            check_rule(hip, g, ORDERED)
    finally:
        g.set_group_rows(0)


def test_split_members_equal_the_per_pair_calls(gpu_hip):
    """Few items: every link's right tiles are split over several workgroups, in both sweeps.  The per-pair calls on the GPU
    are the yardstick at this size."""
    hip = gpu_hip
    members = planted_gallery(4097, [130, 4000, 5000])[1]
    links = [(0, 1), (1, 2), (2, 1), (2, 2)]
    g, sets = gallery_of(hip, members), [hip.ByteFeatures.from_host(r) for r in members]
    got = g.match_links(links)
    for o in OPTS:
        rows, pairs, offsets = per_pair(sets, links, **o)
        assert got.tobytes() == rows.tobytes()
        assert len(pairs) > 0
        p, off = g.match_pairs_links(links, **o)
        assert np.array_equal(off, offsets) and p.tobytes() == pairs.tobytes(), o
    g.close()


def test_cap_count_and_offsets(gpu_hip, planted):
    hip, g = gpu_hip, planted[0]
    links = tuple(ORDERED)
    n_rows = sum(left_rows(links))
    rows, by_set = rule(links)
    for o, (want, offsets) in zip(OPTS, by_set):
        total = len(want)
        assert total > 2
        rc, n, buf, off = raw_pairs(hip, g, links, total, **o)                     # cap = total: fits
        assert (rc, n) == (hip.OK, total) and buf.tobytes() == want.tobytes() and np.array_equal(off, offsets)
        rc, n, buf, off = raw_pairs(hip, g, links, total - 1, buf_len=total, **o)  # one short: the count, the first cap pairs
        assert (rc, n) == (hip.ERR_TOO_SMALL, total) and np.array_equal(off, offsets)
        assert buf[:total - 1].tobytes() == want[:total - 1].tobytes()
        assert buf[total - 1:].tobytes() == b"\xff" * 16                           # nothing past cap
        rc, n, _, off = raw_pairs(hip, g, links, 0, null=True, **o)                # the counts alone
        assert (rc, n) == (hip.ERR_TOO_SMALL, total) and np.array_equal(off, offsets)
        rc, n, buf, off = raw_pairs(hip, g, links, n_rows, **o)                    # R[n_links] is always enough
        assert (rc, n) == (hip.OK, total) and buf[:total].tobytes() == want.tobytes() and np.array_equal(off, offsets)
        assert buf[total:].tobytes() == b"\xff" * 16 * (n_rows - total)
    l = hip.as_links(links)
    out = np.full(n_rows, 7, np.int32).repeat(5).view(MATCH_DTYPE)
    assert hip.lib().popsift_hip_match_links(g._h, l.ctypes.data, len(l), out.ctypes.data, n_rows - 1) == hip.ERR_TOO_SMALL
    assert (out.view(np.int32) == 7).all()                                         # all or nothing
    assert hip.lib().popsift_hip_match_links(g._h, l.ctypes.data, len(l), None, n_rows) == hip.ERR_INVALID
    assert hip.lib().popsift_hip_match_links(g._h, l.ctypes.data, len(l), out.ctypes.data, n_rows) == hip.OK
    assert out.tobytes() == rows.tobytes()
    bad = hip.as_links([(0, 1), (1, len(SIZES))])
    assert hip.lib().popsift_hip_match_links(g._h, bad.ctypes.data, 2, out.ctypes.data, n_rows) == hip.ERR_INVALID
    with pytest.raises(hip.PopsiftHipError) as e:
        g.match_pairs_links([(0, 1), (1, len(SIZES))])
    assert e.value.status == hip.ERR_INVALID


def test_growth_keeps_earlier_links(gpu_hip):
    hip = gpu_hip
    # the first allocation holds 1024 descriptors: the first seven members (645) fit, all nine (2029) do not
    assert sum(SIZES[:7]) < 1024 < sum(SIZES)
    g = gallery_of(hip, MEMBERS[:7])
    old = tuple((a, b) for a, b in ORDERED if a < 7 and b < 7)
    rows7 = g.match_links(old)
    pairs7 = [g.match_pairs_links(old, **o) for o in OPTS]
    check_rule(hip, g, old)
    for r in MEMBERS[7:]:
        g.add(r)
    assert g.match_links(old).tobytes() == rows7.tobytes()
    for o, (p7, off7) in zip(OPTS, pairs7):
        p, off = g.match_pairs_links(old, **o)
        assert p.tobytes() == p7.tobytes() and off.tobytes() == off7.tobytes()
    check_rule(hip, g, tuple((a, b) for a, b in ORDERED if a >= 7 or b >= 7))      # links into the new members
    g.close()


def test_the_query_path_is_untouched(gpu_hip, planted):
    hip, (g, sets) = gpu_hip, planted
    L = hip.ByteFeatures.from_host(planted_gallery(700, SIZES)[0])
    for o in OPTS:
        rows, (p, off) = g.match(L), g.match_pairs(L, **o)
        g.match_links(ORDERED)
        g.match_pairs_links(ORDERED, **o)
        p2, off2 = g.match_pairs(L, **o)
        assert g.match(L).tobytes() == rows.tobytes() and p2.tobytes() == p.tobytes() and off2.tobytes() == off.tobytes()
        assert len(p) > 0


def point_sets(hip, n=400, seed=5):
    """Four views of one plane: view k holds the base points under a known homography, in an order of its own, with the
    base descriptors under a little noise; a quarter of every view is unrelated clutter.  -> (float sets, xy, Hs)"""
    rng = np.random.default_rng(seed)
    scale = np.float32(200)                                          # descriptors in byte units, as norm_multi = 9 leaves them
    base = rng.random((n, 128), np.float32) * scale
    xy0 = (rng.random((n, 2)) * [600, 440] + 20).astype(np.float64)
    Hs = [np.eye(3), np.array([[0.98, -0.05, 12.0], [0.04, 1.01, -7.0], [1e-5, -2e-5, 1.0]]),
          np.array([[1.05, 0.02, -20.0], [-0.03, 0.97, 15.0], [-3e-5, 1e-5, 1.0]]),
          np.array([[0.9, 0.1, 30.0], [-0.1, 0.9, 40.0], [2e-5, 2e-5, 1.0]])]
    sets, xys = [], []
    for k, H in enumerate(Hs):
        order = rng.permutation(n)[:n - 17 * k]                      # views of different sizes
        q = np.c_[xy0[order], np.ones(len(order))] @ H.T
        xy = (q[:, :2] / q[:, 2:3]).astype(np.float32)
        d = base[order] + rng.normal(0, 2.0, (len(order), 128)).astype(np.float32)
        clutter = len(order) // 4
        d[:clutter] = rng.random((clutter, 128), np.float32) * scale
        sets.append(hip.DevFeatures.from_host_points(np.clip(d, 0, None), xy))
        xys.append(xy)
    return sets, xys, Hs


def test_link_points_equal_the_per_pair_points(gpu_hip):
    hip, lib = gpu_hip, gpu_hip.lib()
    sets, xys, _ = point_sets(hip)
    g = hip.Gallery()
    assert [g.add_set(s) for s in sets] == [0, 1, 2, 3]
    assert g.add(sets[1].download_u8()) == 4                          # the bytes of view 1, without positions
    assert g.add_set(hip.DevFeatures.from_host_points(np.zeros((0, 128), np.float32), np.zeros((0, 2), np.float32))) == 5
    links = [(a, b) for a in range(4) for b in range(4)] + [(5, 1), (2, 5)]
    pairs, off = g.match_pairs_links(links, cross_check=True)
    pts = g.link_points(links, pairs, off)
    assert pts.shape == (len(pairs), 4) and pts.dtype == np.float32
    for e, (a, b) in enumerate(links):
        p = pairs[off[e]:off[e + 1]]
        assert (len(p) > 100) == (a < 4 and b < 4), (a, b, len(p))
        if a < 4 and b < 4:
            assert pts[off[e]:off[e + 1]].tobytes() == sets[a].pair_points(sets[b], p).tobytes(), (a, b)
            assert pts[off[e]:off[e + 1]].tobytes() == np.c_[xys[a][p["l"]], xys[b][p["r"]]].tobytes(), (a, b)
    # a link that touches the member without positions: refused with pairs, accepted without
    for bad in ([(0, 4)], [(4, 0)], [(4, 4)]):
        p, o = g.match_pairs_links(bad, cross_check=True)
        assert len(p) > 100
        out = np.full((len(p), 4), 7.0, np.float32)
        l = hip.as_links(bad)
        assert lib.popsift_hip_gallery_link_points(g._h, l.ctypes.data, 1, p.ctypes.data, o.ctypes.data,
                                                   out.ctypes.data) == hip.ERR_INVALID and (out == 7.0).all()
        assert g.link_points(bad, p[:0], np.zeros(2, np.int32)).shape == (0, 4)
    g.close()


def test_a_collection_verified_end_to_end(gpu_hip):
    """matching plus verification of an image collection in three calls"""
    hip = gpu_hip
    sets, xys, Hs = point_sets(hip)
    g = hip.Gallery()
    for s in sets:
        g.add_set(s)
    links = hip.all_links(4)
    pairs, off = g.match_pairs_links(links, cross_check=True)
    pts = g.link_points(links, pairs, off)
    v = hip.Verifier()
    max_err = 1.0
    res, mask = v.ransac_many(pts, off, "homography", 256, max_err, 3)
    assert len(res) == len(links) == 6
    for e, (a, b) in enumerate(links.tolist()):
        p = pairs[off[e]:off[e + 1]]
        one, one_mask = v.ransac(sets[a].pair_points(sets[b], p), "homography", 256, max_err, 3)
        assert res[e].tobytes() == one.tobytes() and mask[off[e]:off[e + 1]].tobytes() == one_mask.tobytes(), (a, b)
        # a base point is a real (non-clutter) point of view k with probability 0.75 n_k / 400: the two smallest views
        # expect 0.75^2 x 366 x 349 / 400 = 180 common points, every other link more; half of that must be inliers
        assert res[e]["n_inliers"] >= 90 and res[e]["n_inliers"] == mask[off[e]:off[e + 1]].sum()
        # the model is the planted one: H_b H_a^-1 moves a's points onto b's, here in float64
        Hab = Hs[b] @ np.linalg.inv(Hs[a])
        got = res[e]["H"].astype(np.float64).reshape(3, 3)
        probe = np.array([[50.0, 60.0, 1.0], [600.0, 80.0, 1.0], [320.0, 400.0, 1.0]])
        q1, q2 = probe @ Hab.T, probe @ got.T
        assert np.abs(q1[:, :2] / q1[:, 2:3] - q2[:, :2] / q2[:, 2:3]).max() < max_err
    v.close()
    g.close()
