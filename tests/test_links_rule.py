"""popsift_hip_match_links / popsift_hip_match_pairs_links / popsift_hip_gallery_link_points without a GPU: the new symbols,
the argument checks of the C ABI (made before any GPU call), and the link lists of tests/links_rule.py doing the job the
GPU tests give them."""
import ctypes as C

import numpy as np

from gallery_rule import SIZES
from links_rule import ALL_PAIRS, EMPTY, EMPTY_LEFT, EMPTY_RUN, MEMBERS, ORDERED, REPEATED, expected_links, left_rows
from match_pairs_rule import OPTION_SETS
from test_match_bytes import byte_opts

NEW = ["popsift_hip_match_links", "popsift_hip_match_pairs_links", "popsift_hip_gallery_link_points"]


def test_new_symbols_are_exported_and_bound(hip):
    bound = {n for n, _, _ in hip.SYMBOLS}
    for n in NEW:
        assert n in bound and hasattr(hip.lib(), n), n
    for m in ("match_links", "match_pairs_links", "link_counts", "link_points"):
        assert callable(getattr(hip.Gallery, m))
    assert hip.LINK_DTYPE.itemsize == 8 and hip.LINK_DTYPE.names == ("a", "b")


def test_link_list_helpers(hip):
    assert hip.all_links(4).tolist() == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert hip.all_links(9).tolist() == ALL_PAIRS and len(hip.all_links(64)) == 2016
    assert len(hip.all_links(1)) == len(hip.all_links(0)) == 0 and hip.all_links(1).dtype == hip.LINK_DTYPE
    assert hip.sequential_links(4, 2).tolist() == [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)]
    assert hip.sequential_links(3, 5).tolist() == [(0, 1), (0, 2), (1, 2)]
    assert len(hip.sequential_links(256, 4)) == 4 * 256 - 10 and len(hip.sequential_links(5, 0)) == 0
    assert hip.as_links([(3, 1)]).tobytes() == np.array([3, 1], np.int32).tobytes()


def fake_gallery(hip, counts):
    """A block of zeros stands in for a gallery without members.  With `counts`, the three host tables of the record are
    filled in as well -- members that have rows on no GPU -- for the checks that need members; such a block only ever
    goes into calls that are rejected, or answered, before any GPU call."""
    g = C.create_string_buffer(512)
    if not counts:
        return g, ()
    n = len(counts)
    first = (C.c_int64 * n)(*np.concatenate([[0], np.cumsum(counts)[:-1]]).tolist())
    count = (C.c_int * n)(*counts)
    has_xy = (C.c_uint8 * n)(*([1] * (n - 1) + [0]))                  # the last member has no positions
    # devfeatures.h: int device, n_members; int64 n_desc; d_desc, d_norm; cap; first, count, has_xy
    C.c_int.from_buffer(g, 4).value = n
    C.c_int64.from_buffer(g, 8).value = int(sum(counts))
    for k, tab in enumerate((first, count, has_xy)):
        C.c_void_p.from_buffer(g, 40 + 8 * k).value = C.addressof(tab)
    return g, (first, count, has_xy)


def default_opts(hip, **kw):
    o = hip.MatchOpts()
    hip.lib().popsift_hip_default_match_opts(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_invalid_arguments_are_rejected_without_a_gpu(hip):
    lib = hip.lib()
    g, _ = fake_gallery(hip, [])
    links = hip.as_links([(0, 0), (0, 0)])
    out = np.full(4, 7, np.int32).repeat(5).view(hip.MATCH_DTYPE)
    pairs = np.full(4, 7, np.int32).repeat(4).view(hip.PAIR_DTYPE)
    offsets = np.full(4, -1, np.int32)
    pts = np.full((4, 4), 7, np.float32)
    n = C.c_int(-1)

    def rows(g=g, links=links.ctypes.data, n_links=0, out=out.ctypes.data, cap=4):
        return lib.popsift_hip_match_links(g, links, n_links, out, cap)

    def prs(opts, g=g, links=links.ctypes.data, n_links=0, pairs=pairs.ctypes.data, cap=4, offsets=offsets.ctypes.data,
            n_pairs=C.byref(n)):
        return lib.popsift_hip_match_pairs_links(g, links, n_links, C.byref(opts) if opts is not None else None, pairs, cap,
                                                 offsets, n_pairs)

    def points(g=g, links=links.ctypes.data, n_links=0, pairs=pairs.ctypes.data, offsets=offsets.ctypes.data,
               pts=pts.ctypes.data):
        return lib.popsift_hip_gallery_link_points(g, links, n_links, pairs, offsets, pts)

    o = default_opts(hip)
    # n_links == 0: OK, one offset, no pairs, no rows
    assert rows() == hip.OK and rows(links=None, out=None, cap=0) == hip.OK
    assert prs(o) == hip.OK and n.value == 0 and offsets.tolist() == [0, -1, -1, -1]
    n.value, offsets[0] = -1, -1
    assert prs(o, links=None, pairs=None, cap=0) == hip.OK and n.value == 0 and offsets.tolist() == [0, -1, -1, -1]
    assert points() == hip.OK and points(links=None, pairs=None, pts=None) == hip.OK
    n.value, offsets[0] = -1, -1

    # what is rejected whatever the gallery holds
    assert rows(g=None) == prs(o, g=None) == points(g=None) == hip.ERR_INVALID
    assert prs(None) == prs(o, offsets=None) == prs(o, n_pairs=None) == points(offsets=None) == hip.ERR_INVALID
    assert prs(o, pairs=None) == hip.ERR_INVALID                     # cap > 0 without a buffer
    for bad in (-1, (1 << 20) + 1):
        assert rows(n_links=bad) == prs(o, n_links=bad) == points(n_links=bad) == hip.ERR_INVALID
    assert rows(links=None, n_links=1) == prs(o, links=None, n_links=1) == points(links=None, n_links=1) == hip.ERR_INVALID
    # no members: every index is out of range
    assert rows(n_links=1) == prs(o, n_links=2) == points(n_links=1) == hip.ERR_INVALID
    for kw in (dict(ratio=-0.1), dict(ratio=float("nan")), dict(ratio=float("inf")), dict(max_dist2=float("nan")),
               dict(reserved=1), dict(cross_check=2), dict(cross_check=-1)):
        assert prs(default_opts(hip, **kw)) == hip.ERR_INVALID, kw
    offsets[0] = 1
    assert points() == hip.ERR_INVALID                               # offsets[0] != 0

    # a gallery with members (their rows are never touched): 3, 0 and 5 descriptors, the last without positions
    g, keep = fake_gallery(hip, [3, 0, 5])
    for bad in ([(0, 3)], [(3, 0)], [(-1, 0)], [(0, -1)], [(0, 1), (1, 2), (2, 5)]):
        l = hip.as_links(bad)
        assert rows(g=g, links=l.ctypes.data, n_links=len(l)) == hip.ERR_INVALID, bad
        assert prs(o, g=g, links=l.ctypes.data, n_links=len(l)) == hip.ERR_INVALID, bad
        offsets[:] = 0
        assert points(g=g, links=l.ctypes.data, n_links=len(l)) == hip.ERR_INVALID, bad
        offsets[:] = -1
    l = hip.as_links([(0, 1), (2, 0)])                               # R = 3 + 5 rows
    at = dict(g=g, links=l.ctypes.data, n_links=2)
    assert rows(out=None, cap=8, **at) == hip.ERR_INVALID            # rows to write, no buffer
    assert rows(cap=7, **at) == hip.ERR_TOO_SMALL                    # all or nothing
    for kw in (dict(ratio=-0.1), dict(reserved=1), dict(cross_check=2)):
        assert prs(default_opts(hip, **kw), **at) == hip.ERR_INVALID, kw
    assert prs(o, pairs=None, **at) == hip.ERR_INVALID
    # links whose left member is empty have no rows and no pairs: answered on the host
    l0 = hip.as_links([(1, 0), (1, 1), (1, 2)])
    assert rows(g=g, links=l0.ctypes.data, n_links=3, out=None, cap=0) == hip.OK
    assert n.value == -1 and (offsets == -1).all()                   # nothing above wrote anything
    assert prs(o, g=g, links=l0.ctypes.data, n_links=3) == hip.OK and n.value == 0 and offsets.tolist() == [0, 0, 0, 0]
    assert points(g=g, links=l0.ctypes.data, n_links=3) == hip.OK
    # R[n_links] past INT32_MAX: 2^20 links of 2^11 left rows each
    big, _keep = fake_gallery(hip, [1 << 11])
    lb = np.zeros(1 << 20, hip.LINK_DTYPE)
    n.value, offsets[:] = -1, -1
    assert rows(g=big, links=lb.ctypes.data, n_links=len(lb)) == hip.ERR_INVALID
    assert prs(o, g=big, links=lb.ctypes.data, n_links=len(lb)) == hip.ERR_INVALID
    assert rows(g=big, links=lb.ctypes.data, n_links=len(lb) - 1, cap=4) == hip.ERR_TOO_SMALL   # 2^31 - 2^11 rows: valid

    # link_points on the host: the CSR and the pair indices
    def pts_of(link_list, offs, prs_):
        l = hip.as_links(link_list)
        offs = np.array(offs, np.int32)
        p = np.zeros(max(len(prs_), 1), hip.PAIR_DTYPE)
        for k, (pl, pr) in enumerate(prs_):
            p[k]["l"], p[k]["r"] = pl, pr
        return lib.popsift_hip_gallery_link_points(g, l.ctypes.data, len(l), p.ctypes.data, offs.ctypes.data, pts.ctypes.data)

    assert pts_of([(0, 0), (0, 1)], [0, 0, 0], []) == hip.OK         # no pairs: nothing to gather
    assert pts_of([(0, 0), (0, 1)], [0, 2, 1], [(0, 0), (1, 1)]) == hip.ERR_INVALID     # a decreasing offset
    assert pts_of([(0, 0)], [0, 1], [(3, 0)]) == hip.ERR_INVALID     # l outside member 0
    assert pts_of([(0, 0)], [0, 1], [(0, 3)]) == hip.ERR_INVALID     # r outside member 0
    assert pts_of([(0, 0)], [0, 1], [(-1, 0)]) == hip.ERR_INVALID
    assert pts_of([(0, 1)], [0, 1], [(0, 0)]) == hip.ERR_INVALID     # the empty member has no descriptor 0
    assert pts_of([(0, 2)], [0, 1], [(0, 0)]) == hip.ERR_INVALID     # member 2 has no positions: right
    assert pts_of([(2, 0)], [0, 1], [(0, 0)]) == hip.ERR_INVALID     # ... and left
    assert pts_of([(2, 0), (0, 0)], [0, 0, 0], []) == hip.OK         # ... but an empty list on such a link is fine
    lq = hip.as_links([(0, 0)])
    one = np.array([0, 1], np.int32)
    assert lib.popsift_hip_gallery_link_points(g, lq.ctypes.data, 1, None, one.ctypes.data, pts.ctypes.data) == hip.ERR_INVALID
    assert lib.popsift_hip_gallery_link_points(g, lq.ctypes.data, 1, pairs.ctypes.data, one.ctypes.data, None) == hip.ERR_INVALID
    # a rejected call writes nothing
    assert (out.view(np.int32) == 7).all() and (pairs.view(np.int32) == 7).all() and (pts == 7).all()
    del keep, _keep


def test_the_link_lists_do_their_job():
    """The conditions the GPU tests rely on: under every option set enough links with pairs, a link with two non-empty
    sides and none, and links with the empty member on either side."""
    assert [len(r) for r in MEMBERS] == SIZES and SIZES[EMPTY] == 0
    assert len(ALL_PAIRS) == 36 and len(ORDERED) == 81 and sum(left_rows(ORDERED)) == 18261
    found = []
    for o in map(byte_opts, OPTION_SETS):
        rows, pairs, offsets = expected_links(MEMBERS, ALL_PAIRS, **o)
        assert len(rows) == sum(left_rows(ALL_PAIRS)) and offsets[0] == 0 and offsets[-1] == len(pairs)
        counts = np.diff(offsets)
        found.append(int((counts > 0).sum()))
        assert found[-1] >= 4, (o, counts)
        both = np.array([SIZES[a] > 0 and SIZES[b] > 0 for a, b in ALL_PAIRS])
        if o.get("ratio", 0.8) == 0 and "max_dist2" not in o:
            assert (counts[both] > 0).all(), (o, counts)             # the cross-check alone: the closest two rows are a pair
        else:
            assert (counts[both] == 0).any(), (o, counts)            # two non-empty sides and no pairs
        assert counts[~both].sum() == 0
    print(found)
    assert any(a == EMPTY for a, _ in ALL_PAIRS) and any(b == EMPTY for _, b in ALL_PAIRS)
    # the empty-left lists plant what their names say, and keep links with pairs next to the empty ones
    assert all(a == EMPTY for a, _ in EMPTY_LEFT["only"])
    assert EMPTY_LEFT["start"][0][0] == EMPTY and EMPTY_LEFT["start"][-1][0] != EMPTY
    assert EMPTY_LEFT["end"][-1][0] == EMPTY and EMPTY_LEFT["end"][0][0] != EMPTY
    assert [a == EMPTY for a, _ in EMPTY_LEFT["alternating"]] == [True, False, True, False, True, True, False, True]
    assert [a == EMPTY for a, _ in EMPTY_RUN] == [False, False, True, True, True, False, False]
    for name, links in list(EMPTY_LEFT.items()) + [("run", EMPTY_RUN), ("repeated", REPEATED)]:
        _, pairs, offsets = expected_links(MEMBERS, links)
        assert (np.diff(offsets) >= 0).all()
        if name != "only":
            assert (np.diff(offsets) > 0).sum() >= 2, (name, offsets)
        else:
            assert len(pairs) == 0
    rows, pairs, offsets = expected_links(MEMBERS, REPEATED)
    c = np.diff(offsets)
    assert c[0] == c[2] == c[4] > 0                                  # the repeated link is answered three times
    # an empty right member: rows without a candidate
    rows = expected_links(MEMBERS, [(6, EMPTY)])[0]
    assert len(rows) == 3 and np.isinf(rows["dist_best"]).all() and (rows["best"] == 0).all()
