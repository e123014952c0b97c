"""popsift_hip_gallery_* / popsift_hip_match_gallery / popsift_hip_match_pairs_gallery without a GPU: the new symbols, the
argument checks of the C ABI (made before any GPU call), and the galleries of tests/gallery_rule.py doing the job the GPU
tests give them."""
import ctypes as C

import numpy as np
import pytest

from gallery_rule import SIZES, coded_gallery, expected, planted_gallery
from match_pairs_rule import OPTION_SETS
from test_match_bytes import byte_opts

NEW = ["popsift_hip_gallery_create", "popsift_hip_gallery_free", "popsift_hip_gallery_add", "popsift_hip_gallery_add_host",
       "popsift_hip_gallery_info", "popsift_hip_gallery_member", "popsift_hip_gallery_download",
       "popsift_hip_gallery_debug_set_group_rows", "popsift_hip_match_gallery", "popsift_hip_match_pairs_gallery"]


def test_new_symbols_are_exported_and_bound(hip):
    bound = {n for n, _, _ in hip.SYMBOLS}
    for n in NEW:
        assert n in bound and hasattr(hip.lib(), n), n
    for m in ("add", "info", "member", "download", "match", "match_pairs", "counts", "set_group_rows"):
        assert callable(getattr(hip.Gallery, m))
    assert hip.GALLERY_GROUP_ROWS == 1 << 22


def test_invalid_arguments_are_rejected_without_a_gpu(hip):
    """Blocks of zeros stand in for a set and for a gallery: the set is empty and the gallery has no members, so nothing
    reaches a GPU even where a check is missing."""
    lib = hip.lib()
    l, g = C.create_string_buffer(512), C.create_string_buffer(512)
    h = C.c_void_p(1)
    desc = np.zeros((2, 128), np.uint8)
    m = C.c_int(-7)
    assert lib.popsift_hip_gallery_create(0, None) == hip.ERR_INVALID
    if hip.device_count() == 0:
        assert lib.popsift_hip_gallery_create(0, C.byref(h)) == hip.ERR_NO_DEVICE
        assert h.value is None                                       # a failed call leaves no handle behind
    assert lib.popsift_hip_gallery_free(None) == hip.OK
    assert lib.popsift_hip_gallery_add(None, l, C.byref(m)) == hip.ERR_INVALID
    assert lib.popsift_hip_gallery_add(g, None, C.byref(m)) == hip.ERR_INVALID
    assert lib.popsift_hip_gallery_add_host(None, desc.ctypes.data, 2, C.byref(m)) == hip.ERR_INVALID
    assert lib.popsift_hip_gallery_add_host(g, desc.ctypes.data, -1, C.byref(m)) == hip.ERR_INVALID
    assert lib.popsift_hip_gallery_add_host(g, None, 2, C.byref(m)) == hip.ERR_INVALID
    # past 2^30 descriptors: rejected on the count alone, the bytes are never read
    assert lib.popsift_hip_gallery_add_host(g, desc.ctypes.data, (1 << 30) + 1, C.byref(m)) == hip.ERR_INVALID
    assert m.value == -7                                             # a rejected add writes nothing
    assert lib.popsift_hip_gallery_info(None, None, None, None) == hip.ERR_INVALID
    d, nm, nd = C.c_int(-1), C.c_int(-1), C.c_int64(-1)
    assert lib.popsift_hip_gallery_info(g, C.byref(d), C.byref(nm), C.byref(nd)) == hip.OK
    assert (d.value, nm.value, nd.value) == (0, 0, 0)
    first, count = C.c_int64(-1), C.c_int(-1)
    assert lib.popsift_hip_gallery_member(None, 0, C.byref(first), C.byref(count)) == hip.ERR_INVALID
    for bad in (-1, 0, 1):                                           # no members: every index is out of range
        assert lib.popsift_hip_gallery_member(g, bad, C.byref(first), C.byref(count)) == hip.ERR_INVALID
        assert lib.popsift_hip_gallery_download(g, bad, desc.ctypes.data) == hip.ERR_INVALID
    assert lib.popsift_hip_gallery_download(None, 0, desc.ctypes.data) == hip.ERR_INVALID
    assert (first.value, count.value) == (-1, -1)
    assert lib.popsift_hip_gallery_debug_set_group_rows(None, 0) == hip.ERR_INVALID
    assert lib.popsift_hip_gallery_debug_set_group_rows(g, -1) == hip.ERR_INVALID
    assert lib.popsift_hip_gallery_debug_set_group_rows(g, 129) == hip.OK
    assert lib.popsift_hip_gallery_debug_set_group_rows(g, 0) == hip.OK

    out = np.full(4, 7, np.int32).repeat(5).view(hip.MATCH_DTYPE)
    assert lib.popsift_hip_match_gallery(None, g, out.ctypes.data, 4) == hip.ERR_INVALID
    assert lib.popsift_hip_match_gallery(l, None, out.ctypes.data, 4) == hip.ERR_INVALID
    assert lib.popsift_hip_match_gallery(l, g, out.ctypes.data, 4) == hip.OK    # no rows: nothing is written
    assert lib.popsift_hip_match_gallery(l, g, None, 0) == hip.OK
    assert (out.view(np.int32) == 7).all()

    pairs = np.zeros(4, hip.PAIR_DTYPE)
    offsets = np.full(3, -1, np.int32)
    n = C.c_int(-1)

    def call(opts, l=l, g=g, pairs=pairs.ctypes.data, cap=4, offsets=offsets.ctypes.data, n_pairs=C.byref(n)):
        return lib.popsift_hip_match_pairs_gallery(l, g, C.byref(opts) if opts is not None else None, pairs, cap, offsets,
                                                   n_pairs)

    def opts(**kw):
        o = hip.MatchOpts()
        lib.popsift_hip_default_match_opts(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    assert call(opts(), l=None) == hip.ERR_INVALID
    assert call(opts(), g=None) == hip.ERR_INVALID
    assert call(None) == hip.ERR_INVALID
    assert call(opts(), n_pairs=None) == hip.ERR_INVALID
    assert call(opts(), offsets=None) == hip.ERR_INVALID
    assert call(opts(), pairs=None) == hip.ERR_INVALID               # cap > 0 without a buffer
    for kw in (dict(ratio=-0.1), dict(ratio=float("nan")), dict(ratio=float("inf")), dict(max_dist2=float("nan")),
               dict(reserved=1), dict(cross_check=2), dict(cross_check=-1)):
        assert call(opts(**kw)) == hip.ERR_INVALID, kw
    assert n.value == -1 and (offsets == -1).all()                   # a rejected call writes nothing
    for kw in (dict(), dict(ratio=0.0), dict(max_dist2=0.0), dict(cross_check=1)):
        n.value = -1
        offsets[:] = -1
        assert call(opts(**kw)) == hip.OK and n.value == 0, kw
        assert offsets[0] == 0 and (offsets[1:] == -1).all()         # n_members + 1 = 1 offset
    n.value = -1
    assert call(opts(), pairs=None, cap=0) == hip.OK and n.value == 0


def check_counts(nl, by_set):
    """the conditions the GPU tests rely on; by_set[k][m]: pairs of member m under OPTION_SETS[k]"""
    for k, counts in enumerate(by_set):
        assert (counts > 0).sum() >= 4, (nl, k, counts)
        nonempty = np.array(SIZES) > 0
        if k in (1, 2, 4):
            assert (counts[nonempty] == 0).any(), (nl, k, counts)   # a non-empty member without pairs
        assert (counts[1:] != nl).all(), (nl, k, counts)
        assert counts[~nonempty].sum() == 0
    assert by_set[0][0] == nl                                        # one descriptor: d / inf passes every ratio
    assert by_set[3][0] == 1                                         # ... and has one nearest query row


@pytest.mark.parametrize("nl", [33, 129, 700])
def test_the_planted_gallery_does_its_job(nl):
    l, members = planted_gallery(nl, SIZES)
    assert [len(r) for r in members] == SIZES and all(r.dtype == np.uint8 for r in members)
    by_set = []
    for o in map(byte_opts, OPTION_SETS):
        rows, pairs, offsets = expected(l, members, **o)
        assert rows.shape == (len(SIZES), nl) and offsets[0] == 0 and offsets[-1] == len(pairs)
        by_set.append(np.diff(offsets))
    print(nl, [c.tolist() for c in by_set])
    check_counts(nl, by_set)
    # ties inside a member: rows nr - 1 and nr // 2 are copies of row 1
    for r in members:
        if len(r) > 4:
            assert np.array_equal(r[1], r[-1]) and np.array_equal(r[1], r[len(r) // 2])


def test_the_coded_gallery_shares_rows():
    l, members = coded_gallery(129, SIZES)
    rows, _, _ = expected(l, members)
    assert np.array_equal(members[3][:127], members[1])              # members share their first rows
    same = expected(l, [members[2], members[2]])[0]
    assert same[0].tobytes() == same[1].tobytes()                    # equal members give equal rows
    assert np.isinf(rows[4]["dist_best"]).all() and (rows[4]["best"] == 0).all()   # the empty member
    assert (rows[0]["second"] == 0).all() and np.isinf(rows[0]["dist_second"]).all() and (rows[0]["accept"] == 1).all()
