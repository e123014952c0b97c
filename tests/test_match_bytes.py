"""popsift_hip_match_bytes / popsift_hip_match_pairs_bytes without a GPU: the new symbols, the argument checks of the C ABI
(made before any GPU call), and the numpy rule the GPU tests compare with (tests/match_bytes_rule.py) pinned to the oracle:
integer-valued floats below 2^24 make the oracle's float arithmetic exact, so its rows on float32(bytes) ARE the rule's."""
import ctypes as C

import numpy as np
import pytest

from match_bytes_rule import CAP_BYTES, D_MAX, MATCH_DTYPE, brute_rows, match_rows, planted_bytes, position_coded
from match_pairs_rule import OPTION_SETS, expected_pairs, keep_masks

NEW = ["popsift_hip_bytefeatures_from_host", "popsift_hip_bytefeatures_from_set", "popsift_hip_clone_results_u8",
       "popsift_hip_bytefeatures_free", "popsift_hip_bytefeatures_info", "popsift_hip_bytefeatures_download",
       "popsift_hip_match_bytes", "popsift_hip_match_pairs_bytes"]


def byte_opts(o):
    """an entry of OPTION_SETS with its cap in byte units squared"""
    return dict(o, max_dist2=CAP_BYTES) if "max_dist2" in o else o


def test_new_symbols_are_exported_and_bound(hip):
    bound = {n for n, _, _ in hip.SYMBOLS}
    for n in NEW:
        assert n in bound and hasattr(hip.lib(), n), n
    assert hip.MATCH_DTYPE == MATCH_DTYPE
    for m in ("from_host", "from_set", "download", "match", "match_pairs"):
        assert callable(getattr(hip.ByteFeatures, m))
    assert callable(hip.Context.clone_results_u8)


def test_invalid_arguments_are_rejected_without_a_gpu(hip):
    """Blocks of zeros stand in for sets: as sets they are empty, so nothing reaches a GPU even where a check is missing."""
    lib = hip.lib()
    l, r = C.create_string_buffer(512), C.create_string_buffer(512)
    h = C.c_void_p(1)
    desc = np.zeros((2, 128), np.uint8)
    assert lib.popsift_hip_bytefeatures_from_host(0, desc.ctypes.data, 2, None) == hip.ERR_INVALID
    assert lib.popsift_hip_bytefeatures_from_host(0, desc.ctypes.data, -1, C.byref(h)) == hip.ERR_INVALID
    assert lib.popsift_hip_bytefeatures_from_host(0, None, 2, C.byref(h)) == hip.ERR_INVALID
    assert lib.popsift_hip_bytefeatures_from_set(None, C.byref(h)) == hip.ERR_INVALID
    assert lib.popsift_hip_bytefeatures_from_set(l, None) == hip.ERR_INVALID
    assert lib.popsift_hip_clone_results_u8(None, 0, C.byref(h)) == hip.ERR_INVALID
    assert lib.popsift_hip_bytefeatures_free(None) == hip.OK
    assert lib.popsift_hip_bytefeatures_info(None, None, None) == hip.ERR_INVALID
    assert lib.popsift_hip_bytefeatures_download(None, None, None) == hip.ERR_INVALID
    if hip.device_count() == 0:
        assert lib.popsift_hip_bytefeatures_from_host(0, desc.ctypes.data, 2, C.byref(h)) == hip.ERR_NO_DEVICE
        assert h.value is None                                       # a failed call leaves no handle behind

    out = np.zeros(4, hip.MATCH_DTYPE)
    assert lib.popsift_hip_match_bytes(None, r, out.ctypes.data) == hip.ERR_INVALID
    assert lib.popsift_hip_match_bytes(l, None, out.ctypes.data) == hip.ERR_INVALID
    assert lib.popsift_hip_match_bytes(l, r, None) == hip.OK         # an empty left set writes nothing
    d, n = C.c_int(-1), C.c_int(-1)
    assert lib.popsift_hip_bytefeatures_info(l, C.byref(d), C.byref(n)) == hip.OK and (d.value, n.value) == (0, 0)

    pairs = np.zeros(4, hip.PAIR_DTYPE)
    n = C.c_int(-1)

    def call(opts, l=l, r=r, pairs=pairs.ctypes.data, cap=4, n_pairs=C.byref(n)):
        return lib.popsift_hip_match_pairs_bytes(l, r, C.byref(opts) if opts is not None else None, pairs, cap, n_pairs)

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
    assert call(opts(), pairs=None) == hip.ERR_INVALID               # cap > 0 without a buffer
    for kw in (dict(ratio=-0.1), dict(ratio=float("nan")), dict(ratio=float("inf")), dict(max_dist2=float("nan")),
               dict(reserved=1), dict(cross_check=2), dict(cross_check=-1)):
        assert call(opts(**kw)) == hip.ERR_INVALID, kw
    assert n.value == -1                                             # a rejected call writes nothing
    for kw in (dict(), dict(ratio=0.0), dict(ratio=-0.0), dict(max_dist2=0.0), dict(max_dist2=-1.0), dict(cross_check=1),
               dict(ratio=1e30, max_dist2=float("inf"))):
        n.value = -1
        assert call(opts(**kw)) == hip.OK and n.value == 0, kw
    n.value = -1
    assert call(opts(), pairs=None, cap=0) == hip.OK and n.value == 0


def test_the_rule_is_its_definition_on_small_sets():
    for build in (planted_bytes, position_coded):
        for nl, nr in ((1, 1), (3, 1), (5, 2), (40, 60), (30, 300)):
            l, r = build(nl, nr)
            assert match_rows(l, r, chunk=7).tobytes() == brute_rows(l, r).tobytes(), (build.__name__, nl, nr)
    e = np.zeros((0, 128), np.uint8)
    l = np.ones((3, 128), np.uint8)
    assert len(match_rows(e, l)) == 0
    rows = match_rows(l, e)
    assert rows.tobytes() == np.array([(0, 0, 0, np.inf, np.inf)] * 3, MATCH_DTYPE).tobytes()


@pytest.mark.parametrize("nl,nr", [(3, 1), (33, 65), (300, 400), (700, 129), (2500, 3100)])
def test_the_rule_equals_the_oracle_on_the_bytes_as_floats(oracle_mod, nl, nr):
    for build in (planted_bytes, position_coded):
        l, r = build(nl, nr)
        want = oracle_mod.match(l.astype(np.float32), r.astype(np.float32))
        assert match_rows(l, r).tobytes() == want.tobytes(), build.__name__
        assert match_rows(r, l).tobytes() == oracle_mod.match(r.astype(np.float32), l.astype(np.float32)).tobytes()


def test_planted_bytes_hold_what_they_promise():
    """What the GPU tests rely on.  About the cap, CAP * 512^2 = 13107.2: scaled by 512 half of planted()'s uniform values
    saturate at 255, so a near-copy's squared distance is about 64 x 10.24^2 ~ 6700 -- half of what the float sets give.
    The cap therefore separates the near-copies (under it) from the unrelated rows (over it, ~ 10^6) rather than splitting
    the near-copies among themselves: of the rows the ratio test and the cross-check keep, 98 / 1 lie under / over it at
    300 x 400, 830 / 0 at 2500 x 3100 and 1334 / 2 at 5000 x 4000.  Both sides of the cap are non-empty in every set."""
    for nl, nr in ((300, 400), (2500, 3100), (5000, 4000)):
        l, r = planted_bytes(nl, nr)
        F, B = match_rows(l, r), match_rows(r, l)
        # all-0 / all-255: distance 0 to their twins, the largest distance to each other's
        assert (F["best"][11], F["dist_best"][11], F["best"][12], F["dist_best"][12]) == (13, 0.0, 14, 0.0)
        assert int(((l[11].astype(np.int64) - r[14]) ** 2).sum()) == D_MAX == 8323200
        # two different right descriptors at the same distance: the lower index is best, the other second
        assert not np.array_equal(r[20], r[21])
        assert (F["best"][15], F["second"][15], F["dist_best"][15], F["dist_second"][15]) == (20, 21, 9.0, 9.0)
        # exact duplicates in the right set: best and second tie for l[7]
        assert F["dist_best"][7] == F["dist_second"][7] and F["best"][7] < F["second"][7]
        # the cap in byte units: rows on both sides of it, and the three conditions each remove rows of their own
        o = byte_opts(OPTION_SETS[-1])
        assert o["max_dist2"] == CAP_BYTES == 0.05 * 512 * 512
        k_ratio, k_cap, k_cross = keep_masks(F, B, **o)
        print(nl, nr, "rows under / over the cap:", k_cap.sum(), (~k_cap).sum(), "; of those the ratio test and the "
              "cross-check keep:", (k_ratio & k_cross & k_cap).sum(), (k_ratio & k_cross & ~k_cap).sum())
        assert k_cap.any() and (~k_cap).any()
        assert (~k_ratio & k_cap & k_cross).any() and (k_ratio & k_cap & ~k_cross).any()
        assert (k_ratio & k_cap & k_cross).any()
        cap_only = expected_pairs(F, B, **byte_opts(OPTION_SETS[2]))
        assert 0 < len(cap_only) < nl
