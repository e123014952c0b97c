"""What popsift_hip_match_gallery / popsift_hip_match_pairs_gallery must return, stated through the per-pair rules
(match_bytes_rule.match_rows, match_pairs_rule.expected_pairs) member by member -- no new arithmetic -- and the galleries the
tests run it on.  A helper of the tests, not a test."""
import numpy as np

from match_bytes_rule import MATCH_DTYPE, match_rows, planted_bytes, position_coded
from match_pairs_rule import PAIR_DTYPE, expected_pairs
from popsift_amd._capi import quantize_u8

# one descriptor, both sides of the 128-row tile, an empty member in the middle, a multi-tile member
SIZES = [1, 127, 128, 129, 0, 257, 3, 1000, 384]


def expected(l, members, **opts):
    """(rows (n_members, nl), pairs, offsets (n_members + 1,) int32) of the rule"""
    rows = np.zeros((len(members), len(l)), MATCH_DTYPE)
    pairs, offsets = [], np.zeros(len(members) + 1, np.int32)
    for m, r in enumerate(members):
        rows[m] = match_rows(l, r)
        p = expected_pairs(rows[m], match_rows(r, l), **opts)
        pairs.append(p)
        offsets[m + 1] = offsets[m] + len(p)
    return rows, (np.concatenate(pairs) if pairs else np.zeros(0, PAIR_DTYPE)), offsets


def planted_gallery(nl, sizes, seed=0):
    """The query of planted_bytes(nl, 1000) and one member per entry of `sizes`: random rows, of which (unless m % 4 == 2,
    an unrelated image) a third are near-copies of query rows, and for more than 4 rows two copies of row 1 (ties inside a
    member)."""
    l = planted_bytes(nl, 1000)[0]
    lf = l.astype(np.float32) / np.float32(512)
    members = []
    for m, nr in enumerate(sizes):
        rng = np.random.default_rng(1000003 * (seed + 1) + 7919 * m + nr)
        r = rng.random((nr, 128), np.float32)
        if m % 4 != 2:
            k = min(nl, nr) // 3
            r[rng.permutation(nr)[:k]] = lf[rng.permutation(nl)[:k]] + rng.normal(0, 0.02, (k, 128)).astype(np.float32)
        if nr > 4:
            r[nr - 1] = r[1]
            r[nr // 2] = r[1]
        members.append(quantize_u8(r * np.float32(512)).reshape(nr, 128))
    return l, members


def coded_gallery(nl, sizes):
    """position_coded rows: members share their first rows, so equal members must give equal rows"""
    return position_coded(nl, 1)[0], [position_coded(1, nr)[1] for nr in sizes]


BUILDERS = {"planted": planted_gallery, "coded": coded_gallery}
