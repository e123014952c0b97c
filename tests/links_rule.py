"""What popsift_hip_match_links / popsift_hip_match_pairs_links must return, stated through the per-pair rules
(match_bytes_rule.match_rows, match_pairs_rule.expected_pairs) link by link -- no new arithmetic -- and the link lists the
tests run it on.  A helper of the tests, not a test."""
import functools

import numpy as np

from gallery_rule import SIZES, planted_gallery
from match_bytes_rule import MATCH_DTYPE, match_rows
from match_pairs_rule import PAIR_DTYPE, expected_pairs

EMPTY = SIZES.index(0)                                               # member 4: the empty one


def expected_links(members, links, **opts):
    """(rows (R[n_links],), pairs, offsets (n_links + 1,) int32) of the rule; links: (a, b) pairs"""
    rows, pairs, offsets = [np.zeros(0, MATCH_DTYPE)], [np.zeros(0, PAIR_DTYPE)], np.zeros(len(links) + 1, np.int32)
    for e, (a, b) in enumerate(links):
        fwd, back = both_ways(members, a, b)
        rows.append(fwd)
        pairs.append(expected_pairs(fwd, back, **opts))
        offsets[e + 1] = offsets[e] + len(pairs[-1])
    return np.concatenate(rows), np.concatenate(pairs), offsets


def both_ways(members, a, b):
    """match_rows(A, B) and match_rows(B, A); for the shared members below each ordered pair is computed once"""
    if members is MEMBERS:
        return shared_rows(a, b), shared_rows(b, a)
    return match_rows(members[a], members[b]), match_rows(members[b], members[a])


@functools.lru_cache(maxsize=None)
def shared_rows(a, b):
    rows = match_rows(MEMBERS[a], MEMBERS[b])
    rows.setflags(write=False)
    return rows


# the members of the planted gallery: most are near-copies of rows of one query, and so of each other's
MEMBERS = planted_gallery(700, SIZES)[1]
N = len(SIZES)

ALL_PAIRS = [(a, b) for a in range(N) for b in range(a + 1, N)]      # the 36 links a < b
ORDERED = [(a, b) for a in range(N) for b in range(N)]               # all 81, a == b included: 18 261 left rows
REPEATED = [(7, 5), (3, 1), (7, 5), (5, 7), (7, 5)]                  # one link three times

# links whose left member is empty have no rows: at the start, at the end, alternating, and nothing else
EMPTY_LEFT = {
    "start": [(EMPTY, 1), (EMPTY, 7), (3, 5), (7, 3)],
    "end": [(3, 5), (7, 3), (EMPTY, 1), (EMPTY, EMPTY), (EMPTY, 7)],
    "alternating": [(EMPTY, 1), (3, 5), (EMPTY, 7), (7, 3), (EMPTY, 3), (EMPTY, 5), (5, 7), (EMPTY, 0)],
    "only": [(EMPTY, b) for b in (1, 7, EMPTY, 3)],
}
# a run of empty-left links in the middle of a list, for a group edge that falls inside the run
EMPTY_RUN = [(3, 5), (1, 7), (EMPTY, 1), (EMPTY, 7), (EMPTY, 3), (7, 3), (5, 1)]


def left_rows(links, sizes=SIZES):
    return [sizes[a] for a, _ in links]
