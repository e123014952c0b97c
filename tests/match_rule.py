"""The 2-NN rule of popsift_hip_match_sets restated in float64, and float sets built against the screening path's
argument (match_mfma.hip).  A helper of the tests, not a test.

The rule.  D64[i, j] = sum_k (l[i][k] - r[j][k])^2 in float64, formed from the differences themselves (never as
|l|^2 + |r|^2 - 2 l.r: large norms would cancel).  Right row j is a candidate of left row i when the float32 distance of
the pair is finite and not NaN; that does not depend on the order of the float32 sum:
    a NaN anywhere in the difference vector (a NaN element, or Inf - Inf) drops the pair,
    an overflow of the float32 sum drops it: D64 >= 2^128 (1 - 2^-20) (the cases stay away from that magnitude).
A row {best, second, accept, dist_best, dist_second} satisfies the rule when
    D64[i, best]   <= (1 + 2e-6) * the smallest D64 of the candidates,
    D64[i, second] <= (1 + 2e-6) * the second smallest,
    |dist_best - D64[i, best]| <= 1e-6 D64[i, best], and the same for second,
    among right rows that are element for element equal (their float32 distances are bit-equal whatever the summation
    order) best, and then second, is the lowest index,
    accept = dist_best / dist_second < 0.8 in float32,
    with one candidate second is {0, +inf}, with none the row is {0, 0, 0, +inf, +inf}.
The constants are derived, not measured: a float32 distance carries at most 11 roundings (one in the subtraction, which
squaring doubles; four in the FMA chain of a float4; five in the add tree), a relative error of at most
11 * 2^-24 ~ 6.6e-7 < 1e-6, and the quotient of two such values is within 1.4e-6 < 2e-6 of the true one.  That assumes
no underflow: the rule is applied to sets whose smallest nonzero (l - r)^2 term is at least 1e-30 (min_term below);
zeros_and_tiny()'s block of magnitude 1e-22 is held to the oracle alone.  No row is ever left out of the rule.
"""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from match_pairs_rule import planted

MATCH_DTYPE = np.dtype([("best", np.int32), ("second", np.int32), ("accept", np.int32),
                        ("dist_best", np.float32), ("dist_second", np.float32)])
OVERFLOW = 2.0 ** 128 * (1 - 2.0 ** -20)
R_RANK, R_DIST = 2e-6, 1e-6
MIN_TERM = 1e-30
EMPTY_ROW = (0, 0, 0, np.inf, np.inf)


def dist64(l, r, threads=8, min_term=False):
    """D64 with +inf where the pair is no candidate.  With min_term: also the smallest nonzero (l - r)^2 term.
    Blocks of 16 x 256 pairs stay in cache; numpy releases the GIL inside, so a few threads share the blocks."""
    l64, r64 = np.asarray(l, np.float64).reshape(-1, 128), np.asarray(r, np.float64).reshape(-1, 128)
    D = np.full((len(l64), len(r64)), np.inf)
    starts = [(a, b) for a in range(0, len(l64), 16) for b in range(0, len(r64), 256)]

    def block(ab):
        a, b = ab
        with np.errstate(invalid="ignore", over="ignore"):
            d = l64[a:a + 16, None, :] - r64[None, b:b + 256, :]
            np.multiply(d, d, out=d)
            s = d.sum(-1)
            s[~(s < OVERFLOW)] = np.inf                     # NaN, Inf and float32 overflow
            D[a:a + 16, b:b + 256] = s
            if min_term:
                d[~(d > 0)] = np.inf
                return d.min() if d.size else np.inf
        return np.inf

    if starts:
        with ThreadPoolExecutor(threads) as ex:
            m = min(ex.map(block, starts, chunksize=max(1, len(starts) // (8 * threads))))
    else:
        m = np.inf
    return (D, m) if min_term else D


def duplicate_ranks(r):
    """For every row of r: the lowest and the second lowest index among the rows equal to it element for element
    (-1 where there is no second)."""
    r = np.ascontiguousarray(r, np.float32).reshape(-1, 128)
    first, second = np.arange(len(r)), np.full(len(r), -1)
    if len(r) == 0:
        return first, second
    _, inv = np.unique((r + np.float32(0)).view(np.uint32), axis=0, return_inverse=True)   # + 0: -0.0 equals 0.0
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable")
    grp = inv[order]
    head = np.r_[True, grp[1:] != grp[:-1]]
    lowest = order[np.flatnonzero(head)[np.cumsum(head) - 1]]
    first[order] = lowest
    is2 = np.r_[False, head[:-1]] & ~head
    sec = np.full(grp.max() + 1, -1)
    sec[grp[is2]] = order[is2]
    second[order] = sec[grp]
    return first, second


def violations(l, r, rows, D=None):
    """Why each row of `rows` (MATCH_DTYPE, one per row of l) breaks the rule: a list of (row, reason), empty when all
    rows satisfy it.  D: dist64(l, r) when the caller has it already."""
    l = np.ascontiguousarray(l, np.float32).reshape(-1, 128)
    r = np.ascontiguousarray(r, np.float32).reshape(-1, 128)
    assert rows.dtype == MATCH_DTYPE and len(rows) == len(l)
    D = dist64(l, r) if D is None else D
    nl, nr = D.shape
    bad = []
    if nl == 0:
        return bad
    idx = np.arange(nl)
    n_cand = np.isfinite(D).sum(1)
    low = np.full((nl, 2), np.inf)
    if nr >= 2:
        low = np.partition(D, 1, axis=1)[:, :2]
    elif nr == 1:
        low[:, 0] = D[:, 0]
    first, second = duplicate_ranks(r)
    b, s = rows["best"].astype(np.int64), rows["second"].astype(np.int64)
    db, ds = rows["dist_best"].astype(np.float64), rows["dist_second"].astype(np.float64)

    def flag(mask, reason):
        bad.extend((int(i), reason) for i in np.flatnonzero(mask))

    flag((b < 0) | (b >= max(nr, 1)) | (s < 0) | (s >= max(nr, 1)), "index out of range")
    if bad:
        return bad
    with np.errstate(divide="ignore", invalid="ignore"):
        flag(rows["accept"] != (rows["dist_best"] / rows["dist_second"] < np.float32(0.8)), "accept")
    Db = D[idx, b] if nr else np.full(nl, np.inf)
    Ds = D[idx, s] if nr else np.full(nl, np.inf)
    none, one, two = n_cand == 0, n_cand == 1, n_cand >= 2
    flag(none & ~((b == 0) & (s == 0) & np.isposinf(db) & np.isposinf(ds)), "no candidate: not the empty record")
    flag(one & ~((s == 0) & np.isposinf(ds)), "one candidate: second is not {0, +inf}")
    some = ~none
    with np.errstate(invalid="ignore"):                           # inf - inf: the comparison with NaN fails, as wanted
        eb, es = np.abs(db - Db), np.abs(ds - Ds)
    flag(some & ~np.isfinite(Db), "best is no candidate")
    flag(some & ~(Db <= (1 + R_RANK) * low[:, 0]), "best is not the nearest")
    flag(some & ~(eb <= R_DIST * Db), "dist_best")
    flag(some & (b != first[b] if nr else False), "best: an equal row has a lower index")
    flag(two & ~np.isfinite(Ds), "second is no candidate")
    flag(two & (s == b), "second repeats best")
    flag(two & ~(Ds <= (1 + R_RANK) * low[:, 1]), "second is not the second nearest")
    flag(two & ~(es <= R_DIST * Ds), "dist_second")
    if nr:
        want = np.where(first[s] == b, second[s], first[s])      # an equal row of best's group: the group's second
        flag(two & (s != want), "second: an equal row has a lower index")
    return bad


# ---------------------------------------------------------------------------------------------------- the case sets

def snap(x, q):
    """x rounded to multiples of q (a power of two): differences of such values are 0 or at least q"""
    return (np.round(np.asarray(x, np.float64) / q) * q).astype(np.float32)


def all_undecidable(nl, K):
    """K distinct random right rows, each present four times at shuffled positions; random left rows.  The four copies of
    a row's nearest right row have bit-equal screened distances, so the fourth candidate equals the second whatever the
    rounding: every left row goes to the exact kernel."""
    rng = np.random.default_rng(1000 * nl + K)
    l = rng.random((nl, 128), np.float32)
    r = np.repeat(rng.random((K, 128), np.float32), 4, axis=0)[rng.permutation(4 * K)]
    return l, r


ALL_UNDECIDABLE_SIZES = [(31, 40), (32, 40), (33, 40), (2047, 40), (2048, 40), (2049, 40), (2048 + 32, 40),
                         (2048 + 33, 40), (4096 + 5, 40), (2081, 520)]


def mostly_undecidable(nl=3000, nr=1200):
    """Even left rows lie near a right row that is present four times (undecidable), odd left rows near a unique right
    row c + step that has a near-copy c + 1.2 step (planted()'s 0.69 quotient; decided by the screening pass).  Returns
    (l, r, n_undecidable)."""
    rng = np.random.default_rng(nl * 7919 + nr)
    nq, npair = nr // 8, nr // 4                                   # nq quadruples and npair pairs fill nr rows
    assert 4 * nq + 2 * npair == nr
    base = rng.random((nq, 128), np.float32)
    centre = rng.random((npair, 128), np.float32)
    step = rng.normal(0, 0.02, (npair, 128)).astype(np.float32)
    r = np.concatenate([np.repeat(base, 4, axis=0), centre + step, centre + np.float32(1.2) * step])
    r = r[rng.permutation(nr)]
    l = np.empty((nl, 128), np.float32)
    even, odd = np.arange(0, nl, 2), np.arange(1, nl, 2)
    l[even] = base[rng.integers(0, nq, len(even))] + rng.normal(0, 0.01, (len(even), 128)).astype(np.float32)
    l[odd] = centre[rng.integers(0, npair, len(odd))] + rng.normal(0, 0.003, (len(odd), 128)).astype(np.float32)
    return l, r, len(even)


SCALES = np.array([1e-3, 1.0, 3.0, 30.0, 1e3])
N_OUTSIDER_ROWS = 50
# squared distances of the outsider construction (see mixed_norms) and the squared norm of the outsiders
OUT_BEST, OUT_SECOND, OUT_GAP, OUT_NORM2 = 0.8, 0.9, 1e-4, 3.6


def _at_distance(rng, l, norm2, dist2):
    """A vector of squared norm norm2 at squared distance dist2 from the unit vector l (float64)"""
    c = (1.0 + norm2 - dist2) / 2.0                                # l . r
    assert norm2 - c * c > 0, "no such vector (Cauchy-Schwarz)"
    v = rng.normal(0, 1, 128)
    v -= (v @ l) * l
    v /= np.linalg.norm(v)
    return c * l + np.sqrt(norm2 - c * c) * v


def mixed_norms(nl, nr):
    """Rows scaled by factors from {1e-3, 1, 3, 30, 1e3} on both sides, values on a grid fine enough for float32 and
    coarse enough for MIN_TERM; a third of the right rows are near-copies of left rows within the left row's scale.
    The first 50 left rows are unit vectors with a construction the margin of k_match_select never sees: right rows
    4 i .. 4 i + 3 are, for left row i, a best (squared norm 1, squared distance 0.8), a second (1, 0.9) and two
    outsiders of squared norm 3.6 at 0.9 +- up to 1e-4: rows whose own rounding scale is 3.6 times the one eps is built
    from.  (An outsider of squared norm 6 at squared distance 1.1 from a unit vector does not exist:
    |l - r|^2 >= (sqrt 6 - 1)^2 = 2.1; and beyond squared distance 1 the rows of scale 1e-3, which sit at the origin,
    would be nearer than the construction.  3.6 is the largest round norm that keeps it the nearest: (sqrt 3.6 - 1)^2 =
    0.80.)"""
    rng = np.random.default_rng(nl * 7919 + nr + 1)
    sl, sr = SCALES[rng.integers(0, 5, nl)], SCALES[rng.integers(0, 5, nr)]
    q = lambda s: 2.0 ** (np.floor(np.log2(s)) - 23)[:, None]
    l = snap(rng.random((nl, 128)) * sl[:, None], q(sl))
    r = snap(rng.random((nr, 128)) * sr[:, None], q(sr))
    k = min(nl, nr) // 3
    src, dst = rng.permutation(nl)[:k], rng.permutation(nr)[:k]
    r[dst] = snap(l[src] + rng.normal(0, 0.02, (k, 128)) * sl[src, None], q(sl[src]))
    for i in range(N_OUTSIDER_ROWS):
        u = rng.normal(0, 1, 128)
        u = snap(u / np.linalg.norm(u), 2.0 ** -30).astype(np.float64)
        u /= np.linalg.norm(u)                                     # the float64 unit vector the others are built on
        l[i] = snap(u, 2.0 ** -30)
        r[4 * i] = snap(_at_distance(rng, u, 1.0, OUT_BEST), 2.0 ** -30)
        r[4 * i + 1] = snap(_at_distance(rng, u, 1.0, OUT_SECOND), 2.0 ** -30)
        for j in (2, 3):
            r[4 * i + j] = snap(_at_distance(rng, u, OUT_NORM2, OUT_SECOND + rng.uniform(-OUT_GAP, OUT_GAP)), 2.0 ** -30)
    return l, r


def signed(nl=700, nr=900):
    """Components in [-1, 1), rows of unit length: squared distances up to 4 |l|^2.  Right rows 0 .. 49 are the
    antipodes of left rows 0 .. 49 (d = 4), a third of the rest near-copies."""
    rng = np.random.default_rng(nl * 7919 + nr + 2)
    l = rng.uniform(-1, 1, (nl, 128))
    r = rng.uniform(-1, 1, (nr, 128))
    l = snap(l / np.linalg.norm(l, axis=1, keepdims=True), 2.0 ** -30)
    r = snap(r / np.linalg.norm(r, axis=1, keepdims=True), 2.0 ** -30)
    r[:50] = -l[:50]
    k = min(nl, nr) // 3
    src, dst = rng.permutation(nl)[:k], 50 + rng.permutation(nr - 50)[:k]
    r[dst] = snap(l[src] + rng.normal(0, 0.002, (k, 128)), 2.0 ** -30)
    return l, r


N_TINY_L, N_TINY_R = 40, 50


def zeros_and_tiny(nl=300, nr=400):
    """All-zero rows on both sides (left 0 .. 9, right 0 .. 7 and 200: distance 0 ties) among random rows, and at the end
    of both sets a block of rows of magnitude 1e-22, whose squares are denormal or 0.  zeros_only() is the part the
    float64 rule applies to."""
    rng = np.random.default_rng(nl * 7919 + nr + 3)
    l = rng.random((nl, 128), np.float32)
    r = rng.random((nr, 128), np.float32)
    l[:10] = 0
    r[:8] = 0
    r[200] = 0
    r[20] = l[30]
    l[nl - N_TINY_L:] = (1e-22 * rng.random((N_TINY_L, 128))).astype(np.float32)
    r[nr - N_TINY_R:] = (1e-22 * rng.random((N_TINY_R, 128))).astype(np.float32)
    r[nr - 1] = l[nl - 1]
    r[nr - 2] = 0
    return l, r


def zeros_only(nl=300, nr=400):
    l, r = zeros_and_tiny(nl, nr)
    return l[:nl - N_TINY_L].copy(), r[:nr - N_TINY_R].copy()


# non_finite(): which rows carry what
NF_COPIES = (210, 250)                     # right rows that are near-copies of the left rows of the same index
NF_R_NAN, NF_R_PINF, NF_R_NINF = [3, 50, 129, 250, 399], [0, 64, 128, 200, 300], [7, 127, 391]
NF_L_NAN = [2, 31, 32, 150, 299]
NF_L_PINF, NF_R_SAME_PINF = 40, 41         # +Inf at the same position: the difference is NaN
NF_L_NAN_AT_ZERO, NF_R_ZERO = 60, 61       # a NaN where the right row has a 0


def non_finite(nl=300, nr=400):
    """Random rows with a NaN element in 5 right and 5 left rows, +Inf in 5 right rows, -Inf in 3, a left and a right
    row that are +Inf at the same position, and a left row with a NaN where a right row is 0.  The (3, 2) case: both
    right rows NaN."""
    rng = np.random.default_rng(nl * 7919 + nr + 4)
    l = rng.random((nl, 128), np.float32)
    r = rng.random((nr, 128), np.float32)
    if (nl, nr) == (3, 2):
        r[0, 5] = r[1, 127] = np.nan
        return l, r
    a, b = NF_COPIES
    r[a:b] = l[a:b] + rng.normal(0, 0.02, (b - a, 128)).astype(np.float32)               # clean near-copies
    for n, j in enumerate(NF_R_NAN):
        r[j, (37 * n) % 128] = np.nan
    for n, j in enumerate(NF_R_PINF):
        r[j, (41 * n + 1) % 128] = np.inf
    for n, j in enumerate(NF_R_NINF):
        r[j, (43 * n + 2) % 128] = -np.inf
    for n, i in enumerate(NF_L_NAN):
        l[i, (47 * n + 3) % 128] = np.nan
    l[NF_L_PINF, 9] = r[NF_R_SAME_PINF, 9] = np.inf
    r[NF_R_ZERO, 11] = 0
    l[NF_L_NAN_AT_ZERO, 11] = np.nan
    return l, r


NF_POISONED_R = sorted(NF_R_NAN + NF_R_PINF + NF_R_NINF + [NF_R_SAME_PINF])
NF_POISONED_L = sorted(NF_L_NAN + [NF_L_PINF, NF_L_NAN_AT_ZERO])


def huge_finite(nl, nr):
    """Rows 3e18 (0.5 + 0.5 u): |x|^2 overflows float32 (~ 7e38) while every squared distance is finite (below 2.9e38).
    Right row 3 = left row 2 x 1.001, and a few more planted copies."""
    rng = np.random.default_rng(nl * 7919 + nr + 5)
    l = (3e18 * (0.5 + 0.5 * rng.random((nl, 128)))).astype(np.float32)
    r = (3e18 * (0.5 + 0.5 * rng.random((nr, 128)))).astype(np.float32)
    r[3] = l[2] * np.float32(1.001)
    for n in range(10):
        r[10 + 7 * n] = l[5 + 3 * n] * np.float32(1.0 + 0.002 * (n + 1))
    r[nr - 1] = r[10]                                              # an exact duplicate: the lower index wins
    return l, r


# several right tiles per screening split: see several_tiles_per_split() in test_match_rule.py for the size
SEVERAL_TILES = (16385, 3073)


def several_tiles_per_split():
    return planted(*SEVERAL_TILES)


@functools.lru_cache(maxsize=None)
def case(name, *size):
    """(l, r) of a case set by name, computed once per process and shared (read-only) among the tests."""
    out = globals()[name](*size)[:2]
    for a in out:
        a.setflags(write=False)
    return out


# every case as (name, size): what test_match_rule.py and test_gpu_match_edges.py run.  RULE_CASES: the float64 rule
# applies; zeros_and_tiny is held to the oracle alone.
RULE_CASES = ([("all_undecidable", s) for s in ALL_UNDECIDABLE_SIZES] +
              [("mostly_undecidable", (3000, 1200)), ("mixed_norms", (700, 900)), ("mixed_norms", (5000, 4000)),
               ("signed", (700, 900)), ("zeros_only", (300, 400)), ("non_finite", (300, 400)), ("non_finite", (3, 2)),
               ("huge_finite", (64, 96)), ("huge_finite", (300, 400)), ("several_tiles_per_split", ())])
ORACLE_ONLY_CASES = [("zeros_and_tiny", (300, 400))]
