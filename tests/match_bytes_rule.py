"""numpy restatement of popsift_hip_match_bytes' row rule (include/popsift_hip.h), and the byte sets the tests run it on.
A helper of the tests, not a test.

    d(i, j)  = sum_k (l[i][k] - r[j][k])^2, an integer <= 8 323 200 < 2^24
    best, second: the two smallest under lexicographic (d, j); one right descriptor: second = 0, dist_second = inf
    accept   = float32(d_best) / float32(d_second) < 0.8f (0 / 0 and inf / inf are NaN and fail)
    no right descriptor: every row is {0, 0, 0, inf, inf}
"""
import numpy as np

from match_pairs_rule import CAP, planted
from popsift_amd._capi import quantize_u8

MATCH_DTYPE = np.dtype([("best", np.int32), ("second", np.int32), ("accept", np.int32),
                        ("dist_best", np.float32), ("dist_second", np.float32)])
D_MAX = 128 * 255 * 255                      # 8 323 200
CAP_BYTES = CAP * 512.0 * 512.0              # match_pairs_rule's cap in byte units squared (the sets are scaled by 512)


def match_rows(l, r, chunk=512):
    """The rows of the rule for uint8 sets l (nl, 128) and r (nr, 128).  The distances come from a float32 GEMM of the
    bytes minus 128: products are below 2^14 and every partial sum below 2^21, so each float operation is exact whatever
    order the BLAS adds in; norms and the final combination are int64.  Chunked over left rows."""
    l = np.ascontiguousarray(l, np.uint8).reshape(-1, 128)
    r = np.ascontiguousarray(r, np.uint8).reshape(-1, 128)
    out = np.zeros(len(l), MATCH_DTYPE)
    out["dist_best"] = out["dist_second"] = np.inf
    if len(l) == 0 or len(r) == 0:
        return out
    rs = r.astype(np.float32) - np.float32(128)
    rn = (rs.astype(np.int64) ** 2).sum(1)
    big = np.int64(1) << 40
    for a in range(0, len(l), chunk):
        ls = l[a:a + chunk].astype(np.float32) - np.float32(128)
        ln = (ls.astype(np.int64) ** 2).sum(1)
        d = ln[:, None] + rn[None, :] - 2 * (ls @ rs.T).astype(np.int64)
        rows = np.arange(len(ls))
        b = d.argmin(1)                       # first occurrence: the lowest index among equals
        db = d[rows, b]
        o = out[a:a + chunk]
        o["best"], o["dist_best"] = b, db.astype(np.float32)
        if len(r) > 1:
            d[rows, b] = big
            s = d.argmin(1)
            o["second"], o["dist_second"] = s, d[rows, s].astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["accept"] = out["dist_best"] / out["dist_second"] < np.float32(0.8)
    return out


def brute_rows(l, r):
    """The same rows from the definition, pair by pair in Python integers (small sets only): what match_rows is held to."""
    out = np.zeros(len(l), MATCH_DTYPE)
    for i, a in enumerate(np.asarray(l, np.int64)):
        cand = sorted((int(((a - b) ** 2).sum()), j) for j, b in enumerate(np.asarray(r, np.int64)))
        (d1, j1), (d2, j2) = (cand + [(np.inf, 0), (np.inf, 0)])[:2]
        with np.errstate(invalid="ignore"):
            acc = np.float32(d1) / np.float32(d2) < np.float32(0.8)
        out[i] = (j1, j2, acc, d1, d2)
    return out


def planted_bytes(nl, nr):
    """planted() of match_pairs_rule.py scaled by 512 and quantized by the header's rule (near-copies, exact duplicates in
    the right set, values saturated at 255).  Big enough sets also get
      * l[11] all 0 and l[12] all 255, r[13] all 0 and r[14] all 255: distance 0 and the largest distance, 8 323 200,
      * r[20] and r[21] = l[15] with ONE byte each (not the same one) moved by 3: two different right descriptors at
        distance 9 from l[15], so best / second is decided by the index alone."""
    l, r = planted(nl, nr)
    l, r = quantize_u8(l * np.float32(512)), quantize_u8(r * np.float32(512))
    if nl > 20 and nr > 44:
        l[11], l[12], r[13], r[14] = 0, 255, 0, 255
        for k, j in ((0, 20), (1, 21)):
            r[j] = l[15]
            r[j, k] = l[15, k] + 3 if l[15, k] <= 252 else l[15, k] - 3
    return l, r


def position_coded(nl, nr):
    """l[i][k] = (7 i + 13 k) & 255, r[j][k] = (11 j + 3 k^2 + k) & 255: asymmetric in i / j and in k, values on both sides
    of 128 -- a wrong operand map, a row / column swap or a sign error cannot cancel.  Rows repeat with period 256: every
    left row has many equal nearest neighbours from 257 right rows on."""
    k = np.arange(128, dtype=np.int64)
    l = (7 * np.arange(nl, dtype=np.int64)[:, None] + 13 * k[None, :]) & 255
    r = (11 * np.arange(nr, dtype=np.int64)[:, None] + (3 * k * k + k)[None, :]) & 255
    return l.astype(np.uint8), r.astype(np.uint8)
