"""numpy restatement of popsift_hip_match_pairs' rule (include/popsift_hip.h): which rows of the forward search
F = match(l, r) become pairs, given the reverse search B = match(r, l) and the options.  A helper of the tests, not a
test."""
import numpy as np

PAIR_DTYPE = np.dtype([("l", np.int32), ("r", np.int32), ("dist_best", np.float32), ("dist_second", np.float32)])


def keep_masks(F, B, ratio=0.8, max_dist2=np.inf, cross_check=False):
    """Conditions 2, 3 and 4 on F's rows, one mask each (all True where the option is off).  len(B) >= 1."""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = F["dist_best"] / F["dist_second"]                      # float32 / float32: the kernels' IEEE division
        k_ratio = q < np.float32(ratio) if ratio != 0 else np.ones(len(F), bool)   # a NaN quotient fails
    k_cap = F["dist_best"] <= np.float32(max_dist2)
    k_cross = B["best"][F["best"]] == np.arange(len(F)) if cross_check else np.ones(len(F), bool)
    return k_ratio, k_cap, k_cross


def expected_pairs(F, B, ratio=0.8, max_dist2=np.inf, cross_check=False):
    """The pair array of the rule: F has one row per left descriptor, B one per right descriptor."""
    if len(F) == 0 or len(B) == 0:                                 # condition 1
        return np.zeros(0, PAIR_DTYPE)
    k_ratio, k_cap, k_cross = keep_masks(F, B, ratio, max_dist2, cross_check)
    i = np.flatnonzero(k_ratio & k_cap & k_cross)
    out = np.zeros(len(i), PAIR_DTYPE)
    out["l"], out["r"] = i, F["best"][i]
    out["dist_best"], out["dist_second"] = F["dist_best"][i], F["dist_second"][i]
    return out


# the option sets the tests run: default, a tighter ratio, a cap alone, the cross-check alone, all three together.
# CAP sits in the middle of the planted near-copies' squared distances (128 x 0.02^2 ~ 0.051): it splits them.
CAP = 0.05
OPTION_SETS = [
    dict(),
    dict(ratio=0.6),
    dict(ratio=0.0, max_dist2=CAP),
    dict(ratio=0.0, cross_check=True),
    dict(ratio=0.8, max_dist2=CAP, cross_check=True),
]


def planted(nl, nr):
    """Random descriptors with a third of them near-copies and exact duplicates in the right set, as
    test_random_sets_match_the_oracle plants them.  Big enough sets also get
      * l[7]'s near-copy three times in the right set: best and second tie, the ratio test alone removes the row,
      * l[9]'s near-copy twice at distances 1 : 1.2 -- a quotient of 0.69, between the two ratios of OPTION_SETS,
      * l[200] = l[50], with one near-copy of them on the right: the cross-check alone removes row 200."""
    rng = np.random.default_rng(nl * 7919 + nr)
    l = rng.random((nl, 128), np.float32)
    r = rng.random((nr, 128), np.float32)
    k = min(nl, nr) // 3
    r[rng.permutation(nr)[:k]] = l[rng.permutation(nl)[:k]] + rng.normal(0, 0.02, (k, 128)).astype(np.float32)
    if nr > 4:
        r[nr - 1] = r[1]                     # exact duplicates: ties go to the lower index
        r[nr // 2] = r[1]
    if nl > 200 and nr > 8:
        r[1] = l[7] + rng.normal(0, 0.005, 128).astype(np.float32)
        r[nr - 1] = r[1]
        r[nr // 2] = r[1]
        step = rng.normal(0, 0.02, 128).astype(np.float32)
        r[5], r[6] = l[9] + step, l[9] + np.float32(1.2) * step
        l[200] = l[50]
        r[3] = l[50] + rng.normal(0, 0.005, 128).astype(np.float32)
    return l, r
