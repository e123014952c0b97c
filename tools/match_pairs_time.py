"""Wall time of correspondences between two 1080p images (about 95 k descriptors a side), each a median of 5 with min
and max:
  (a) match_sets l -> r                                   (b) match_sets both ways + the numpy filter (the yardstick)
  (c) match_pairs, default options                        (d) match_pairs with ratio, distance cap and cross-check
  (e) match_pairs with the cross-check and a ratio no row passes: the forward sweep, the target kernels and the 4-byte
      read-back of |J| between the sweeps, nothing after it -- (e) - (a) bounds what that synchronisation costs
      (only where no row passes: bit-identical descriptors on both sides have distance 0 and pass every ratio)
for an unrelated pair (few rows match) and a shifted pair (most match).  A library without popsift_hip_match_pairs
(POPSIFT_HIP_LIB pointing at an older build) gets (a) and (b) only."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from popsift_amd import _capi as hip
from popsift_amd.synth import synth

REPS = 5
has_pairs = hasattr(__import__("ctypes").CDLL(hip.LIB_PATH), "popsift_hip_match_pairs")
if not has_pairs:
    hip.SYMBOLS = [s for s in hip.SYMBOLS if s[0] not in ("popsift_hip_match_pairs", "popsift_hip_default_match_opts")]


def timed(fn):
    fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, "%8.3f ms (min %8.3f, max %8.3f)" % (np.median(ts), min(ts), max(ts))


def host_filter(F, B, ratio, cap, cross):
    with np.errstate(divide="ignore", invalid="ignore"):
        keep = (F["dist_best"] / F["dist_second"] < np.float32(ratio)) & (F["dist_best"] <= np.float32(cap))
    if cross:
        keep &= B["best"][F["best"]] == np.arange(len(F))
    return np.flatnonzero(keep)


img = synth(2, 1920, 1080)
for name, other in (("unrelated", synth(102, 1920, 1080)), ("shifted", np.roll(img, (3, 5), axis=(0, 1)))):
    L, R = hip.Context().submit(img).clone_results(), hip.Context().submit(other).clone_results()
    F, ta = timed(lambda: L.match(R))
    cap = float(np.median(F["dist_best"][F["accept"] == 1]))
    both, tb = timed(lambda: host_filter(L.match(R), R.match(L), 0.8, cap, True))
    targets = np.unique(F["best"][host_filter(F, None, 0.8, cap, False)])
    print("%s: %d x %d descriptors, cap %.4f, |J| %d" % (name, L.info()[2], R.info()[2], cap, len(targets)))
    print("  (a) match_sets l->r                 %s  accepted %d" % (ta, int(F["accept"].sum())))
    print("  (b) match_sets both ways + filter   %s  pairs %d" % (tb, len(both)))
    if has_pairs:
        pc, tc = timed(lambda: L.match_pairs(R))
        pd, td = timed(lambda: L.match_pairs(R, ratio=0.8, max_dist2=cap, cross_check=True))
        print("  (c) match_pairs, defaults           %s  pairs %d" % (tc, len(pc)))
        print("  (d) match_pairs, all three filters  %s  pairs %d" % (td, len(pd)))
        pe, te = timed(lambda: L.match_pairs(R, ratio=1e-30, cross_check=True))
        print("  (e) forward sweep + |J| read-back   %s  pairs %d" % (te, len(pe)))
        assert np.array_equal(pd["l"], both) and np.array_equal(pc["l"], np.flatnonzero(F["accept"] == 1))
    sys.stdout.flush()
