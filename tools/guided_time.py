"""Wall time of guided matching between two 1080p images (about 95 k descriptors a side): synth(2) and its np.roll by
(3, 5), so the true model is the translation (5, 3).  Each call includes its downloads; 2 warm-ups, then a median of 5 with
min and max:
  (a) match_pairs, ratio 0.8 + cross-check                (the unguided search both ways)
  (b) match_pairs_guided, homography = the translation, max_err 2, the same filters
  (c) match_pairs_guided, the translation's fundamental matrix, max_err 2
  (d) (b) with max_err 50
`--only b` (or c) runs that call alone, 3 times after a warm-up: the run to put under rocprofv3 --kernel-trace --stats for
the kernels' own times."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from popsift_amd import _capi as hip
from popsift_amd.synth import synth

WARM, REPS = 2, 5
SHIFT = (3, 5)                                           # rows, columns
H = np.array([[1, 0, SHIFT[1]], [0, 1, SHIFT[0]], [0, 0, 1]], np.float32)
F = np.array([[0, 0, SHIFT[0]], [0, 0, -SHIFT[1]], [-SHIFT[0], SHIFT[1], 0]], np.float32) / 5   # [t]_x, t = (5, 3, 0)


def timed(fn):
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, "%8.3f ms (min %8.3f, max %8.3f)" % (np.median(ts), min(ts), max(ts))


img = synth(2, 1920, 1080)
L, R = hip.Context().submit(img).clone_results(), hip.Context().submit(np.roll(img, SHIFT, axis=(0, 1))).clone_results()
calls = dict(
    a=("match_pairs, ratio 0.8 + cross-check     ", lambda: L.match_pairs(R, cross_check=True)),
    b=("guided, homography, max_err 2            ", lambda: L.match_pairs_guided(R, "homography", H, 2.0, cross_check=True)),
    c=("guided, epipolar, max_err 2              ", lambda: L.match_pairs_guided(R, "epipolar", F, 2.0, cross_check=True)),
    d=("guided, homography, max_err 50           ", lambda: L.match_pairs_guided(R, "homography", H, 50.0, cross_check=True)),
)
if len(sys.argv) == 3 and sys.argv[1] == "--only":
    for _ in range(4):
        n = len(calls[sys.argv[2]][1]())
    print("(%s) alone, 4 calls, pairs %d" % (sys.argv[2], n))
    sys.exit(0)
print("%d x %d descriptors" % (L.info()[2], R.info()[2]))
out = {}
for k, (name, fn) in calls.items():
    out[k], t = timed(fn)
    print("  (%s) %s %s  pairs %d" % (k, name, t, len(out[k])))
    sys.stdout.flush()
for k in "bcd":
    rows = L.match_guided(R, "epipolar" if k == "c" else "homography", F if k == "c" else H, 50.0 if k == "d" else 2.0)
    print("  (%s) candidates found a best in %d rows, a second in %d" % (k, (rows["best"] >= 0).sum(), (rows["second"] >= 0).sum()))
# every unguided pair that agrees with the translation within 2 px is a guided pair (b)
pts = L.pair_points(R, out["a"])
agree = np.hypot(pts[:, 0] + SHIFT[1] - pts[:, 2], pts[:, 1] + SHIFT[0] - pts[:, 3]) <= 1.999
print("  unguided pairs within 2 px of the translation: %d, of them among (b): %d"
      % (agree.sum(), np.isin(out["a"]["l"][agree], out["b"]["l"]).sum()))
