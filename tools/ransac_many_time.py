"""Wall time of one popsift_hip_ransac_many against the loop of per-list calls (popsift_hip_ransac / popsift_hip_epipolar)
over the same lists on the same verifier, transfers and synchronisations included: both are synchronous calls, so the host
clock around them is what a caller pays.  T = 2048, max_err 0.5, homography on the planted scene of tests/ransac_rule.py
and the fundamental matrix on the two-view scene of tests/epipolar_rule.py, for 64, 256 and 1024 lists of 100 pairs and one
mixed set of 48 lists with 10 .. 2000 pairs.  After 3 warm-ups of both, 21 repeats alternating the two; the median with
minimum and maximum.  The two must return the same bytes, or the line says DIFFERENT and the exit status is 1.

--once NAME KIND [loop] runs the grouped call alone (with `loop`: the per-list calls alone) five times on one workload
(64x100, 256x100, 1024x100, mixed, 8x2000; homography, epipolar): the run to put under a kernel trace for the launches per
call, the score kernel's share, and the two score kernels side by side on long lists."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import ransac_rule as R
import epipolar_rule as E
from popsift_amd import _capi as hip

T, MAX_ERR, SEED, WARM, REPS = 2048, 0.5, 1, 3, 21
MIXED = [int(round(x)) for x in np.geomspace(10, 2000, 48)]
WORKLOADS = {"64x100": [100] * 64, "256x100": [100] * 256, "1024x100": [100] * 1024, "mixed": MIXED}
ONCE_ONLY = {"8x2000": [2000] * 8}     # long lists alone, for the two score kernels side by side under a trace


def lists_of(kind, lengths):
    """list k is the kind's planted scene of its length under scene seed 1 + k % 16"""
    made = {}
    out = []
    for k, n in enumerate(lengths):
        key = (n, 1 + k % 16)
        if key not in made:
            made[key] = E.two_view(*key)[0] if kind == "epipolar" else R.planted(*key)[0]
        out.append(made[key])
    return out


def csr(lists):
    offsets = np.zeros(len(lists) + 1, np.int32)
    offsets[1:] = np.cumsum([len(p) for p in lists])
    return np.concatenate(lists).astype(np.float32), offsets


def loop(v, kind, lists):
    if kind == "epipolar":
        return [v.epipolar(p, T, MAX_ERR, SEED) for p in lists]
    return [v.ransac(p, kind, T, MAX_ERR, SEED) for p in lists]


def main():
    v = hip.Verifier()
    if len(sys.argv) >= 4 and sys.argv[1] == "--once":
        lists = lists_of(sys.argv[3], {**WORKLOADS, **ONCE_ONLY}[sys.argv[2]])
        flat, offsets = csr(lists)
        for _ in range(5):
            if sys.argv[4:] == ["loop"]:
                loop(v, sys.argv[3], lists)
            else:
                v.ransac_many(flat, offsets, sys.argv[3], T, MAX_ERR, SEED)
        return 0
    print("T %d, wall ms, median of %d (min, max) after %d warm-ups, the two alternating" % (T, REPS, WARM))
    bad = 0
    for kind in ("homography", "epipolar"):
        for name, lengths in WORKLOADS.items():
            lists = lists_of(kind, lengths)
            flat, offsets = csr(lists)
            for _ in range(WARM):
                loop(v, kind, lists)
                v.ransac_many(flat, offsets, kind, T, MAX_ERR, SEED)
            tm, tl = [], []
            for _ in range(REPS):
                t0 = time.perf_counter()
                each = loop(v, kind, lists)
                tl.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                res, mask = v.ransac_many(flat, offsets, kind, T, MAX_ERR, SEED)
                tm.append((time.perf_counter() - t0) * 1e3)
            same = (res.tobytes() == b"".join(r.tobytes() for r, _ in each) and
                    mask.tobytes() == b"".join(m.tobytes() for _, m in each))
            bad += not same
            print("%-10s %-9s lists %5d pairs %7d | loop %9.3f ms (%9.3f, %9.3f) | many %9.3f ms (%9.3f, %9.3f) | x %6.2f | "
                  "inliers %7d  %s" % (kind, name, len(lists), len(flat), np.median(tl), min(tl), max(tl), np.median(tm), min(tm),
                                        max(tm), np.median(tl) / np.median(tm), int(res["n_inliers"].sum()),
                                        "same bytes" if same else "DIFFERENT"))
            sys.stdout.flush()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
