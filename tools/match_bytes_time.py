"""Wall time of popsift_hip_match_bytes next to the float popsift_hip_match_sets (AUTO path) on float32 of the same bytes,
in one process per size: planted_bytes sets (tests/match_bytes_rule.py) of 95 386 x 95 386 -- the descriptor count of a dense
1080p image -- and of 5 000 x 4 000.  2 warm-ups, then REPS calls each; median and min - max.  The rows of the two paths are
compared byte for byte.  Requirement at the large size: the byte median lies below the float median by more than the two
spreads (max - min) together; the exit status says whether it held.

    python tools/match_bytes_time.py            every size, each in a child process of its own under `timeout -k 10`,
                                                one after the other, stopping at the first that fails
    python tools/match_bytes_time.py NL NR      one size, in this process
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SIZES = [(5000, 4000), (95386, 95386)]
WARMUP, REPS = 2, 9
STEP_SECONDS = 420


def timed(fn):
    for _ in range(WARMUP):
        out = fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return out, ts[len(ts) // 2], ts[0], ts[-1]


def one_size(nl, nr):
    import numpy as np
    from match_bytes_rule import planted_bytes
    from popsift_amd import _capi as hip

    l, r = planted_bytes(nl, nr)
    L, R = hip.ByteFeatures.from_host(l), hip.ByteFeatures.from_host(r)
    LF, RF = hip.DevFeatures.from_host(l.astype(np.float32)), hip.DevFeatures.from_host(r.astype(np.float32))
    rows_b, mb, lo_b, hi_b = timed(lambda: L.match(R))
    rows_f, mf, lo_f, hi_f = timed(lambda: LF.match(RF))
    same = rows_b.tobytes() == rows_f.tobytes()
    clear = mf - mb > (hi_b - lo_b) + (hi_f - lo_f)
    print("%d x %d descriptors, %d warm-ups, %d calls each" % (nl, nr, WARMUP, REPS))
    print("  match_bytes           median %8.3f ms   min %8.3f   max %8.3f" % (mb, lo_b, hi_b))
    print("  match_sets (float)    median %8.3f ms   min %8.3f   max %8.3f" % (mf, lo_f, hi_f))
    print("  float / bytes %.2f x; medians apart by %.3f ms, spreads together %.3f ms: %s; rows identical: %s"
          % (mf / mb, mf - mb, (hi_b - lo_b) + (hi_f - lo_f), "clear" if clear else "NOT clear", same))
    sys.stdout.flush()
    return 0 if same and (clear or (nl, nr) != SIZES[-1]) else 1


def main():
    if len(sys.argv) == 3:
        return one_size(int(sys.argv[1]), int(sys.argv[2]))
    from popsift_amd.srchash import kernel_source_hash
    print("# tools/match_bytes_time.py, kernel source hash %s" % kernel_source_hash())
    sys.stdout.flush()
    for nl, nr in SIZES:
        rc = subprocess.call(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), str(nl), str(nr)])
        if rc != 0:
            print("# %d x %d ended with status %d: stopping" % (nl, nr, rc))
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
