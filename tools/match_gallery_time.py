"""Wall time of popsift_hip_match_pairs_gallery next to the loop of popsift_hip_match_pairs_bytes over the same members, in
one process per shape: planted_gallery sets (tests/gallery_rule.py).  Both are called through ctypes with buffers made
before the clock starts, so a time is the call with its download and nothing else.  The two alternate call by call: 2
warm-ups each, then REPS timed calls each; median and min - max.  Before any timing the pairs and offsets of the two are
compared byte for byte.  The yardstick is the per-pair loop.

Requirements: at 8 192 x 64 members of 8 192 the gallery median lies below the loop median by more than the two spreads
(max - min) together; at 95 386 x 1 member of 95 386, where grouping can win nothing, it is not above the per-pair call's
median by more than that call's spread.  The exit status says whether they held.

    python tools/match_gallery_time.py            every shape, each in a child process of its own under `timeout -k 10`,
                                                  one after the other; a shape that misses its requirement is
                                                  reported and the next one runs, any other failure stops the run
    python tools/match_gallery_time.py NL NM NR   a query of NL against NM members of NR, in this process
"""
import ctypes as C
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SHAPES = [(8192, 64, 8192), (8192, 8, 8192), (95386, 1, 95386)]
WARMUP, REPS = 2, 9
STEP_SECONDS = 420


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def one_shape(nl, nm, nr):
    import numpy as np
    from gallery_rule import planted_gallery
    from popsift_amd import _capi as hip

    lib = hip.lib()
    l, members = planted_gallery(nl, [nr] * nm)
    L = hip.ByteFeatures.from_host(l)
    sets = [hip.ByteFeatures.from_host(r) for r in members]
    g = hip.Gallery()
    for s in sets:
        g.add(s)
    g_pairs, g_off, g_n = np.zeros(nm * nl, hip.PAIR_DTYPE), np.zeros(nm + 1, np.int32), C.c_int(0)
    p_pairs, p_n = np.zeros((nm, nl), hip.PAIR_DTYPE), C.c_int(0)
    p_ptrs = [p_pairs[m].ctypes.data for m in range(nm)]
    p_counts = np.zeros(nm, np.int64)
    ok = True
    print("%d x %d members of %d descriptors, %d warm-ups, %d calls each, alternating" % (nl, nm, nr, WARMUP, REPS))
    for name, cross in (("default", 0), ("cross_check", 1)):
        opts = hip.MatchOpts(0.8, np.inf, cross, 0)

        def gallery():
            rc = lib.popsift_hip_match_pairs_gallery(L._h, g._h, C.byref(opts), g_pairs.ctypes.data, nm * nl,
                                                     g_off.ctypes.data, C.byref(g_n))
            assert rc == hip.OK, rc

        def loop():
            for m, s in enumerate(sets):
                rc = lib.popsift_hip_match_pairs_bytes(L._h, s._h, C.byref(opts), p_ptrs[m], nl, C.byref(p_n))
                assert rc == hip.OK, rc
                p_counts[m] = p_n.value

        gallery()
        loop()
        want = np.concatenate([p_pairs[m, :p_counts[m]] for m in range(nm)])
        same = (np.array_equal(np.diff(g_off), p_counts) and g_n.value == len(want) and
                g_pairs[:g_n.value].tobytes() == want.tobytes())
        tg, tp = [], []
        for k in range(WARMUP + REPS):
            for fn, ts in ((gallery, tg), (loop, tp)):
                t0 = time.perf_counter()
                fn()
                if k >= WARMUP:
                    ts.append((time.perf_counter() - t0) * 1e3)
        (mg, lo_g, hi_g), (mp, lo_p, hi_p) = stats(tg), stats(tp)
        print("  %-11s %8d pairs; identical: %s" % (name, g_n.value, same))
        print("    match_pairs_gallery          median %8.3f ms   min %8.3f   max %8.3f" % (mg, lo_g, hi_g))
        print("    loop of match_pairs_bytes    median %8.3f ms   min %8.3f   max %8.3f" % (mp, lo_p, hi_p))
        if nm > 1:
            held = mp - mg > (hi_g - lo_g) + (hi_p - lo_p)
            print("    loop / gallery %.2f x; medians apart by %.3f ms, spreads together %.3f ms: %s"
                  % (mp / mg, mp - mg, (hi_g - lo_g) + (hi_p - lo_p), "clear" if held else "NOT clear"))
            held = held or (nl, nm, nr) != SHAPES[0]
        else:
            held = mg - mp <= hi_p - lo_p
            print("    gallery - per-pair call %.3f ms; spread of the per-pair call %.3f ms: %s"
                  % (mg - mp, hi_p - lo_p, "not slower" if held else "SLOWER"))
        ok = ok and same and held
    sys.stdout.flush()
    return 0 if ok else 1


def main():
    if len(sys.argv) == 4:
        return one_shape(*map(int, sys.argv[1:]))
    from popsift_amd.srchash import kernel_source_hash
    print("# tools/match_gallery_time.py, kernel source hash %s" % kernel_source_hash())
    sys.stdout.flush()
    worst = 0
    for shape in SHAPES:
        rc = subprocess.call(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__)] +
                             [str(v) for v in shape])
        if rc not in (0, 1):
            print("# %d x %d x %d ended with status %d: stopping" % (shape + (rc,)))
            return rc
        worst = max(worst, rc)
    return worst


if __name__ == "__main__":
    sys.exit(main())
