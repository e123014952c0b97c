"""Wall time of popsift_hip_match_pairs_links next to the two things a caller could do without it, in one process per shape:
planted_gallery sets (tests/gallery_rule.py).
  (i)  the loop of popsift_hip_match_pairs_bytes over the same links, with every member as a byte set made beforehand;
  (ii) one popsift_hip_match_pairs_gallery per distinct left member, with that member as a prepared query set.
All are called through ctypes with buffers made before the clock starts, so a time is the call with its download and
nothing else.  The three alternate call by call: 2 warm-ups each, then REPS timed calls each; median and min - max.  Before
any timing the pairs and offsets of the links call are compared byte for byte with (i), and the lists (ii) returns for the
links with them.

Requirements: on the first two shapes the links median lies below the faster of (i) and (ii) by more than the two spreads
(max - min) together; on the single link it is not above the per-pair call's median by more than that sum.  The exit status
says whether they held.

    python tools/match_links_time.py               every shape, each in a child process of its own under `timeout -k 10`,
                                                   one after the other; a shape that misses its requirement is
                                                   reported and the next one runs, any other failure stops the run
    python tools/match_links_time.py NM NR KIND K  NM members of NR; KIND all, seq (K successors) or one (the link (0, 1))
"""
import ctypes as C
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SHAPES = [(64, 8192, "all", 0), (256, 2048, "seq", 4), (2, 95386, "one", 0)]
WARMUP, REPS = 2, 9
STEP_SECONDS = 540


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def one_shape(nm, nr, kind, k):
    import numpy as np
    from gallery_rule import planted_gallery
    from popsift_amd import _capi as hip

    lib = hip.lib()
    members = planted_gallery(nr, [nr] * nm)[1]
    sets = [hip.ByteFeatures.from_host(r) for r in members]
    g = hip.Gallery()
    for s in sets:
        g.add(s)
    links = {"all": hip.all_links(nm), "seq": hip.sequential_links(nm, k), "one": hip.as_links([(0, 1)])}[kind]
    n_links, rows = len(links), len(links) * nr
    lefts = np.unique(links["a"]).tolist()
    l_pairs, l_off, l_n = np.zeros(rows, hip.PAIR_DTYPE), np.zeros(n_links + 1, np.int32), C.c_int(0)
    p_pairs, p_n = np.zeros((n_links, nr), hip.PAIR_DTYPE), C.c_int(0)
    p_ptrs = [p_pairs[e].ctypes.data for e in range(n_links)]
    p_counts = np.zeros(n_links, np.int64)
    q_pairs, q_off, q_n = np.zeros((len(lefts), nm * nr), hip.PAIR_DTYPE), np.zeros((len(lefts), nm + 1), np.int32), C.c_int(0)
    ok = True
    print("%d members of %d descriptors, %d links (%s), %d warm-ups, %d calls each, alternating"
          % (nm, nr, n_links, kind if kind != "seq" else "seq %d" % k, WARMUP, REPS))
    for name, cross in (("default", 0), ("cross_check", 1)):
        opts = hip.MatchOpts(0.8, np.inf, cross, 0)

        def by_links():
            rc = lib.popsift_hip_match_pairs_links(g._h, links.ctypes.data, n_links, C.byref(opts), l_pairs.ctypes.data, rows,
                                                   l_off.ctypes.data, C.byref(l_n))
            assert rc == hip.OK, rc

        def by_pair():
            for e in range(n_links):
                rc = lib.popsift_hip_match_pairs_bytes(sets[links["a"][e]]._h, sets[links["b"][e]]._h, C.byref(opts), p_ptrs[e], nr,
                                                       C.byref(p_n))
                assert rc == hip.OK, rc
                p_counts[e] = p_n.value

        def by_query():
            for i, a in enumerate(lefts):
                rc = lib.popsift_hip_match_pairs_gallery(sets[a]._h, g._h, C.byref(opts), q_pairs[i].ctypes.data, nm * nr,
                                                         q_off[i].ctypes.data, C.byref(q_n))
                assert rc == hip.OK, rc

        by_links()
        by_pair()
        by_query()
        want = np.concatenate([p_pairs[e, :p_counts[e]] for e in range(n_links)])
        same = (np.array_equal(np.diff(l_off), p_counts) and l_n.value == len(want) and
                l_pairs[:l_n.value].tobytes() == want.tobytes())
        for e in range(n_links):
            i, b = lefts.index(int(links["a"][e])), int(links["b"][e])
            same = same and q_pairs[i, q_off[i, b]:q_off[i, b + 1]].tobytes() == l_pairs[l_off[e]:l_off[e + 1]].tobytes()
        times = {"links": [], "pair": [], "query": []}
        for r in range(WARMUP + REPS):
            for fn, key in ((by_links, "links"), (by_pair, "pair"), (by_query, "query")):
                t0 = time.perf_counter()
                fn()
                if r >= WARMUP:
                    times[key].append((time.perf_counter() - t0) * 1e3)
        (ml, lo_l, hi_l), (mp, lo_p, hi_p), (mq, lo_q, hi_q) = stats(times["links"]), stats(times["pair"]), stats(times["query"])
        print("  %-11s %8d pairs; identical: %s" % (name, l_n.value, same))
        print("    match_pairs_links                 median %9.3f ms   min %9.3f   max %9.3f" % (ml, lo_l, hi_l))
        print("    (i)  loop of match_pairs_bytes    median %9.3f ms   min %9.3f   max %9.3f   %.2f x" % (mp, lo_p, hi_p, mp / ml))
        print("    (ii) match_pairs_gallery per left median %9.3f ms   min %9.3f   max %9.3f   %.2f x" % (mq, lo_q, hi_q, mq / ml))
        if kind != "one":
            mo, lo_o, hi_o = min((mp, lo_p, hi_p), (mq, lo_q, hi_q))
            both = (hi_l - lo_l) + (hi_o - lo_o)
            held = mo - ml > both
            print("    the faster of (i) and (ii) / links %.2f x; medians apart by %.3f ms, spreads together %.3f ms: %s"
                  % (mo / ml, mo - ml, both, "clear" if held else "NOT clear"))
        else:
            both = (hi_l - lo_l) + (hi_p - lo_p)
            held = ml - mp <= both
            print("    links - per-pair call %.3f ms; spreads together %.3f ms: %s" % (ml - mp, both, "not slower" if held else "SLOWER"))
        ok = ok and same and held
    sys.stdout.flush()
    return 0 if ok else 1


def main():
    if len(sys.argv) == 5:
        return one_shape(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4]))
    from popsift_amd.srchash import kernel_source_hash
    print("# tools/match_links_time.py, kernel source hash %s" % kernel_source_hash())
    sys.stdout.flush()
    worst = 0
    for shape in SHAPES:
        rc = subprocess.call(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__)] +
                             [str(v) for v in shape])
        if rc not in (0, 1):
            print("# %s ended with status %d: stopping" % (shape, rc))
            return rc
        worst = max(worst, rc)
    return worst


if __name__ == "__main__":
    sys.exit(main())
