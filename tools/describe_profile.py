"""Driver for the describe profile: a 1080p synthetic image is extracted, then described with the
extraction's own keypoints (one frame per feature, octave / level hints set, given orientation = the first one) and with
100 000 random frames (uniform positions, log-uniform sigma, hints -1), in both orientation modes, REPS times each.
Run it under `rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/describe_profile.py` for the kernels'
own times; it prints the device time of each run (HIP events, popsift_hip_report.ms_device).
`python tools/describe_profile.py --summarize <dir>/run_results.db` turns that trace into the per-run kernel table of
profiles/r05_describe_*.txt: runs are cut at the level-0 blur launch that starts each one, the first run of every kind is
dropped, and each kernel's own time is the median over the others."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from popsift_amd import _capi as hip  # noqa: E402
from popsift_amd.synth import synth  # noqa: E402

REPS = int(os.environ.get("REPS", "5"))


RUNS = ("extract", "own/given", "own/compute", "random/given", "random/compute")


def summarize(db):
    import sqlite3
    rows = sqlite3.connect(db).execute("select name, start, end from kernels order by start").fetchall()
    runs, cur = [], None
    for name, start, end in rows:
        if "k_blur_tile<" in name and ", 1, " in name:  # level 0 from the u8 input: the first launch of a run
            cur = []
            runs.append(cur)
        if cur is not None:
            cur.append((name, start, end))
    runs = runs[1:]  # the extraction that made the frames
    per = len(runs) // len(RUNS)
    short = lambda n: n.replace("void ", "").replace("popsift_hip::(anonymous namespace)::", "").split("(")[0]
    for i, kind in enumerate(RUNS):
        group = runs[i * per + 1:(i + 1) * per]
        span = [(r[-1][2] - r[0][1]) / 1e3 for r in group]
        busy = [sum(e - s for _, s, e in r) / 1e3 for r in group]
        print("%s: %d runs, first kernel -> last kernel %.1f us (median), kernels' own time %.1f us" % (
            kind, len(group), float(np.median(span)), float(np.median(busy))))
        names = []
        for name, _, _ in group[0]:
            if short(name) not in names:
                names.append(short(name))
        for n in names:
            t = [sum(e - s for nm, s, e in r if short(nm) == n) / 1e3 for r in group]
            c = sum(1 for nm, _, _ in group[0] if short(nm) == n)
            if "blur" in n or "pyr_" in n:
                continue
            print("    %-60s %3d launches %9.1f us" % (n[:60], c, float(np.median(t))))
        pyr = [sum(e - s for nm, s, e in r if "blur" in short(nm) or "pyr_" in short(nm)) / 1e3 for r in group]
        print("    %-60s             %9.1f us" % ("pyramid (every blur / tail launch)", float(np.median(pyr))))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--summarize":
        return summarize(sys.argv[2])
    img = synth(1, 1920, 1080)
    ctx = hip.Context(hip.default_params())
    feats, desc = ctx.submit(img).fetch()
    ext = ctx.extrema()
    own = np.zeros(len(feats), hip.FRAME_DTYPE)
    for k in ("xpos", "ypos", "sigma"):
        own[k] = feats[k]
    own["orientation"] = feats["orientation"][:, 0]
    own["octave"], own["level"] = feats["debug_octave"], ext["lpos"]
    rng = np.random.default_rng(0)
    n = 100000
    rnd = np.zeros(n, hip.FRAME_DTYPE)
    rnd["xpos"], rnd["ypos"] = rng.uniform(0, 1919, n), rng.uniform(0, 1079, n)
    rnd["sigma"] = np.exp2(rng.uniform(-0.5, 4.5, n))
    rnd["orientation"] = rng.uniform(-np.pi, np.pi, n)
    rnd["octave"], rnd["level"] = -1, -1
    runs = [("extract", None, None), ("own/given", own, "given"), ("own/compute", own, "compute"),
            ("random/given", rnd, "given"), ("random/compute", rnd, "compute")]
    for name, fr, mode in runs:
        ms = []
        for _ in range(REPS + 1):
            if fr is None:
                nf, nd = ctx.submit(img).wait()
            else:
                ctx.describe_batch_async([img], [fr], mode)
                nf, nd = ctx.wait()
            ms.append(ctx.report().ms_device)
        r = ctx.report()
        print("%-15s frames %6s features %6d valid %6d descriptors %6d  device ms (median of %d, first dropped) %.3f" % (
            name, "-" if fr is None else len(fr), nf, r.ext_total, nd, REPS, float(np.median(ms[1:]))))
    ctx.close()


if __name__ == "__main__":
    main()
