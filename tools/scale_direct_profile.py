"""Driver for the ScaleDirect profile: synthetic 1920x1080 and 640x480 images, one and sixteen per
launch, through the default scaling mode, ScaleDirect's fused path (SCALE_PATH 0) and its yardstick path (SCALE_PATH 1).
`python tools/scale_direct_profile.py` prints the pyramid stage of every configuration (set_profile(2): HIP events
around the pyramid's launches, popsift_hip_report.ms_stage[PYRAMID]; median of REPS submits after one warm-up).
Run it under `rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/scale_direct_profile.py --trace` for the
kernels' own times (profiling off, the same submits); `python tools/scale_direct_profile.py --summarize
<dir>/run_results.db` cuts that trace into submits at the first pyramid kernel after a keypoint kernel and prints, per
configuration, the pyramid launches per submit and each pyramid kernel's own time (median over the submits after the
first), and for the yardstick path the level-0 launch of each octave."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from popsift_amd import _capi as hip  # noqa: E402
from popsift_amd.synth import synth  # noqa: E402

REPS = int(os.environ.get("REPS", "10"))
SIZES = ((1920, 1080), (640, 480))
BATCHES = (1, 16)
MODES = (("default", 0, 0), ("scale_direct fused", 1, 0), ("scale_direct yardstick", 1, 1))
CONFIGS = [(s, nb, m) for s in SIZES for nb in BATCHES for m in MODES]


def _is_pyr(name):
    return "blur" in name or "pyr_" in name


def _short(n):
    return n.replace("void ", "").replace("popsift_hip::(anonymous namespace)::", "").split("(")[0]


def summarize(db):
    import sqlite3
    rows = sqlite3.connect(db).execute("select name, start, end from kernels order by start").fetchall()
    subs, cur, prev_pyr = [], None, False
    for name, start, end in rows:
        pyr = _is_pyr(name)
        if pyr and not prev_pyr:
            cur = []
            subs.append(cur)
        prev_pyr = pyr
        if cur is not None and pyr:
            cur.append((_short(name), start, end))
    per = REPS + 1
    assert len(subs) == per * len(CONFIGS), (len(subs), per * len(CONFIGS))
    for i, ((w, h), nb, (mode, _, _)) in enumerate(CONFIGS):
        group = subs[i * per + 1:(i + 1) * per]
        span = [(r[-1][2] - r[0][1]) / 1e3 for r in group]
        busy = [sum(e - s for _, s, e in r) / 1e3 for r in group]
        print("%dx%d, %2d per launch, %-22s: %3d pyramid launches per submit, first -> last kernel %8.1f us, kernels' own "
              "time %8.1f us (median of %d)" % (w, h, nb, mode, len(group[0]), float(np.median(span)),
                                                float(np.median(busy)), len(group)))
        names = []
        for n, _, _ in group[0]:
            if n not in names:
                names.append(n)
        for n in names:
            t = [sum(e - s for nm, s, e in r if nm == n) / 1e3 for r in group]
            c = sum(1 for nm, _, _ in group[0] if nm == n)
            print("    %-58s %3d launches %9.1f us" % (n[:58], c, float(np.median(t))))
            if n.startswith("k_blur_tile_sep"):
                # the yardstick's level-0 launches one by one, octave 0 first: octave 0 stages its source texels in LDS,
                # the downsampled octaves gather them from global memory
                per_oct = [[e - s for nm, s, e in r if nm == n] for r in group]
                print("        per octave: " + " ".join("%.1f" % (float(np.median([p[o] for p in per_oct])) / 1e3)
                                                  for o in range(c)) + " us")


def main(trace):
    for (w, h), nb, (mode, sd, path) in CONFIGS:
        imgs = [synth(1 + k, w, h) for k in range(nb)]
        ctx = hip.Context(hip.default_params(scale_direct=sd))
        if sd:
            ctx.debug_set(hip.DEBUG_SCALE_PATH, path)
        if not trace:
            ctx.set_profile(2)
        ms, dev = [], []
        for _ in range(REPS + 1):
            ctx.submit_batch(imgs)
            counts = ctx.wait_batch()
            r = ctx.report()
            ms.append(r.ms_stage[0])  # POPSIFT_HIP_STAGE_PYRAMID
            dev.append(r.ms_device)
        px = r.pyramid_pixels
        if trace:
            print("%dx%d, %2d per launch, %-22s features of image 0: %d" % (w, h, nb, mode, counts[0][0]))
        else:
            p = float(np.median(ms[1:]))
            print("%dx%d, %2d per launch, %-22s pyramid stage %.3f ms per launch, %.3f ms per image "
                  "(%.1f Mpix of planes per image), device %.3f ms, features of image 0: %d" % (
                      w, h, nb, mode, p, p / nb, px / 1e6, float(np.median(dev[1:])), counts[0][0]))
        ctx.close()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        main("--trace" in sys.argv[1:])
