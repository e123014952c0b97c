"""Device time of an extraction with popsift_hip_set_keep_strongest: the 1080p synthetic image of bench.py with
popsift_hip_set_profile(ctx, 2), alone and in a batch of 16, with the setting off, at INT32_MAX (responses only, nothing
thinned) and at 32000, 8000 and 2000.  One context per batch size; the settings alternate from submit to submit.  After 2
warm-up rounds the median of 9 rounds with minimum and maximum, per stage (report().ms_stage: the pass of strongest.hip
sits in `refine`) and for the whole sequence (ms_device).  The stage events of a batch bracket the launches of the whole
batch.
    python tools/strongest_time.py [--out profiles/strongest_time.txt]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from popsift_amd import _capi as hip
from popsift_amd.synth import synth

WARM, REPS = 2, 9
W, H = 1920, 1080
SETTINGS = (0, 2 ** 31 - 1, 32000, 8000, 2000)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strongest_time.txt"))
args = ap.parse_args()

distinct = [synth(s, W, H) for s in (2, 100, 101, 102)]     # bench.py: seed 2 is image 0, seeds 100.. the rest of a batch
lines = []


def say(s):
    print(s)
    sys.stdout.flush()
    lines.append(s)


def stat(v):
    return "%8.4f (%8.4f ... %8.4f)" % (np.median(v), min(v), max(v))


def name(n):
    return "off" if n == 0 else "INT32_MAX" if n == 2 ** 31 - 1 else str(n)


say("%s, %d x %d, ms: median of %d (min ... max) after %d warm-ups" % (hip.device_info().name.decode(), W, H, REPS, WARM))
for nb in (1, 16):
    imgs = [distinct[k % len(distinct)] for k in range(nb)]
    ctx = hip.Context(hip.default_params())
    ctx.set_profile(2)
    rows = {n: [] for n in SETTINGS}
    kept = {}
    for it in range(WARM + REPS):
        for n in SETTINGS:
            counts = ctx.set_keep_strongest(n).submit_batch(imgs).wait_batch()
            r = ctx.report()
            kept[n] = counts[0]
            if it >= WARM:
                rows[n].append(list(r.ms_stage)[:len(hip.STAGES)] + [r.ms_device])
    ctx.close()
    rows = {n: np.array(v) for n, v in rows.items()}
    for n in SETTINGS:
        say("batch %2d  keep_strongest %-9s  image 0: %d features, %d descriptors" % (nb, name(n), kept[n][0], kept[n][1]))
        for j, st in enumerate(hip.STAGES + ("ms_device",)):
            say("    %-12s %s" % (st, stat(rows[n][:, j])))
    j = hip.STAGES.index("refine")
    k = [hip.STAGES.index(s) for s in ("orientation", "scan", "descriptor")]
    for n in SETTINGS[1:]:
        d = np.median(rows[n], 0) - np.median(rows[0], 0)
        say("batch %2d  %-9s - off: refine %+.4f ms, orientation + scan + descriptor %+.4f ms, ms_device %+.4f ms (%+.4f ms per image)"
            % (nb, name(n), d[j], d[k].sum(), d[-1], d[-1] / nb))
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
