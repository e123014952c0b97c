"""Device time of an extraction in both feature orders (params.feature_order): the 1080p synthetic image of bench.py with
popsift_hip_set_profile(ctx, 2), alone and in a batch of 16, arrival order and raster order.  After 2 warm-ups the median
of 9 submits with minimum and maximum, per stage (report().ms_stage: the ordering pass of order.hip sits in `refine`) and
for the whole sequence (ms_device).  The stage events of a batch bracket the launches of the whole batch.
    python tools/order_time.py [--out profiles/order_time.txt]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from popsift_amd import _capi as hip
from popsift_amd.synth import synth

WARM, REPS = 2, 9
W, H = 1920, 1080
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "order_time.txt"))
args = ap.parse_args()

distinct = [synth(s, W, H) for s in (2, 100, 101, 102)]     # bench.py: seed 2 is image 0, seeds 100.. the rest of a batch
lines = []


def say(s):
    print(s)
    sys.stdout.flush()
    lines.append(s)


def stat(v):
    return "%8.4f (%8.4f ... %8.4f)" % (np.median(v), min(v), max(v))


say("%s, %d x %d, ms: median of %d (min ... max) after %d warm-ups" % (hip.device_info().name.decode(), W, H, REPS, WARM))
res = {}
for nb in (1, 16):
    imgs = [distinct[k % len(distinct)] for k in range(nb)]
    for order, name in ((hip.ORDER_ARRIVAL, "arrival"), (hip.ORDER_RASTER, "raster")):
        ctx = hip.Context(hip.default_params(feature_order=order))
        ctx.set_profile(2)
        rows = []
        for it in range(WARM + REPS):
            ctx.submit_batch(imgs).wait_batch()
            r = ctx.report()
            if it >= WARM:
                rows.append(list(r.ms_stage)[:len(hip.STAGES)] + [r.ms_device])
        rows = np.array(rows)
        res[(nb, name)] = rows
        say("batch %2d  %-7s  features of image 0: %d" % (nb, name, r.ext_total))
        for j, st in enumerate(hip.STAGES + ("ms_device",)):
            say("    %-12s %s" % (st, stat(rows[:, j])))
        ctx.close()
    d = np.median(res[(nb, "raster")], 0) - np.median(res[(nb, "arrival")], 0)
    j = hip.STAGES.index("refine")
    say("batch %2d  raster - arrival: refine %+.4f ms, ms_device %+.4f ms (%+.4f ms per image)" % (nb, d[j], d[-1], d[-1] / nb))
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
