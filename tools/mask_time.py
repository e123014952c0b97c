"""What an extraction mask buys (popsift_hip_submit_batch_masked): the dense 1080p synthetic image of bench.py
(seed 2) in a batch of 16 with popsift_hip_set_profile(ctx, 2), for no mask, an all-visible mask, a checker of 64 px blocks,
10 % visible (one centred rectangle) and the masked entry point with null entries (the unmasked kernels).  The cases take
turns from submit to submit (--reversed: in the opposite order); after 3 warm-up rounds the median of 9 rounds with minimum
and maximum, per stage (report().ms_stage) and for the whole sequence (ms_device), in ms for the whole batch.
    python tools/mask_time.py [--reversed] [--out FILE]      (the two tables of profiles/mask_extraction.txt)"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from popsift_amd import _capi as hip
from popsift_amd.synth import synth

WARM, REPS, B = 3, 9, 16
W, H = 1920, 1080
ap = argparse.ArgumentParser()
ap.add_argument("--reversed", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()

img = synth(2, W, H)
my, mx = np.mgrid[0:H, 0:W]
checker = ((((mx // 64) + (my // 64)) % 2 == 0) * 255).astype(np.uint8)
rect = np.zeros((H, W), np.uint8)
rh, rw = int(H * 0.1 ** 0.5), int(W * 0.1 ** 0.5)
rect[(H - rh) // 2:(H - rh) // 2 + rh, (W - rw) // 2:(W - rw) // 2 + rw] = 255
cases = [("no mask", None), ("all visible", [np.full((H, W), 255, np.uint8)] * B), ("checker 64", [checker] * B),
         ("10 % rectangle", [rect] * B), ("null entries", [None] * B)]
if args.reversed:
    cases.reverse()

ctx = hip.Context(hip.default_params())
ctx.set_profile(2)
rows = {name: [] for name, _ in cases}
counts = {}
for it in range(WARM + REPS):
    for name, masks in cases:
        ctx.submit_batch([img] * B, masks)
        counts[name] = ctx.wait_batch()[0]
        rep = ctx.report()
        if it >= WARM:
            rows[name].append([rep.ms_device] + list(rep.ms_stage[:len(hip.STAGES)]))
ctx.close()

lines = ["dense 1080p image (synth seed 2), batch of %d, median of %d submits per case after %d warm-ups, the cases taking "
         "turns%s; ms for the whole batch, profile mode 2" % (B, REPS, WARM, " in reversed order" if args.reversed else ""),
         "%-16s %9s %8s %9s | %s" % ("case", "feats/img", "desc/img", "ms_device", "  ".join("%-11s" % s for s in hip.STAGES))]
for name, _ in cases:
    r = np.array(rows[name])
    med, lo, hi = np.median(r, axis=0), r.min(axis=0), r.max(axis=0)
    lines.append("%-16s %9d %8d %9.3f | %s" % (name, counts[name][0], counts[name][1], med[0],
                                               "  ".join("%-11.4f" % v for v in med[1:])))
    lines.append("%-16s %9s %8s %9s | %s" % ("  (min..max)", "", "", "%.3f..%.3f" % (lo[0], hi[0]),
                                             "  ".join("%.3f..%.3f" % (a, b) for a, b in zip(lo[1:], hi[1:]))))
print("\n".join(lines))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
