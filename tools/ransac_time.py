"""Wall time of popsift_hip_ransac and popsift_hip_epipolar, transfers included (the points go up, the result record and the
mask come down): after 2 warm-ups the median of 9 calls with minimum and maximum, for n in {2 000, 90 000} pairs x T in
{1 024, 16 384} hypotheses, both models on the planted scene of tests/ransac_rule.py and the fundamental matrix on the
two-view scene of tests/epipolar_rule.py (60 % inliers, max_err 0.5).  Beside each figure, for context only, one run of the
CPU restatement (tests/ransac_ref.c, tests/epipolar_ref.c) on one core for the same input (built with -march=native so that
fmaf is an instruction, which does not change its results), and whether the two agree as bytes.  Then, per n and model,
popsift_hip_refit from the last winner on the same points (4 and 16 rounds enqueued; the exact scene converges after one),
beside one run of tests/refit_ref.c."""
import os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import ransac_rule as R
import epipolar_rule as E
import refit_rule as F
from popsift_amd import _capi as hip

WARM, REPS = 2, 9
ref = R.Ref(tempfile.mkdtemp(), extra_flags=("-march=native",))
eref = E.Ref(tempfile.mkdtemp(), extra_flags=("-march=native",))
fref = F.Ref(tempfile.mkdtemp(), extra_flags=("-march=native",))
v = hip.Verifier()
print("popsift_hip_ransac / popsift_hip_epipolar: wall ms, median of %d (min, max) after %d warm-ups | tests/ransac_ref.c, one core, one run" % (REPS, WARM))
for n in (2000, 90000):
    for model, name in ((R.HOMOGRAPHY, "homography"), (R.AFFINE, "affine"), (None, "epipolar")):
        pts = E.two_view(n, 1)[0] if model is None else R.planted(n, 1, model)[0]
        gpu = (lambda T: v.epipolar(pts, T, 0.5, 1)) if model is None else (lambda T: v.ransac(pts, model, T, 0.5, 1))
        cpu_ref = ((lambda T: eref.epipolar(pts, T, 0.5, 1, trace=False)) if model is None else
                   (lambda T: ref.ransac(pts, model, T, 0.5, 1, trace=False)))
        for T in (1024, 16384):
            for _ in range(WARM):
                gpu(T)
            ts = []
            for _ in range(REPS):
                t0 = time.perf_counter()
                res, mask = gpu(T)
                ts.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            want = cpu_ref(T)
            cpu = (time.perf_counter() - t0) * 1e3
            same = res.tobytes() == want["result"].tobytes() and mask.tobytes() == want["mask"].tobytes()
            print("n %6d  T %6d  %-10s  %8.3f ms (min %8.3f, max %8.3f) | cpu %10.1f ms | inliers %6d  valid %6d  %s"
                  % (n, T, name, np.median(ts), min(ts), max(ts), cpu, res["n_inliers"], res["n_valid"],
                     "same bytes" if same else "DIFFERENT"))
            sys.stdout.flush()
        kind = F.EPIPOLAR if model is None else model
        for rounds in (4, 16):
            for _ in range(WARM):
                v.refit(pts, kind, res["H"], 0.5, rounds)
            ts = []
            for _ in range(REPS):
                t0 = time.perf_counter()
                fit, mask = v.refit(pts, kind, res["H"], 0.5, rounds)
                ts.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            want = fref.refit(pts, kind, res["H"], 0.5, rounds)
            cpu = (time.perf_counter() - t0) * 1e3
            same = fit.tobytes() == want["result"].tobytes() and mask.tobytes() == want["mask"].tobytes()
            print("n %6d  refit %2d  %-10s  %8.3f ms (min %8.3f, max %8.3f) | cpu %10.1f ms | inliers %6d -> %6d  rounds %d  stop %d  %s"
                  % (n, rounds, name, np.median(ts), min(ts), max(ts), cpu, fit["n_start"], fit["n_inliers"], fit["rounds"],
                     fit["stop"], "same bytes" if same else "DIFFERENT"))
            sys.stdout.flush()
