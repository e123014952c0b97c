"""ctypes front of tests/ransac_ref.c, the CPU restatement of the verifier's rule (include/popsift_hip.h,
popsift_hip_ransac), and the scenes the verifier's tests share."""
import ctypes as C
import os
import subprocess

import numpy as np

from popsift_amd.synth import oxford_like_homographies

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ransac_ref.c")
HOMOGRAPHY, AFFINE = 0, 1
SAMPLE_SIZE = {HOMOGRAPHY: 4, AFFINE: 3}
RESULT_DTYPE = np.dtype([("H", np.float32, (9,)), ("n_inliers", np.int32), ("hypothesis", np.int32),
                         ("n_valid", np.int32), ("reserved", np.int32)])
TIE_TO_HIGHEST, NO_W_TEST = 1, 2   # `variant` bits of rr_ransac: a deliberately broken step
W, H = 800, 640                    # the image the scenes' points lie in


class Ref:
    """Built with gcc -O2 -ffp-contract=off into `build_dir` (extra flags only for timing: they must not change results)."""

    def __init__(self, build_dir, extra_flags=()):
        so = os.path.join(str(build_dir), "libransac_ref.so")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", *extra_flags, "-fPIC", "-shared", "-o", so, SRC, "-lm"])
        self.lib = C.CDLL(so)
        vp = C.c_void_p
        self.lib.rr_ransac.restype = None
        self.lib.rr_ransac.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint32, C.c_int, vp, vp, vp, vp, vp]
        self.lib.rr_samples.restype = None
        self.lib.rr_samples.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, vp, vp]

    def ransac(self, pts, model, T, max_err, seed, variant=0, trace=True):
        """-> dict(samples (T, 4), models (T, 9), counts (T,), result (RESULT_DTYPE record), mask (n,) uint8)"""
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        n = len(pts)
        out = dict(samples=np.zeros((T, 4), np.int32), models=np.zeros((T, 9), np.float32), counts=np.zeros(T, np.int32),
                   mask=np.zeros(n, np.uint8))
        res = np.zeros(1, RESULT_DTYPE)
        ptr = lambda a: a.ctypes.data if trace and a.size else None
        self.lib.rr_ransac(pts.ctypes.data if n else None, n, model, T, max_err, seed, variant, ptr(out["samples"]),
                           ptr(out["models"]), ptr(out["counts"]), res.ctypes.data, out["mask"].ctypes.data if n else None)
        out["result"] = res[0]
        return out

    def samples(self, seed, n, model, T):
        """-> (samples (T, 4), valid (T,))"""
        s, v = np.zeros((T, 4), np.int32), np.zeros(T, np.int32)
        self.lib.rr_samples(seed, n, model, T, s.ctypes.data, v.ctypes.data)
        return s, v


# ---- scenes: (n, 4) float32 rows (x, y, x', y')

def pixel_homography(k=2):
    """homography k of popsift_amd.synth.oxford_like_homographies (given in normalised image coordinates) in pixels"""
    cx, cy, sc = (W - 1) / 2.0, (H - 1) / 2.0, 0.5 * np.hypot(W, H)
    N = np.array([[1 / sc, 0, -cx / sc], [0, 1 / sc, -cy / sc], [0, 0, 1]])
    return np.linalg.inv(N) @ oxford_like_homographies()[k] @ N


def project(Hm, xy):
    """float64 projection of (n, 2) points"""
    xy = np.asarray(xy, np.float64)
    q = np.c_[xy, np.ones(len(xy))] @ np.asarray(Hm, np.float64).T
    return q[:, :2] / q[:, 2:3]


def planted(n=1000, seed=1, model=HOMOGRAPHY, inlier_frac=0.6):
    """-> (pts, planted mask, the planted 3 x 3 map).  The right point of an inlier is the float64 image of its left point
    rounded to float32, no noise; an outlier lies 20 .. 200 px from its true image."""
    rng = np.random.default_rng(seed)
    Hm = pixel_homography()
    if model == AFFINE:
        Hm = np.vstack([Hm[:2] / Hm[2, 2], [0.0, 0.0, 1.0]])
    left = (rng.random((n, 2)) * [W - 1, H - 1]).astype(np.float32)
    right = project(Hm, left)
    inl = np.zeros(n, bool)
    inl[rng.permutation(n)[:int(round(n * inlier_frac))]] = True
    ang, r = rng.random(n) * 2 * np.pi, 20.0 + 180.0 * rng.random(n)
    right[~inl] += np.c_[r * np.cos(ang), r * np.sin(ang)][~inl]
    return np.c_[left, right.astype(np.float32)].astype(np.float32), inl.astype(np.uint8), Hm


def all_outliers(n, seed=2):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 4)) * [W - 1, H - 1, W - 1, H - 1]).astype(np.float32)


def collinear(n, seed=3):
    """left points on one line: every sample is degenerate for both models"""
    rng = np.random.default_rng(seed)
    t = rng.random(n) * 600.0
    left = np.c_[50.0 + t, 40.0 + 0.5 * t]
    return np.c_[left, project(pixel_homography(), left)].astype(np.float32)


def identical(n):
    return np.tile(np.array([[100.0, 50.0, 120.0, 60.0]], np.float32), (n, 1))


def with_nan(n, seed=4, model=HOMOGRAPHY):
    """the planted scene with one pair whose left x is NaN and one whose right y is +inf"""
    pts, inl, _ = planted(n, seed, model)
    pts[n // 3, 0] = np.nan
    pts[n // 2, 3] = np.inf
    return pts


def horizon(n, seed=5):
    """every pair follows ONE homography whose horizon (x = 300) crosses the left points.  A model's denominator is positive
    at the centre of the left bounding box (x near 400), so the pairs left of the horizon have w < 0: e <= lim holds for
    them, w > 0 does not."""
    rng = np.random.default_rng(seed)
    left = (rng.random((n, 2)) * [W - 1, H - 1]).astype(np.float32)
    left = left[np.abs(left[:, 0] - 300.0) > 30.0]        # keep the images finite and well conditioned
    Hm = np.array([[1.0, 0.02, 3.0], [0.01, 1.0, -2.0], [-1.0 / 300.0, 0.0, 1.0]])
    return np.c_[left, project(Hm, left)].astype(np.float32)


def scene(name, n, model):
    """the scenes by name, cut or built to exactly n pairs"""
    if name == "planted":
        return planted(n, 1, model)[0]
    if name == "outliers":
        return all_outliers(n)
    if name == "collinear":
        return collinear(n)
    if name == "identical":
        return identical(n)
    if name == "nan":
        return with_nan(n, 4, model)
    if name == "horizon":
        return horizon(2 * n + 64)[:n]
    raise KeyError(name)
