"""ctypes front of tests/epipolar_ref.c, the CPU restatement of the epipolar verifier's rule (include/popsift_hip.h,
popsift_hip_epipolar), and the scenes its tests share."""
import ctypes as C
import os
import subprocess

import numpy as np

from ransac_rule import RESULT_DTYPE, W, H, all_outliers, collinear, identical   # noqa: F401  (the sibling's, unchanged)

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "epipolar_ref.c")
SAMPLE = 8
# `variant` bits of er_epipolar: a deliberately broken step
TIE_TO_HIGHEST, NO_G_TEST, LAST_UNKNOWN_FIXED, NO_RANK2 = 1, 2, 4, 8


class Ref:
    """Built with gcc -O2 -ffp-contract=off into `build_dir` (extra flags only for timing: they must not change results)."""

    def __init__(self, build_dir, extra_flags=()):
        so = os.path.join(str(build_dir), "libepipolar_ref.so")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", *extra_flags, "-fPIC", "-shared", "-o", so, SRC, "-lm"])
        self.lib = C.CDLL(so)
        vp = C.c_void_p
        self.lib.er_epipolar.restype = None
        self.lib.er_epipolar.argtypes = [vp, C.c_int, C.c_int, C.c_float, C.c_uint32, C.c_int, vp, vp, vp, vp, vp]
        self.lib.er_samples.restype = None
        self.lib.er_samples.argtypes = [C.c_uint32, C.c_int, C.c_int, vp, vp]

    def epipolar(self, pts, T, max_err, seed, variant=0, trace=True):
        """-> dict(samples (T, 8), models (T, 9), counts (T,), result (RESULT_DTYPE record, H = F), mask (n,) uint8)"""
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        n = len(pts)
        out = dict(samples=np.zeros((T, SAMPLE), np.int32), models=np.zeros((T, 9), np.float32), counts=np.zeros(T, np.int32),
                   mask=np.zeros(n, np.uint8))
        res = np.zeros(1, RESULT_DTYPE)
        ptr = lambda a: a.ctypes.data if trace and a.size else None
        self.lib.er_epipolar(pts.ctypes.data if n else None, n, T, max_err, seed, variant, ptr(out["samples"]),
                             ptr(out["models"]), ptr(out["counts"]), res.ctypes.data, out["mask"].ctypes.data if n else None)
        out["result"] = res[0]
        return out

    def samples(self, seed, n, T):
        """-> (samples (T, 8), valid (T,))"""
        s, v = np.zeros((T, SAMPLE), np.int32), np.zeros(T, np.int32)
        self.lib.er_samples(seed, n, T, s.ctypes.data, v.ctypes.data)
        return s, v


# ---- float64 geometry the tests measure with

def sampson(F, pts):
    """float64 Sampson distance (px) of (n, 4) pairs to [x' y' 1] F [x y 1]^T = 0"""
    p = np.asarray(pts, np.float64)
    F = np.asarray(F, np.float64).reshape(3, 3)
    xl, xr = np.c_[p[:, :2], np.ones(len(p))], np.c_[p[:, 2:], np.ones(len(p))]
    Fx, Ftx = xl @ F.T, xr @ F
    r = (xr * Fx).sum(1)
    return np.abs(r) / np.sqrt(Fx[:, 0] ** 2 + Fx[:, 1] ** 2 + Ftx[:, 0] ** 2 + Ftx[:, 1] ** 2)


def line_distance(F, pts):
    """float64 distance (px) of the right points to the epipolar lines F [x y 1]^T of their left points"""
    p = np.asarray(pts, np.float64)
    l = np.c_[p[:, :2], np.ones(len(p))] @ np.asarray(F, np.float64).reshape(3, 3).T
    return np.abs((np.c_[p[:, 2:], np.ones(len(p))] * l).sum(1)) / np.hypot(l[:, 0], l[:, 1])


# ---- scenes: (n, 4) float32 rows (x, y, x', y')

def cameras():
    """-> (K, R, t): one pinhole camera in two positions, a rotation about all three axes and a general translation"""
    K = np.array([[700.0, 0.0, (W - 1) / 2.0], [0.0, 700.0, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
    ax, ay, az = 0.03, -0.08, 0.05
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return K, Rz @ Ry @ Rx, np.array([0.6, -0.15, 0.25])


def true_F():
    K, Rm, t = cameras()
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    return Ki.T @ tx @ Rm @ Ki


def two_view(n=1000, seed=1, inlier_frac=0.6, depth=(4.0, 12.0)):
    """-> (pts, planted mask, the true F).  Random left points at random depth seen by cameras().  The right point of an
    inlier is its float64 projection rounded to float32, no noise; an outlier is moved 20 .. 200 px perpendicular to its
    true epipolar line (either side) and up to 100 px along it, so no outlier lies near its line by accident."""
    rng = np.random.default_rng(seed)
    K, Rm, t = cameras()
    left = (rng.random((n, 2)) * [W - 1, H - 1]).astype(np.float32)
    z = depth[0] + (depth[1] - depth[0]) * rng.random(n)
    X = (np.c_[left.astype(np.float64), np.ones(n)] @ np.linalg.inv(K).T) * z[:, None]
    q = (X @ Rm.T + t) @ K.T
    right = q[:, :2] / q[:, 2:3]
    inl = np.zeros(n, bool)
    inl[rng.permutation(n)[:int(round(n * inlier_frac))]] = True
    F = true_F()
    l = np.c_[left.astype(np.float64), np.ones(n)] @ F.T
    nrm = l[:, :2] / np.hypot(l[:, 0], l[:, 1])[:, None]
    off = (20.0 + 180.0 * rng.random(n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    slide = 200.0 * rng.random(n) - 100.0
    right[~inl] += (off[:, None] * nrm + slide[:, None] * np.c_[-nrm[:, 1], nrm[:, 0]])[~inl]
    return np.c_[left, right.astype(np.float32)].astype(np.float32), inl.astype(np.uint8), F


def translation(n, seed=6):
    """identical cameras, one moved sideways: x' = x + disparity, y' = y; every pair is an inlier and F22 = 0"""
    rng = np.random.default_rng(seed)
    left = (rng.random((n, 2)) * [W - 101, H - 1]).astype(np.float32)
    disparity = 5.0 + 90.0 * rng.random(n)
    return np.c_[left, left[:, 0].astype(np.float64) + disparity, left[:, 1]].astype(np.float32)


def planar(n, seed=7):
    """all depths equal: the pairs follow a homography, every sample is degenerate for a fundamental matrix"""
    return two_view(n, seed, 1.0, (8.0, 8.0))[0]


def with_nan(n, seed=4):
    """the two-view scene with one pair whose left x is NaN and one whose right y is +inf"""
    pts = two_view(n, seed)[0]
    pts[n // 3, 0] = np.nan
    pts[n // 2, 3] = np.inf
    return pts


def scene(name, n):
    """the scenes by name, built to exactly n pairs"""
    if name == "two_view":
        return two_view(n, 1)[0]
    if name == "translation":
        return translation(n)
    if name == "planar":
        return planar(n)
    if name == "outliers":
        return all_outliers(n)
    if name == "collinear":
        return collinear(n)
    if name == "identical":
        return identical(n)
    if name == "nan":
        return with_nan(n)
    raise KeyError(name)
