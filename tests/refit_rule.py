"""ctypes front of tests/refit_ref.c, the CPU restatement of the verifier's least-squares refit (include/popsift_hip.h,
popsift_hip_refit), float64 yardsticks, and the scenes its tests share (those of ransac_rule / epipolar_rule, plus noise)."""
import ctypes as C
import os
import subprocess

import numpy as np

import epipolar_rule as E
import ransac_rule as R

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "refit_ref.c")
HOMOGRAPHY, AFFINE, EPIPOLAR = 0, 1, 2
KINDS = (HOMOGRAPHY, AFFINE, EPIPOLAR)
SAMPLE_SIZE = {HOMOGRAPHY: 4, AFFINE: 3, EPIPOLAR: 8}
ROUNDS, CONVERGED, NOT_BETTER, NO_FIT, NO_SUPPORT = range(5)     # popsift_hip_refit_result.stop
SLOTS, MAX_ROUNDS, CHUNK = 45, 16, 1024
USED_SLOTS = {HOMOGRAPHY: list(range(29)), AFFINE: list(range(6)) + list(range(21, 27)), EPIPOLAR: list(range(45))}
RESULT_DTYPE = np.dtype([("M", np.float32, (9,)), ("n_inliers", np.int32), ("n_start", np.int32), ("rounds", np.int32),
                         ("stop", np.int32)])
# `variant` bits of rf_refit: a deliberately broken step
ALL_PAIRS, LEFT_TO_RIGHT, ACCEPT_LOWER, NO_W_TEST, NON_FINITE_ENTERS = 1, 2, 4, 8, 16
IDENTITY = np.eye(3, dtype=np.float32).reshape(9)


class Ref:
    """Built with gcc -O2 -ffp-contract=off into `build_dir` (extra flags only for timing: they must not change results)."""

    def __init__(self, build_dir, extra_flags=()):
        so = os.path.join(str(build_dir), "librefit_ref.so")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", *extra_flags, "-fPIC", "-shared", "-o", so, SRC, "-lm"])
        self.lib = C.CDLL(so)
        vp = C.c_void_p
        self.lib.rf_refit.restype = None
        self.lib.rf_refit.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_float, vp, C.c_int, vp, vp, vp, vp, vp, vp]
        self.lib.rf_mask.restype = None
        self.lib.rf_mask.argtypes = [vp, C.c_int, C.c_int, C.c_float, vp, vp]
        self.lib.rf_terms.restype = None
        self.lib.rf_terms.argtypes = [vp, C.c_int, C.c_int, vp]

    def refit(self, pts, kind, M, max_err, rounds=4, variant=0):
        """-> dict(sums (rounds, 45) float64, models (rounds, 9), counts (rounds,), accepted (rounds,), result (RESULT_DTYPE
        record), mask (n,) uint8)"""
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        n = len(pts)
        M = np.ascontiguousarray(np.asarray(M, np.float32).reshape(9))
        out = dict(sums=np.zeros((rounds, SLOTS), np.float64), models=np.zeros((rounds, 9), np.float32),
                   counts=np.zeros(rounds, np.int32), accepted=np.zeros(rounds, np.int32), mask=np.zeros(n, np.uint8))
        res = np.zeros(1, RESULT_DTYPE)
        self.lib.rf_refit(pts.ctypes.data if n else None, n, kind, rounds, max_err, M.ctypes.data, variant,
                          out["sums"].ctypes.data, out["models"].ctypes.data, out["counts"].ctypes.data,
                          out["accepted"].ctypes.data, res.ctypes.data, out["mask"].ctypes.data if n else None)
        out["result"] = res[0]
        return out

    def mask(self, pts, kind, M, max_err):
        """-> (n,) uint8: the inliers of M under the kind's test"""
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        M = np.ascontiguousarray(np.asarray(M, np.float32).reshape(9))
        out = np.zeros(len(pts), np.uint8)
        self.lib.rf_mask(pts.ctypes.data, len(pts), kind, max_err, M.ctypes.data, out.ctypes.data)
        return out

    def terms(self, pts, kind):
        """-> (n, 45) float64: the terms of every pair, inlier or not"""
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        out = np.zeros((len(pts), SLOTS), np.float64)
        self.lib.rf_terms(pts.ctypes.data, len(pts), kind, out.ctypes.data)
        return out


def tree(terms, a, L):
    """rule 3b as written: the pairwise tree over the pair index, terms (n, slots) float64 with the pairs that are no
    inliers already zero; numpy adds float64 with one IEEE operation per element"""
    if L == 1:
        return terms[a] if a < len(terms) else np.zeros(terms.shape[1])
    if a >= len(terms):
        return np.zeros(terms.shape[1])             # a subtree of padding: +0.0
    return tree(terms, a, L // 2) + tree(terms, a + L // 2, L // 2)


def root(terms):
    P = 1
    while P < len(terms):
        P *= 2
    return tree(terms, 0, P)


# ---- float64 yardsticks

def rms(d):
    return float(np.sqrt(np.mean(np.square(d))))


def normalisers(pts):
    """the rule's step 1 in float64: (cx, cy, k) of either side from the bounding box of the finite values"""
    out = []
    for c in (0, 2):
        cols = [pts[:, c + i][np.isfinite(pts[:, c + i])].astype(np.float64) for i in (0, 1)]
        ctr = [(col.min() + col.max()) * 0.5 for col in cols]
        half = max((col.max() - col.min()) * 0.5 for col in cols)
        out.append((ctr[0], ctr[1], 1.0 / (half if half > 0 else 1.0)))
    return out


def lstsq_model(pts, mask, kind):
    """numpy.linalg.lstsq in float64 on the pairs of `mask`: normalised, inhomogeneous (h8 = 1) -> the 3 x 3 map in pixels"""
    (cx, cy, k), (dx, dy, kr) = normalisers(pts)
    p = pts[mask.astype(bool)].astype(np.float64)
    x, y, u, v = (p[:, 0] - cx) * k, (p[:, 1] - cy) * k, (p[:, 2] - dx) * kr, (p[:, 3] - dy) * kr
    one, zero = np.ones(len(p)), np.zeros(len(p))
    if kind == AFFINE:
        A = np.c_[x, y, one]
        G = np.vstack([np.linalg.lstsq(A, u, rcond=None)[0], np.linalg.lstsq(A, v, rcond=None)[0], [0, 0, 1]])
    else:
        A = np.vstack([np.c_[x, y, one, zero, zero, zero, -u * x, -u * y], np.c_[zero, zero, zero, x, y, one, -v * x, -v * y]])
        G = np.append(np.linalg.lstsq(A, np.r_[u, v], rcond=None)[0], 1.0).reshape(3, 3)
    Tl = np.array([[k, 0, -cx * k], [0, k, -cy * k], [0, 0, 1]])
    Tr = np.array([[kr, 0, -dx * kr], [0, kr, -dy * kr], [0, 0, 1]])
    return np.linalg.inv(Tr) @ G @ Tl


def eigen_F(pts, mask):
    """the float64 eigenvector under the smallest eigenvalue of the same normal matrix N (normalised coordinates), made
    rank 2 by an SVD and denormalised: the textbook 8-point least-squares F on the pairs of `mask`"""
    (cx, cy, k), (dx, dy, kr) = normalisers(pts)
    p = pts[mask.astype(bool)].astype(np.float64)
    x, y, u, v = (p[:, 0] - cx) * k, (p[:, 1] - cy) * k, (p[:, 2] - dx) * kr, (p[:, 3] - dy) * kr
    A = np.c_[u * x, u * y, u, v * x, v * y, v, x, y, np.ones(len(p))]
    w, V = np.linalg.eigh(A.T @ A)
    U, s, Vt = np.linalg.svd(V[:, 0].reshape(3, 3))
    Fn = U @ np.diag([s[0], s[1], 0.0]) @ Vt
    Tl = np.array([[k, 0, -cx * k], [0, k, -cy * k], [0, 0, 1]])
    Tr = np.array([[kr, 0, -dx * kr], [0, kr, -dy * kr], [0, 0, 1]])
    return Tr.T @ Fn @ Tl


# ---- scenes: (n, 4) float32 rows (x, y, x', y')

def noisy(pts, inl, sigma, seed=11):
    """Gaussian noise of `sigma` px on the right points of the planted inliers"""
    rng = np.random.default_rng(seed)
    out = pts.astype(np.float64)
    out[:, 2:] += sigma * rng.standard_normal((len(pts), 2)) * inl.astype(bool)[:, None]
    return out.astype(np.float32)


def noisy_planted(n=1000, seed=1, kind=HOMOGRAPHY, sigma=0.3, inlier_frac=0.6):
    """-> (pts, planted mask, planted map): ransac_rule.planted with noise on its inliers"""
    pts, inl, Hm = R.planted(n, seed, kind, inlier_frac)
    return noisy(pts, inl, sigma), inl, Hm


def noisy_two_view(n=1000, seed=1, sigma=0.3):
    pts, inl, F = E.two_view(n, seed)
    return noisy(pts, inl, sigma), inl, F


def collinear_row(n, seed=3):
    """left points on one image row, exactly: their normalised y is 0.0 in every pair, and the normal matrix has a row of
    zeros.  (ransac_rule.collinear is a line only up to float32 rounding: its normal matrix is ill conditioned, not
    singular.)  Every pair follows pixel_homography()."""
    rng = np.random.default_rng(seed)
    left = np.c_[50.0 + rng.random(n) * 600.0, np.full(n, 40.0)].astype(np.float32)
    return np.c_[left, R.project(R.pixel_homography(), left)].astype(np.float32)


def sparse_chunks(kind=HOMOGRAPHY):
    """3 chunks of the accumulating kernel: chunk 0 is the noisy planted scene, chunk 1 holds no inlier, and chunk 2's only
    inliers are its first and its last pair -> (pts, planted mask, planted map)"""
    n = 3 * CHUNK
    if kind == EPIPOLAR:       # the outliers of two_view lie 20 px and more off their epipolar lines; random pairs would not
        good, _, Hm = E.two_view(n, 3, 1.0)
        far = E.two_view(n, 3, 0.0)[0]
    else:
        good, _, Hm = R.planted(n, 3, kind, 1.0)
        far = R.all_outliers(n, 9)
    inl = np.zeros(n, np.uint8)
    inl[:CHUNK] = 1
    inl[[2 * CHUNK, n - 1]] = 1
    good = noisy(good, inl, 0.3)
    return np.where(inl.astype(bool)[:, None], good, far), inl, Hm


def scene(name, n, kind):
    """the scenes by name, built to exactly n pairs; `noisy` and `exact` are the kind's planted scene"""
    if name == "noisy":
        return (noisy_two_view(n, 1) if kind == EPIPOLAR else noisy_planted(n, 1, kind))[0]
    if name == "rough":                # 1 px of noise: the minimal-sample winner misses a third of the planted inliers
        return (noisy_two_view(n, 1, 1.0) if kind == EPIPOLAR else noisy_planted(n, 1, kind, 1.0))[0]
    if name == "exact":
        return (E.two_view(n, 1) if kind == EPIPOLAR else R.planted(n, 1, kind))[0]
    if name in ("two_view", "translation", "planar"):
        return E.scene(name, n)
    if name == "nan" and kind == EPIPOLAR:
        return E.with_nan(n)
    return R.scene(name, n, min(kind, AFFINE))


def planted_model(name, n, kind):
    """the map the scene was built with, as the nine floats a caller would pass (F scaled to a largest entry of 1)"""
    if kind == EPIPOLAR:
        Fm = E.true_F()
        return (Fm / Fm.flat[np.abs(Fm).argmax()]).astype(np.float32).reshape(9)
    return R.planted(4, 1, kind)[2].astype(np.float32).reshape(9)


def start_model(name, n, kind, ransac_ref, epipolar_ref, max_err):
    """-> (pts, M): the scene and the model its refit starts from: the winner of the kind's RANSAC reference at 300
    hypotheses on the first 2000 pairs (on all of them the reference's T x n loop would dominate the test), the identity
    where it finds none; on the two degenerate scenes of the homography and the affine map a map every pair follows, so
    that the fit itself meets the degeneracy."""
    pts = scene(name, n, kind)
    if name == "identical" and kind != EPIPOLAR:
        return pts, np.array([1, 0, 20, 0, 1, 10, 0, 0, 1], np.float32)
    if name == "collinear" and kind == HOMOGRAPHY:
        return pts, R.pixel_homography().astype(np.float32).reshape(9)
    if kind == EPIPOLAR:
        res = epipolar_ref.epipolar(pts[:2000], 300, max_err, 5, trace=False)["result"]
    else:
        res = ransac_ref.ransac(pts[:2000], kind, 300, max_err, 5, trace=False)["result"]
    return pts, (res["H"].copy() if res["hypothesis"] >= 0 else IDENTITY.copy())
