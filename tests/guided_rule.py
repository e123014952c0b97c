"""ctypes front of tests/guided_ref.c, the CPU restatement of the guided matcher's rule (include/popsift_hip.h,
popsift_hip_match_guided), and the scenes the guided matcher's tests share.  A helper of the tests, not a test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import epipolar_rule
import match_pairs_rule
import ransac_rule
from match_pairs_rule import PAIR_DTYPE

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "guided_ref.c")
HOMOGRAPHY, EPIPOLAR = 0, 1
MATCH_DTYPE = np.dtype([("best", np.int32), ("second", np.int32), ("accept", np.int32),
                        ("dist_best", np.float32), ("dist_second", np.float32)])
W, H = ransac_rule.W, ransac_rule.H            # the 800 x 640 image the scenes' points lie in
ALL_PASS_ERR = np.float32(3e38)                # a homography's lim = max_err^2 * w^2 overflows to +inf: every pair passes
IDENTITY = np.eye(3, dtype=np.float32)


class Ref:
    """Built with gcc -O2 -ffp-contract=off into `build_dir`."""

    def __init__(self, build_dir):
        so = os.path.join(str(build_dir), "libguided_ref.so")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, SRC, "-lm"])
        self.lib = C.CDLL(so)
        vp, f = C.c_void_p, C.c_float
        self.lib.gr_ok.restype = C.c_int
        self.lib.gr_ok.argtypes = [C.c_int, vp, f, f, f, f, f]
        self.lib.gr_ok_pairs.restype = None
        self.lib.gr_ok_pairs.argtypes = [C.c_int, vp, f, vp, C.c_int, vp]
        self.lib.gr_dist.restype = f
        self.lib.gr_dist.argtypes = [vp, vp]
        self.lib.gr_rows.restype = None
        self.lib.gr_rows.argtypes = [C.c_int, vp, f, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp]
        self.lib.gr_pairs.restype = C.c_int
        self.lib.gr_pairs.argtypes = [vp, C.c_int, vp, f, f, vp]

    @staticmethod
    def _model(M):
        return np.ascontiguousarray(np.asarray(M, np.float32).reshape(9))

    def ok(self, model, M, max_err, x, y, xr, yr):
        return bool(self.lib.gr_ok(model, self._model(M).ctypes.data, max_err, x, y, xr, yr))

    def ok_pairs(self, model, M, max_err, pts):
        """ok(k, k) of (n, 4) pairs (x, y, x', y') -> (n,) uint8"""
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        mask = np.zeros(len(pts), np.uint8)
        self.lib.gr_ok_pairs(model, self._model(M).ctypes.data, max_err, pts.ctypes.data, len(pts), mask.ctypes.data)
        return mask

    def dist(self, l, r):
        l, r = np.ascontiguousarray(l, np.float32), np.ascontiguousarray(r, np.float32)
        return np.float32(self.lib.gr_dist(l.ctypes.data, r.ctypes.data))

    def rows(self, model, M, max_err, l, lxy, r, rxy, back=False):
        """-> (rows, candidates per row): a row per left descriptor, or with back a row per right descriptor"""
        l = np.ascontiguousarray(l, np.float32).reshape(-1, 128)
        r = np.ascontiguousarray(r, np.float32).reshape(-1, 128)
        lxy = np.ascontiguousarray(lxy, np.float32).reshape(-1, 2)
        rxy = np.ascontiguousarray(rxy, np.float32).reshape(-1, 2)
        assert len(lxy) == len(l) and len(rxy) == len(r)
        n = len(r) if back else len(l)
        out, ncand = np.zeros(n, MATCH_DTYPE), np.zeros(n, np.int32)
        self.lib.gr_rows(model, self._model(M).ctypes.data, max_err, l.ctypes.data, lxy.ctypes.data, len(l), r.ctypes.data,
                         rxy.ctypes.data, len(r), 1 if back else 0, out.ctypes.data, ncand.ctypes.data)
        return out, ncand

    def pairs(self, F, B=None, ratio=0.8, max_dist2=np.inf, cross_check=False):
        """the pair rule on the rows F and, with the cross-check, the reverse rows B"""
        F = np.ascontiguousarray(F, MATCH_DTYPE)
        out = np.zeros(len(F), PAIR_DTYPE)
        if cross_check:
            B = np.ascontiguousarray(B, MATCH_DTYPE)
        n = self.lib.gr_pairs(F.ctypes.data, len(F), B.ctypes.data if cross_check else None, ratio, max_dist2, out.ctypes.data)
        return out[:n]


@pytest.fixture(scope="session")
def guided_ref(tmp_path_factory):
    return Ref(tmp_path_factory.mktemp("guided_ref"))


class Expected:
    """The rule's answers for one (scene, model, max_err): rows both ways once, pairs per option set."""

    def __init__(self, ref, model, M, max_err, s):
        self.ref = ref
        self.F, self.ncand = ref.rows(model, M, max_err, s["l"], s["lxy"], s["r"], s["rxy"])
        self.B, _ = ref.rows(model, M, max_err, s["l"], s["lxy"], s["r"], s["rxy"], back=True)

    def pairs(self, ratio=0.8, max_dist2=np.inf, cross_check=False):
        return self.ref.pairs(self.F, self.B, ratio, max_dist2, cross_check)


# ---- scenes: dict(l (nl, 128), lxy (nl, 2), r (nr, 128), rxy (nr, 2)), all float32

def near_copies(l, r):
    """(i, j) of the near-copy descriptor pairs match_pairs_rule.planted hides in its sets: squared distance below 1,
    where unrelated uniform descriptors lie near 128 / 6"""
    l64, r64 = l.astype(np.float64), r.astype(np.float64)
    d = (l64 ** 2).sum(1)[:, None] + (r64 ** 2).sum(1)[None, :] - 2.0 * l64 @ r64.T
    i, j = np.nonzero(d < 1.0)
    _, first = np.unique(j, return_index=True)          # one left partner per right descriptor
    i, j = i[first], j[first]
    _, first = np.unique(i, return_index=True)          # and one right partner per left one
    return i[first], j[first]


def scene(nl, nr, seed=0):
    """Left points uniform in the image.  Half of min(nl, nr) right points are the float64 image of a random left point
    under ransac_rule.pixel_homography() plus N(0, 0.4 px); half as many further right points lie near the same images
    with N(0, 0.6 px); the rest are uniform.  Descriptors: match_pairs_rule.planted(nl, nr), re-indexed so that planted
    point pairs carry near-copy descriptors.  -> (scene, the homography as float32)"""
    rng = np.random.default_rng(1000003 * seed + 7919 * nl + nr)
    Hm = ransac_rule.pixel_homography()
    lxy = rng.random((nl, 2)) * [W - 1, H - 1]
    rxy = rng.random((nr, 2)) * [W - 1, H - 1]
    k = min(nl, nr) // 2
    a = rng.permutation(nl)[:k]                          # left points with an image on the right
    b = rng.permutation(nr)[:k + k // 2]                 # where the images go, then the second points near them
    img = ransac_rule.project(Hm, lxy[a])
    rxy[b[:k]] = img + rng.normal(0, 0.4, (k, 2))
    rxy[b[k:]] = img[:k // 2] + rng.normal(0, 0.6, (k // 2, 2))
    l, r = match_pairs_rule.planted(nl, nr)
    ci, cj = near_copies(l, r)
    m = min(len(ci), k)
    # left descriptor ci[t] goes to left point a[t], right descriptor cj[t] to right point b[t]; the others fill the rest
    lperm, rperm = np.full(nl, -1), np.full(nr, -1)
    lperm[a[:m]], rperm[b[:m]] = ci[:m], cj[:m]
    lperm[lperm < 0] = np.setdiff1d(np.arange(nl), ci[:m])
    rperm[rperm < 0] = np.setdiff1d(np.arange(nr), cj[:m])
    s = dict(l=np.ascontiguousarray(l[lperm]), lxy=lxy.astype(np.float32), r=np.ascontiguousarray(r[rperm]),
             rxy=rxy.astype(np.float32))
    return s, Hm.astype(np.float32)


def scene_F():
    """epipolar_rule.true_F() of epipolar_rule.cameras(), its largest entry scaled to 1 as the verifier returns it, float32"""
    F = epipolar_rule.true_F()
    return (F / F.flat[np.argmax(np.abs(F))]).astype(np.float32)


def translation_H(tx, ty):
    return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float32)


def translation_F(tx, ty):
    """the fundamental matrix of x' = x + s tx, y' = y + s ty for any s (a camera moved sideways): [t]_x, t = (tx, ty, 0)"""
    return np.array([[0, 0, ty], [0, 0, -tx], [-ty, tx, 0]], np.float32)


def planted_cases():
    """A scene under the translation (10, 5) at max_err = 2 in which the rule differs from "match, then filter".  Left
    points on a 40 px grid; a right point is far from every image (below y = 400) unless placed here.
      rows 0 .. 5   r[100 + i] is a very near copy of l[i] far from its image, r[110 + i] a looser copy at its image: the
                    unguided best fails ok, the guided row has r[110 + i]
      row 10        r[20] = r[40], copies of l[10]; r[20] is no candidate, r[40] is: the higher index wins the tie
      rows 12, 13   left points 1 px apart, r[50] between their images and a copy of l[13]: both rows have r[50] alone,
                    the search the other way round sees both and takes 13 -- the cross-check, and nothing else, removes
                    (12, 50)
      row 15        r[60] at its image and a copy of l[15]; l[16] is a still nearer copy of r[60] but no candidate: the
                    unguided reverse search would take 16 and drop (15, 60), the guided one keeps it
    -> (scene, M, max_err)"""
    rng = np.random.default_rng(77)
    nl, nr = 70, 300
    M, t = translation_H(10, 5), np.array([10.0, 5.0])
    idx = np.arange(nl)
    lxy = np.c_[40.0 + 40.0 * (idx % 16), 40.0 + 40.0 * (idx // 16)]
    rxy = np.c_[rng.random(nr) * (W - 1), 400.0 + rng.random(nr) * (H - 401)]
    l = rng.random((nl, 128)).astype(np.float32)
    r = rng.random((nr, 128)).astype(np.float32)
    noise = lambda s: rng.normal(0, s, 128).astype(np.float32)
    for i in range(6):
        r[100 + i] = l[i] + noise(0.002)
        r[110 + i] = l[i] + noise(0.05)
        rxy[110 + i] = lxy[i] + t + [0.5, -0.5]
    r[20] = l[10] + noise(0.01)
    r[40] = r[20]
    rxy[40] = lxy[10] + t
    lxy[13] = lxy[12] + [1.0, 0.0]
    r[50] = l[13] + noise(0.01)
    rxy[50] = lxy[12] + t + [0.5, 0.0]
    r[60] = l[15] + noise(0.05)
    rxy[60] = lxy[15] + t
    l[16] = r[60] + noise(0.001)
    s = dict(l=l, lxy=lxy.astype(np.float32), r=r, rxy=rxy.astype(np.float32))
    return s, M, np.float32(2.0)
