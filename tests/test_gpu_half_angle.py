"""k_descriptor and k_orientation on the gradients that the half-angle arctangent (half_angle_bins, keypoint.hip) treats
apart: gx < 0 with gy = +-0 (the mirrored half, on the cut of atan2), a zero gradient (tangent 0 / 1e-18), gradients so small
that their squares underflow (|g| = 0 where gy is not: the tails of a blob on a black background), exact diagonals
(|t| = tan(pi / 8), and in k_orientation ON a bin edge), and a patch cut by the border.

64 x 64 images, so octave 0 is 128 x 128; frames with given orientations go through the describe path, sigma 1.8 in octave
units: 27 patch rows at angle 0, 38 at 45 degrees.  Every element of every descriptor must lie inside the interval of
tests/desc_rule.py, read from the device's own plane and frame, as in tests/test_gpu_desc_rule.py -- no allowance.
Extraction of the checker holds k_orientation to tests/ori_rule.py and gives the same bytes twice."""
import numpy as np
import pytest

import desc_rule
import ori_rule
from util import bits, sorted_features

pytestmark = pytest.mark.gpu

N = 64
SIGMA = 1.8                                                          # octave units
ANGLES = np.array([0.0, -0.0, 0.7, np.float32(np.pi / 4)], np.float32)
INSIDE = ((64.3, 64.6), (80.5, 70.25), (50.75, 52.5), (64.0, 82.0))  # octave units, all within reach of the blob
BORDER = ((5.5, 60.25), (124.0, 64.5), (60.5, 126.0))                # the patch leaves the plane on one side


def _ramp():
    """falls from left to right: gx < 0 and gy = +-0 in every sample"""
    return np.tile((250 - 3 * np.arange(N)).astype(np.uint8), (N, 1))


def _blob():
    """flat but for one Gaussian blob of sigma 1.5 pixels: most of every patch has a gradient of exactly zero"""
    yy, xx = np.mgrid[0:N, 0:N].astype(np.float64)
    return (30.0 + np.rint(200.0 * np.exp(-((xx - 32.0) ** 2 + (yy - 32.0) ** 2) / (2.0 * 1.5 ** 2)))).astype(np.uint8)


def _blob_on_black():
    """the same blob on a background of exactly 0: blurred level after level its tails fall to 1e-20 and below, down to
    the denormals -- gradients whose squares underflow, so that |g| comes out as 0 where gy is not"""
    yy, xx = np.mgrid[0:N, 0:N].astype(np.float64)
    return np.rint(255.0 * np.exp(-((xx - 32.0) ** 2 + (yy - 32.0) ** 2) / (2.0 * 1.5 ** 2))).astype(np.uint8)


def _checker45():
    """a checkerboard turned by 45 degrees: the edges, and the gradients on them, are exact diagonals"""
    yy, xx = np.mgrid[0:N, 0:N]
    return (((((xx + yy) // 6) + ((xx - yy) // 6)) & 1) * 255).astype(np.uint8)


PLANES = {"ramp": (_ramp, INSIDE + BORDER), "blob": (_blob, INSIDE), "blob_on_black": (_blob_on_black, INSIDE), "checker45": (_checker45, INSIDE + BORDER)}


def _frames(dtype, positions):
    rows = [(x, y, a, 1 + k % 3) for a in ANGLES for k, (x, y) in enumerate(positions)]
    fr = np.zeros(len(rows), dtype)
    for i, (x, y, a, lvl) in enumerate(rows):
        fr[i] = (np.float32(x) / 2, np.float32(y) / 2, np.float32(SIGMA) / 2, a, 0, lvl)   # image units, exactly halved
    return fr


@pytest.mark.parametrize("name", list(PLANES))
def test_given_frames_satisfy_the_descriptor_rule(gpu_hip, name):
    hip = gpu_hip
    make, positions = PLANES[name]
    img = make()
    fr = _frames(hip.FRAME_DTYPE, positions)
    ctx = hip.Context(hip.default_params())
    try:
        df, dd = ctx.describe(img, fr, "given")
        e = ctx.extrema()
        planes = {lvl: ctx.plane(0, 0, lvl) for lvl in (1, 2, 3)}
    finally:
        ctx.close()
    assert planes[1].shape == (2 * N, 2 * N)
    assert len(df) == len(fr) == len(e) and (df["num_ori"] == 1).all() and (e["octave"] == 0).all()
    assert np.array_equal(e["cell"], np.arange(len(fr))) and np.array_equal(e["lpos"], fr["level"])
    assert np.array_equal(bits(df["orientation"][:, 0]), bits(fr["orientation"]))
    desc = dd[df["desc_idx"][:, 0]]
    assert np.isfinite(desc).all()
    if name == "ramp":                      # what the plane is for: away from the border, gy is +-0 and gx < 0
        p = planes[1].astype(np.float64)[20:108, 20:108]
        assert (p[2:, 1:-1] - p[:-2, 1:-1] == 0).all() and (p[1:-1, 2:] - p[1:-1, :-2] < 0).all()
    if name == "blob":
        p = planes[1].astype(np.float64)
        assert ((p[2:, 1:-1] == p[:-2, 1:-1]) & (p[1:-1, 2:] == p[1:-1, :-2])).mean() > 0.5
    bad, worst, rows, ns, under = [], 0.0, [], [], 0
    for i in range(len(fr)):
        r = desc_rule.analyse(planes[int(e["lpos"][i])], e["xpos"][i], e["ypos"][i], e["sigma"][i], df["orientation"][i, 0])
        rows.append(r.patch.rows)
        ns.append(r.patch.n)
        q, P = r.patch, planes[int(e["lpos"][i])].astype(np.float64)
        g = np.hypot(P[q.row, q.col + 1] - P[q.row, q.col - 1], P[q.row + 1, q.col] - P[q.row - 1, q.col])[q.inside]
        under += int(((g > 0) & (g < 1.1e-19)).sum())
        off = desc_rule.check(r, desc[i])
        if off:
            bad.append(desc_rule.format_offenders(r, off, "%s frame %d" % (name, i)))
        worst = max(worst, desc_rule.error_ratio(r, desc[i]))
    print("%s: %d frames, patch rows %d .. %d, samples %d .. %d, %d below 1.1e-19, %d with offenders, largest error / bound %.3f" % (
        name, len(fr), min(rows), max(rows), min(ns), max(ns), under, len(bad), worst))
    if name == "blob_on_black":             # what the plane is for: samples whose squares underflow (12 each in two patches)
        assert under >= 20, under
    inside = [i for i in range(len(fr)) if i % len(positions) < len(INSIDE)]
    assert min(rows[i] for i in inside) >= 20 and max(rows) <= 40
    cut = [i for i in range(len(fr)) if i % len(positions) >= len(INSIDE)]
    assert all(ns[i] < min(ns[k] for k in inside) for i in cut)          # the border really cuts those patches
    assert not bad, "%d descriptor(s) outside the rule\n    %s" % (len(bad), "\n    ".join(bad[:5]))


def test_checker_orientations_satisfy_the_rule_twice(gpu_hip):
    img = _checker45()
    ctx = gpu_hip.Context(gpu_hip.default_params())
    try:
        fh, dh = ctx.submit(img).fetch()
        eh = ctx.extrema()
        assert len(fh) > 0 and ori_rule.aligned(eh, fh, 1.0)
        rules = ori_rule.analyse_all(lambda o, l: ctx.plane(o, 0, l), eh, 3 + 3)
        bad = ori_rule.check(rules, eh, fh)
        print("checker45: %d keypoints, %d decided, %d offenders" % (len(rules), sum(r.decided for r in rules), len(bad)))
        assert not bad, ori_rule.format_offenders(bad)
        f1, d1 = sorted_features(fh, dh)
        f2, d2 = sorted_features(*ctx.submit(img).fetch())
    finally:
        ctx.close()
    for n in ("debug_octave", "xpos", "ypos", "sigma", "num_ori", "orientation"):
        assert f1[n].tobytes() == f2[n].tobytes(), n
    assert d1.tobytes() == d2.tobytes()
