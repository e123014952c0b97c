"""k_descriptor where its histogram words and cell addresses are read from the bits of f32 denormals (keypoint.hip,
"ISA: weights" and PS_CELL; the arithmetic alone: tests/test_desc_words.py).

64 x 64 float images, so octave 0 is 128 x 128; frames with given orientations go through the describe path at sigma 1.8
in octave units (27 .. 38 patch rows, fbits 14: the largest words), one of them in a corner.  Three planes:

  radial     a wide blob plus noise: gradients in every direction under every orientation, so that every combination of
             lower bin and cell column reaches the slot sum 32 cx0 + 8 bin + 8 copy + DESC_SLOT_BIAS -- a wrong sign, scale
             or bias there permutes the bins of a cell.  The orientations run through the bin edges +-0, +-pi/4 .. +-pi, just
             inside +-pi, on to +-2 pi and to either side of the 16 bins beyond which make_desc_rec brings the angle back
             into [-4, 4] bins (every finite angle is accepted; the float32 4 pi is the largest that stays as given), and
             +-100 and +-1e4 radians, which are reduced.  The test restates the slot sum per sample and asserts that the
             sweep takes it below -150 (without the bias) and through all 8 slots of all 5 cell columns.
  faint      a faint narrow blob (peak 0.02 of the range) on a background of exactly 0: its tail runs through the float32
             denormals down to 0, 28 .. 47 pixels from the centre, and with it the gradient, its magnitude (0: the
             squares underflow), the weights and the fraction do0.  The frames lie between the blob's last non-zero
             words and that ring, so that every patch holds both (at least 20 samples with a denormal gradient).
  checker01  a 0 / 1 checkerboard of 3-pixel fields: the steepest gradients a unit-range image has, at fbits 14.

Every element of every descriptor lies inside the interval of tests/desc_rule.py, read from the device's own plane and
frame -- no allowance; the descriptors are finite and of length 1; the short-pass run (DEBUG_DESC_ROWS = 8,
DEBUG_DESC_LIST = 64) leaves the same bytes.

Temporary mutations of the new lines, each built and run once on an MI355X against this file and
tests/test_gpu_desc_rule.py: DESC_SLOT_BIAS = 0, `fx` in place of `fxs` and 2^-148 on the copy number
fail both; DESC_SLOT_BIAS = 128, too small for the 16 bins of orientation make_desc_rec hands over, fails only this
file (the sweep beyond +-pi);
2^-99 in place of 2^-100 on the bin shares -- a product scale of 2^-148 -- passes both and cannot fail either: it
doubles every word, and the normalisation divides it out (tests/test_desc_words.py holds the scales to the grid)."""
import numpy as np
import pytest

import desc_rule
from util import bits

pytestmark = pytest.mark.gpu

N = 64
SIGMA = 1.8                                                          # octave units
PI32 = np.float32(np.pi)
INSIDE = ((64.3, 64.6), (80.5, 70.25), (50.75, 52.5))                # octave units, within reach of either blob
CORNER = ((3.5, 2.25),)
# between the faint blob's last non-zero words (12 .. 16 pixels from its centre at levels 1 .. 3) and the ring where its
# tail is denormal (28 .. 47 pixels): every patch holds both
FAINT = ((84.3, 64.6), (64.25, 88.0), (45.5, 45.75))
_EDGES = [k * np.float32(np.pi / 4) for k in range(1, 4)] + [PI32, np.nextafter(PI32, np.float32(0.0))]
_FAR = [np.float32(2.0 * np.pi), np.float32(4.0 * np.pi), np.nextafter(np.float32(4.0 * np.pi), np.float32(np.inf)),
        np.float32(100.0), np.float32(1e4)]
SWEEP = np.array([0.0, -0.0] + [s * a for a in _EDGES + _FAR for s in (1.0, -1.0)], np.float32)
FEW = np.array([0.0, -0.0, 0.7, -PI32, np.float32(np.pi / 4), np.float32(-100.0)], np.float32)
ANG_LIMIT = 16.0                                                     # make_desc_rec: bins, beyond which the angle is reduced


def _radial():
    yy, xx = np.mgrid[0:N, 0:N].astype(np.float64)
    noise = np.random.Generator(np.random.PCG64(21)).uniform(0.0, 0.1, (N, N))
    return (0.3 + 0.5 * np.exp(-((xx - 32.0) ** 2 + (yy - 32.0) ** 2) / (2.0 * 9.0 ** 2)) + noise).astype(np.float32)


def _faint():
    yy, xx = np.mgrid[0:N, 0:N].astype(np.float64)
    with np.errstate(under="ignore"):
        return (0.02 * np.exp(-((xx - 32.0) ** 2 + (yy - 32.0) ** 2) / (2.0 * 0.7 ** 2))).astype(np.float32)


def _checker01():
    yy, xx = np.mgrid[0:N, 0:N]
    return (((xx // 3) + (yy // 3)) & 1).astype(np.float32)


PLANES = {"radial": (_radial, INSIDE + CORNER, SWEEP), "faint": (_faint, FAINT, FEW), "checker01": (_checker01, INSIDE + CORNER, FEW)}


def _frames(dtype, positions, angles):
    rows = [(x, y, a, 1 + k % 3) for a in angles for k, (x, y) in enumerate(positions)]
    fr = np.zeros(len(rows), dtype)
    for i, (x, y, a, lvl) in enumerate(rows):
        fr[i] = (np.float32(x) / 2, np.float32(y) / 2, np.float32(SIGMA) / 2, a, 0, lvl)   # image units, exactly halved
    return fr


def _slot_terms(rule, plane, angle):
    """(cx0, bin) per sample inside the square, as the kernel forms them: the cell column floor(u + 1.5) and the floor of the
    gradient's angle in [-2, 6) bins (x < 0 mirrors) minus the frame's angle in bins, reduced beyond ANG_LIMIT.  Samples
    with next to no gradient are left out: their angle is not the float64 one."""
    q, P = rule.patch, plane.astype(np.float64)
    gx, gy = P[q.row, q.col + 1] - P[q.row, q.col - 1], P[q.row + 1, q.col] - P[q.row - 1, q.col]
    theta = np.arctan2(gy, gx) * 4.0 / np.pi
    theta = np.where(theta < -2.0, theta + 8.0, theta)
    with np.errstate(over="ignore"):
        ang_bins = float(np.float32(angle) * np.float32(4.0 / np.pi))
    if not abs(ang_bins) <= ANG_LIMIT:
        ang_bins = np.remainder(float(angle) * 4.0 / np.pi + 4.0, 8.0) - 4.0
    keep = q.inside & (q.mod > 1e-4)
    return np.floor(q.u + 1.5)[keep].astype(np.int64), np.floor(theta - ang_bins)[keep].astype(np.int64)


@pytest.mark.parametrize("name", list(PLANES))
def test_given_frames_satisfy_the_descriptor_rule(gpu_hip, name):
    hip = gpu_hip
    make, positions, angles = PLANES[name]
    img = make()
    assert img.dtype == np.float32 and img.shape == (N, N)
    fr = _frames(hip.FRAME_DTYPE, positions, angles)
    assert desc_rule.fbits_of(SIGMA) == 14
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
    length = np.linalg.norm(desc.astype(np.float64), axis=1)
    assert np.abs(length - 1.0).max() < 1e-5, length

    bad, worst, cols, lows, tiny = [], 0.0, [], [], 0
    for i in range(len(fr)):
        plane = planes[int(e["lpos"][i])]
        r = desc_rule.analyse(plane, e["xpos"][i], e["ypos"][i], e["sigma"][i], df["orientation"][i, 0])
        assert r.patch.fbits == 14
        cx0, low = _slot_terms(r, plane, df["orientation"][i, 0])
        cols.append(cx0)
        lows.append(low)
        tiny += int(((r.patch.mod > 0) & (r.patch.mod < np.finfo(np.float32).tiny) & r.patch.inside).sum())
        off = desc_rule.check(r, desc[i])
        if off:
            bad.append(desc_rule.format_offenders(r, off, "%s frame %d" % (name, i)))
        worst = max(worst, desc_rule.error_ratio(r, desc[i]))
    cols, lows = np.concatenate(cols), np.concatenate(lows)
    sums = 32 * cols + 8 * lows if len(cols) else np.zeros(1, np.int64)
    print("%s: %d frames, slot sums without the bias %d .. %d, %d samples with a denormal gradient, %d with offenders, "
          "largest error / bound %.3f" % (name, len(fr), sums.min(), sums.max(), tiny, len(bad), worst))
    if name == "radial":                    # what the sweep is for
        assert sums.min() < -150 and sums.max() > 150
        assert cols.min() == -1 and cols.max() == 3
        assert len(set(zip(cols.tolist(), (lows & 7).tolist()))) == 5 * 8
    if name == "faint":
        assert tiny >= 20, tiny
    assert not bad, "%d descriptor(s) outside the rule\n    %s" % (len(bad), "\n    ".join(bad[:5]))

    # short passes: 8 rows or 64 list positions, whichever comes first -- the same bytes
    ctx = hip.Context(hip.default_params())
    try:
        ctx.debug_set(hip.DEBUG_DESC_ROWS, 8).debug_set(hip.DEBUG_DESC_LIST, 64)
        sf, sd = ctx.describe(img, fr, "given")
    finally:
        ctx.close()
    assert sf.tobytes() == df.tobytes() and sd.tobytes() == dd.tobytes()
