"""The orientation rule of one keypoint in float64, with decision margins (no GPU).

`analyse` restates orientation_one (oracle/popsift_oracle.c; ori_par, s_orientation.cu:60-242) from a Gaussian plane and
an extremum.  The INTEGER decisions are formed exactly as the oracle and the device form them, in float32: the window
radius roundf(3 * 1.5 * sigma), the window clamped to 1 .. w-2 / 1 .. h-2, sq_dist = (int)(dx*dx + dy*dy).  Everything
else is float64: gradient, hypot, atan2, exp(sq_dist * factor), the bin coordinate t = 36 (theta + pi) / 2 pi, the
36-bin histogram and the six 3-tap box passes.  The rule is the same in every sift_mode (the oracle's has no mode).

Every comparison of the rule then gets an explicit uncertainty, so a keypoint is either DECIDED -- the number of
orientations and every angle are fixed, whatever a correct float32 / fixed-point implementation rounds -- or OPEN, and
`check` says which reported features break which of the two sets of requirements.

delta, the amount by which one SMOOTHED bin of a correct implementation may differ from the float64 one, is the sum of

  U               the total weight of the samples whose t lies within EDGE_EPS = 1e-4 of a bin edge k + 0.5: such a
                  sample may fall into either bin (1e-4 is 45 times the 2.2e-6 bins of the device's cheap arctangent,
                  which hands every sample nearer than 1e-4 to an edge to its accurate one; keypoint.hip, atan2_bins);
  n * 2^-20       the device's fixed-point resolution (from_fix, keypoint_dev.h): each of the n samples inside the circle
                  is truncated to a multiple of 2^-20, losing less than one unit;
  TAU * max(H)    float32 rounding of the weights and the sums, TAU = 1e-5, relative to the largest SMOOTHED bin: a
                  relative error TAU * raw[i] per raw bin averages to TAU * H[b] <= TAU * max(H).  The oracle needs
                  1e-7; the two orders above it are for the device's hardware exp2, rcp and sqrt.

The six box passes are one circular convolution with non-negative taps that sum to 1: a smoothed bin is an AVERAGE of
raw bins.  Moving a sample of weight w to the neighbouring raw bin changes a smoothed bin by w times the difference of
two neighbouring taps, less than w; the other two terms are bounds per raw bin and pass through the average unchanged.
Hence the factors:

  2 delta   a difference of two smoothed bins (the peak test H[b] > max(H[b-1], H[b+1])) moves by at most 2 delta;
  4 delta   the interpolated height is the maximum over the offset of the quadratic through three bins, and for a fixed
            offset in [0, 2] that quadratic is a combination of the three bins with Lagrange weights whose absolute sum
            is at most 1.25: the height moves by at most 1.25 delta, a height against 0.8 of another by 2.25 delta, the
            difference of two heights by 2.5 delta.  4 delta covers each with room.

A bin that is only POSSIBLY a peak (margin within +-2 delta) gets, as the upper estimate of its height, the parabola with
its centre raised to the larger neighbour where it is lower (the parabola through a non-peak is meaningless), and the
bin centre as its angle.  The largest height is itself uncertain when the best peak is uncertain: `must` is taken
against the largest upper estimate, `may` against the largest certain height.
"""
import numpy as np

NB = 36
EDGE_EPS = 1e-4
FIX_RES = 2.0 ** -20
TAU = 1e-5
BIN_RAD = 2.0 * np.pi / NB
ANGLE_FLOOR = 1e-6          # rad: float32 rounding of an angle of magnitude <= pi and of the quotient num / denB
OPEN_REACH = 0.75 * BIN_RAD  # 1.5 half-bins: an interpolated peak lies within half a bin of its bin's centre


def _roundf(v):
    """roundf of a float32 (half away from zero) as an int."""
    v = float(v)
    return int(np.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def _bin_angle(pos):
    return BIN_RAD * pos - np.pi


def adiff(p, q):
    d = abs(float(p) - float(q)) % (2 * np.pi)
    return min(d, 2 * np.pi - d)


class Rule:
    """What the rule says about one keypoint.  peaks: bin -> dict(height, angle, curv, certain)."""
    __slots__ = ("H", "raw", "U", "n", "delta", "peaks", "must", "may", "decided", "expect", "flat", "why")


def histogram(plane, x, y, sigma):
    """-> (raw float64 histogram, U, n): see the module docstring."""
    h, w = plane.shape
    f32 = np.float32
    x, y, sigma = f32(x), f32(y), f32(sigma)
    sigw = f32(1.5) * sigma
    rad = _roundf(f32(3.0) * sigw)
    factor = -0.5 / (float(sigw) * float(sigw))
    xmin, xmax = max(1, _roundf(x) - rad), min(w - 2, _roundf(x) + rad)
    ymin, ymax = max(1, _roundf(y) - rad), min(h - 2, _roundf(y) + rad)
    raw = np.zeros(NB)
    if xmax < xmin or ymax < ymin:
        return raw, 0.0, 0
    xs, ys = np.arange(xmin, xmax + 1), np.arange(ymin, ymax + 1)
    dx, dy = xs.astype(f32) - x, ys.astype(f32) - y
    sq = ((dx * dx)[None, :] + (dy * dy)[:, None]).astype(f32)   # float32 products, float32 sum
    sq_dist = sq.astype(np.int64)                                 # (int): truncation, the values are >= 0
    inside = sq_dist <= rad * rad
    P = plane.astype(np.float64)
    gx = P[ymin:ymax + 1, xmin + 1:xmax + 2] - P[ymin:ymax + 1, xmin - 1:xmax]
    gy = P[ymin + 1:ymax + 2, xmin:xmax + 1] - P[ymin - 1:ymax, xmin:xmax + 1]
    wgt = (np.hypot(gx, gy) * np.exp(sq_dist * factor))[inside]
    t = (NB * (np.arctan2(gy, gx) + np.pi) / (2 * np.pi))[inside]
    raw = np.bincount(np.floor(t + 0.5).astype(np.int64) % NB, weights=wgt, minlength=NB).astype(np.float64)
    on_edge = np.abs(t - np.floor(t) - 0.5) < EDGE_EPS
    return raw, float(wgt[on_edge].sum()), int(inside.sum())


def smooth(raw):
    H = np.asarray(raw, np.float64)
    for _ in range(6):
        H = (np.roll(H, 1) + H + np.roll(H, -1)) / 3.0
    return H


def _parabola(hp, hv, hn, b):
    """The oracle's formulae: -> (height, position in bins in [0, 36), denB), or None where the offset leaves [0, 2]."""
    num = 3.0 * hp - 4.0 * hv + hn
    den = 2.0 * (hp - 2.0 * hv + hn)
    newbin = num / den
    if not (0.0 <= newbin <= 2.0):
        return None
    pos = (b - 1) % NB + newbin
    if pos >= NB:
        pos -= NB
    return -(num * num) / (4.0 * den) + hp, pos, den


def analyse(plane, x, y, sigma, tau=TAU, fixed_point=True):
    """fixed_point=False leaves the device's n * 2^-20 out of delta (an implementation that sums in floats, the oracle)."""
    r = Rule()
    r.raw, r.U, r.n = histogram(plane, x, y, sigma)
    r.H = H = smooth(r.raw)
    r.delta = d = r.U + (r.n * FIX_RES if fixed_point else 0.0) + tau * float(H.max())
    r.peaks, r.why = {}, ""
    # a histogram of zeros has no peak: every height is -inf, -inf >= 0.8 * -inf holds four times, and each of the four
    # orientations is the "no peak" position -1 (oracle and device alike)
    r.flat = not (r.raw.max() > 0.0)
    if r.flat:
        r.must = r.may = r.expect = []
        r.decided = True
        return r
    for b in range(NB):
        hp, hv, hn = H[b - 1], H[b], H[(b + 1) % NB]
        margin = hv - max(hp, hn)
        if margin <= -2 * d:
            continue
        certain = margin > 2 * d
        par = _parabola(hp, hv, hn, b) if certain else None
        if certain and par is not None:
            r.peaks[b] = dict(height=par[0], angle=_bin_angle(par[1]), curv=abs(par[2]), certain=True, margin=margin)
        else:
            top = max(hv, hp, hn)
            par = _parabola(hp, top, hn, b) if 2.0 * top - hp - hn > 0.0 else None
            r.peaks[b] = dict(height=par[0] if par else top, angle=_bin_angle(b), curv=0.0, certain=False, margin=margin)
    hi = max(p["height"] for p in r.peaks.values())
    lo = max([p["height"] for p in r.peaks.values() if p["certain"]] + [-np.inf])
    r.must = sorted(b for b, p in r.peaks.items() if p["certain"] and p["height"] > 0.8 * hi + 4 * d)
    r.may = sorted(b for b, p in r.peaks.items() if p["height"] > 0.8 * lo - 4 * d)
    r.decided = r.must == r.may
    if not r.decided:
        r.why = "must %s, may %s" % (r.must, r.may)
    by_height = sorted(r.must, key=lambda b: -r.peaks[b]["height"])
    if r.decided and len(by_height) > 4 and r.peaks[by_height[3]]["height"] - r.peaks[by_height[4]]["height"] <= 4 * d:
        r.decided = False
        r.why = "the 4th and 5th of %d peaks within 4 delta" % len(by_height)
    r.expect = by_height[:4]
    return r


def angle_bound(r, b):
    """How far a correct implementation's angle of the certain peak b may be from the float64 one (rad)."""
    return BIN_RAD * r.delta / r.peaks[b]["curv"] + ANGLE_FLOOR


def analyse_all(plane_of, ext, n_planes, tau=TAU, fixed_point=True):
    """plane_of(octave, level) -> the Gaussian plane; ext: EXTREMUM_DTYPE, octave units; n_planes = levels + 3."""
    cache, out = {}, []
    for e in ext:
        key = (int(e["octave"]), min(max(int(e["lpos"]), 0), n_planes - 1))
        if key not in cache:
            cache[key] = plane_of(*key)
        out.append(analyse(cache[key], e["xpos"], e["ypos"], e["sigma"], tau, fixed_point))
    return out


def aligned(ext, feats, upscale_factor):
    """ext[i] (octave units) and feats[i] (image units) are the same keypoint, for every i: a feature's position and
    scale are its extremum's times 2^(octave - upscale), a power of two."""
    sc = np.exp2(ext["octave"].astype(np.float64) - int(upscale_factor)).astype(np.float32)
    return len(ext) == len(feats) and np.array_equal(ext["octave"], feats["debug_octave"]) and all(
        np.array_equal((ext[n] * sc).view(np.uint32), np.ascontiguousarray(feats[n]).view(np.uint32)) for n in ("xpos", "ypos", "sigma"))


def check(rules, ext, feats):
    """rules[i], ext[i] and feats[i] belong to one keypoint (the extremum list and the features are in the same order).
    Returns the offenders: dicts with octave, x, y (octave units), decided, what, margin and a message."""
    assert len(rules) == len(ext) == len(feats), (len(rules), len(ext), len(feats))
    assert np.array_equal(ext["octave"], feats["debug_octave"])
    bad = []

    def offend(i, what, margin, msg):
        e, r = ext[i], rules[i]
        bad.append(dict(index=i, octave=int(e["octave"]), x=float(e["xpos"]), y=float(e["ypos"]), decided=r.decided, what=what,
                        margin=float(margin), msg="octave %d (%.3f, %.3f) sigma %.3f, %s, delta %.3g (U %.3g, n %d, max H %.4g): %s" % (
                            e["octave"], e["xpos"], e["ypos"], e["sigma"], "decided" if r.decided else "open (%s)" % r.why,
                            r.delta, r.U, r.n, r.H.max(), msg)))

    for i, (r, f) in enumerate(zip(rules, feats)):
        n = int(f["num_ori"])
        got = [float(a) for a in f["orientation"][:max(0, min(n, 4))]]
        if r.flat:
            if n != 4 or any(adiff(a, _bin_angle(-1.0)) > ANGLE_FLOOR for a in got):
                offend(i, "flat", n, "an empty histogram gives four orientations at position -1, got %d: %s" % (n, got))
            continue
        if not 1 <= n <= 4:
            offend(i, "num_ori", n, "num_ori %d outside 1 .. 4" % n)
            continue
        if r.decided:
            if n != len(r.expect):
                offend(i, "num_ori", n - len(r.expect), "num_ori %d, the rule gives %d (bins %s, heights %s against 0.8 x %.6g)" % (
                    n, len(r.expect), r.expect, ["%.6g" % r.peaks[b]["height"] for b in r.expect],
                    max(p["height"] for p in r.peaks.values())))
                continue
            free = list(range(n))
            for b in r.expect:
                want = r.peaks[b]["angle"]
                j = min(free, key=lambda j: adiff(got[j], want))
                free.remove(j)
                err, bound = adiff(got[j], want), angle_bound(r, b)
                if err > bound:
                    offend(i, "angle", err / bound, "bin %d: angle %.7f, the rule gives %.7f: off by %.3g rad, bound %.3g" % (
                        b, got[j], want, err, bound))
        else:
            for a in got:
                reach = min(adiff(a, _bin_angle(b)) for b in r.may)
                if reach > OPEN_REACH:
                    offend(i, "stray", reach / OPEN_REACH, "angle %.6f is %.3g rad from the nearest possible peak (bins %s)" % (
                        a, reach, r.may))
            if n < 4:
                for b in r.must:
                    reach = min(adiff(a, _bin_angle(b)) for a in got)
                    if reach > OPEN_REACH:
                        offend(i, "missing", reach / OPEN_REACH, "certain peak in bin %d (height %.6g) not among the %d reported: %s" % (
                            b, r.peaks[b]["height"], n, got))
    return bad


def format_offenders(bad, limit=20):
    return "%d offender(s)\n    %s" % (len(bad), "\n    ".join(o["msg"] for o in bad[:limit]))
