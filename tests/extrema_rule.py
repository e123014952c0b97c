"""Detection and refinement of DoG extrema as a plain float64 rule (a helper of tests/test_extrema_rule.py and
tests/test_gpu_extrema_rule.py, not a test).

Written from the statement of the reference's extremum search (s_extrema.cu:56-120 the strict 26-neighbour test,
:145-298 the three sift modes, :300-504 the refinement loop, s_solve.h the 3 x 3 solve) and the header's parameter
notes, not from extrema.hip: numpy planes D[z][y][x], every quantity a Python float (float64), reads clamped as the
reference's layered texture clamps them (x, y to the plane, z to the DoG planes 0 .. levels + 1).

refine() returns
    name    the path the candidate took: "singular+" prefix, the number of moves, the iteration it ended in, "/top" when
            it ended on the top DoG plane, the guards that held it back and the exit (accept or the reject reason);
    tags    the same as a set, for the census of tests/extrema_cases.py;
    result  (xn, yn, sn, lpos, sigma, cell) or None;
    margin  the smallest relative distance of any compared quantity from the threshold it was compared with, over all
            iterations.  A comparison with zero (the two determinants, the lower range bounds) is measured against the
            sum of the magnitudes of the terms of the quantity (the solve's determinant on a scale of its own, COND_MIN).
            A candidate whose margin is below THIN has no single right answer in float32 and is not used as a case.
            Two things differ from that plain definition, on purpose: the solve's determinant is thin below COND_MIN = 1e-3
            (stricter, see there), and equalities that float32 reproduces exactly are not thin (exact zeros of small dyadic
            entries, an offset equal to 0.6f in the reference's own float32 solve, |v| equal to the first threshold).

The thresholds are the float32 values the header names (1.6f * threshold, floorf(threshold), 2 * threshold,
(e + 1)^2 / e, 0.5f, 0.6f, 1.5f), converted to float64.

`variant` breaks exactly one step (VARIANTS); the committed cases must tell every one of them from the rule.
"""
import math

import numpy as np

POPSIFT, OPENCV, VLFEAT = 0, 1, 2
MODE_NAMES = {POPSIFT: "popsift", OPENCV: "opencv", VLFEAT: "vlfeat"}
THIN = 1e-4
MAX_ITERATIONS = 5
# The 3 x 3 determinant is a sum of six float32 products of three: its rounding error is about 3 * 2^-24 = 2e-7 of the
# sum of the magnitudes of its terms.  Where |det| is below COND_MIN of that sum, the offsets lose 2e-4 of their value
# and more, and a sigma held to 1e-5 (4e-5 of a level) has no single right answer either: such a candidate is thin.
# For offsets above 1 the same holds at |det| / max|d| (the absolute error is what sigma and the position see).
COND_MIN = 1e-3

VARIANTS = (
    "nonstrict_26",          # >= / <= against the neighbours
    "centre_in_own_plane",   # the own plane's 3 x 3 extreme taken with the centre in it
    "gt_at_0.6",             # d > 0.6f where the reference has d >= 0.6f (and d < -0.6f for d <= -0.6f)
    "no_x_guard",            # the step in x taken at nx = 1 / nx = width - 2 as well
    "no_z_guard",            # the step up taken on the top DoG plane as well
    "no_top_clamp",          # the plane above the top one read as zeros
    "two_sided_1.5",         # |d| >= 1.5 where the reference tests d >= 1.5 only
    "det_lt_0",              # det < 0 where the reference has det <= 0
    "singular_rejects",      # a singular solve drops the candidate
    "opencv_fifth_accepts",  # OpenCV mode keeps a candidate that converges in the fifth iteration
    "opencv_level_bound",    # OpenCV mode lets a candidate move to level maxlevel - 1
)

F = np.float32
H6, H5, H15 = float(F(0.6)), 0.5, 1.5


class Consts:
    """the float32 constants of one parameter set (oracle/popsift_oracle.c init_tables), as float64"""

    def __init__(self, mode=POPSIFT, levels=3, threshold=0.04, edge_limit=10.0, sigma=1.6, grid=2):
        self.mode, self.levels, self.grid = mode, levels, grid
        thr = F(F(F(threshold) * F(0.5)) * F(255.0)) / F(levels)
        self.threshold = float(thr)
        if mode == OPENCV:
            self.first_thr = float(np.floor(thr))
        elif mode == VLFEAT:
            self.first_thr = float(F(F(0.8) * F(2.0)) * thr)
        else:
            self.first_thr = float(F(1.6) * thr)
        self.contrast_thr = float(F(2.0) * thr)
        e = F(edge_limit)
        self.edge_thr = float(F(F(e + F(1.0)) * F(e + F(1.0))) / e)
        self.sigma0 = float(F(sigma))
        self.sigma_k = float(np.power(F(2.0), F(1.0) / F(levels)))
        self.border = 5 if mode == OPENCV else 1


def detect(D, C, variant=None):
    """candidates [(x, y, level)] of the planes D (NP, h, w) in the reference's order: level, then row, then column"""
    D = np.asarray(D, np.float64)
    NP, h, w = D.shape
    b = C.border
    out = []
    if w - 2 * b < 1 or h - 2 * b < 1:
        return out
    for z in range(1, C.levels + 1):
        v = D[z, b:h - b, b:w - b]
        gt = np.ones(v.shape, bool)
        lt = np.ones(v.shape, bool)
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dx == 0 and dy == 0 and dz == 0 and variant != "centre_in_own_plane":
                        continue
                    f = D[z + dz, b + dy:h - b + dy, b + dx:w - b + dx]     # b >= 1: no read leaves the plane
                    if variant == "nonstrict_26":
                        gt &= v >= f
                        lt &= v <= f
                    else:
                        gt &= v > f
                        lt &= v < f
        hit = (np.abs(v) >= C.first_thr) & (gt | lt)
        ys, xs = np.nonzero(hit)
        out += [(int(x) + b, int(y) + b, z) for y, x in zip(ys, xs)]
    return out


def _round_half_away(v):
    return math.floor(abs(v) + 0.5) * (1 if v >= 0 else -1)


def _solve3(A, b):
    """Cramer's rule on the symmetric 3 x 3 system, as s_solve.h states it; -> (d or None, |det| / sum of |terms|)"""
    (a00, a01, a02), (_, a11, a12), (_, _, a22) = A
    det0 = a11 * a22 - a12 * a12
    det1 = a12 * a02 - a01 * a22
    det2 = a01 * a12 - a11 * a02
    det3 = a00 * a22 - a02 * a02
    det4 = a01 * a02 - a00 * a12
    det5 = a00 * a11 - a01 * a01
    det = a00 * det0 + a01 * det1 + a02 * det2
    mag = (abs(a00) * (abs(a11 * a22) + a12 * a12) + abs(a01) * (abs(a12 * a02) + abs(a01 * a22))
           + abs(a02) * (abs(a01 * a12) + abs(a11 * a02)))
    if det == 0:
        # exactly singular in float32 too only where every product is exact there: entries that are multiples of 1/4 below 16
        # (24 bits hold the product of three such numbers), or where the in-plane block or the level row is zero (every term has a zero factor)
        small = all(abs(v) < 16 and v * 4 == int(v * 4) for v in (a00, a01, a02, a11, a12, a22))
        return None, (math.inf if small or (a00 == 0 and a01 == 0 and a11 == 0) or (a02 == 0 and a12 == 0 and a22 == 0)
                      else 0.0)
    inv = ((det0, det1, det2), (det1, det3, det4), (det2, det4, det5))
    d = [sum(inv[r][k] * b[k] for k in range(3)) / det for r in range(3)]
    return d, abs(det) / mag


def _solve3_f32(A, b):
    """s_solve.h operation by operation in float32 (no contraction): the offsets as the reference and the device hold them.
    None where an input is not a float32 value (then float32 Hessian entries are not these numbers either)."""
    (a00, a01, a02), (_, a11, a12), (_, _, a22) = A
    vals = [a00, a01, a02, a11, a12, a22, b[0], b[1], b[2]]
    f = [F(v) for v in vals]
    if any(float(q) != v for q, v in zip(f, vals)):
        return None
    i00, i01, i02, i11, i12, i22, b0, b1, b2 = f
    det0 = F(-i12 * i12) + F(i11 * i22)
    det1 = F(-i01 * i22) + F(i12 * i02)
    det2 = F(-i11 * i02) + F(i01 * i12)
    det3 = F(-i02 * i02) + F(i00 * i22)
    det4 = F(-i00 * i12) + F(i01 * i02)
    det5 = F(-i01 * i01) + F(i00 * i11)
    det = F(i00 * det0)
    det = F(det + F(i01 * det1))
    det = F(det + F(i02 * det2))
    if det == 0:
        return None
    rsd = F(F(1.0) / det)
    m00, m10, m20, m11, m12, m22 = (F(v * rsd) for v in (det0, det1, det2, det3, det4, det5))
    out = []
    for r in ((m00, m10, m20), (m10, m11, m12), (m20, m12, m22)):
        v = F(0.0)
        for m, q in zip(r, (b0, b1, b2)):
            v = F(v + F(m * q))
        out.append(v)
    return out


def refine(D, x, y, level, C, variant=None):
    """one candidate of detect() -> (name, tags, result, margin)"""
    NP, h, w = D.shape
    maxlevel = NP                       # the reference passes levels + 2: DoG planes 0 .. maxlevel - 1
    mode = C.mode
    margin = [math.inf]
    tags = set()

    def near(q, t, scale=None):
        s = abs(t) if scale is None else scale
        margin[0] = min(margin[0], abs(q - t) / s if s > 0 else (math.inf if q != t else 0.0))

    def at(px, py, pz):
        if pz > NP - 1 and variant == "no_top_clamp":
            return 0.0
        return float(D[min(max(pz, 0), NP - 1), min(max(py, 0), h - 1), min(max(px, 0), w - 1)])

    val = at(x, y, level)
    nx, ny, nz = x, y, level
    it, moves, singular = 0, 0, False
    d = [0.0, 0.0, 0.0]
    while True:
        it += 1
        R = lambda dx, dy, dz: at(nx + dx, ny + dy, nz + dz)
        c = R(0, 0, 0)
        Dx, Dy, Dz = 0.5 * (R(1, 0, 0) - R(-1, 0, 0)), 0.5 * (R(0, 1, 0) - R(0, -1, 0)), 0.5 * (R(0, 0, 1) - R(0, 0, -1))
        DDx, DDy, DDz = R(1, 0, 0) + R(-1, 0, 0) - 2 * c, R(0, 1, 0) + R(0, -1, 0) - 2 * c, R(0, 0, 1) + R(0, 0, -1) - 2 * c
        DXx = 0.25 * (R(1, 1, 0) + R(-1, -1, 0) - R(-1, 1, 0) - R(1, -1, 0))
        DXy = 0.25 * (R(1, 0, 1) + R(-1, 0, -1) - R(-1, 0, 1) - R(1, 0, -1))
        DXz = 0.25 * (R(0, 1, 1) + R(0, -1, -1) - R(0, 1, -1) - R(0, -1, 1))
        sol, cond = _solve3(((DDx, DXx, DXy), (DXx, DDy, DXz), (DXy, DXz, DDz)), (-Dx, -Dy, -Dz))
        # the solve's determinant against zero, brought to the scale of THIN (COND_MIN counts as THIN); the error of an offset
        # in pixels or levels, which is what the bars on position and sigma are about, grows with the offset itself
        big = max([1.0] + [abs(v) for v in sol]) if sol is not None else 1.0
        margin[0] = min(margin[0], cond / big * (THIN / COND_MIN))
        if sol is None:
            singular = True
            tags.add("singular")
            d = [0.0, 0.0, 0.0]
            if variant == "singular_rejects":
                return _done("singular_rejected", tags, None, margin[0], singular, moves, it, nz, NP)
            break
        d = sol
        last = it == MAX_ITERATIONS
        if mode == OPENCV:
            for v in d:
                near(abs(v), H5)
            if all(abs(v) < H5 for v in d):
                if last:
                    tags.add("fifth_converged")
                break
            step = []
            for v in d:
                r = _round_half_away(v)
                near(abs(v), max(abs(r) - 0.5, 0.5))
                near(abs(v), abs(r) + 0.5)
                step.append(r)
            nx, ny, nz = nx + step[0], ny + step[1], nz + step[2]
            moves += 1
            top = maxlevel - 1 if variant == "opencv_level_bound" else maxlevel - 2
            if nx < 5 or nx >= w - 5 or ny < 5 or ny >= h - 5 or nz < 1 or nz > top:
                which = "x" if (nx < 5 or nx >= w - 5) else "y" if (ny < 5 or ny >= h - 5) else "z"
                tags.add("left:" + which)
                return _done("left_range", tags, None, margin[0], singular, moves, it, nz, NP)
        else:
            if not last:
                ge = (lambda v: v > H6) if variant == "gt_at_0.6" else (lambda v: v >= H6)
                le = (lambda v: v < -H6) if variant == "gt_at_0.6" else (lambda v: v <= -H6)
                axes = [(0, nx, w - 2, "x"), (1, ny, h - 2, "y")]
                if mode == POPSIFT:
                    axes.append((2, nz, maxlevel - 1, "z"))
                t = [0, 0, 0]
                # An offset that EQUALS 0.6f as the float32 number the reference's solve yields is decided there, by `>=`:
                # like an exact zero it is no thin case (the float64 offset is 0.6, 2.4e-8 below 0.6f).  Everywhere else
                # float64 decides, with its margin.
                d32 = None
                if any(abs(abs(d[k]) - H6) < 1e-6 for k, _, _, _ in axes):
                    d32 = _solve3_f32(((DDx, DXx, DXy), (DXx, DDy, DXz), (DXy, DXz, DDz)), (-Dx, -Dy, -Dz))
                dc = list(d)
                for k, n, hi, nm in axes:
                    if d32 is not None and abs(float(d32[k])) == H6:
                        dc[k] = float(d32[k])
                        tags.add("step_equal")
                        continue
                    near(d[k], H6)
                    near(d[k], -H6)
                for k, n, hi, nm in axes:
                    free = (variant == "no_x_guard" and nm == "x") or (variant == "no_z_guard" and nm == "z" and d[k] > 0)
                    if ge(dc[k]):
                        if n < hi or free:
                            t[k] = 1
                        else:
                            tags.add("guard:%s_hi" % nm)
                    if le(dc[k]):
                        if n > 1 or free:
                            t[k] -= 1
                        else:
                            tags.add("guard:%s_lo" % nm)
                if t == [0, 0, 0]:
                    break
                nx, ny, nz = nx + t[0], ny + t[1], nz + t[2]
                moves += 1
        if it >= MAX_ITERATIONS:
            break

    def done(exit_, result=None):
        return _done(exit_, tags, result, margin[0], singular, moves, it, nz, NP)

    if it >= MAX_ITERATIONS and mode == OPENCV and variant != "opencv_fifth_accepts":
        return done("fifth_iteration")
    if mode != OPENCV:
        for v in d:
            near(v, H15)
            if variant == "two_sided_1.5":
                near(v, -H15)
        if any(v <= -H15 for v in d):
            tags.add("far_negative")
        if any(v >= H15 or (variant == "two_sided_1.5" and v <= -H15) for v in d):
            return done("far_positive")
    xn, yn, sn = nx + d[0], ny + d[1], nz + d[2]
    if mode != OPENCV:
        for q, hi in ((xn, w - 1.0), (yn, h - 1.0), (sn, float(maxlevel))):
            if not singular:            # after a singular solve the offset is 0 and these are comparisons of integers
                near(q, 0.0, 1.0)
                near(q, hi)
        if xn < 0 or xn > w - 1.0 or yn < 0 or yn > h - 1.0 or sn < 0 or sn > maxlevel:
            return done("out_of_range")
    contr = val + 0.5 * (Dx * d[0] + Dy * d[1] + Dz * d[2])
    tr = DDx + DDy
    det = DDx * DDy - DXx * DXx
    # an exact zero of small dyadic entries (multiples of 1/4 below 16) is exact in float32 as well: no thin case
    if not (det == 0 and all(abs(v) < 16 and v * 4 == int(v * 4) for v in (DDx, DDy, DXx))):
        near(det, 0.0, abs(DDx * DDy) + DXx * DXx)
    if det < 0 or (det == 0 and variant != "det_lt_0"):
        return done("det_nonpos")
    near(abs(contr), C.contrast_thr)
    if abs(contr) < C.contrast_thr:
        return done("low_contrast")
    if det == 0:                        # variant det_lt_0 only: the edge value is +inf (tr != 0) or NaN
        return done("edge") if tr != 0 else done("accept", _result(xn, yn, sn, w, h, C, near))
    edge = tr * tr / det
    near(edge, C.edge_thr)
    if edge >= C.edge_thr:
        return done("edge")
    return done("accept", _result(xn, yn, sn, w, h, C, near))


def _result(xn, yn, sn, w, h, C, near):
    lpos = _round_half_away(sn)
    near(sn, max(lpos - 0.5, 0.5))
    near(sn, lpos + 0.5)
    qx, qy = xn / (w / C.grid), yn / (h / C.grid)
    for q in (qx, qy):
        k = math.floor(q)
        near(q, float(k), max(k, 1.0))
        near(q, k + 1.0)
    cell = int(math.floor(qy) * C.grid + math.floor(qx))
    return (xn, yn, sn, int(lpos), C.sigma0 * C.sigma_k ** sn, cell)


def _done(exit_, tags, result, margin, singular, moves, it, nz, NP):
    tags = set(tags)
    tags.add("exit:" + exit_)
    tags.add("moves:%d" % moves)
    top = nz == NP - 1
    if result is not None:
        if top:
            tags.add("top_accept")
        if singular:
            tags.add("singular_accept")
        if it == MAX_ITERATIONS:
            tags.add("fifth_accept")
    guards = "".join("/" + g for g in sorted(t for t in tags if t.startswith("guard:") or t.startswith("left:")))
    name = "%smoves%d/iter%d%s%s/%s" % ("singular+" if singular else "", moves, it, "/top" if top else "", guards, exit_)
    return name, tags, result, margin


EXT = np.dtype([("octave", np.int32), ("x", np.int32), ("y", np.int32), ("level", np.int32), ("xn", np.float64),
                ("yn", np.float64), ("sn", np.float64), ("lpos", np.int32), ("sigma", np.float64), ("cell", np.int32)])


def run(D, C, variant=None, octave=0):
    """all candidates of one octave -> (trace, extrema): trace = [(x, y, level, name, tags, margin, result)] of every candidate,
    extrema = EXT records of the accepted ones in the reference's order"""
    D = np.asarray(D, np.float64)
    trace, ext = [], []
    for x, y, z in detect(D, C, variant):
        name, tags, res, margin = refine(D, x, y, z, C, variant)
        trace.append((x, y, z, name, tags, margin, res))
        if res is not None:
            ext.append((octave, x, y, z) + res)
    return trace, np.array(ext, EXT)
