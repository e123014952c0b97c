"""The loop descriptor of one (plane, x, y, sigma, angle) in float64, with a bound per output element (no GPU).

`analyse` restates descriptor_one (oracle/popsift_oracle.c; ext_desc_loop_sub, s_desc_loop.cu:19-138) and
oracle_normalize.  The five inputs are float32 values in octave units; everything after them is float64.  Scope:
desc_mode = POPSIFT_HIP_DESC_LOOP (k_descriptor, keypoint.hip) -- the only descriptor that is a CONTINUOUS function of its
inputs.  iloop, igrid and notile quantise their texture weights to 1/256 and grid snaps its samples to pixels: step
functions, which need a rule of the kind tests/ori_rule.py is (decisions with margins), not this one.

The rule.  SBP = 3 sigma, (c, s) = the two float32 of sincos_cr(angle), the correctly rounded cosine and sine that oracle and
device both rotate by.  The samples are the pixels (j, i), 1 <= j <= w-2, 1 <= i <= h-2, of
the plane P inside the rotated square |u|, |v| < 2.5,

    u = (c (j - x) + s (i - y)) / SBP,    v = (c (i - y) - s (j - x)) / SBP.

A sample has the central-difference gradient g = (P[i, j+1] - P[i, j-1], P[i+1, j] - P[i-1, j]), the weight
wm = exp(-(u^2 + v^2) / 8) |g| and the bin coordinate t = (atan2(g) - angle) 4 / pi mod 8.  With hat(z) = max(0, 1 - |z|)
it adds

    wm * hat(v + 1.5 - iy) * hat(u + 1.5 - ix) * hat(circular distance of t and b)

to bin b = 0 .. 7 of cell (iy, ix), iy, ix = 0 .. 3: element iy * 32 + ix * 8 + b of the raw histogram h.  That is the
reference's (1 - |nx|)(1 - |ny|) per cell and (1 - d, d) per bin pair, and the device's (1 - fx, fx) x (1 - fy, fy) "on the
cells that exist" -- the hats of the cells -1 and 4 are simply absent.  Every factor is continuous, and the weights fall
to zero at the edge of the square, so which side of |u| = 2.5 a rounding puts a sample on does not matter.

Each raw element carries delta = A + F + P + T, by how much a correct float32 / fixed-point implementation may differ:

  A  arctangent.  A shift of t by e moves e * wm * (cell weight) between two neighbouring bins, so
         A[b] = e * sum over the samples whose t lies within 1 + 1e-4 of b of wm * hat * hat.
     e = A_POLY = 1.5e-5 bins, the stated maximum error of the device's degree-9 arctangent (atan2_bins9, keypoint.hip;
     tests/test_desc_rule.py re-measures it from the polynomial's coefficients), plus A_FLOAT = 1.5e-6 for float32
     angle arithmetic on either side: theta - angle is rounded at a magnitude of up to 2 pi (ulp 4.8e-7 rad = 6.1e-7
     bins), t at up to 8 (ulp 4.8e-7; the reference rounds it UP, __fmul_ru), and atan2f itself is good to 1e-7.
     A_FLOAT is an addition to the 1.5e-5 the polynomial alone accounts for, and it stays on when the polynomial's
     part is switched off: without it the ORACLE leaves the rule on 0 .. 4 descriptors per case (near-empty bins that
     hold only the tail of a neighbouring bin's shares; test_float_angle_term_is_needed).
  F  fixed point.  k_descriptor adds round-to-nearest(share * weight * 2^fbits) (the 2^23 trick) to one half of a 64-bit
     word per (sample, cell that exists), low half for bin floor(t), high half for floor(t) + 1: half a unit of 2^-fbits
     per (sample, cell) that touches the element.  fbits is restated from make_desc_rec.
  P  position.  |d hat / dz| <= 1 and |d exp(-(u^2 + v^2) / 8) / du| <= |u| / 4, so a position error of eps cell units in
     each of u and v moves an element by at most
         eps * sum wm * share * ([hat_x alive] hat_y + [hat_y alive] hat_x + (|u| + |v|) / 4 * hat_x * hat_y),
     "alive" = within 1 + 1e-4 of the cell centre (a sample next to a cell's support may enter it).  Samples up to 1e-4
     outside the square are part of this sum for the same reason.  This term is needed: the oracle's raw-bin error does
     not scale with the bin, it scales with this sum (test_desc_rule.py measures the ratio).  eps from the arithmetic:
       oracle   the cell centre ptx = fmaf(csbp, offx, fmaf(-ssbp, offy, x)) is a float32 at the magnitude M of the plane
                coordinate: two roundings, one ulp(M); rotated into cell units: (|c| + |s|) ulp(M) / SBP.  Then
                dx = j - ptx, the two FMAs of nx / ny and dnx = nx + offx: five roundings of values <= 2.5 (|c| + |s|)
                plus crsbp / srsbp themselves (cos rounded, SBP rounded, the quotient rounded: 2 ulp relative).
                eps_oracle = (|c| + |s|) ulp32(M) / SBP + 12 * 2^-24 * (|c| + |s|)^2 * 2.5
       device   the integers c, r of a sample enter u = fmaf(crsbp, fc, fmaf(srsbp, fr, u0)) with u0 = fmaf(crsbp, ox,
                srsbp * oy), (ox, oy) the keypoint's offset from the patch corner: five roundings (the offset, the
                product, three FMAs) of cell-unit values of at most 2 U, U = 2.5 (|c| + |s|)^2 + (|c| + |s|) / SBP the
                largest |u| in the bounding box, the same 2 ulp of crsbp / srsbp on two terms of at most U each, and
                tu = u + 1.5 (<= 4).   eps_device = 2^-24 * (9 U + 4)
     The plane coordinate does not enter the device's arithmetic after the (exact or 2^-24-relative) subtraction
     xmin - x, which is why it is the sharper of the two wherever x is large.
  T  TAU * h[b], TAU = 1e-5: float32 products and sums, the hardware exp2, sqrt, rcp and rsq.  The same TAU as
     tests/ori_rule.py; it is not a knob.

Normalisation.  delta goes through oracle_normalize by interval arithmetic; with h in [h - delta, h + delta] (not below 0):

  RootSift  out[b] = 2^m sqrt(h[b] / S), S = sum h, monotone in h[b] and in S:
                lo = 2^m sqrt(max(h - delta, 0) / (S + D)),  hi = 2^m sqrt((h + delta) / (S - D)),  D = sum delta.
            The square root magnifies near-empty bins: delta / S = 1e-8 on an empty bin is 1e-4 of the descriptor.
  classic   n1 = |h|, cl = min(h, 0.2 n1), out = 2^m cl / |cl|: min and the norms are monotone in every h[b], so
                n1 in [|h_lo|, |h_hi|],  cl in [min(h_lo, 0.2 n1_lo), min(h_hi, 0.2 n1_hi)],
                out in [cl_lo / |cl_hi|, cl_hi / |cl_lo|].
            A bin within delta of the clip is covered: its interval contains both h and 0.2 n1.
  Both ends move out by 2^-23 |out| plus one float32 unit of out: the quotient, the root and the final rounding.

`check` says which elements of a reported descriptor leave [lo, hi].  The rule has no allowance.
"""
import numpy as np

A_POLY = 1.5e-5
A_FLOAT = 1.5e-6
TAU = 1e-5
REACH = 1e-4            # cell units resp. bins: how near to a support a sample must be to count as "may enter it"
DESC_MAGNIFY = 3.0
ROOTSIFT, CLASSIC = 0, 1
_K4, _K8 = np.arange(4.0), np.arange(8.0)


def _ulp32(v):
    v = np.abs(np.asarray(v, np.float32))
    return (np.nextafter(v, np.float32(np.inf)) - v).astype(np.float64)


def fbits_of(sigma):
    """make_desc_rec (keypoint.hip), in float32 as there."""
    f32 = np.float32
    sbp = np.abs(f32(DESC_MAGNIFY) * f32(sigma))
    side = f32(2.83) * sbp + f32(1.0)
    cell_px = f32(side * side)
    return int(min(max(31 - int(np.ceil(np.log2(np.float64(f32(361.0) * cell_px)))), 2), 14))


class Patch:
    """The samples of one descriptor (arrays over the samples) and what `evaluate` needs of its frame."""
    __slots__ = ("x", "y", "sigma", "angle", "w", "h", "col", "row", "u", "v", "mod", "t", "inside", "cs", "sbp", "fbits")

    @property
    def n(self):
        return int(self.inside.sum())

    @property
    def rows(self):
        return len(np.unique(self.row[self.inside]))


def uv_float64(p, xs, ys):
    c, s = p.cs
    dx, dy = (xs - p.x)[None, :], (ys - p.y)[:, None]
    return (c * dx + s * dy) / p.sbp, (c * dy - s * dx) / p.sbp


def uv_device(p, xs, ys):
    """u, v as k_descriptor forms them: float32, FMAs on the column and row counted from the patch corner (a double
    product plus a double sum rounded once is the FMA up to double rounding)."""
    f32, f64 = np.float32, np.float64
    fma = lambda a, b, c: (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)
    arr = lambda v: np.asarray(v, f32)
    c, s = f32(p.cs[0]), f32(p.cs[1])
    sbp = np.abs(f32(DESC_MAGNIFY) * f32(p.sigma))
    crsbp, srsbp = arr(c / sbp), arr(s / sbp)
    ox, oy = arr(f32(xs[0]) - f32(p.x)), arr(f32(ys[0]) - f32(p.y))
    u0, v0 = fma(crsbp, ox, arr(srsbp * oy)), fma(crsbp, oy, arr(-srsbp * ox))
    fc, fr = (xs - xs[0]).astype(f32)[None, :], (ys - ys[0]).astype(f32)[:, None]
    u = fma(crsbp, fc, fma(srsbp, fr, u0))
    v = fma(crsbp, fr, fma(-srsbp, fc, v0))
    return u.astype(f64), v.astype(f64)


def samples(plane, x, y, sigma, angle, uv=uv_float64):
    h, w = plane.shape
    p = Patch()
    p.x, p.y, p.sigma, p.angle = (float(np.float32(v)) for v in (x, y, sigma, angle))
    p.w, p.h = w, h
    p.sbp = DESC_MAGNIFY * abs(p.sigma)
    p.cs = (float(np.float32(np.cos(p.angle))), float(np.float32(np.sin(p.angle))))   # the two floats of sincos_cr
    p.fbits = fbits_of(sigma)
    empty = np.zeros(0)
    p.col = p.row = np.zeros(0, np.int64)
    p.u = p.v = p.mod = p.t = empty
    p.inside = np.zeros(0, bool)
    if not p.sbp > 0.0:
        return p
    r = 2.5 * (abs(p.cs[0]) + abs(p.cs[1])) * p.sbp + 1.0
    x0, x1 = max(1, int(np.floor(p.x - r))), min(w - 2, int(np.ceil(p.x + r)))
    y0, y1 = max(1, int(np.floor(p.y - r))), min(h - 2, int(np.ceil(p.y + r)))
    if x1 < x0 or y1 < y0:
        return p
    xs, ys = np.arange(x0, x1 + 1), np.arange(y0, y1 + 1)
    u, v = uv(p, xs.astype(np.float64), ys.astype(np.float64))
    near = (np.abs(u) < 2.5 + REACH) & (np.abs(v) < 2.5 + REACH)
    iy, ix = np.nonzero(near)
    P = plane[y0 - 1:y1 + 2, x0 - 1:x1 + 2].astype(np.float64)
    gx = (P[1:-1, 2:] - P[1:-1, :-2])[iy, ix]
    gy = (P[2:, 1:-1] - P[:-2, 1:-1])[iy, ix]
    p.col, p.row, p.u, p.v = xs[ix], ys[iy], u[iy, ix], v[iy, ix]
    p.inside = (np.abs(p.u) < 2.5) & (np.abs(p.v) < 2.5)
    p.mod = np.hypot(gx, gy)
    p.t = ((np.arctan2(gy, gx) - p.angle) * (4.0 / np.pi)) % 8.0
    return p


def _hats(p):
    ax, ay = np.abs((p.u + 1.5)[:, None] - _K4), np.abs((p.v + 1.5)[:, None] - _K4)
    dist = np.abs((p.t[:, None] - _K8 + 4.0) % 8.0 - 4.0)
    return ax, ay, dist


def _acc(fy, fx, fb, wgt):
    """sum over the samples of wgt * fy[:, iy] * fx[:, ix] * fb[:, b] -> 128 elements"""
    n = len(wgt)
    return ((fy * wgt[:, None]).T @ (fx[:, :, None] * fb[:, None, :]).reshape(n, 32)).reshape(128)


def raw_histogram(p, mult=None, t_shift=0.0):
    """The raw histogram alone.  mult: a factor per sample (0 drops it, 2 counts it twice); t_shift: added to every t.
    Both are for the doctored implementations of tests/test_desc_rule.py."""
    if len(p.u) == 0:
        return np.zeros(128)
    q = p
    if t_shift:
        q = Patch()
        for name in Patch.__slots__:
            setattr(q, name, getattr(p, name))
        q.t = (p.t + t_shift) % 8.0
    ax, ay, dist = _hats(q)
    wm = np.exp(-(q.u * q.u + q.v * q.v) / 8.0) * q.mod * q.inside
    if mult is not None:
        wm = wm * mult
    return _acc(np.clip(1.0 - ay, 0.0, None), np.clip(1.0 - ax, 0.0, None), np.clip(1.0 - dist, 0.0, None), wm)


def eps_oracle(p):
    k = abs(p.cs[0]) + abs(p.cs[1])
    big = max(abs(p.x), abs(p.y)) + 1.5 * k * p.sbp
    return k * float(_ulp32(big)) / p.sbp + 12.0 * 2.0 ** -24 * 2.5 * k * k


def eps_device(p):
    k = abs(p.cs[0]) + abs(p.cs[1])
    return 2.0 ** -24 * (9.0 * (2.5 * k * k + k / p.sbp) + 4.0)


class Rule:
    """h, delta and the four terms: raw, 128 each.  out, lo, hi: the normalised descriptor and its interval."""
    __slots__ = ("patch", "h", "delta", "terms", "sens", "out", "lo", "hi", "norm_mode", "norm_multi", "eps")

    @property
    def bound_l2(self):
        """L2 of the per-element bound relative to the descriptor's length 2^norm_multi"""
        return float(np.linalg.norm(np.maximum(self.hi - self.out, self.out - self.lo)) / 2.0 ** self.norm_multi)


def normalize(h, norm_mode, norm_multi):
    h = np.asarray(h, np.float64)
    m = 2.0 ** norm_multi
    with np.errstate(all="ignore"):
        if norm_mode == ROOTSIFT:
            return m * np.sqrt(h / h.sum())
        cl = np.minimum(h, 0.2 * np.linalg.norm(h))
        return m * cl / np.linalg.norm(cl)


def interval(h, delta, norm_mode, norm_multi):
    """-> (out, lo, hi): the module docstring's interval arithmetic.  A histogram whose sum (norm) may be zero is
    unbounded above."""
    m = 2.0 ** norm_multi
    out = normalize(h, norm_mode, norm_multi)
    hl, hh = np.maximum(h - delta, 0.0), h + delta
    with np.errstate(all="ignore"):
        if norm_mode == ROOTSIFT:
            lo = m * np.sqrt(hl / hh.sum())
            hi = m * np.sqrt(hh / hl.sum())
        else:
            cl_lo = np.minimum(hl, 0.2 * np.linalg.norm(hl))
            cl_hi = np.minimum(hh, 0.2 * np.linalg.norm(hh))
            lo, hi = m * cl_lo / np.linalg.norm(cl_hi), m * cl_hi / np.linalg.norm(cl_lo)
    hi = np.where(np.isfinite(hi), hi, np.inf)
    lo = np.where(np.isfinite(lo), lo, 0.0)
    fin = np.where(np.isfinite(out), out, 0.0)
    r = 2.0 ** -23 * np.abs(fin) + _ulp32(fin)
    return out, lo - r, hi + r


def evaluate(p, norm_mode=ROOTSIFT, norm_multi=0, arctan=True, fixed_point=True, eps="device", tau=TAU, a_float=A_FLOAT):
    """eps: "device", "oracle", "both" (the larger) or a number.  arctan / fixed_point False: an implementation with a
    libm arctangent that sums floats -- the oracle.  a_float = 0 only to show that the float32 angle term is needed."""
    r = Rule()
    r.patch, r.norm_mode, r.norm_multi = p, norm_mode, norm_multi
    zero = np.zeros(128)
    r.terms = dict(A=zero, F=zero, P=zero, T=zero)
    r.h = r.sens = zero
    r.eps = 0.0
    if len(p.u):
        r.eps = {"device": eps_device(p), "oracle": eps_oracle(p), "both": max(eps_device(p), eps_oracle(p))}.get(eps, eps)
        ax, ay, dist = _hats(p)
        wx, wy, sh = np.clip(1.0 - ax, 0.0, None), np.clip(1.0 - ay, 0.0, None), np.clip(1.0 - dist, 0.0, None)
        win = np.exp(-(p.u * p.u + p.v * p.v) / 8.0) * p.mod          # samples beyond the square: hats of 0, P alone
        wm = win * p.inside
        r.h = _acc(wy, wx, sh, wm)
        touch = (dist < 1.0 + REACH).astype(np.float64)
        A = (a_float + (A_POLY if arctan else 0.0)) * _acc(wy, wx, touch, wm)
        F = zero
        if fixed_point:
            cx, cy, b0 = np.floor(p.u + 1.5)[:, None], np.floor(p.v + 1.5)[:, None], np.floor(p.t)[:, None]
            vx, vy = ((_K4 == cx) | (_K4 == cx + 1)).astype(np.float64), ((_K4 == cy) | (_K4 == cy + 1)).astype(np.float64)
            vb = ((_K8 == b0 % 8) | (_K8 == (b0 + 1) % 8)).astype(np.float64)
            F = 0.5 * 2.0 ** -p.fbits * _acc(vy, vx, vb, p.inside.astype(np.float64))
        sx, sy = (ax < 1.0 + REACH).astype(np.float64), (ay < 1.0 + REACH).astype(np.float64)
        r.sens = _acc(wy, sx, sh, win) + _acc(sy, wx, sh, win) + _acc(wy, wx, sh, win * (np.abs(p.u) + np.abs(p.v)) / 4.0)
        r.terms = dict(A=A, F=F, P=r.eps * r.sens, T=tau * r.h)
    r.delta = r.terms["A"] + r.terms["F"] + r.terms["P"] + r.terms["T"]
    r.out, r.lo, r.hi = interval(r.h, r.delta, norm_mode, norm_multi)
    return r


def analyse(plane, x, y, sigma, angle, norm_mode=ROOTSIFT, norm_multi=0, **kw):
    return evaluate(samples(plane, x, y, sigma, angle), norm_mode, norm_multi, **kw)


def emulate_device(plane, x, y, sigma, angle, rng):
    """A correct device in numpy: float32 positions formed as k_descriptor forms them, a uniform +-1.5e-5 bins of angle
    noise per sample, every (sample, cell) word half rounded to nearest at fbits.  -> the raw histogram."""
    p = samples(plane, x, y, sigma, angle, uv=uv_device)
    if len(p.u) == 0:
        return np.zeros(128)
    k = p.inside
    u, v, mod = p.u[k].astype(np.float32).astype(np.float64), p.v[k].astype(np.float32).astype(np.float64), p.mod[k]
    t = (p.t[k] + rng.uniform(-A_POLY, A_POLY, len(u))) % 8.0
    wm = np.exp(-(u * u + v * v) / 8.0) * mod * 2.0 ** p.fbits
    tu, tv = u + 1.5, v + 1.5
    cx, cy, b0 = np.floor(tu), np.floor(tv), np.floor(t)
    fx, fy, d = tu - cx, tv - cy, t - b0
    acc = np.zeros((6, 6, 8))                                   # cells -1 .. 4: the outer ring is dropped
    for oy, wy in ((0, 1.0 - fy), (1, fy)):
        for ox, wx in ((0, 1.0 - fx), (1, fx)):
            wgt = wy * wm * wx
            iy, ix = (cy + oy + 1).astype(np.int64), (cx + ox + 1).astype(np.int64)
            np.add.at(acc, (iy, ix, b0.astype(np.int64) % 8), np.rint((1.0 - d) * wgt))
            np.add.at(acc, (iy, ix, (b0.astype(np.int64) + 1) % 8), np.rint(d * wgt))
    return acc[1:5, 1:5].reshape(128) * 2.0 ** -p.fbits


def check(rule, descriptor):
    """-> the offenders of one descriptor (128 float32): element, cell, bin, value, expected, bound and the dominant term"""
    d = np.asarray(descriptor, np.float64).reshape(128)
    bad = []
    for i in np.nonzero(~((d >= rule.lo) & (d <= rule.hi)))[0]:
        terms = {k: float(v[i]) for k, v in rule.terms.items()}
        bad.append(dict(element=int(i), cell=(int(i) // 32, (int(i) // 8) % 4), bin=int(i) % 8, value=float(d[i]),
                        expected=float(rule.out[i]), lo=float(rule.lo[i]), hi=float(rule.hi[i]),
                        bound=float(max(rule.hi[i] - rule.out[i], rule.out[i] - rule.lo[i])), raw=float(rule.h[i]),
                        delta=float(rule.delta[i]), terms=terms, dominant=max(terms, key=terms.get)))
    return bad


def error_ratio(rule, descriptor, floor=0.0):
    """the largest |value - expected| / bound over the elements (at most 1 where `check` finds nothing); floor: only the
    elements expected at floor * 2^norm_multi or above -- a near-empty bin that the fixed point rounds to exactly 0 sits
    ON its bound, which says nothing about the rest"""
    d = np.asarray(descriptor, np.float64).reshape(128)
    bound = np.maximum(rule.hi - rule.out, rule.out - rule.lo)      # the "bound" of an offender's record
    with np.errstate(all="ignore"):
        ok = np.isfinite(bound) & (bound > 0) & (rule.out >= floor * 2.0 ** rule.norm_multi)
        q = np.where(ok, np.abs(d - rule.out) / bound, 0.0)
    return float(np.nanmax(q))


def offender_rows(bad, limit=8):
    return ["cell (%d, %d) bin %d: %.9g, expected %.9g in [%.9g, %.9g]: off by %.3g, bound %.3g; raw %.6g +- %.3g (%s), %s dominates" % (
        o["cell"][0], o["cell"][1], o["bin"], o["value"], o["expected"], o["lo"], o["hi"], abs(o["value"] - o["expected"]), o["bound"],
        o["raw"], o["delta"], ", ".join("%s %.2g" % kv for kv in o["terms"].items()), o["dominant"]) for o in bad[:limit]]


def format_offenders(rule, bad, name="", limit=8):
    p = rule.patch
    head = "%s(%.4f, %.4f) sigma %.4f angle %.7f, %s x 2^%d, %d samples in %d rows, fbits %d, eps %.2g: %d element(s) outside" % (
        name + " " if name else "", p.x, p.y, p.sigma, p.angle, "RootSift" if rule.norm_mode == ROOTSIFT else "classic",
        rule.norm_multi, p.n, p.rows if p.n else 0, p.fbits, rule.eps, len(bad))
    return head + "\n        " + "\n        ".join(offender_rows(bad, limit))
