"""The grid and interpolated descriptors of one (plane, x, y, sigma, angle) in float64, with a bound per output element
(no GPU): one rule per LATTICE, in the style of tests/desc_rule.py, whose normalize / interval / check / error_ratio /
Rule it uses unchanged and whose offender_rows its format_offenders shares.

    NOTILE  desc_mode 4 and 3 (igrid)  descriptor_notile_one / descriptor_igrid_one    k_descriptor_notile<false>
    ILOOP   desc_mode 1                descriptor_iloop_one                            k_descriptor_notile<true>
    GRID    desc_mode 2                descriptor_grid_one                             k_descriptor_grid

(the kernels: popsift_amd/csrc/desc_modes.hip).  These descriptors are step functions of their inputs (texture weights in steps of 1/256, samples snapped to pixels, an
inclusion test), but every step is a function of the POSITION alone, and kernel and oracle form the positions with the
same float32 operations (both are built with -ffp-contract=off).  So the rule needs no decision margins: `samples`
restates every integer or step decision in float32, operation by operation (numpy float32 arithmetic rounds every
operation; fmaf is a float64 product and sum rounded once), and everything continuous after them in float64.  (c, s) are
the float64 cosine and sine of the float32 angle rounded once to float32, the two floats of sincos_cr.

The lattices (SBP = |3 sigma| in float32; "read" = tex_linear: floor, fraction a -> floorf(a * 256 + 0.5) / 256, the four
clamped pixels, the bilinear sum in float64):

  NOTILE  1600 points (newx, newy), 0 .. 39: step = -2.5 + 1/16 + new / 8 (exact), pt = (c stepx - s stepy, c stepy +
          s stepx), p = (x, y) + pt * SBP.  Gradient g = (read(p + (c, s)) - read(p - (c, s)), read(p + (-s, c)) -
          read(p - (-s, c))), weight exp(-|step|^2 / 8) |g| (desc_gauss), t = atan2(g) 4 / pi mod 8, and for every
          cell cx with 8 cx <= newx <= 8 cx + 15 the tent desc_tile[newx - 8 cx] = 1 - |-1 + 1/16 + (newx - 8 cx) / 8|
          (the same in y).  igrid is the same lattice walked cell by cell.
  ILOOP   per cell (ix, iy) a 32 x 32 lattice d = -bsz + k * bsz / 16, bsz = |c| + |s|; n = (fma(c, dx, s dy),
          fma(c, dy, -s dx)); the points with |nx| < 1 and |ny| < 1 in float32; p = (x + ptx + dx SBP, y + pty + dy SBP)
          with pt = (fma(c SBP, offx, -s SBP offy), fma(c SBP, offy, s SBP offx)), off = (ix, iy) - 1.5; the rotated
          interpolated gradient of NOTILE; weight exp(-|n + off|^2 / 8) (1 - |nx|) (1 - |ny|) |g|; own 8 bins.
  GRID    per cell 16 x 16 points pixo = lft_dn + (xd + .5) rgt_stp + (yd + .5) up_stp, snapped: pix = roundf(pt + pixo
          SBP) - pt, pixel (int)(pt + pix) -- float -> int truncation -- central differences of POINT reads with clamp
          addressing, n = rotated pix / SBP, weight exp(-|n + off|^2 / 8) (1 - |nx|) (1 - |ny|) |g| where both tents
          are >= 0, t = (atan2(g) - angle) 4 / pi mod 8; own 8 bins.

Bin b of a cell receives weight * hat(circular distance of t and b): the (1 - d, d) pair of every implementation.

Each raw element carries delta = A + F + G + W + S + T, by how much a correct implementation may differ:

  A  arctangent.  e * sum of weight over the samples whose t lies within 1 + 1e-4 of b.  e = A_ACC = 2e-7 bins, the stated
     error of atan2_acc (keypoint_dev.h: "|error| ~ 1.5e-7 rad" = 1.9e-7 bins), a device-only term, plus desc_rule.A_FLOAT =
     1.5e-6 bins for float32 angle arithmetic on either side (th + 2 pi and th - angle rounded at up to 2 pi, t at up to
     8, rounded UP by the oracle's mul_up, atan2f itself), which stays on for the oracle.
  F  fixed point (device only; none for GRID, which sums floats).  k_descriptor_notile adds (unsigned)(share * weight *
     2^FBITS + 0.5) to one half of a 64-bit word per (sample, cell): half a unit of 2^-FBITS (14, iloop 13) per (sample,
     cell) whose t lies within 1 + 1e-4 of b.
  G  float32 rounding of the bilinear reads (NOTILE, ILOOP), an ABSOLUTE gradient error per sample.  (1 - a) is exact; the
     two products and the sum of a row, then the two products and the sum of the column, each round by at most 2^-24 of
     at most V, the largest of the four pixels in magnitude: 4 * 2^-24 V per read, so eg = 4 * 2^-24 sqrt((V1 + V2)^2 +
     (V3 + V4)^2) on the gradient vector.  It moves the magnitude by eg and the direction by asin(eg / |g|) 4 / pi bins
     (any direction where eg >= |g| / 2: a flat saturated patch has |g| = 0 in float64 and rounding noise in float32):
         G[b] = sum over the samples whose t lies within 1 + e_t + 1e-4 of b of  lattice weight * (eg + min(|g| e_t, |g|)).
     The rounding of the difference of two reads is relative and belongs to T.
  W  the tents 1 - |nx|, 1 - |ny| of ILOOP and GRID are float32 differences: 2^-24 absolute each, however small the tent:
     2^-23 * sum of exp(..) |g| over the samples whose t lies within 1 + 1e-4 of b.  None for NOTILE (desc_tile is exact).
  S  summation.  The oracle sums floats: NOTILE 32 additions per lane and 3 in the tree, round to nearest: 35 * 2^-24 h;
     ILOOP 32 + 1 + 5 and GRID 16 + 1 + 4 additions that fma_up rounds UP: 38 resp. 21 * 2^-23 h.  k_descriptor_grid adds
     4 x 2 per lane and 6 in the butterfly, fewer than the oracle; the fixed-point kernels add integers.
  T  TAU * h, TAU = 1e-5: float32 products, the difference of two reads, the hardware exp2 and sqrt.  The TAU of
     tests/ori_rule.py and tests/desc_rule.py; it is not a knob.

There is no position term: the positions are the oracle's bit for bit, and the weights are functions of them.
delta goes through both normalisations by desc_rule.interval.  `check` has no allowance.
"""
import numpy as np

import desc_rule
from desc_rule import A_FLOAT, CLASSIC, REACH, ROOTSIFT, TAU, Rule, check, error_ratio, interval, normalize  # noqa: F401

NOTILE, ILOOP, GRID = "notile", "iloop", "grid"
DESC_MODE = {"iloop": 1, "grid": 2, "igrid": 3, "notile": 4}          # POPSIFT_HIP_DESC_*
LATTICE = {"iloop": ILOOP, "grid": GRID, "igrid": NOTILE, "notile": NOTILE}
FBITS = {NOTILE: 14, ILOOP: 13, GRID: None}
A_ACC = 2e-7
SUM_ROUNDINGS = {NOTILE: 35 * 2.0 ** -24, ILOOP: 38 * 2.0 ** -23, GRID: 21 * 2.0 ** -23}
U24 = 2.0 ** -24
DESC_MAGNIFY = np.float32(3.0)
_K4, _K8 = np.arange(4.0), np.arange(8.0)
f32, f64 = np.float32, np.float64


def _fma(a, b, c):
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def tex_linear(plane, X, Y, q=256.0, skip_outside=False, reads32=False):
    """tex_linear of kernel and oracle at the float32 positions X, Y -> (value, largest |pixel| of the four).  q: the
    steps of the weights (128 is a doctored one); skip_outside: a read that needs a clamp returns 0 (doctored);
    reads32: the bilinear sum in float32, as every implementation forms it."""
    h, w = plane.shape
    fx, fy = np.floor(X), np.floor(Y)
    a, b = X - fx, Y - fy
    a = np.floor(a * f32(q) + f32(0.5)) * f32(1.0 / q)
    b = np.floor(b * f32(q) + f32(0.5)) * f32(1.0 / q)
    i, j = fx.astype(np.int64), fy.astype(np.int64)
    x0, x1, y0, y1 = np.clip(i, 0, w - 1), np.clip(i + 1, 0, w - 1), np.clip(j, 0, h - 1), np.clip(j + 1, 0, h - 1)
    t00, t10, t01, t11 = plane[y0, x0], plane[y0, x1], plane[y1, x0], plane[y1, x1]
    big = np.maximum(np.maximum(np.abs(t00), np.abs(t10)), np.maximum(np.abs(t01), np.abs(t11))).astype(f64)
    if reads32:
        one = f32(1.0)
        val = ((one - b) * ((one - a) * t00 + a * t10) + b * ((one - a) * t01 + a * t11)).astype(f64)
    else:
        a, b = a.astype(f64), b.astype(f64)
        t00, t10, t01, t11 = (t.astype(f64) for t in (t00, t10, t01, t11))
        val = (1.0 - b) * ((1.0 - a) * t00 + a * t10) + b * ((1.0 - a) * t01 + a * t11)
    if skip_outside:
        val = np.where((i < 0) | (i + 1 > w - 1) | (j < 0) | (j + 1 > h - 1), 0.0, val)
    return val, big


class Samples:
    """The lattice points of one descriptor (arrays over the points) and what `evaluate` needs of its frame.
    fy, fx: (n, 4) weights over the cell rows / columns, their product is the point's weight in cell (iy, ix);
    g: the Gaussian; gx, gy: the gradient; eg: its absolute error; t: the bin coordinate."""
    __slots__ = ("lattice", "x", "y", "sigma", "angle", "w", "h", "cs", "sbp", "fbits", "fy", "fx", "g", "gx", "gy", "mod",
                 "t", "eg", "col", "cell", "px", "py")

    @property
    def n(self):
        return len(self.g)


def _rot_gradient(plane, px, py, c, s, **kw):
    r = [tex_linear(plane, px + dx, py + dy, **kw) for dx, dy in ((c, s), (-c, -s), (-s, c), (s, -c))]
    gx, gy = r[0][0] - r[1][0], r[2][0] - r[3][0]
    eg = 4.0 * U24 * np.hypot(r[0][1] + r[1][1], r[2][1] + r[3][1])
    return gx, gy, eg


def samples(lattice, plane, x, y, sigma, angle, tent_shift=0, **tex):
    """tent_shift: the index of the tent weights moved by one (a doctored implementation); tex: see tex_linear."""
    h, w = plane.shape
    p = Samples()
    p.lattice, p.w, p.h = lattice, w, h
    x, y, sigma, angle = f32(x), f32(y), f32(sigma), f32(angle)
    p.x, p.y, p.sigma, p.angle = float(x), float(y), float(sigma), float(angle)
    c, s = f32(np.cos(f64(angle))), f32(np.sin(f64(angle)))
    p.cs = (float(c), float(s))
    sbp = np.abs(DESC_MAGNIFY * sigma)
    p.sbp, p.fbits = float(sbp), FBITS[lattice]
    if not sbp > 0:
        p.fy = p.fx = np.zeros((0, 4))
        p.g = p.gx = p.gy = p.mod = p.t = p.eg = p.px = p.py = np.zeros(0)
        p.col = p.cell = np.zeros(0, np.int64)
        return p
    one = f32(1.0)
    if lattice == NOTILE:
        new = np.arange(40)
        newy, newx = (v.reshape(-1) for v in np.meshgrid(new, new, indexing="ij"))
        stepbase = f32(-2.5) + f32(1.0 / 16.0)
        stepx, stepy = stepbase + f32(0.125) * newx.astype(f32), stepbase + f32(0.125) * newy.astype(f32)
        ptx, pty = c * stepx + -s * stepy, c * stepy + s * stepx
        px, py = x + ptx * sbp, y + pty * sbp
        tent = lambda n: np.where((n[:, None] - 8 * _K4 >= 0) & (n[:, None] - 8 * _K4 <= 15),
                                  1.0 - np.abs(-1.0 + 1.0 / 16.0 + 0.125 * (n[:, None] - 8 * _K4 + tent_shift)), 0.0)
        p.fy, p.fx = np.clip(tent(newy), 0.0, None), np.clip(tent(newx), 0.0, None)
        p.g = np.exp(-(stepx.astype(f64) ** 2 + stepy.astype(f64) ** 2) / 8.0)
        p.col, p.cell = newx, np.full(1600, -1)
        p.gx, p.gy, p.eg = _rot_gradient(plane, px, py, c, s, **tex)
        t_off = 0.0
    else:
        cell = np.repeat(np.arange(16), 1024 if lattice == ILOOP else 256)
        ix, iy = cell & 3, cell >> 2
        offx, offy = ix.astype(f32) - f32(1.5), iy.astype(f32) - f32(1.5)
        csbp, ssbp = c * sbp, s * sbp
        if lattice == ILOOP:
            k = np.arange(32)
            i, j = (np.tile(v.reshape(-1), 16) for v in np.meshgrid(k, k, indexing="ij"))
            bsz = np.abs(c) + np.abs(s)
            dx, dy = -bsz + j.astype(f32) * bsz / f32(16.0), -bsz + i.astype(f32) * bsz / f32(16.0)
            nx, ny = _fma(c, dx, s * dy), _fma(c, dy, -s * dx)
            ptx, pty = _fma(csbp, offx, -ssbp * offy), _fma(csbp, offy, ssbp * offx)
            px, py = x + ptx + dx * sbp, y + pty + dy * sbp
            keep = (np.abs(nx) < one) & (np.abs(ny) < one)
            p.col = j
            t_off = 0.0
        else:
            k = np.arange(16)
            yd, xd = (np.tile(v.reshape(-1), 16) for v in np.meshgrid(k, k, indexing="ij"))
            ptx, pty = _fma(csbp, offx, _fma(-ssbp, offy, x)), _fma(csbp, offy, _fma(ssbp, offx, y))
            ldx, ldy = -c + s, -c - s
            rsx, rsy, usx, usy = c / f32(8.0), s / f32(8.0), -s / f32(8.0), c / f32(8.0)
            xh, yh = xd.astype(f32) + f32(0.5), yd.astype(f32) + f32(0.5)
            pixox, pixoy = ldx + xh * rsx + yh * usx, ldy + xh * rsy + yh * usy
            pixx, pixy = pixox * sbp, pixoy * sbp
            def rnd(v):                                 # roundf: halves away from zero; v - trunc(v) is exact
                tr = np.trunc(v)
                return tr + np.where(np.abs(v - tr) >= f32(0.5), np.copysign(one, v), f32(0.0))
            pixx, pixy = rnd(ptx + pixx) - ptx, rnd(pty + pixy) - pty
            pixox, pixoy = pixx / sbp, pixy / sbp
            px, py = ptx + pixx, pty + pixy
            nx, ny = _fma(c, pixox, s * pixoy), _fma(c, pixoy, -s * pixox)
            keep = ~((one - np.abs(nx) < 0) | (one - np.abs(ny) < 0))
            p.col = xd
            t_off = float(angle)
        wx, wy = (one - np.abs(nx)).astype(f64), (one - np.abs(ny)).astype(f64)       # float32 differences, as everywhere
        dnx, dny = (nx + offx).astype(f64), (ny + offy).astype(f64)
        k = np.nonzero(keep)[0]
        px, py, cell, ix, iy, p.col = px[k], py[k], cell[k], ix[k], iy[k], p.col[k]
        p.cell = cell
        p.fy, p.fx = (iy[:, None] == _K4) * wy[k, None], (ix[:, None] == _K4) * wx[k, None]
        if tent_shift:                                  # the tents of the lattice neighbour
            p.fy = np.where(iy[:, None] == _K4, np.roll(wy[k], tent_shift)[:, None], 0.0)
            p.fx = np.where(ix[:, None] == _K4, np.roll(wx[k], tent_shift)[:, None], 0.0)
        p.g = np.exp(-(dnx[k] ** 2 + dny[k] ** 2) / 8.0)
        if lattice == ILOOP:
            p.gx, p.gy, p.eg = _rot_gradient(plane, px, py, c, s, **tex)
        else:
            gx, gy = px.astype(np.int64), py.astype(np.int64)                         # (int): truncation
            skip = tex.get("skip_outside", False)
            P = plane.astype(f64)
            rd = lambda xx, yy: np.where(skip & ((xx < 0) | (xx > w - 1) | (yy < 0) | (yy > h - 1)), 0.0,
                                         P[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)])
            p.gx, p.gy = rd(gx + 1, gy) - rd(gx - 1, gy), rd(gx, gy + 1) - rd(gx, gy - 1)
            p.eg = np.zeros(len(k))
    p.px, p.py = np.asarray(px, f64), np.asarray(py, f64)
    p.mod = np.hypot(p.gx, p.gy)
    p.t = ((np.arctan2(p.gy, p.gx) - t_off) * (4.0 / np.pi)) % 8.0
    return p


def _dist(t):
    return np.abs((t[:, None] - _K8 + 4.0) % 8.0 - 4.0)


def _acc(p, fy, fx, fb, wgt):
    """desc_rule._acc; a point of ILOOP and GRID has one cell and the points are in the order of their cells, so there
    it is one sum per run of points"""
    if p.lattice == NOTILE:
        return desc_rule._acc(fy, fx, fb, wgt)
    count = np.bincount(p.cell, minlength=16)
    start = np.cumsum(count) - count
    out = np.zeros((16, 8))
    out[count > 0] = np.add.reduceat((fy.sum(1) * fx.sum(1) * wgt)[:, None] * fb, start[count > 0], axis=0)
    return out.reshape(128)


def raw_histogram(p, mult=None, t_shift=0.0):
    """The raw histogram alone.  mult: a factor per point (0 drops it); t_shift: added to every t (doctored)."""
    if p.n == 0:
        return np.zeros(128)
    wm = p.g * p.mod if mult is None else p.g * p.mod * mult
    return _acc(p, p.fy, p.fx, np.clip(1.0 - _dist((p.t + t_shift) % 8.0), 0.0, None), wm)


def evaluate(p, norm_mode=ROOTSIFT, norm_multi=0, device=True, tau=TAU):
    """device False: an implementation with a libm arctangent that sums floats -- the oracle: A_ACC and F off."""
    r = Rule()
    r.patch, r.norm_mode, r.norm_multi, r.eps = p, norm_mode, norm_multi, 0.0
    zero = np.zeros(128)
    r.terms = dict(A=zero, F=zero, G=zero, W=zero, S=zero, T=zero)
    r.h = r.sens = zero
    if p.n:
        dist = _dist(p.t)
        sh = np.clip(1.0 - dist, 0.0, None)
        touch = (dist < 1.0 + REACH).astype(f64)
        wm = p.g * p.mod
        r.h = _acc(p, p.fy, p.fx, sh, wm)
        A = (A_FLOAT + (A_ACC if device else 0.0)) * _acc(p, p.fy, p.fx, touch, wm)
        F = W = G = zero
        ay, ax = (p.fy > 0).astype(f64), (p.fx > 0).astype(f64)
        if device and p.fbits is not None:
            F = 0.5 * 2.0 ** -p.fbits * _acc(p, ay, ax, touch, np.ones(p.n))
        if p.lattice != NOTILE:
            W = 2.0 ** -23 * _acc(p, ay, ax, touch, wm)
        if p.eg.any():
            with np.errstate(all="ignore"):
                e_t = np.where(p.eg < 0.5 * p.mod, np.arcsin(np.minimum(p.eg / p.mod, 0.5)) * (4.0 / np.pi), 8.0)
            reach = (dist < 1.0 + REACH + e_t[:, None]).astype(f64)
            G = _acc(p, p.fy, p.fx, reach, p.g * (p.eg + np.minimum(p.mod * e_t, p.mod)))
        r.terms = dict(A=A, F=F, G=G, W=W, S=SUM_ROUNDINGS[p.lattice] * r.h, T=tau * r.h)
    r.delta = sum(r.terms.values())
    r.out, r.lo, r.hi = interval(r.h, r.delta, norm_mode, norm_multi)
    return r


def analyse(lattice, plane, x, y, sigma, angle, norm_mode=ROOTSIFT, norm_multi=0, **kw):
    return evaluate(samples(lattice, plane, x, y, sigma, angle), norm_mode, norm_multi, **kw)


def low_half_peak(p):
    """The largest sum a low word half of k_descriptor_notile can reach on this descriptor, as a fraction of 2^32: the
    shares (1 - d) * weight * 2^FBITS of the points whose floor(t) is the word's bin, summed per cell (the two LDS copies
    taken together, so an upper bound of either)."""
    if p.n == 0 or p.fbits is None:
        return 0.0
    b0 = np.floor(p.t) % 8
    own = (b0[:, None] == _K8) * (1.0 - (p.t - np.floor(p.t)))[:, None]
    return float(_acc(p, p.fy, p.fx, own, p.g * p.mod).max() * 2.0 ** p.fbits / 2.0 ** 32)


def emulate_device(lattice, plane, x, y, sigma, angle, rng, truncate=False):
    """A correct device in numpy: gradients from float32 bilinear reads, a uniform +-A_ACC bins of angle noise per point,
    every (point, cell) word half rounded to nearest at FBITS (truncate: cut off instead, a doctored one); GRID: float32
    weights summed in float32.  -> the raw histogram."""
    p = samples(lattice, plane, x, y, sigma, angle, reads32=True)
    if p.n == 0:
        return np.zeros(128)
    t = (p.t + rng.uniform(-A_ACC, A_ACC, p.n)) % 8.0
    b0 = np.floor(t).astype(np.int64) % 8
    d = t - np.floor(t)
    if lattice == GRID:
        wgt = (p.g.astype(f32) * p.fx.sum(1).astype(f32) * p.fy.sum(1).astype(f32) * p.mod.astype(f32))
        acc = np.zeros((16, 8), f32)
        np.add.at(acc, (p.cell, b0), (wgt - d.astype(f32) * wgt))
        np.add.at(acc, (p.cell, (b0 + 1) % 8), d.astype(f32) * wgt)
        return acc.reshape(128).astype(f64)
    scale = 2.0 ** p.fbits
    fix = (lambda v: np.floor(v)) if truncate else (lambda v: np.floor(v + 0.5))
    acc = np.zeros((4, 4, 8))
    wm = (p.g * p.mod * scale).astype(f32).astype(f64)
    for iy in range(4):
        for ix in range(4):
            wgt = p.fy[:, iy] * p.fx[:, ix]
            k = np.nonzero(wgt > 0)[0]
            a1 = d[k] * wm[k]
            a0 = wm[k] - a1
            np.add.at(acc[iy, ix], b0[k], fix(a0 * wgt[k]))
            np.add.at(acc[iy, ix], (b0[k] + 1) % 8, fix(a1 * wgt[k]))
    return acc.reshape(128) / scale


def format_offenders(rule, bad, name="", limit=8):
    p = rule.patch
    head = "%s%s (%.4f, %.4f) sigma %.4f angle %.7f, %s x 2^%d, %d points: %d element(s) outside" % (
        name + " " if name else "", p.lattice, p.x, p.y, p.sigma, p.angle, "RootSift" if rule.norm_mode == ROOTSIFT else "classic",
        rule.norm_multi, p.n, len(bad))
    return head + "\n        " + "\n        ".join(desc_rule.offender_rows(bad, limit))
