"""half_angle_bins (keypoint.hip), the arctangent of k_descriptor and k_orientation, restated in float32 numpy (no GPU).

    d  = (|gx| + 1e-18f) + |g|               |g| = v_sqrt(fma(gx, gx, gy * gy)), which the kernels have for the weight
    t  = gy * v_rcp(d)                       tan(theta' / 2), theta' = the angle of (|gx|, gy)
    th = t * P(t * t)                        (8 / pi) atan(t): theta' in bins of pi / 4
    fma(th, sg, fma(-2, sg, k0))             sg = copysign(scale, gx): gx < 0 mirrors, theta = 4 - theta'

v_sqrt and v_rcp are good to one ulp, so the emulated root and reciprocal are moved by -1, 0 or +1 ulp at random.  The
result must lie within desc_rule.A_POLY of the float64 arctan2 (the device rule tests of k_descriptor rest on that
constant), and 4.5 times the error -- k_orientation's 36 bins -- within half of the 1e-4 band next to a bin edge inside
which k_orientation asks the accurate arctangent instead.  Those bounds are for gradients of 1e-6 and more; below that a
sample's weight is zero in the kernels' fixed point and the angle only has to stay finite and in range, which is checked
down to the smallest denormal: the squares of a gradient below 1.1e-19 underflow, so |g| comes out as 0 where gy is not."""
import os
import re

import numpy as np

import desc_rule

f32, f64 = np.float32, np.float64
COEFFS = ("-0.02984253503382206", "0.13406537473201752", "-0.2964776158332825", "0.4928465187549591", "-0.8470170497894287",
          "2.5464210510253906")
KEYPOINT_HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "popsift_amd", "csrc", "keypoint.hip")


def _fma(a, b, c):
    """a double product plus a double sum rounded once: the FMA up to double rounding"""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def _nudge(v, rng):
    """-1, 0 or +1 ulp at random"""
    k = rng.integers(-1, 2, v.shape)
    up, down = np.nextafter(v, f32(np.inf)), np.nextafter(v, f32(-np.inf))
    return np.where(k > 0, up, np.where(k < 0, down, v)).astype(f32)


def _ftz(v):
    return np.where(np.abs(v) < np.finfo(f32).tiny, f32(0.0), v).astype(f32)


def half_angle_bins(gy, gx, rng, scale=1.0, k0=2.0, flush=False):
    """flush: denormal products, sums and roots count as zero (either setting of the device must be harmless)"""
    gy, gx = np.asarray(gy, f32), np.asarray(gx, f32)
    sq = _fma(gx, gx, _ftz(gy * gy) if flush else gy * gy)
    root = np.sqrt((_ftz(sq) if flush else sq).astype(f64)).astype(f32)
    mod = np.where(root == 0, root, _nudge(root, rng)).astype(f32)          # an exact zero stays zero
    d = (np.abs(gx) + f32(1e-18)) + mod
    t = gy * _nudge((1.0 / d.astype(f64)).astype(f32), rng)
    s = t * t
    p = _fma(f32(COEFFS[0]), s, f32(COEFFS[1]))
    for c in COEFFS[2:]:
        p = _fma(p, s, f32(c))
    th = t * p
    sg = np.copysign(f32(scale), gx)
    return _fma(th, sg, _fma(f32(-2.0), sg, f32(k0)))


def gradients(rng, n=1 << 20):
    """(gy, gx) float32: random directions over magnitudes 1e-6 .. 300, then the special ones"""
    mag = 10.0 ** rng.uniform(-6.0, np.log10(300.0), n)
    phi = rng.uniform(-np.pi, np.pi, n)
    gy, gx = [(mag * np.sin(phi)).astype(f32)], [(mag * np.cos(phi)).astype(f32)]
    m = (10.0 ** rng.uniform(-6.0, np.log10(300.0), 1 << 14)).astype(f32)
    zero, nzero = np.zeros_like(m), -np.zeros_like(m)
    tiny = (m.astype(f64) * 1e-6).astype(f32)
    for y, x in ((m, zero), (-m, zero), (m, nzero), (-m, nzero),              # gx = +-0
                 (zero, m), (nzero, m), (zero, -m), (nzero, -m),              # gy = +-0
                 (m, m), (m, -m), (-m, m), (-m, -m),                          # exact diagonals
                 (tiny, -m), (-tiny, -m), (tiny, m), (-tiny, m)):             # next to the axis, both sides of the cut
        gy.append(y)
        gx.append(x)
    return np.concatenate(gy), np.concatenate(gx)


def test_coefficients_are_the_kernels():
    with open(KEYPOINT_HIP) as f:
        text = f.read()
    body = text[text.index("float half_angle_bins("):]
    body = body[:body.index("\n}\n")]
    assert re.findall(r"(-?\d\.\d+)f(?=[,)])", body)[:6] == list(COEFFS), body
    assert "1e-18f" in body and "__builtin_amdgcn_rcpf" in body and "copysignf(scale, x)" in body


def test_error_against_float64_arctan2():
    rng = np.random.Generator(np.random.PCG64(2))
    gy, gx = gradients(rng)
    assert len(gx) >= 1000000
    got = half_angle_bins(gy, gx, rng).astype(f64)
    want = np.arctan2(gy.astype(f64), gx.astype(f64)) * 4.0 / np.pi
    err = np.abs((got - want + 4.0) % 8.0 - 4.0)
    worst = int(err.argmax())
    print("half_angle_bins: max error %.3g bins at (gy, gx) = (%.9g, %.9g) over %d gradients; in k_orientation's bins %.3g"
          % (err[worst], gy[worst], gx[worst], len(gx), 4.5 * err[worst]))
    assert np.isfinite(got).all() and got.min() >= -2.0 - 1e-5 and got.max() <= 6.0 + 1e-5
    assert err.max() <= desc_rule.A_POLY
    assert 4.5 * err.max() <= 0.5e-4


def test_orientation_scale_and_offset():
    """k_orientation's call: scale 4.5, k0 = 27 -> 4.5 theta + 18 in [9, 45], the 36-bin coordinate up to a multiple of 36"""
    rng = np.random.Generator(np.random.PCG64(3))
    gy, gx = gradients(rng, 1 << 16)
    got = half_angle_bins(gy, gx, rng, 4.5, 27.0).astype(f64)
    want = np.arctan2(gy.astype(f64), gx.astype(f64)) * 18.0 / np.pi + 18.0
    err = np.abs((got - want + 18.0) % 36.0 - 18.0)
    print("half_angle_bins(4.5, 27): max error %.3g of 36 bins, range %.6g .. %.6g" % (err.max(), got.min(), got.max()))
    assert got.min() >= 9.0 - 1e-4 and got.max() <= 45.0 + 1e-4        # k_orientation's histogram has bins 0 .. 45
    assert err.max() <= 0.5e-4


def test_zero_gradient_is_finite():
    rng = np.random.Generator(np.random.PCG64(4))
    z = np.array([0.0, -0.0, 0.0, -0.0], f32), np.array([0.0, 0.0, -0.0, -0.0], f32)
    got = half_angle_bins(*z, rng)
    assert np.isfinite(got).all() and got[0] == 0.0, got
    assert np.isfinite(half_angle_bins(*z, rng, 4.5, 27.0)).all()


def test_underflowing_gradients_stay_in_range():
    """|g| from the smallest denormal to 1e-6, where gx * gx + gy * gy loses bits or underflows to 0 (flushed to zero or
    not): |t| stays at most 1 + 1e-2, so the polynomial cannot overflow and no NaN reaches a histogram word"""
    rng = np.random.Generator(np.random.PCG64(5))
    n = 1 << 18
    mag = 10.0 ** rng.uniform(-45.0, -6.0, n)
    phi = rng.uniform(-np.pi, np.pi, n)
    gy, gx = (mag * np.sin(phi)).astype(f32), (mag * np.cos(phi)).astype(f32)
    gy = np.concatenate([gy, mag.astype(f32), -mag.astype(f32), np.zeros(n, f32)])
    gx = np.concatenate([gx, np.zeros(n, f32), -np.zeros(n, f32), -mag.astype(f32)])
    for flush in (False, True):                      # with and without denormal support in the squares and the root
        with np.errstate(under="ignore"):
            got = half_angle_bins(gy, gx, rng, flush=flush)
            got36 = half_angle_bins(gy, gx, rng, 4.5, 27.0, flush=flush)
        assert np.isfinite(got).all() and got.min() >= -2.05 and got.max() <= 6.05, (flush, got.min(), got.max())
        assert np.isfinite(got36).all() and got36.min() >= 8.8 and got36.max() <= 45.2, (flush, got36.min(), got36.max())
