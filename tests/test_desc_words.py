"""k_descriptor's histogram words and cell addresses read from the bits of f32 denormals (keypoint.hip), restated in
float32 numpy against exact integer arithmetic (no GPU).

For an integer 0 <= n < 2^24 the float32 n * 2^-149 has the bit pattern n.  The kernel scales the bin shares by 2^-100
and the column weights by 2^-49, so that a word is the bits of ONE product, rounded by the multiplier to the nearest
integer, ties to even -- what  bits(fma(w, wgt, 2^23)) & 0x7fffff  gave before (the FMA is the exact w * wgt + 2^23
rounded once, in a binade whose step is 1: round_half_even(w * wgt) for a product below 2^23).  The scales and the slot
bias are read out of keypoint.hip, so the test is about the kernel's constants.

The words: (do0, fx, fy, wm) -> the eight words of a sample, old chain / new chain / exact rationals, over the special
fractions 0, the smallest denormal, 2^-30, 2^-26 and 1 - 2^-24, random ones, gradient magnitudes from 1e-30 to 2 under
window weights down to exp(-12.5 / 8), fbits 2 .. 14, and the largest sample make_desc_rec allows (361 * 2^14); the new
chain alone against the rationals up to 2^24.  The addresses: every (cx0, cy0, bin, copy) against the integer formula."""
import math
import os
import re

import numpy as np

f32, f64, i64 = np.float32, np.float64, np.int64
KEYPOINT_HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "popsift_amd", "csrc", "keypoint.hip")
HEX = r"(0x1p-\d+)f"


def _one(pattern, text):
    m = re.findall(pattern, text)
    assert len(m) == 1, (pattern, m)
    return m[0]


def constants():
    with open(KEYPOINT_HIP) as f:
        text = f.read()
    c = {}
    w = _one(r"const float w0 = fmaf\(-do0, %s, %s\), do0s = do0 \* %s;" % (HEX, HEX, HEX), text)
    x = _one(r"const float wx0 = fmaf\(-fx, %s, %s\), fxs = fx \* %s;" % (HEX, HEX, HEX), text)
    assert len(set(w)) == 1 and len(set(x)) == 1, (w, x)
    c["bin_scale"], c["col_scale"] = float.fromhex(w[0]), float.fromhex(x[0])
    c["s0"] = tuple(float.fromhex(v) for v in _one(
        r"s0 = __float_as_uint\(fmaf\(fcx, %s, fmaf\(ffo, %s, cpy8f\)\)\) & 56u;" % (HEX, HEX), text))
    c["cb"] = tuple(float.fromhex(v) for v in _one(
        r"cb = __float_as_uint\(fmaf\(fcy, \(float\)\(DESC_RS \* 8\) \* %s, fmaf\(fcx, %s, hbasef\)\)\);" % (HEX, HEX), text))
    c["hbase_scale"] = float.fromhex(_one(r"hbasef = \(float\)\(unsigned int\)\(size_t\)\(lds_fix64\*\)\(hall \+ cpy \* DESC_CS\) \* %s;" % HEX, text))
    c["cpy_scale"] = float.fromhex(_one(r"cpy8f = \(float\)\(\(cpy << 3\) \+ DESC_SLOT_BIAS\) \* %s;" % HEX, text))
    c["bias"] = int(_one(r"constexpr int DESC_SLOT_BIAS = (\d+);", text))
    c["rs"] = int(_one(r"constexpr int DESC_RS = (\d+);", text))
    c["copies"] = int(_one(r"#define DESC_NCOPY (\d+)", text))
    c["ang_limit"] = float(_one(r"if \(!\(fabsf\(r\.ang_bins\) <= (\d+\.\d+)f\)\) r\.ang_bins = \(float\)remainder\(", text))
    assert "lo = __float_as_uint(w0 * wgt);" in text and "hi = __float_as_uint(do0s * wgt);" in text
    assert text.count("wy0 * fxs") == 1 and text.count("wy1 * fxs") == 1 and "wy0 * fx)" not in text and "wy1 * fx)" not in text
    return c


C = constants()
GRID = 2.0 ** -149


def _fma(a, b, c):
    """fma(a, b, c) for the chains below.  The double product is exact; the double sum is exact or, where c = 1 and the
    product is below 2^-30, so close to 1 that both roundings give 1 -- the float32 result is the FMA's."""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def _mant_exp(v):
    """float32 >= 0 -> (m, e) int64 with v = m * 2^e exactly, m < 2^24"""
    m, e = np.frexp(np.asarray(v, f64))
    return np.round(m * 2.0 ** 24).astype(i64), e.astype(i64) - 24


def exact_word(w, wgt):
    """round_half_even(w * wgt) of two float32 >= 0 in integer arithmetic (the product of the mantissas has 48 bits)"""
    (mw, ew), (mg, eg) = _mant_exp(w), _mant_exp(wgt)
    m, e = mw * mg, ew + eg
    assert (e <= 0).all()                                   # w <= 1 and wgt < 2^24
    s = np.minimum(-e, 62)                                  # m < 2^48: a shift of 50 and more leaves less than 1/4
    q, r, half = m >> s, m & ((i64(1) << s) - 1), (i64(1) << s) >> 1
    return q + (((r > half) | ((r == half) & (s > 0) & ((q & 1) == 1)))).astype(i64)


def old_chain(do0, fx, fy, wm):
    """the parent's weights; its words are fma(w, wgt, 2^23) & 0x7fffff = round_half_even(w * wgt) below 2^23"""
    wx0, wy0, wy1 = f32(1.0) - fx, (f32(1.0) - fy) * wm, fy * wm
    w0 = f32(1.0) - do0
    cells = (wy0 * wx0, wy0 * fx, wy1 * wx0, wy1 * fx)
    return [(w0, g) for g in cells] + [(do0, g) for g in cells]


def new_words(do0, fx, fy, wm):
    """the kernel's chain in float32 (the host's multiplier rounds denormal results as the device's does)"""
    bs, cs = f32(C["bin_scale"]), f32(C["col_scale"])
    wy0, wy1 = (f32(1.0) - fy) * wm, fy * wm
    wx0, fxs = _fma(-fx, cs, cs), fx * cs
    w0, do0s = _fma(-do0, bs, bs), do0 * bs
    cells = (wy0 * wx0, wy0 * fxs, wy1 * wx0, wy1 * fxs)
    return [(w0 * g).view(np.uint32).astype(i64) for g in cells] + [(do0s * g).view(np.uint32).astype(i64) for g in cells]


SPECIAL = np.array([0.0, 2.0 ** -149, 2.0 ** -30, 2.0 ** -26, 1.0 - 2.0 ** -24], f32)


def inputs(rng):
    """(do0, fx, fy, wm): the special fractions in every combination and random ones, times window weight x magnitude x
    2^fbits; then the largest sample of make_desc_rec (|g| = 361, window weight 1, fbits 14) with every fraction"""
    n_rand = 20
    frac = np.concatenate([SPECIAL, rng.uniform(0.0, 1.0, n_rand).astype(f32), (10.0 ** rng.uniform(-9.0, 0.0, 8)).astype(f32)])
    do0, fx, fy = (a.ravel() for a in np.meshgrid(frac, frac[:9], frac[5:15], indexing="ij"))
    sp = np.stack([a.ravel() for a in np.meshgrid(SPECIAL, SPECIAL, SPECIAL, indexing="ij")])
    do0, fx, fy = np.concatenate([do0, sp[0]]), np.concatenate([fx, sp[1]]), np.concatenate([fy, sp[2]])
    mags = np.concatenate([10.0 ** np.linspace(-30.0, np.log10(2.0), 9), [361.0]])
    out = []
    for fbits in range(2, 15):
        for mag in mags:
            win = np.exp(-rng.uniform(0.0, 12.5, len(do0)) / 8.0)
            out.append((do0, fx, fy, (win * mag * 2.0 ** fbits).astype(f32)))
    big = f32(361.0 * 2.0 ** 14)
    out.append((do0, fx, fy, np.full(len(do0), big, f32)))
    return [np.concatenate(a) for a in zip(*out)]


def test_host_keeps_denormals():
    assert f32(2.0 ** -140) * f32(0.5) != 0 and (f32(3.0) * f32(GRID)).view(np.uint32) == 3


def test_constants():
    assert C["bin_scale"] * C["col_scale"] == GRID                      # a product's unit is the grid's step
    # a scaled fraction of 2^-26 and more is a normal float; below that its word is 0 either way
    assert C["bin_scale"] * 2.0 ** -26 >= 2.0 ** -126 and C["col_scale"] * 2.0 ** -26 >= 2.0 ** -126
    assert C["s0"] == (32 * GRID, 8 * GRID) and C["cb"] == (GRID, 64 * GRID)
    assert C["hbase_scale"] == GRID and C["cpy_scale"] == GRID
    assert C["bias"] % 64 == 0


def test_words_equal_exact_rounding():
    rng = np.random.Generator(np.random.PCG64(11))
    do0, fx, fy, wm = inputs(rng)
    assert len(do0) >= 400000
    new = new_words(do0, fx, fy, wm)
    old = old_chain(do0, fx, fy, wm)
    n, largest = 0, 0
    for k, ((w, g), got) in enumerate(zip(old, new)):
        want = exact_word(w, g)
        assert want.max() < 1 << 23                                     # the old trick's own bound: make_desc_rec's fbits
        bad = np.nonzero(want != got)[0]
        assert len(bad) == 0, "word %d: %d of %d differ, first at do0 %r fx %r fy %r wm %r: exact %d, kernel %d" % (
            k, len(bad), len(got), do0[bad[0]], fx[bad[0]], fy[bad[0]], wm[bad[0]], want[bad[0]], got[bad[0]])
        n, largest = n + len(got), max(largest, int(want.max()))
    print("%d words equal to the exactly rounded products, largest %d = 361 * 2^14 (%s)" % (n, largest, largest == 361 << 14))
    assert largest == 361 << 14


def test_words_up_to_2_24():
    """the new form's own bound: below 2^24 the bits are still the integer (the old trick stopped at 2^23)"""
    rng = np.random.Generator(np.random.PCG64(12))
    n = 1 << 16
    do0, fx, fy = (rng.uniform(0.0, 1.0, n).astype(f32) for _ in range(3))
    do0[:8], fx[:8], fy[:8] = 0.0, 0.0, 0.0
    wm = rng.uniform(2.0 ** 22, 2.0 ** 24, n).astype(f32)
    wm[:8] = np.nextafter(f32(2.0 ** 24), f32(0.0))
    new = new_words(do0, fx, fy, wm)
    for (w, g), got in zip(old_chain(do0, fx, fy, wm), new):
        want = exact_word(w, g)
        assert want.max() < 1 << 24 and np.array_equal(want, got)
    assert new[0].max() == (1 << 24) - 1


def ffo_range():
    """floor of half_angle_bins(.., 1, 2 - ang_bins): the angle in [-2, 6] bins minus ang_bins, |ang_bins| <= the limit
    beyond which make_desc_rec reduces it, the polynomial's error (5e-6) on either side"""
    lim = C["ang_limit"]
    return int(math.floor(-2.0 - lim - 1e-5)), int(math.floor(6.0 + lim + 1e-5))


def test_addresses_equal_the_integer_formula():
    lo, hi = ffo_range()
    assert (lo, hi) == (-19, 22)
    rs8 = C["rs"] * 8
    fcx, fcy, ffo, cpy = (a.ravel() for a in np.meshgrid(np.arange(-1, 5), np.arange(-1, 5), np.arange(lo, hi + 1),
                                                         np.arange(C["copies"]), indexing="ij"))
    # the slot sum is positive for every one of them, and the bias is invisible to the mask and the xor
    raw = 32 * fcx + 8 * ffo + 8 * cpy
    assert (raw + C["bias"]).min() > 0 and (raw + C["bias"]).max() < 1 << 23 and raw.min() < 0
    cpy8f = ((cpy * 8 + C["bias"]).astype(f32) * f32(C["cpy_scale"])).astype(f32)
    s0 = _fma(fcx.astype(f32), f32(C["s0"][0]), _fma(ffo.astype(f32), f32(C["s0"][1]), cpy8f)).view(np.uint32).astype(i64) & 56
    assert np.array_equal(s0, raw & 56)
    # histogram bases: the first wave's copies (cell (-1, -1) of copy 0 is 352 bytes in front: ROW_WORDS * 4 = 640) and
    # the last ones that fit into 64 KiB of LDS
    for hbase in (640, 640 + 1120, 640 + 3 * 1120, 5120 * 7 + 640, 65536 - 1120):
        hbasef = (np.full(len(fcx), hbase).astype(f32) * f32(C["hbase_scale"])).astype(f32)
        cb = _fma(fcy.astype(f32), f32(rs8) * f32(C["cb"][0]), _fma(fcx.astype(f32), f32(C["cb"][1]), hbasef)).view(np.uint32).astype(i64)
        want = hbase + rs8 * fcy + 64 * fcx
        assert want.min() >= 0 and np.array_equal(cb, want)
        assert np.array_equal(cb + s0, want + (raw & 56)) and np.array_equal((s0 ^ 32) + cb, ((raw & 56) ^ 32) + want)


def test_reduced_orientation_is_the_same_angle():
    """make_desc_rec beyond the limit: remainder(angle * 4 / pi, 8) in double lies in [-4, 4] and is the same bin count
    up to a multiple of 8; up to the limit the float product stays what it was"""
    rng = np.random.Generator(np.random.PCG64(13))
    angles = np.concatenate([rng.uniform(-1e4, 1e4, 2000), 10.0 ** rng.uniform(1.0, 38.5, 200), [np.finfo(f32).max, -np.finfo(f32).max]]).astype(f32)
    for a in angles:
        with np.errstate(over="ignore"):                    # the float product overflows for the largest angles: inf > limit
            b = f32(a) * f32(4.0 / np.pi)
        if abs(b) <= C["ang_limit"]:
            continue
        r = math.remainder(float(a) * (4.0 / math.pi), 8.0)
        assert abs(r) <= 4.0
        if abs(a) < 1e6:
            assert abs(math.remainder(r - float(a) * 4.0 / math.pi, 8.0)) < 1e-9
