"""The float64 descriptor rule (tests/desc_rule.py) itself, without a GPU: the oracle's own float32 output must satisfy
it on every case the GPU test uses, its bound must be SHARP on the strong images, it must flag an implementation with a
single defect, and it must not flag an emulated correct device.

Descriptors / share with a bound of at most 3e-4 L2 / median bound (the device's rule, all terms; printed by
test_sharpness; RootSift unless "classic9" = norm_mode 1, norm_multi 9):

    synth7-default            798  99.7 %  1.07e-04      noise2-classic9           830  99.4 %  1.32e-04
    noise1_240x180-default    499  99.0 %  6.67e-05      contrast6-classic9        894  99.6 %  1.32e-04
    noise2-default            830  99.6 %  7.31e-05      checker8_warped-classic9  929  99.9 %  1.70e-04
    contrast6-default         894  99.9 %  7.60e-05      synth7_float-default      798  99.7 %  1.07e-04
    checker8_warped-default   929  98.5 %  9.74e-05
  no bar (shown for the record): synth7_96x72-default 268 / 99.3 % / 1.09e-04; noise1-default (160 x 120) 216 / 98.6 % /
  6.67e-05; the 192 crafted frames: median 2.0e-04 (noise2, RootSift) to 7.0e-04 (synth7, classic), maximum 1.0e-03 -- a
  patch of 10 000 to 28 000 samples at fbits 10.

Doctored implementations, flagged / tried (printed by test_doctored_implementations); the asserted rates (RATES) are the
smallest of each column rounded down, 90 % for the dropped sample:

                              sample     first column  column w-2  row twice  t + 1e-4
    synth7-default            785 / 798  798 / 798     58 / 62     784 / 798  747 / 798
    noise1_240x180-default    494 / 499  499 / 499     22 / 23     494 / 499  477 / 499
    noise2-default            822 / 830  830 / 830     63 / 64     818 / 830  823 / 830
    contrast6-default         884 / 894  894 / 894     71 / 74     882 / 894  892 / 894
    checker8_warped-default   914 / 929  929 / 929    113 / 119    912 / 929  520 / 929
    synth7_float-default      785 / 798  798 / 798     58 / 62     784 / 798  747 / 798
    synth7_96x72-default      263 / 268  268 / 268     36 / 36     262 / 268  250 / 268

A dropped sample or a doubled row that goes unseen has no gradient to speak of (saturated and binary images); 1e-4 bins is
six times A, and on the warped checkerboard, whose few strong edges fill few bins, T and the norm's interval hide it in
four descriptors of nine.
"""
import numpy as np
import pytest

import desc_cases
import desc_rule
from desc_cases import BORDER_CASE, EXTRACTION_CASES, FRAME_CASES, STRONG_CASES

ALL_CASES = EXTRACTION_CASES + FRAME_CASES
DOCTOR_CASES = [c for c in STRONG_CASES if c.endswith("default")] + [BORDER_CASE]
ORACLE_TERMS = dict(arctan=False, fixed_point=False, eps="oracle")


def _offenders(ref, rules, desc):
    out = []
    for i, r in enumerate(rules):
        bad = desc_rule.check(r, desc[i])
        if bad:
            out.append(desc_rule.format_offenders(r, bad, ref.name(i)))
    return out


@pytest.mark.parametrize("case", ALL_CASES)
def test_oracle_satisfies_the_rule(oracle_mod, case):
    """With all terms (the wider of the two position terms), and with A and F switched off, since the oracle has neither
    a polynomial arctangent nor fixed point; the raw histograms are held to delta directly as well."""
    ref = desc_cases.reference(oracle_mod, case)
    for kw in (dict(eps="both"), ORACLE_TERMS):
        rules = ref.rules(**kw)
        bad = _offenders(ref, rules, ref.desc)
        assert not bad, "%d descriptor(s)\n    %s" % (len(bad), "\n    ".join(bad[:5]))
        worst = max(desc_rule.error_ratio(r, ref.desc[i]) for i, r in enumerate(rules))
        raw = [i for i, r in enumerate(rules) if not (np.abs(ref.raw[i] - r.h) <= r.delta).all()]
        assert not raw, "raw histograms outside delta: %s" % [ref.name(i) for i in raw[:5]]
        print("%s (%s): %d descriptors, largest error / bound %.3f" % (case, ",".join("%s=%s" % i for i in kw.items()), len(rules), worst))


@pytest.mark.parametrize("case", ("synth7-default", "noise2-default", "contrast6-default", "checker8_warped-default"))
def test_position_term_against_the_oracle(oracle_mod, case):
    """The oracle's raw error does not scale with the bin, it scales with the position sensitivity: on the elements that
    carry at least a quarter of their descriptor's largest sensitivity, |error| / sensitivity peaks at 2.4e-6 .. 2.7e-6 on
    all four images, while |error| / h reaches 1.3e-5 .. 1.9e-5 -- beyond TAU, so T alone would not cover a correct
    implementation.  eps_oracle (median 4.5e-6 .. 5.6e-6) lies above the ratio on every descriptor, and within a factor
    of five of the largest: derived from the arithmetic, and not loose."""
    ref = desc_cases.reference(oracle_mod, case)
    rules = ref.rules(**ORACLE_TERMS)
    ratio, rel = [], []
    for i, r in enumerate(rules):
        k = r.sens >= 0.25 * r.sens.max()
        err = np.abs(ref.raw[i] - r.h)
        ratio.append((err[k] / r.sens[k]).max())
        rel.append((err[k] / r.h[k]).max())
    ratio, eps = np.array(ratio), np.array([r.eps for r in rules])
    print("%s: |error| / sensitivity: median %.2e, max %.2e; eps_oracle median %.2e; largest ratio / eps %.2f; |error| / h up to %.2e" % (
        case, np.median(ratio), ratio.max(), np.median(eps), (ratio / eps).max(), max(rel)))
    assert (ratio <= eps).all()
    assert ratio.max() > 0.2 * np.median(eps)
    assert max(rel) > desc_rule.TAU


def test_float_angle_term_is_needed(oracle_mod):
    """"A and F switched off" leaves A_FLOAT = 1.5e-6 bins on, the float32 arithmetic of theta - angle and of t.  Without
    it the oracle itself leaves the rule: 4 of 268 descriptors on the border image (0 .. 4 on every case measured, always
    on near-empty bins that hold only the tail of a neighbouring bin's shares)."""
    ref = desc_cases.reference(oracle_mod, BORDER_CASE)
    bad = sum(bool(desc_rule.check(desc_rule.evaluate(p, *ref.norm, a_float=0.0, **ORACLE_TERMS), ref.desc[i]))
              for i, p in enumerate(ref.patches))
    print("%s: %d of %d oracle descriptors outside the rule without A_FLOAT" % (BORDER_CASE, bad, len(ref.patches)))
    assert bad >= 1


def test_cases_are_what_they_claim(oracle_mod):
    for case in STRONG_CASES:
        assert len(desc_cases.reference(oracle_mod, case).desc) >= 400, case
    ref = desc_cases.reference(oracle_mod, BORDER_CASE)
    cut = 0
    for p in ref.patches:
        r = 2.5 * (abs(p.cs[0]) + abs(p.cs[1])) * p.sbp
        cut += bool(np.floor(p.x - r) < 1 or np.floor(p.y - r) < 1 or np.floor(p.x + r) + 1 > p.w - 2 or np.floor(p.y + r) + 1 > p.h - 2)
    assert len(ref.patches) >= 200 and 3 * cut >= len(ref.patches), (len(ref.patches), cut)
    for case in FRAME_CASES:
        ref = desc_cases.reference(oracle_mod, case)
        zero = sum(p.angle == 0.0 for p in ref.patches)             # +0 and -0
        tall = sum(p.rows > 96 for p in ref.patches)                # DESC_MAXROWS
        long_ = sum(p.n > 3456 for p in ref.patches)                # DESC_LISTCAP: the device's list is a superset
        fb = sorted({p.fbits for p in ref.patches})
        print("%s: %d frames, %d at angle +-0, %d with more than 96 rows, %d with more than 3456 samples, up to %d rows, fbits %s" % (
            case, len(ref.patches), zero, tall, long_, max(p.rows for p in ref.patches), fb))
        assert len(ref.patches) == 192 and zero >= 40 and tall >= 40 and long_ >= 40
        assert max(p.rows for p in ref.patches) >= 165 and fb[0] == 10


@pytest.mark.parametrize("case", STRONG_CASES)
def test_sharpness(oracle_mod, case):
    """At least 90 % of the descriptors carry a bound of at most 3e-4 L2 (an image that falls short is replaced, never
    the bar): three to fifteen times below the 1e-3 of descriptor_parity, and without its allowance."""
    rules = desc_cases.reference(oracle_mod, case).rules()
    b = np.array([r.bound_l2 for r in rules])
    print("%-26s %4d  %.1f %%  %.2e" % (case, len(b), 100.0 * (b <= 3e-4).mean(), np.median(b)))
    assert (b <= 3e-4).mean() >= 0.9


# flagged / tried must reach these shares, per case: the measured ones rounded down
RATES = {"sample": 0.9, "first_column": 1.0, "last_column": 0.9, "row_twice": 0.97, "t_shift": 0.55}


def _doctored(p, rng):
    """-> {defect: raw histogram of the rule recomputed with it}; a defect that does not apply to the patch is absent"""
    k = np.nonzero(p.inside)[0]
    out = {}
    if len(k) == 0:
        return out
    one = lambda idx, f: np.where(np.isin(np.arange(len(p.u)), idx), f, 1.0)
    out["sample"] = desc_rule.raw_histogram(p, one(rng.choice(k), 0.0))
    rows, first = np.unique(p.row[k], return_index=True)               # samples are in raster order: the first of each row
    out["first_column"] = desc_rule.raw_histogram(p, one(k[first], 0.0))
    last = k[p.col[k] == p.w - 2]
    if len(last):
        out["last_column"] = desc_rule.raw_histogram(p, one(last, 0.0))
    out["row_twice"] = desc_rule.raw_histogram(p, one(k[p.row[k] == rng.choice(rows)], 2.0))
    out["t_shift"] = desc_rule.raw_histogram(p, t_shift=1e-4)
    return out


@pytest.mark.parametrize("case", DOCTOR_CASES)
def test_doctored_implementations(oracle_mod, case):
    """The rule recomputed with ONE defect per descriptor -- a random in-square sample dropped; the first column of every
    row's interval dropped; column w - 2 dropped (where the patch has it); a random row counted twice; t moved by 1e-4
    bins -- normalised, rounded to float32 and checked against the device's rule."""
    ref = desc_cases.reference(oracle_mod, case)
    rng = np.random.default_rng(5)
    tried, flagged = dict.fromkeys(RATES, 0), dict.fromkeys(RATES, 0)
    for p, r in zip(ref.patches, ref.rules()):
        assert not desc_rule.check(r, desc_rule.normalize(r.h, *ref.norm).astype(np.float32))
        for name, h in _doctored(p, rng).items():
            tried[name] += 1
            flagged[name] += bool(desc_rule.check(r, desc_rule.normalize(h, *ref.norm).astype(np.float32)))
    print("%-26s %s" % (case, "  ".join("%s %d / %d" % (n, flagged[n], tried[n]) for n in RATES)))
    for name, rate in RATES.items():
        assert flagged[name] >= rate * tried[name], (name, flagged[name], tried[name])
    assert tried["sample"] == len(ref.patches) and (case != BORDER_CASE or tried["last_column"] >= 20)


@pytest.mark.parametrize("case", DOCTOR_CASES + FRAME_CASES)
def test_emulated_device_is_not_flagged(oracle_mod, case):
    """The converse: float32 positions formed as the kernel forms them, +-1.5e-5 bins of angle noise on every sample,
    every word half rounded to nearest at fbits -- a correct device, never flagged."""
    ref = desc_cases.reference(oracle_mod, case)
    rng = np.random.default_rng(9)
    worst = 0.0
    for i, (row, r) in enumerate(zip(ref.rows, ref.rules())):
        d = desc_rule.normalize(desc_rule.emulate_device(ref.plane(row), *row[2:], rng), *ref.norm).astype(np.float32)
        bad = desc_rule.check(r, d)
        assert not bad, desc_rule.format_offenders(r, bad, ref.name(i))
        worst = max(worst, desc_rule.error_ratio(r, d))
    print("%s: %d descriptors, largest error / bound %.3f" % (case, len(ref.rows), worst))


def test_arctangent_constant():
    """A_POLY restated from the kernel's own text: the degree-9 polynomial of atan2_bins9 (keypoint.hip), in float32, is
    within 1.5e-5 bins of atan(r) * 4 / pi on [0, 1] -- and not within half of that, so the constant is not loose."""
    f32 = np.float32
    r = np.linspace(0.0, 1.0, 200001).astype(f32)
    s = r * r
    p = f32(0.026540832594037056) * s + f32(-0.1084246039390564)
    for c in (0.22938621044158936, -0.4205572307109833, 1.2730693817138672):
        p = p * s + f32(c)
    err = np.abs((p * r).astype(np.float64) - np.arctan(r.astype(np.float64)) * 4.0 / np.pi).max()
    print("atan2_bins9: max error %.3g bins" % err)
    assert 0.5 * desc_rule.A_POLY < err <= desc_rule.A_POLY


def test_fbits_restated():
    """make_desc_rec: 31 - ceil(log2(361 * (2.83 * 3 sigma + 1)^2)) clamped to 2 .. 14, against values worked out by hand:
    sigma 1.6 -> side 14.584, 361 * 212.7 = 76 784 < 2^17 -> 14; sigma 3.2 -> side 28.168, 286 430 < 2^19 -> 12;
    sigma 8 -> side 68.92, 1 714 723 < 2^21 -> 10; sigma 1e6 -> clamped to 2"""
    assert [desc_rule.fbits_of(s) for s in (1e-3, 1.6, 3.2, 8.0, 1e6)] == [14, 14, 12, 10, 2]


def test_rule_on_a_ramp():
    """A plane of constant gradient at angle 0: every sample has t = 0 exactly, so only bin 0 of every cell is filled,
    the 16 cells mirror each other, and a patch cut by the border loses exactly the samples beyond columns 1 .. w - 2."""
    yy, xx = np.mgrid[0:80, 0:90].astype(np.float64)
    plane = (2.0 * xx).astype(np.float32)
    r = desc_rule.analyse(plane, 45.0, 40.0, 2.0, 0.0)
    h = r.h.reshape(4, 4, 8)
    assert (h[:, :, 1:] == 0).all() and (h[:, :, 0] > 0).all()
    np.testing.assert_allclose(h[:, :, 0], h[::-1, ::-1, 0], rtol=1e-12)
    assert r.patch.n == 29 * 29 and r.patch.rows == 29             # |dx|, |dy| < 2.5 * 6 = 15
    cut = desc_rule.analyse(plane, 86.0, 40.0, 2.0, 0.0)           # columns 72 .. 88 = w - 2 of 71 .. 101
    assert cut.patch.n == 17 * 29 and cut.patch.col.max() == 88
