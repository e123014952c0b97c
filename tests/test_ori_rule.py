"""The float64 orientation rule (tests/ori_rule.py) itself, without a GPU: the oracle's own float32 output must satisfy
it on every case the GPU test uses, it must DECIDE most keypoints of the strong images, and it must reject an output
that is wrong for a single keypoint.

Keypoints / decided share per case (image-parameters; printed by test_decided_share):

    image             default      opencv       vlfeat       levels5      no_upscale
    synth7            649  96.5 %  559  96.4 %                            122  98.4 %
    noise1            149  93.3 %  135  96.3 %
    noise2            575  86.6 %  554  92.2 %  573  87.1 %  728  86.5 %
    contrast6         655  95.7 %  524  95.8 %
    checker8_warped   345  86.7 %  171  88.9 %  352  87.8 %  830  91.2 %  161  93.8 %
    synth7_float      649  96.5 %  559  96.4 %
  open images (ties: no bar, shown for the record)
    checker7          389   0.5 %  315   0.0 %
    checker8           42  61.9 %  235   0.0 %   42  61.9 %   62  29.0 %   55  16.4 %
    noise4            645  59.1 %  457  70.2 %

The share is set by samples ON bin edges (gradients of exactly 45 degrees and their like), not by rounding: it does not
move when TAU goes from 1e-5 to 1e-7.  An image that falls short of 85 % gets another seed, never another bar (the 2 px
noise: seed 102 gave 83.6 % in the default mode, seed 22 is above the bar in all four of its modes), and one that
meets the 100 keypoints with none to spare gets another seed too (1 px noise: seed 101 gave exactly 100 in OpenCV mode).
"""
import numpy as np
import pytest

import ori_cases
import ori_rule
from ori_cases import CASE_IDS, CASES, STRONG

STRONG_CASES = [c for c in CASES if c[0] in STRONG]
# the doctored outputs: the default mode of every strong image, and the case with the most four-orientation keypoints
DOCTOR_CASES = [c for c in STRONG_CASES if c[1] == "default"] + [("checker8_warped", "no_upscale")]


def ids(cases):
    return ["%s-%s" % c for c in cases]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_oracle_satisfies_the_rule(oracle_mod, case):
    orc, ext, rules = ori_cases.reference(oracle_mod, *case)
    feats, _ = orc.fetch()
    assert ori_rule.aligned(ext, feats, ori_cases.PARAMS[case[1]].get("upscale_factor", 1.0))
    bad = ori_rule.check(rules, ext, feats)
    assert not bad, ori_rule.format_offenders(bad)


def test_oracle_satisfies_the_rule_at_its_own_rounding(oracle_mod):
    """TAU = 1e-5 is room for the device's hardware exp2 / rcp / sqrt: the oracle itself (libm, float32 sums) stays
    inside the rule with 1e-7 and without the device's fixed-point term (classification and angle bounds alike), and the
    decided share does not move -- it is set by samples on bin edges."""
    for case in (("synth7", "default"), ("noise2", "default"), ("checker8_warped", "opencv")):
        orc, ext, rules = ori_cases.reference(oracle_mod, *case)
        kw = ori_cases.PARAMS[case[1]]
        # the fixed-point term is the device's: without it delta is the edge weight and the rounding alone
        tight = ori_rule.analyse_all(lambda o, l: orc.plane(o, 0, l), ext, max(2, kw.get("levels", 3)) + 3, tau=1e-7,
                                     fixed_point=False)
        feats, _ = orc.fetch()
        bad = ori_rule.check(tight, ext, feats)
        assert not bad, ori_rule.format_offenders(bad)
        a, b = sum(r.decided for r in rules), sum(r.decided for r in tight)
        assert abs(a - b) <= max(2, len(rules) // 100), (case, a, b)


@pytest.mark.parametrize("case", STRONG_CASES, ids=ids(STRONG_CASES))
def test_decided_share(oracle_mod, case):
    _, ext, rules = ori_cases.reference(oracle_mod, *case)
    n, decided = len(rules), sum(r.decided for r in rules)
    print("%s-%s: %d keypoints, %d decided (%.1f %%)" % (case[0], case[1], n, decided, 100.0 * decided / max(n, 1)))
    assert n >= 100, n
    assert decided >= 0.85 * n, (decided, n)


def test_open_images_are_open(oracle_mod):
    """The tie-heavy images are in the set for what they leave open; if they were decided they would be strong ones."""
    for case in [c for c in CASES if c[0] in ori_cases.OPEN]:
        _, _, rules = ori_cases.reference(oracle_mod, *case)
        n, decided = len(rules), sum(r.decided for r in rules)
        print("%s-%s: %d keypoints, %d decided (%.1f %%)" % (case[0], case[1], n, decided, 100.0 * decided / max(n, 1)))
        assert n >= 40 and decided < 0.85 * n, (case, n, decided)


def one(rules, ext, feats, i, f):
    """check() on keypoint i alone with the feature record f in place of the oracle's."""
    g = feats[i:i + 1].copy()
    g[0] = f
    return ori_rule.check(rules[i:i + 1], ext[i:i + 1], g)


@pytest.mark.parametrize("case", DOCTOR_CASES, ids=ids(DOCTOR_CASES))
def test_doctored_output_is_rejected(oracle_mod, case):
    """One keypoint wrong in one way, for every decided keypoint the doctoring applies to: an offender each time."""
    orc, ext, rules = ori_cases.reference(oracle_mod, *case)
    feats, _ = orc.fetch()
    done = dict(removed=0, stray=0, moved=0, capped=0)
    for i, r in enumerate(rules):
        if not r.decided or r.flat:
            continue
        n = int(feats[i]["num_ori"])
        ang = feats[i]["orientation"].copy()
        assert not one(rules, ext, feats, i, feats[i])
        for k in range(n) if n >= 2 else []:                        # one orientation removed
            f = feats[i].copy()
            f["orientation"][:] = 0.0
            f["orientation"][:n - 1] = np.delete(ang[:n], k)
            f["num_ori"] = n - 1
            assert one(rules, ext, feats, i, f), ("removed", i, k)
            done["removed"] += 1
        if 2 <= n <= 3:                                             # a stray one half-way between two peaks
            a = np.sort(ang[:n])
            f = feats[i].copy()
            f["orientation"][n] = 0.5 * (a[0] + a[1])
            f["num_ori"] = n + 1
            assert one(rules, ext, feats, i, f), ("stray", i)
            done["stray"] += 1
        for k in range(n):                                          # one angle moved by ten times its bound
            b = min(r.expect, key=lambda b: ori_rule.adiff(r.peaks[b]["angle"], ang[k]))
            for sign in (-1.0, 1.0):
                f = feats[i].copy()
                moved = float(ang[k]) + sign * 10.0 * ori_rule.angle_bound(r, b)
                f["orientation"][k] = (moved + np.pi) % (2 * np.pi) - np.pi
                assert one(rules, ext, feats, i, f), ("moved", i, k, sign)
                done["moved"] += 1
        if n == 4:                                                  # num_ori capped at 3
            f = feats[i].copy()
            f["num_ori"] = 3
            f["orientation"][3] = 0.0
            assert one(rules, ext, feats, i, f), ("capped", i)
            done["capped"] += 1
    print(case, done)
    assert done["removed"] >= 20 and done["stray"] >= 20 and done["moved"] >= 200
    if case[0] == "checker8_warped":
        assert done["capped"] >= 50


def test_doctored_open_keypoints_are_rejected(oracle_mod):
    """An open keypoint is not a free one: an orientation far from every possible peak and a missing certain peak are
    offenders there too."""
    orc, ext, rules = ori_cases.reference(oracle_mod, "noise4", "default")
    feats, _ = orc.fetch()
    stray = missing = 0
    for i, r in enumerate(rules):
        if r.decided:
            continue
        n = int(feats[i]["num_ori"])
        gaps = [a for a in np.arange(-np.pi, np.pi, ori_rule.BIN_RAD)
                if min(ori_rule.adiff(a, ori_rule._bin_angle(b)) for b in r.may) > 1.5 * ori_rule.BIN_RAD]
        if gaps and n < 4:
            f = feats[i].copy()
            f["orientation"][n] = gaps[0]
            f["num_ori"] = n + 1
            assert [o for o in one(rules, ext, feats, i, f) if o["what"] == "stray"], i
            stray += 1
        if r.must and n >= 2:
            b = r.must[0]
            k = min(range(n), key=lambda k: ori_rule.adiff(feats[i]["orientation"][k], ori_rule._bin_angle(b)))
            f = feats[i].copy()
            f["orientation"][:] = 0.0
            f["orientation"][:n - 1] = np.delete(feats[i]["orientation"][:n], k)
            f["num_ori"] = n - 1
            assert [o for o in one(rules, ext, feats, i, f) if o["what"] == "missing"], i
            missing += 1
    assert stray >= 20 and missing >= 5, (stray, missing)


def ramp(a, b):
    yy, xx = np.mgrid[0:40, 0:48].astype(np.float64)
    return (a * xx + b * yy).astype(np.float32)


def test_rule_on_a_ramp():
    """A plane of constant gradient puts every sample into one bin: one orientation at that bin's centre, decided --
    unless the gradient's angle is ON a bin edge (45 degrees is: 22.5 bins), where nothing is."""
    r = ori_rule.analyse(ramp(3.0, 1.0), 24.25, 19.5, 2.0)
    t = ori_rule.NB * (np.arctan2(1.0, 3.0) + np.pi) / (2 * np.pi)
    assert r.decided and r.expect == [int(np.floor(t + 0.5))] and r.U == 0.0
    assert abs(r.peaks[r.expect[0]]["angle"] - ori_rule._bin_angle(np.floor(t + 0.5))) < 1e-12
    # the window: radius roundf(4.5 * 2) = 9 around (24, 20), the circle (int)(d^2) <= 81
    dx, dy = np.meshgrid(np.arange(15, 34) - np.float32(24.25), np.arange(11, 30) - np.float32(19.5))
    assert r.n == int(((dx * dx + dy * dy).astype(np.int64) <= 81).sum())
    r = ori_rule.analyse(ramp(2.0, 2.0), 24.25, 19.5, 2.0)
    assert not r.decided and r.U == pytest.approx(r.raw.sum())


def test_rule_window_clamps_at_the_border():
    """Next to the border the window is cut at 1 and w - 2, h - 2: the sample count says so."""
    p = ramp(3.0, 1.0)
    r = ori_rule.analyse(p, 2.0, 37.0, 2.0)
    xs, ys = np.arange(1, 12), np.arange(28, 39)      # 1 .. min(46, 2 + 9), max(1, 37 - 9) .. min(38, 46)
    dx, dy = np.meshgrid(xs - np.float32(2.0), ys - np.float32(37.0))
    assert r.n == int(((dx * dx + dy * dy).astype(np.int64) <= 81).sum())
    assert r.decided and len(r.expect) == 1


def test_rule_on_an_empty_histogram():
    """No gradient anywhere: no peak, and the reference's selection then reports four orientations at position -1."""
    r = ori_rule.analyse(np.full((30, 30), 255.0, np.float32), 15.0, 15.0, 1.6)
    assert r.flat and r.decided
    f = np.zeros(1, [("debug_octave", np.int32), ("num_ori", np.int32), ("orientation", np.float32, (4,))])
    e = np.zeros(1, [("octave", np.int32), ("xpos", np.float32), ("ypos", np.float32), ("sigma", np.float32)])
    f["num_ori"], f["orientation"] = 4, np.float32(ori_rule._bin_angle(-1.0))
    assert not ori_rule.check([r], e, f)
    f["num_ori"] = 1
    assert ori_rule.check([r], e, f)
