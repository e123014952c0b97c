"""The tails of the two keypoint kernels' sample walks: k_orientation takes exactly ceil(window / 64) steps of 64 window
positions -- double steps while a further step follows, then one or two single ones -- and k_descriptor ends its list
the same way, pass by pass.  A wrong tail drops or repeats the last positions of a window or of a pass, so the cases
here are chosen by their step counts and asserted to be what they were chosen for:

  extraction      synth(7, 96, 72): the smallest windows extraction gives are a radius of 7 cut by a corner, three
                  steps; it has windows of 3 .. 24 steps, odd and even;
  crafted frames  on the 2 px noise and on synth(7, 160, 120), through the describe path with computed orientations:
                  scales of 0.3 .. 1.6 octave pixels give whole windows of 9, 49, 121, 169 and 225 positions -- one
                  step (the double-step loop is never entered), two, three, four -- and frames on the border give
                  windows of ONE ROW and of ONE COLUMN (three positions) and corner windows below 64 positions; a
                  scale of 6.5 gives patch rows longer than 64 positions for the forced passes below.

Orientations are held to the float64 rule of tests/ori_rule.py and descriptors, in the device's own frames, to the rule
of tests/desc_rule.py, each with that file's bounds.  The descriptors are then computed again with the passes cut short
(DEBUG_DESC_ROWS / DEBUG_DESC_LIST): the row lengths, restated here in float32, say where the cuts fall, and the sets
are asserted to hold passes cut INSIDE a row, AT A ROW'S END and IN THE FIRST ROW of a pass; every such run must leave
the bytes of the run with whole passes."""
import functools

import numpy as np
import pytest

import desc_cases
import desc_rule
import ori_cases
import ori_rule
from util import bits, sorted_features

pytestmark = pytest.mark.gpu

F32 = np.float32
DESC_MAGNIFY = F32(3.0)
# (DEBUG_DESC_ROWS, DEBUG_DESC_LIST): whole passes are 96 rows / 3456 positions; 4 rows and 64 positions are the least
FORCED = ((None, 64), (None, 65), (4, None), (5, 100))

FRAME_IMAGES = ("noise2", "synth7")
# octave units of octave 0 (320 x 240): whole windows first, then the borders
WINDOW_SIGMAS = (0.3, 0.6, 1.0, 1.3, 1.6)           # radius roundf(4.5 sigma) = 1, 3, 5, 6, 7
INSIDE = ((100.5, 90.25), (150.0, 100.0), (61.3, 170.8))
BORDER = (
    (100.5, 0.4, 0.3), (140.25, 239.0, 0.3),         # one row: top, bottom
    (0.4, 100.5, 0.3), (319.0, 120.5, 0.3),          # one column: left, right
    (3.5, 2.25, 1.0), (317.0, 237.5, 1.0),           # corners: 9 x 7 and smaller
    (2.0, 120.0, 1.6), (160.0, 1.0, 1.6),            # a radius of 7 against the left and the top border
    (160.3, 120.6, 6.5), (100.5, 90.25, 6.5),        # patch rows of up to 138 positions
)


def crafted():
    rows = [(x, y, s) for s in WINDOW_SIGMAS for x, y in INSIDE] + list(BORDER)
    fr = np.zeros(len(rows), [("xpos", F32), ("ypos", F32), ("sigma", F32), ("level", np.int32)])
    for i, (x, y, s) in enumerate(rows):
        fr[i] = (x, y, s, 1 + i % 3)
    return fr


def window(w, h, x, y, sigma):
    """(columns, rows) of the orientation window, formed as ori_rule.histogram forms it"""
    rad = ori_rule._roundf(F32(3.0) * (F32(1.5) * F32(sigma)))
    wx = min(w - 2, ori_rule._roundf(F32(x)) + rad) - max(1, ori_rule._roundf(F32(x)) - rad) + 1
    hy = min(h - 2, ori_rule._roundf(F32(y)) + rad) - max(1, ori_rule._roundf(F32(y)) - rad) + 1
    return max(wx, 0), max(hy, 0)


def steps_of(wx, hy):
    return (wx * hy + 63) // 64


def row_lengths(w, h, x, y, sigma, angle):
    """The lengths of the rows' column intervals of one patch, top to bottom: k_descriptor's span arithmetic in float32
    (the correctly rounded cos / sin, an IEEE reciprocal where the device takes v_rcp: single positions may differ, which
    is why the assertions below ask for several cuts of each kind, not one)."""
    x, y = F32(x), F32(y)
    sbp = abs(DESC_MAGNIFY * F32(sigma))
    c, s = F32(np.cos(np.float64(angle))), F32(np.sin(np.float64(angle)))
    crsbp, srsbp = c / sbp, s / sbp
    ext_r = F32(2.5) * (abs(c * sbp) + abs(s * sbp))
    xmin, ymin = max(1, int(np.floor(x - ext_r))), max(1, int(np.floor(y - ext_r)))
    xmax, ymax = min(w - 2, int(np.floor(x + ext_r)) + 1), min(h - 2, int(np.floor(y + ext_r)) + 1)
    if xmax < xmin or ymax < ymin:
        return np.zeros(0, np.int64)
    dy = np.arange(ymin, ymax + 1).astype(F32) - y
    a, b = srsbp * dy, crsbp * dy
    lo, hi = np.full(len(dy), -1e30, F32), np.full(len(dy), 1e30, F32)
    ok = np.ones(len(dy), bool)
    if abs(crsbp) > 1e-20:
        inv = F32(1.0) / crsbp
        t0, t1 = (F32(-2.5) - a) * inv, (F32(2.5) - a) * inv
        lo, hi = np.minimum(t0, t1), np.maximum(t0, t1)
    else:
        ok &= np.abs(a) < 2.5
    if abs(srsbp) > 1e-20:
        inv = F32(1.0) / srsbp
        t0, t1 = (b - F32(2.5)) * inv, (b + F32(2.5)) * inv
        lo, hi = np.maximum(lo, np.minimum(t0, t1)), np.minimum(hi, np.maximum(t0, t1))
    else:
        ok &= np.abs(b) < 2.5
    jlo = np.maximum(xmin, np.floor(np.clip(x + lo - F32(1e-3), -1e6, 1e6)).astype(np.int64) + 1)
    jhi = np.minimum(xmax, np.ceil(np.clip(x + hi + F32(1e-3), -1e6, 1e6)).astype(np.int64) - 1)
    return np.where(ok, np.maximum(jhi - jlo + 1, 0), 0)


def cuts(lens, rows, lst):
    """Where the passes of one patch are cut by a full list, as k_descriptor cuts them: a list of 'first' (in the first
    row of a pass), 'end' (at a row's end: nothing of the next row fits) and 'inside'."""
    maxrows, maxlist = min(max(rows or 96, 4), 96), min(max(lst or 3456, 64), 3456)
    out, rb, skip = [], 0, 0
    while rb < len(lens):
        hy = min(len(lens) - rb, maxrows)
        carry, seen, nxt = 0, False, (rb + hy, 0)
        for r in range(hy):
            n = int(lens[rb + r]) - (min(skip, int(lens[rb + r])) if r == 0 else 0)
            if n > 0:
                seen = True
            elif seen:
                n = 1                                  # a row without a sample below the first one that has some
            if carry + n > maxlist:
                taken = maxlist - carry
                out.append("first" if r == 0 else "end" if taken == 0 else "inside")
                nxt = (rb + r, taken + (skip if r == 0 else 0))
                break
            carry += n
        assert nxt > (rb, skip), "no progress"
        rb, skip = nxt
    return out


def assert_cut_kinds(patches, what, need):
    """patches: (w, h, x, y, sigma, angle) per descriptor; need: the kinds of cut the set must hold, five times at least"""
    lens = [row_lengths(*p) for p in patches]
    for rows, lst in FORCED:
        kinds = [k for n in lens for k in cuts(n, rows, lst)]
        count = {k: kinds.count(k) for k in ("inside", "end", "first")}
        print("%s, DESC_ROWS %s DESC_LIST %s: passes cut %s" % (what, rows, lst, count))
        if lst is not None:
            assert count["inside"] >= 5, (what, rows, lst, count)
    kinds = [k for n in lens for rows, lst in FORCED for k in cuts(n, rows, lst)]
    assert all(kinds.count(k) >= 5 for k in need), (what, {k: kinds.count(k) for k in set(kinds)})


def check_orientations(case, rules, ext, feats):
    bad = ori_rule.check(rules, ext, feats)
    print("%s: %d keypoints, %d decided, %d offenders" % (case, len(rules), sum(r.decided for r in rules), len(bad)))
    assert not bad, ori_rule.format_offenders(bad)


def check_descriptors(case, plane_of, ext, feats, desc):
    """every descriptor in the device's own frame (its sigma, its angle) against desc_rule"""
    bad, worst, n = [], 0.0, 0
    for i, (e, f) in enumerate(zip(ext, feats)):
        for k in range(int(f["num_ori"])):
            r = desc_rule.analyse(plane_of(e), e["xpos"], e["ypos"], e["sigma"], f["orientation"][k])
            d = desc[f["desc_idx"][k]]
            off = desc_rule.check(r, d)
            if off:
                bad.append(desc_rule.format_offenders(r, off, "%s keypoint %d orientation %d" % (case, i, k)))
            worst, n = max(worst, desc_rule.error_ratio(r, d)), n + 1
    print("%s: %d descriptors, %d with offenders, largest error / bound %.3f" % (case, n, len(bad), worst))
    assert not bad, "%d descriptor(s) outside the rule\n    %s" % (len(bad), "\n    ".join(bad[:5]))


@functools.lru_cache(maxsize=None)
def planes_of(O, image_name):
    """the oracle's pyramid of one image (no keypoints): computed once, nobody changes it"""
    return O.Oracle(O.default_params(), threads=8).run(desc_cases.image(image_name), keypoints=False)


def test_extraction_windows_of_three_steps_and_more(oracle_mod, gpu_hip):
    hip, name = gpu_hip, "synth7_96x72"
    img, orc = desc_cases.image(name), planes_of(oracle_mod, "synth7_96x72")
    dims = [orc.octave_dims(o)[:2] for o in range(orc.num_octaves)]

    def run(rows=None, lst=None):
        ctx = hip.Context(hip.default_params())
        try:
            if rows:
                ctx.debug_set(hip.DEBUG_DESC_ROWS, rows)
            if lst:
                ctx.debug_set(hip.DEBUG_DESC_LIST, lst)
            f, d = ctx.submit(img).fetch()
            e = ctx.extrema()
            planes = {(o, l): ctx.plane(o, 0, l) for o, l in set(zip(e["octave"].tolist(), np.clip(e["lpos"], 0, 5).tolist()))}
            return f, d, e, planes
        finally:
            ctx.close()

    fh, dh, eh, planes = run()
    for (o, l), p in planes.items():                   # the rules read the oracle's planes
        assert np.array_equal(bits(p), bits(orc.plane(o, 0, l))), (o, l)
    assert ori_rule.aligned(eh, fh, 1.0) and len(eh) >= 200
    steps = [steps_of(*window(*dims[int(e["octave"])], e["xpos"], e["ypos"], e["sigma"])) for e in eh]
    print("%s: windows of %s steps" % (name, sorted(set(steps))))
    assert min(steps) == 3 and {3, 4, 5, 6, 7, 8} <= set(steps)
    assert sum(s % 2 for s in steps) >= 50 and sum(1 - s % 2 for s in steps) >= 50
    plane_of = lambda e: orc.plane(int(e["octave"]), 0, min(max(int(e["lpos"]), 0), 5))
    check_orientations(name, ori_rule.analyse_all(lambda o, l: orc.plane(o, 0, l), eh, 6), eh, fh)
    check_descriptors(name, plane_of, eh, fh, dh)

    # no patch row of this image is longer than 64 positions: cuts in the first row of a pass are the frames' (below)
    assert_cut_kinds([dims[int(e["octave"])] + (e["xpos"], e["ypos"], e["sigma"], f["orientation"][k])
                      for e, f in zip(eh, fh) for k in range(int(f["num_ori"]))], name, ("inside", "end"))
    f0, d0 = sorted_features(fh, dh)                   # the order of the features is not fixed from run to run
    for rows, lst in FORCED:
        f, d = sorted_features(*run(rows, lst)[:2])
        for n in ("debug_octave", "xpos", "ypos", "sigma", "num_ori", "orientation"):
            assert f[n].tobytes() == f0[n].tobytes(), (rows, lst, n)
        assert d.tobytes() == d0.tobytes(), (rows, lst)


@pytest.mark.parametrize("image_name", FRAME_IMAGES)
def test_frame_windows_of_one_to_four_steps_and_on_the_border(oracle_mod, gpu_hip, image_name):
    hip = gpu_hip
    img = ori_cases.image(image_name)
    orc = planes_of(oracle_mod, image_name)
    w, h = orc.octave_dims(0)[:2]
    c = crafted()
    fr = np.zeros(len(c), hip.FRAME_DTYPE)
    for n in ("xpos", "ypos", "sigma"):
        fr[n] = np.ldexp(c[n], -1)                     # image units: octave 0 is the up-scaled image
    fr["octave"], fr["level"] = 0, c["level"]

    # the windows are what they were chosen to be
    win = [window(w, h, f["xpos"], f["ypos"], f["sigma"]) for f in c]
    steps = [steps_of(*x) for x in win]
    whole = len(WINDOW_SIGMAS) * len(INSIDE)
    assert [wx * hy for wx, hy in win[:whole]] == [n for n in (9, 49, 121, 169, 225) for _ in INSIDE]
    assert steps[:whole] == [n for n in (1, 1, 2, 3, 4) for _ in INSIDE]
    assert [x for x in win[whole:whole + 4]] == [(3, 1), (3, 1), (1, 3), (1, 3)]
    assert all(0 < wx * hy < 64 for wx, hy in win[whole + 4:whole + 6])
    assert {2, 3} <= set(steps[whole + 6:whole + 8]) or {2, 4} <= set(steps[whole + 6:whole + 8]), steps[whole + 6:whole + 8]

    def run(rows=None, lst=None):
        ctx = hip.Context(hip.default_params())
        try:
            if rows:
                ctx.debug_set(hip.DEBUG_DESC_ROWS, rows)
            if lst:
                ctx.debug_set(hip.DEBUG_DESC_LIST, lst)
            f, d = ctx.describe(img, fr, "compute")
            return f, d, ctx.extrema(), {l: ctx.plane(0, 0, l) for l in (1, 2, 3)}
        finally:
            ctx.close()

    df, dd, e, planes = run()
    for l, p in planes.items():
        assert np.array_equal(bits(p), bits(orc.plane(0, 0, l))), l
    assert len(df) == len(fr) == len(e) and (df["num_ori"] >= 1).all() and (e["octave"] == 0).all()
    assert np.array_equal(e["lpos"], c["level"])
    for n in ("xpos", "ypos", "sigma"):
        assert np.array_equal(bits(e[n]), bits(c[n])), n
    assert len(dd) == int(df["num_ori"].sum()) and np.isfinite(dd).all()
    case = "frames on " + image_name
    check_orientations(case, ori_rule.analyse_all(lambda o, l: orc.plane(o, 0, l), e, 6), e, df)
    check_descriptors(case, lambda x: orc.plane(0, 0, int(x["lpos"])), e, df, dd)

    assert_cut_kinds([(w, h, x["xpos"], x["ypos"], x["sigma"], f["orientation"][k])
                      for x, f in zip(e, df) for k in range(int(f["num_ori"]))], case, ("inside", "end", "first"))
    for rows, lst in FORCED:
        f, d = run(rows, lst)[:2]
        assert f.tobytes() == df.tobytes() and d.tobytes() == dd.tobytes(), (rows, lst)
