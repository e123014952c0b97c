"""k_descriptor, descriptor by descriptor, against the float64 rule of tests/desc_rule.py (cases: tests/desc_cases.py).

util.descriptor_parity allows 1e-3 relative L2 against the float32 oracle and max(1, n // 5000) descriptors beyond it
without a reason; one patch pixel in the wrong row, dropped or counted twice moves a descriptor by 1e-4 .. 1e-3 of its
norm.  Here every element of every device descriptor, in the device's own frame (its sigma, its angles), lies inside the
interval the rule derives from the kernel's arithmetic -- no allowance.  The crafted frames go through the describe path
with a given orientation: angles of exactly +-0 (the inv_s == 0 branch of the row spans), patches of up to 170 rows at
the largest accepted scale (several passes, fbits 10), a corner and the right border; there the passes are also cut
short (DEBUG_DESC_ROWS = 8, DEBUG_DESC_LIST = 64) and must leave the same bytes.

Largest error / bound per case as printed on an MI355X, and which temporary mutations of keypoint.hip fail this test where
test_hip_matches_oracle and test_gpu_desc_rowbits pass: DESIGN 4.2."""
import numpy as np
import pytest

import desc_cases
import desc_rule
import ori_rule
from desc_cases import EXTRACTION_CASES, FRAME_CASES
from test_gpu_parity import assert_planes_equal
from util import bits

pytestmark = pytest.mark.gpu


def _ekeys(e):
    return sorted(zip(e["octave"].tolist(), e["lpos"].tolist(), bits(e["xpos"]).tolist(), bits(e["ypos"]).tolist()))


def _report(case, what, rules, desc, names):
    bad, worst, worst_filled = [], 0.0, 0.0
    for r, d, name in zip(rules, desc, names):
        off = desc_rule.check(r, d)
        if off:
            bad.append(desc_rule.format_offenders(r, off, name))
        worst, worst_filled = max(worst, desc_rule.error_ratio(r, d)), max(worst_filled, desc_rule.error_ratio(r, d, 0.01))
    print("%s: %d %s, %d with offenders, largest error / bound %.3f, %.3f on elements of at least 1 %% of the length" % (
        case, len(rules), what, len(bad), worst, worst_filled))
    assert not bad, "%d descriptor(s) outside the rule\n    %s" % (len(bad), "\n    ".join(bad[:5]))


@pytest.mark.parametrize("case", EXTRACTION_CASES)
def test_extracted_descriptors_satisfy_the_rule(oracle_mod, gpu_hip, case):
    ref = desc_cases.reference(oracle_mod, case)
    kw = desc_cases.params_of(case)
    ctx = gpu_hip.Context(gpu_hip.default_params(**kw))
    try:
        fh, dh = ctx.submit(desc_cases.image(desc_cases.EXTRACTION[case][0])).fetch()
        eh = ctx.extrema()
        # planes and extrema: bit for bit the oracle's, so the rule reads the oracle's planes
        assert_planes_equal(ref.orc, ctx, kw.get("levels", 3))
        assert _ekeys(ref.orc.extrema()) == _ekeys(eh)
        assert ori_rule.aligned(eh, fh, 1.0)
    finally:
        ctx.close()
    assert len(dh) == int(fh["num_ori"].sum()) and np.isfinite(dh).all()
    planes, rules, desc, names = {}, [], [], []
    n_planes = kw.get("levels", 3) + 3                   # as desc_cases.reference clamps lpos
    for e, f in zip(eh, fh):
        key = (int(e["octave"]), min(max(int(e["lpos"]), 0), n_planes - 1))
        if key not in planes:
            planes[key] = ref.orc.plane(key[0], 0, key[1])
        for k in range(int(f["num_ori"])):
            # the device's own frame: its sigma (powf) and its angle
            rules.append(desc_rule.analyse(planes[key], e["xpos"], e["ypos"], e["sigma"], f["orientation"][k], *ref.norm))
            desc.append(dh[f["desc_idx"][k]])
            names.append("%s octave %d level %d orientation %d" % ((case,) + key + (k,)))
    assert len(rules) >= (200 if case in (desc_cases.BORDER_CASE, "noise1-default") else 400)
    _report(case, "descriptors", rules, desc, names)


@pytest.mark.parametrize("case", FRAME_CASES)
def test_crafted_frames_satisfy_the_rule(oracle_mod, gpu_hip, case):
    hip = gpu_hip
    ref = desc_cases.reference(oracle_mod, case)
    kw = desc_cases.params_of(case)
    img = desc_cases.image(case.split("-")[0][len("frames_"):])
    fr, c = desc_cases.describe_frames(hip.FRAME_DTYPE), desc_cases.crafted()
    ctx = hip.Context(hip.default_params(**kw))
    try:
        df, dd = ctx.describe(img, fr, "given")
        e = ctx.extrema()
        for key, plane in sorted(ref.planes.items()):         # the Gaussian planes the frames lie on: bit for bit the oracle's
            assert np.array_equal(bits(plane), bits(ctx.plane(key[0], 0, key[1]))), key
    finally:
        ctx.close()
    # every frame valid, placed where it was asked to be: octave 0, the hinted level, octave units = image units doubled
    assert len(df) == len(fr) == len(e) and (df["num_ori"] == 1).all() and (df["debug_octave"] == 0).all()
    assert np.array_equal(e["cell"], np.arange(len(fr))) and np.array_equal(e["lpos"], c["level"]) and (e["octave"] == 0).all()
    for n in ("xpos", "ypos", "sigma"):
        assert np.array_equal(bits(e[n]), bits(c[n])), n
    assert np.array_equal(bits(df["orientation"][:, 0]), bits(c["orientation"]))
    desc = dd[df["desc_idx"][:, 0]]
    assert np.isfinite(desc).all()
    _report(case, "frames", ref.rules(), desc, [ref.name(i) for i in range(len(fr))])

    # short passes: 8 rows or 64 list positions, whichever comes first -- the same bytes
    ctx = hip.Context(hip.default_params(**kw))
    try:
        ctx.debug_set(hip.DEBUG_DESC_ROWS, 8).debug_set(hip.DEBUG_DESC_LIST, 64)
        sf, sd = ctx.describe(img, fr, "given")
    finally:
        ctx.close()
    assert sf.tobytes() == df.tobytes() and sd.tobytes() == dd.tobytes()
