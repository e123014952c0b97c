"""k_descriptor_notile<false> (notile, igrid), k_descriptor_notile<true> (iloop) and k_descriptor_grid (desc_modes.hip),
descriptor by descriptor, against the float64 rules of tests/desc_modes_rule.py (cases: tests/desc_modes_cases.py).

util.descriptor_parity holds these modes to 1e-3 relative L2 against the float32 oracle with max(1, n // 5000)
descriptors beyond it; one lattice point dropped, a tent weight one index off or fixed-point rounding turned into
truncation moves a descriptor by 1e-5 .. 1e-3 of its norm.  Here every element of every device descriptor, in the
device's own frame (its sigma, its angles), lies inside the interval the rule derives from the kernel's arithmetic -- no
allowance.  The crafted frames go through the describe path with a given orientation: sigma up to the largest accepted
one, angles of exactly +-0, pi/2 and +-pi, a corner, x = w - 1 and y = h - 1, and frames on a 0 -> 255 step.

Largest error / bound per case as printed on an MI355X, and which temporary mutations of desc_modes.hip fail this test where
test_hip_matches_oracle passes: DESIGN 4.3."""
import numpy as np
import pytest

import desc_modes_cases as C
import desc_modes_rule as R
import ori_rule
from test_gpu_parity import assert_planes_equal
from util import bits

pytestmark = pytest.mark.gpu


def _ekeys(e):
    return sorted(zip(e["octave"].tolist(), e["lpos"].tolist(), bits(e["xpos"]).tolist(), bits(e["ypos"]).tolist()))


def _by_frame(f, d):
    """every descriptor's bytes under its frame's bits, sorted: extraction appends features in arrival order"""
    return sorted((bits(f["xpos"][i:i + 1]).item(), bits(f["ypos"][i:i + 1]).item(), bits(f["sigma"][i:i + 1]).item(),
                   bits(f["orientation"][i, k:k + 1]).item(), d[f["desc_idx"][i, k]].tobytes())
                  for i in range(len(f)) for k in range(int(f["num_ori"][i])))


def _report(case, what, rules, desc, names):
    bad, worst, worst_filled = [], 0.0, 0.0
    for r, d, name in zip(rules, desc, names):
        off = R.check(r, d)
        if off:
            bad.append(R.format_offenders(r, off, name))
        worst, worst_filled = max(worst, R.error_ratio(r, d)), max(worst_filled, R.error_ratio(r, d, 0.01))
    print("%s: %d %s, %d with offenders, largest error / bound %.3f, %.3f on elements of at least 1 %% of the length" % (
        case, len(rules), what, len(bad), worst, worst_filled))
    assert not bad, "%d descriptor(s) outside the rule\n    %s" % (len(bad), "\n    ".join(bad[:5]))


@pytest.mark.parametrize("case", C.EXTRACTION_CASES)
def test_extracted_descriptors_satisfy_the_rule(oracle_mod, gpu_hip, case):
    ref = C.reference(oracle_mod, case)
    kw = dict(C.params_of(case), desc_mode=R.DESC_MODE[C.mode_of(case)])
    img = C.image_of(case)
    ctx = gpu_hip.Context(gpu_hip.default_params(**kw))
    try:
        fh, dh = ctx.submit(img).fetch()
        eh = ctx.extrema()
        # planes and extrema: bit for bit the oracle's, so the rule reads the oracle's planes
        assert_planes_equal(ref.orc, ctx, kw.get("levels", 3))
        assert _ekeys(ref.orc.extrema()) == _ekeys(eh)
        assert ori_rule.aligned(eh, fh, 1.0)
        f2, d2 = ctx.submit(img).fetch()                      # two submits: the same bytes, frame by frame
        assert len(d2) == len(dh) and _by_frame(f2, d2) == _by_frame(fh, dh)
    finally:
        ctx.close()
    assert len(dh) == int(fh["num_ori"].sum()) and np.isfinite(dh).all()
    planes, rules, desc, names = {}, [], [], []
    n_planes = kw.get("levels", 3) + 3                   # as desc_modes_cases.reference clamps lpos
    for e, f in zip(eh, fh):
        key = (int(e["octave"]), min(max(int(e["lpos"]), 0), n_planes - 1))
        if key not in planes:
            planes[key] = ref.orc.plane(key[0], 0, key[1])
        for k in range(int(f["num_ori"])):
            # the device's own frame: its sigma (powf) and its angle
            rules.append(R.analyse(ref.lattice, planes[key], e["xpos"], e["ypos"], e["sigma"], f["orientation"][k], *ref.norm))
            desc.append(dh[f["desc_idx"][k]])
            names.append("%s octave %d level %d orientation %d" % ((case,) + key + (k,)))
    assert len(rules) >= (400 if case in C.STRONG_CASES else 200)
    _report(case, "descriptors", rules, desc, names)


@pytest.mark.parametrize("case", C.FRAME_CASES)
def test_crafted_frames_satisfy_the_rule(oracle_mod, gpu_hip, case):
    hip = gpu_hip
    ref = C.reference(oracle_mod, case)
    kw = dict(C.params_of(case), desc_mode=R.DESC_MODE[C.mode_of(case)])
    img = C.image_of(case)
    fr, c = C.describe_frames(case, hip.FRAME_DTYPE), C.frames_of(case)
    ctx = hip.Context(hip.default_params(**kw))
    try:
        df, dd = ctx.describe(img, fr, "given")
        e = ctx.extrema()
        for key, plane in sorted(ref.planes.items()):         # the Gaussian planes the frames lie on: bit for bit the oracle's
            assert np.array_equal(bits(plane), bits(ctx.plane(key[0], 0, key[1]))), key
        f2, d2 = ctx.describe(img, fr, "given")               # two submits: the same bytes
        assert f2.tobytes() == df.tobytes() and d2.tobytes() == dd.tobytes()
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
