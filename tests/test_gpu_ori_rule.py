"""The device's orientation stage, keypoint by keypoint, against the float64 rule of tests/ori_rule.py on hard-edged
images (tests/ori_cases.py): step edges, binary and saturated planes, gradients of exactly 45 degrees, exact ties.

util.feature_parity allows one feature in 2000 another selection of peaks and gives no reason; here every keypoint is
either DECIDED by the rule -- then the device's number of orientations and every angle must be the rule's -- or OPEN for
a stated reason, and then still bounded.  The pyramid, the extrema and the per-octave counts are bit for bit the
oracle's, two submits give identical bytes, and the descriptors are the oracle's in the device's own frames."""
import numpy as np
import pytest

import ori_cases
import ori_rule
from ori_cases import CASE_IDS, CASES, STRONG
from test_gpu_parity import assert_planes_equal
from util import bits, feature_parity, sorted_features

pytestmark = pytest.mark.gpu


def _ekeys(e):
    return list(zip(e["octave"].tolist(), e["lpos"].tolist(), bits(e["xpos"]).tolist(), bits(e["ypos"]).tolist()))


def _to_oracle_order(eo, eh):
    """index into the oracle's list for every device extremum (same set, bit-exact positions; duplicates in order)"""
    at = {}
    for i, k in enumerate(_ekeys(eo)):
        at.setdefault(k, []).append(i)
    return np.array([at[k].pop(0) for k in _ekeys(eh)], np.int64)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_device_satisfies_the_rule(oracle_mod, gpu_hip, case):
    image_name, param_name = case
    kw = ori_cases.PARAMS[param_name]
    levels = max(2, kw.get("levels", 3))
    img = ori_cases.image(image_name)
    ref, eo, ref_rules = ori_cases.reference(oracle_mod, *case)
    fo_ref, _ = ref.fetch()

    ctx = gpu_hip.Context(gpu_hip.default_params(**kw))
    try:
        ctx.submit(img)
        fh, dh = ctx.fetch()
        eh = ctx.extrema()

        # 1. pyramid, extrema and counts: bit for bit, no allowance (ties in DoG plateaus are strict comparisons on both sides)
        assert_planes_equal(ref, ctx, levels)
        assert sorted(_ekeys(eo)) == sorted(_ekeys(eh))
        assert ref.ext_counts() == list(ctx.report().ext_ct)[:ref.num_octaves]
        # extrema() and fetch() are one list in one order
        assert ori_rule.aligned(eh, fh, kw.get("upscale_factor", 1.0))

        # 2. the rule, for the device's own extrema: the oracle's wherever sigma is the same float (the device's powf may
        # differ in the last bit, and the window radius is a rounding of sigma)
        j = _to_oracle_order(eo, eh)
        # sigma goes through the device's powf: the project's bar, 1e-5 relative, on every case (the rule and the descriptors
        # below FOLLOW the device's sigma, so nothing else would bound it on the open images)
        sig_rel = np.abs(eh["sigma"].astype(np.float64) - eo["sigma"][j]) / eo["sigma"][j]
        assert len(sig_rel) == 0 or sig_rel.max() < 1e-5, "sigma differs by %.2e relative" % sig_rel.max()
        rules = [ref_rules[k] for k in j]
        redo = np.nonzero(bits(eh["sigma"]) != bits(eo["sigma"][j]))[0]
        for i, r in zip(redo, ori_rule.analyse_all(lambda o, l: ref.plane(o, 0, l), eh[redo], levels + 3)):
            rules[i] = r
        bad = ori_rule.check(rules, eh, fh)
        n_dec = sum(r.decided for r in rules)
        print("%s-%s: %d keypoints, %d decided, %d with the device's own sigma, %d offenders" % (
            image_name, param_name, len(rules), n_dec, len(redo), len(bad)))
        assert not bad, ori_rule.format_offenders(bad)

        # 3. two submits, the same bytes (fixed-point histogram sums do not depend on the order of arrival)
        f1, d1 = sorted_features(fh, dh)
        f2, d2 = sorted_features(*ctx.submit(img).fetch())
        for name in ("debug_octave", "xpos", "ypos", "sigma", "num_ori", "orientation"):
            assert f1[name].tobytes() == f2[name].tobytes(), name
        assert d1.tobytes() == d2.tobytes()
    finally:
        ctx.close()

    # 4. descriptors: finite, unit norm, and the oracle's in the device's own frames
    assert len(dh) == int(fh["num_ori"].sum()) and np.isfinite(dh).all()
    np.testing.assert_allclose((dh.astype(np.float64) ** 2).sum(1), 1.0, rtol=1e-4)
    fo = fo_ref[j]                                     # the oracle's features in the device's order
    same = fo["num_ori"] == fh["num_ori"]
    differ = [rules[i].why for i in np.nonzero(~same)[0] if rules[i].decided]
    assert not differ, "another number of orientations than the oracle on %d DECIDED keypoints" % len(differ)
    orc = oracle_mod.Oracle(oracle_mod.default_params(**kw), threads=8).run(img)    # redo_descriptors changes it
    ori = np.ascontiguousarray(fo_ref["orientation"], np.float32).copy()
    assert np.array_equal(orc.extrema(), eo)
    sig = eo["sigma"].copy()
    perm = {}
    for i in np.nonzero(same)[0]:
        n, free, p = int(fh[i]["num_ori"]), list(range(int(fh[i]["num_ori"]))), []
        for k in range(n):                             # the device's angles in the oracle's order
            m = min(free, key=lambda m: ori_rule.adiff(fo[i]["orientation"][k], fh[i]["orientation"][m]))
            free.remove(m)
            p.append(m)
            ori[j[i]][k] = fh[i]["orientation"][m]
        sig[j[i]] = eh[i]["sigma"]                     # octave units
        perm[i] = p
    orc.redo_descriptors(ori, 0, sig, 0)
    fo2, do2 = orc.fetch()
    rel = []
    for i, p in perm.items():
        for k, m in enumerate(p):
            a, b = do2[fo2[j[i]]["desc_idx"][k]], dh[fh[i]["desc_idx"][m]]
            rel.append(float(np.linalg.norm(a - b) / max(np.linalg.norm(a), 1e-20)))
    rel = np.array(rel)
    print("    descriptors in the device's frames: %d, %d outside 1e-3, max %.2e" % (len(rel), int((rel > 1e-3).sum()),
                                                                                    rel.max() if len(rel) else 0.0))
    assert int((rel > 1e-3).sum()) <= max(1, len(rel) // 5000) and (rel < 3e-2).all()

    # 5. the statistical bars stay what they are on the strong images
    if image_name in STRONG:
        ok, msg, _ = feature_parity(ref, fh, dh)
        assert ok, msg
