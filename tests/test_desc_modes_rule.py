"""The float64 rules of the grid and interpolated descriptors (tests/desc_modes_rule.py) themselves, without a GPU: the
oracle's own float32 output must satisfy them on every case the GPU test uses, their bounds must be SHARP on the strong
images, they must flag an implementation with a single defect, and they must not flag an emulated correct device.

The measured figures -- descriptors, share within the 3e-4 bar and median bound per case (test_sharpness), flagged /
tried per defect (test_doctored_implementations), the largest packed low-half sum on the step edge -- are in DESIGN 4.3;
the asserted rates (RATES) are the smallest of each column per lattice, rounded down."""
import numpy as np
import pytest

import desc_modes_cases as C
import desc_modes_rule as R

DOCTOR_CASES = ["notile-synth7-default", "notile-noise2-default", "notile-synth7_96x72-default", "notile-frames_noise2-rootsift",
                "grid-noise2-default", "grid-synth7_96x72-default", "grid-frames_noise2-rootsift", "iloop-synth7_96x72-default",
                "iloop-noise1-default"]
EMULATED_CASES = DOCTOR_CASES + ["notile-frames_noise2-classic9", "notile-noise2-classic9", "grid-noise2-classic9"] + C.STEP_CASES


def _offenders(ref, rules, desc):
    out = []
    for i, r in enumerate(rules):
        bad = R.check(r, desc[i])
        if bad:
            out.append(R.format_offenders(r, bad, ref.name(i)))
    return out


@pytest.mark.parametrize("case", C.ALL_CASES)
def test_oracle_satisfies_the_rule(oracle_mod, case):
    """With all terms, and with the device-only terms (A_ACC, F) switched off; the raw histograms are held to delta
    directly as well."""
    ref = C.reference(oracle_mod, case)
    for device in (True, False):
        rules = ref.rules(device)
        bad = _offenders(ref, rules, ref.desc)
        assert not bad, "%d descriptor(s)\n    %s" % (len(bad), "\n    ".join(bad[:5]))
        worst = max(R.error_ratio(r, ref.desc[i]) for i, r in enumerate(rules))
        raw = [i for i, r in enumerate(rules) if not (np.abs(ref.raw[i] - r.h) <= r.delta).all()]
        assert not raw, "raw histograms outside delta: %s" % [ref.name(i) for i in raw[:5]]
        rel = [np.linalg.norm(ref.raw[i] - r.h) / np.linalg.norm(r.h) for i, r in enumerate(rules) if r.h.any()]
        print("%s (%s terms): %d descriptors, largest error / bound %.3f; raw histograms: relative L2 median %.2e, largest %.2e" % (
            case, "all" if device else "oracle", len(rules), worst, np.median(rel), max(rel)))


def test_cases_are_what_they_claim(oracle_mod):
    for case in C.STRONG_CASES:
        assert len(C.reference(oracle_mod, case).desc) >= 400, case
    for case in C.BORDER_CASES:                 # at least a third of the descriptors read beyond the border: clamp addressing
        ref = C.reference(oracle_mod, case)
        out = sum(bool(((p.px < 0) | (p.px > p.w - 1) | (p.py < 0) | (p.py > p.h - 1)).any()) for p in ref.samples)
        print("%s: %d of %d descriptors have lattice points outside the plane" % (case, out, len(ref.samples)))
        assert len(ref.samples) >= 200 and 3 * out >= len(ref.samples), (case, len(ref.samples), out)
    for case in C.FRAME_CASES:
        ref = C.reference(oracle_mod, case)
        far = max(float(max(-p.px.min(), -p.py.min(), p.px.max() - (p.w - 1), p.py.max() - (p.h - 1))) for p in ref.samples)
        print("%s: %d frames, lattice up to %.1f pixels beyond the border" % (case, len(ref.samples), far))
        if case not in C.STEP_CASES:
            assert len(ref.samples) == 192 and far > 60.0


@pytest.mark.parametrize("case", C.STEP_CASES)
def test_step_edge_fills_one_bin(oracle_mod, case):
    """Frames on a vertical 0 -> 255 step: the gradient of every point is horizontal, so all of a descriptor falls into
    one bin: bin 0 at angle 0, bin 7 at pi / 4, where t = 7 sits on the bin's centre.  The largest packed low-half sum is
    recorded as a fraction of 2^32: the headroom of k_descriptor_notile's words."""
    ref = C.reference(oracle_mod, case)
    peak = 0.0
    for p, r in zip(ref.samples, ref.rules()):
        bins = r.h.reshape(16, 8).sum(0)
        assert bins.max() >= (1.0 - 1e-6) * bins.sum() and bins.argmax() == (0 if p.angle == 0.0 else 7), (p.angle, bins)
        peak = max(peak, R.low_half_peak(p))
    print("%s: %d frames, largest low-half sum %.4f of 2^32" % (case, len(ref.samples), peak))
    assert 0.01 < peak < 0.5


@pytest.mark.parametrize("case", C.STRONG_CASES)
def test_sharpness(oracle_mod, case):
    """At least 90 % of the descriptors carry a bound of at most 3e-4 L2, the loop descriptor's own bar: a
    ceiling, not the expected value.  A case that falls short gets another image, never another bar."""
    rules = C.reference(oracle_mod, case).rules()
    b = np.array([r.bound_l2 for r in rules])
    print("%-34s %4d  %.1f %%  %.2e" % (case, len(b), 100.0 * (b <= 3e-4).mean(), np.median(b)))
    assert (b <= 3e-4).mean() >= 0.9


# flagged / tried must reach these shares, per case of the lattice: the measured ones rounded down
RATES = {
    R.NOTILE: {"point": 0.97, "last_column": 1.0, "tent_shift": 1.0, "truncate": 0.09, "tex128": 0.53, "skip_outside": 0.98, "t_shift": 0.99},
    R.ILOOP: {"point": 0.95, "last_column": 1.0, "tent_shift": 1.0, "truncate": 0.09, "tex128": 1.0, "skip_outside": 0.99, "t_shift": 0.96},
    R.GRID: {"point": 0.96, "last_column": 0.92, "tent_shift": 1.0, "skip_outside": 1.0, "t_shift": 1.0},
}


def _doctored(ref, i, rng):
    """-> {defect: raw histogram of the rule recomputed with it}; a defect that does not apply is absent"""
    p, row, lat = ref.samples[i], ref.rows[i], ref.lattice
    out = {}
    if p.n == 0:
        return out
    again = lambda **kw: R.raw_histogram(R.samples(lat, ref.plane(row), *row[2:], **kw))
    one = lambda idx: np.where(np.isin(np.arange(p.n), idx), 0.0, 1.0)
    out["point"] = R.raw_histogram(p, one(rng.integers(p.n)))         # grid: one of a cell's 256 points
    out["last_column"] = R.raw_histogram(p, one(np.nonzero(p.col == p.col.max())[0]))
    out["tent_shift"] = again(tent_shift=1)
    if lat != R.GRID:
        out["truncate"] = R.emulate_device(lat, ref.plane(row), *row[2:], rng, truncate=True)
        out["tex128"] = again(q=128.0)
    if ((p.px < 1) | (p.px > p.w - 2) | (p.py < 1) | (p.py > p.h - 2)).any():
        out["skip_outside"] = again(skip_outside=True)
    out["t_shift"] = R.raw_histogram(p, t_shift=1e-4)
    return out


@pytest.mark.parametrize("case", DOCTOR_CASES)
def test_doctored_implementations(oracle_mod, case):
    """The rule recomputed with ONE defect per descriptor -- a random lattice point dropped (for grid: one of a cell's 256
    points); the last lattice column dropped; the tent weights taken one index further; fixed point cut off instead of
    rounded; texture weights in steps of 1/128; reads that need the clamp skipped (where the lattice leaves the plane);
    t moved by 1e-4 bins -- normalised, rounded to float32 and checked against the device's rule."""
    ref = C.reference(oracle_mod, case)
    rates = RATES[ref.lattice]
    rng = np.random.default_rng(5)
    tried, flagged = dict.fromkeys(rates, 0), dict.fromkeys(rates, 0)
    for i, r in enumerate(ref.rules()):
        assert not R.check(r, R.normalize(r.h, *ref.norm).astype(np.float32))
        for name, h in _doctored(ref, i, rng).items():
            tried[name] += 1
            flagged[name] += bool(R.check(r, R.normalize(h, *ref.norm).astype(np.float32)))
    print("%-34s %s" % (case, "  ".join("%s %d / %d" % (n, flagged[n], tried[n]) for n in rates)))
    for name, rate in rates.items():
        assert flagged[name] >= rate * tried[name], (name, flagged[name], tried[name])
    assert tried["point"] == len(ref.samples)
    if case in C.BORDER_CASES or case in C.FRAME_CASES:
        assert tried["skip_outside"] >= 20


@pytest.mark.parametrize("case", EMULATED_CASES)
def test_emulated_device_is_not_flagged(oracle_mod, case):
    """The converse: gradients from float32 reads, +-A_ACC bins of angle noise on every point, every word half rounded to
    nearest at FBITS (grid: float32 weights summed in float32) -- a correct device, never flagged."""
    ref = C.reference(oracle_mod, case)
    rng = np.random.default_rng(9)
    worst = 0.0
    for i, (row, r) in enumerate(zip(ref.rows, ref.rules())):
        d = R.normalize(R.emulate_device(ref.lattice, ref.plane(row), *row[2:], rng), *ref.norm).astype(np.float32)
        bad = R.check(r, d)
        assert not bad, R.format_offenders(r, bad, ref.name(i))
        worst = max(worst, R.error_ratio(r, d))
    print("%s: %d descriptors, largest error / bound %.3f" % (case, len(ref.rows), worst))


def test_rule_on_a_ramp():
    """A plane of constant gradient 2 per pixel in x, angle 0: every read is exact, every point has |g| = 4 and t = 0, so
    only bin 0 of every cell is filled and the 16 cells mirror each other; notile's cell sum is the sum of its tents and
    Gaussians.  With the keypoint in a corner the clamp flattens the plane: the cell column that lies wholly outside loses its gradient."""
    yy, xx = np.mgrid[0:80, 0:90].astype(np.float64)
    plane = (2.0 * xx).astype(np.float32)
    for lattice in (R.NOTILE, R.ILOOP, R.GRID):
        r = R.analyse(lattice, plane, 45.0, 40.0, 2.0, 0.0)
        h = r.h.reshape(4, 4, 8)
        assert (h[:, :, 1:] == 0).all() and (h[:, :, 0] > 0).all(), lattice
        np.testing.assert_allclose(h[:, :, 0], h[::-1, ::-1, 0], rtol=1e-12)
        assert r.patch.n == {R.NOTILE: 1600, R.ILOOP: 16 * 31 * 31, R.GRID: 16 * 256}[lattice]
        cut = R.analyse(lattice, plane, 0.0, 0.0, 2.0, 0.0).h.reshape(4, 4, 8)
        assert (cut[:, 0] == 0).all() and (cut[:, 2:, 0] > 0).all(), lattice
    p = R.samples(R.NOTILE, plane, 45.0, 40.0, 2.0, 0.0)
    step = -2.5 + 1.0 / 16.0 + np.arange(40) / 8.0
    tile = 1.0 - np.abs(-1.0 + 1.0 / 16.0 + np.arange(16) / 8.0)
    want = 4.0 * np.outer(np.exp(-step[8:24] ** 2 / 8.0) * tile, np.exp(-step[:16] ** 2 / 8.0) * tile).sum()
    np.testing.assert_allclose(R.raw_histogram(p).reshape(4, 4, 8)[1, 0, 0], want, rtol=1e-12)
