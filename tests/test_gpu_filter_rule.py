"""The grid filter on the device (filter.hip) held to tests/filter_rule.py on the planted cell populations and scale tie
groups of tests/filter_cases.py (480 x 480, 4 octaves; tests/test_filter_rule.py ties the same cases and the rule to the
oracle without a GPU).  Every case runs in all three modes:

  - POPSIFT_HIP_ORDER_RASTER: ctx.extrema() equals the rule's list AS BYTES -- members, order and the cell field -- and
    report().ext_ct the rule's per-octave counts.  The rule is applied to the device's own unfiltered raster list (the
    device's sigma differs from the oracle's in the last bits, its powf), which is itself compared with the oracle's in
    every other field, the cell included;
  - arrival order: filter_rule.check_properties on the survivors (subset, min(count, limit) per cell, no dropped member
    better than a kept one, everything strictly better than the threshold kept), and the oracle's survivor set wherever
    the rule says that no tie group straddles a limit;
  - feature_parity of the survivors against the oracle.
Then a batch whose two images take different decisions at the 10 % test, and describe() on a filtering context.

NOT covered here: totals above 16 384 and 131 072 (where the grid-stride loops of k_filter_count and of k_filter_hist
wrap) and list positions above 65 535 (key bits 16 .. 24 of the reversed position).  They need images of 1080p size;
tests/test_gpu_filter.py::test_filter_at_full_size_and_context_reuse reaches them on a natural image, without ties."""
import numpy as np
import pytest

import filter_cases as C
import filter_rule as F
import order_rule as R
from popsift_amd.synth import synth
from util import bits, feature_parity

pytestmark = pytest.mark.gpu

MODES = [0, 1, 2]
EXACT = ["octave", "lpos", "xpos", "ypos", "cell"]            # the fields the device and the oracle share bit for bit


def device(hip, case, pl, mode=None, order=None, filtered=True):
    order = hip.ORDER_RASTER if order is None else order
    ctx = hip.Context(hip.default_params(store_dog=1, feature_order=order, **case.params(mode, filtered)))
    ctx.submit(np.zeros((C.H, C.W), np.uint8)).wait()
    pl.upload(ctx)
    return ctx.rerun_keypoint_stages()


def ekeys(e):
    return set(zip(e["octave"].tolist(), e["lpos"].tolist(), bits(e["xpos"]).tolist(), bits(e["ypos"]).tolist()))


_unfiltered = {}


def unfiltered(hip, O, case):
    """the device's unfiltered list in raster order (one run per case, never modified)"""
    if case.name not in _unfiltered:
        pl = case.planted(O)
        ctx = device(hip, case, pl, filtered=False)
        e = ctx.extrema()
        assert list(ctx.report().ext_ct)[:C.OCT] == pl.counts
        ctx.close()
        e.setflags(write=False)
        _unfiltered[case.name] = e
    return _unfiltered[case.name]


@pytest.mark.parametrize("name", C.NAMES)
def test_unfiltered_list_and_cell_field(oracle_mod, gpu_hip, name):
    """device, oracle and rule agree on the cell of every extremum (bump centres within 1e-3 px of a cell boundary
    included, grids 7 and 9), and on everything else but the last bits of sigma; the tie groups are the oracle's"""
    case = C.BY_NAME[name]
    pl = case.planted(oracle_mod)
    dev = unfiltered(gpu_hip, oracle_mod, case)
    orc = R.sort(case.unfiltered(oracle_mod))
    assert len(dev) == len(orc) == pl.total
    for f in EXACT:
        assert dev[f].tobytes() == orc[f].tobytes(), f
    assert np.array_equal(F.recompute_cells(dev, pl.dims, case.grid), dev["cell"])
    assert R.is_ordered(dev)
    # equal scales on the device exactly where the oracle has them
    def groups(e):                                   # every record -> the first record that shares its scale
        _, first, inv = np.unique(bits(e["sigma"]) + (e["octave"].astype(np.int64) << 32), return_index=True, return_inverse=True)
        return first[inv]
    assert np.array_equal(groups(dev), groups(orc))


@pytest.mark.parametrize("mode", MODES, ids=["random", "largest_first", "smallest_first"])
@pytest.mark.parametrize("name", C.NAMES)
def test_planted_case(oracle_mod, gpu_hip, name, mode):
    hip, O = gpu_hip, oracle_mod
    case = C.BY_NAME[name]
    pl = case.planted(O)
    unf = unfiltered(hip, O, case)
    want, lim, act = F.expected_raster(unf, case.grid, case.fmax, mode)
    counts = np.bincount(unf["cell"], minlength=case.grid ** 2)
    assert act and (counts > lim).any()                                     # the premise, on the device's own list
    tied = F.straddled(unf, case.grid, case.fmax, mode)
    if "tie" in case.tags:
        assert [g for g in tied if g[2] - g[1] + 1 >= 3 and g[1] < g[3] - 1 < g[2]]
    orc = case.oracle(O, mode)
    eo = orc.extrema()

    # raster order: the rule's bytes
    ctx = device(hip, case, pl, mode)
    got = ctx.extrema()
    assert len(got) == len(want), "limit %d: the rule keeps %d, the device %d" % (lim, len(want), len(got))
    assert got.tobytes() == want.tobytes()
    want_ct = F.octave_counts(want, C.OCT)
    rep = ctx.report()
    assert list(rep.ext_ct) == want_ct + [0] * (len(rep.ext_ct) - C.OCT) and rep.ext_total == len(want)
    assert orc.ext_counts() == want_ct or tied                              # the oracle ties by ITS list position
    fh, dh = ctx.fetch()
    assert len(fh) == len(got)
    if ekeys(got) != ekeys(eo):
        assert tied, "survivors differ from the oracle's although no tie group straddles a limit"
        orc.run_from_extrema(got)                                           # the oracle's features of the device's survivors
    ok, msg, _ = feature_parity(orc, fh, dh)
    assert ok, msg
    ctx.close()

    # arrival order: what holds whichever way the ties fall
    ctx = device(hip, case, pl, mode, order=hip.ORDER_ARRIVAL)
    kept = ctx.extrema()
    assert F.check_properties(unf, kept, case.grid, case.fmax, mode) == lim
    assert np.all(np.diff(kept["octave"]) >= 0)
    assert list(ctx.report().ext_ct)[:C.OCT] == F.octave_counts(kept, C.OCT)
    if not tied:
        assert ekeys(kept) == ekeys(case.oracle(O, mode).extrema()) == ekeys(want)
    fa, da = ctx.fetch()
    assert len(fa) == len(kept) and np.all(np.isfinite(da))
    ctx.close()


# ------------------------------------------------------------------------------------------------- real images

FMAX = 800
BUSY = synth(31, 320, 240)                                                   # 2778 extrema: thinned
QUIET = (synth(5, 320, 240).astype(np.float32) * 0.3 + 100).astype(np.uint8)  # 566 extrema <= int(800 * 1.1): untouched


def _raster(hip, **kw):
    return hip.default_params(feature_order=hip.ORDER_RASTER, **kw)


def _single(hip, img, **kw):
    ctx = hip.Context(_raster(hip, **kw)).submit(img)
    f, d = ctx.fetch()
    e = ctx.extrema()
    ctx.close()
    return f.tobytes(), d.tobytes(), e


@pytest.mark.parametrize("mode", MODES, ids=["random", "largest_first", "smallest_first"])
def test_batch_with_mixed_decisions(gpu_hip, mode):
    """one image over the 10 % test and one under it in one batch, both slot orders: every slot equals its own single
    submit as bytes, and the single submits are the rule's"""
    hip = gpu_hip
    kw = dict(filter_max_extrema=FMAX, filter_sorting=mode, filter_grid_size=3)
    single, full = {}, {}
    for key, img in (("busy", BUSY), ("quiet", QUIET)):
        single[key] = _single(hip, img, **kw)
        full[key] = _single(hip, img, filter_grid_size=3)
        want, lim, act = F.expected_raster(full[key][2], 3, FMAX, mode)
        assert act == (key == "busy")
        assert single[key][2].tobytes() == want.tobytes()
    assert 0 < len(single["busy"][2]) < len(full["busy"][2])                 # one thinned,
    assert len(full["quiet"][2]) > 100 and single["quiet"][:2] == full["quiet"][:2]   # one untouched
    for order in (("busy", "quiet"), ("quiet", "busy"), ("quiet", "busy", "busy", "quiet")):
        ctx = hip.Context(_raster(hip, **kw)).submit_batch([BUSY if k == "busy" else QUIET for k in order])
        for slot, key in enumerate(order):
            f, d = ctx.fetch_item(slot)
            assert (f.tobytes(), d.tobytes()) == single[key][:2], (order, slot)
        ctx.close()


def test_describe_on_a_filtering_context(gpu_hip):
    """frames are not filtered: describe() of more than 1.1 * filter_max frames on a filtering context gives the bytes of
    a context without the filter, and the next submit on it is filtered again, as on a fresh context"""
    hip = gpu_hip
    kw = dict(filter_max_extrema=100, filter_sorting=1, filter_grid_size=2)
    rng = np.random.default_rng(9)
    fr = np.zeros(300, hip.FRAME_DTYPE)
    fr["xpos"], fr["ypos"] = rng.uniform(5, 315, 300), rng.uniform(5, 235, 300)
    fr["sigma"] = rng.uniform(1.0, 6.0, 300)
    fr["octave"] = fr["level"] = -1
    assert len(fr) > int(100 * 1.1)
    plain = hip.Context(_raster(hip))
    f0, d0 = plain.describe(BUSY, fr)
    plain.close()
    assert len(f0) == 300
    fresh = _single(hip, BUSY, **kw)
    assert 0 < len(fresh[2]) < 300
    ctx = hip.Context(_raster(hip, **kw))
    for _ in range(2):
        f, d = ctx.describe(BUSY, fr)
        assert f.tobytes() == f0.tobytes() and d.tobytes() == d0.tobytes()
        ctx.submit(BUSY)
        f, d = ctx.fetch()
        assert (f.tobytes(), d.tobytes()) == fresh[:2] and ctx.extrema().tobytes() == fresh[2].tobytes()
    ctx.close()
