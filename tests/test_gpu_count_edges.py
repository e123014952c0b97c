"""The keypoint stages at the extremum COUNTS where their control flow turns, on scale spaces planted by tests/planted.py
(upload_plane + rerun_keypoint_stages, the oracle's run_keypoint_stages on the same planes).

Boundaries (keypoint.hip unless named):
  - XcdSlice / more(): chunks of KP_CHUNK = 256 keypoints per XCD, 2048 per round; DEBUG_KP_WAVES 32 / 64 makes every
    wave stride;
  - k_scan_local chunks of SCAN_LCHUNK = 64, k_scan_apply chunks of SCAN_CHUNK = 256: the partials of the preceding
    chunks, the counters written by chunk nb - 1, the total == 0 branch, ori_ps of the first extremum of an octave and
    finish()'s backward fill of ori_ct over empty octaves (ctx.hip);
  - capacities at, and one past, the need: OHIST_CAP (hist_short, gc >= hist_cap), CAND_CAP (one detection sub-queue
    exactly full / one short, extrema.hip k_detect), DESC_CAP (desc_short, idx + q >= desc_cap), max_extrema;
  - the grid filter's 10 % rule, int(filter_max * 1.1) < total (filter.hip).
Every case: extrema bit-exact, feature_parity, report() counts equal to the oracle's, the layout contract; where a
switch changes only buffers or launch shapes, the result is bit-identical to the default run."""
import numpy as np
import pytest

import planted as P
from util import bits, capped_parity, feature_parity, sorted_features

pytestmark = pytest.mark.gpu

W = H = 480
OCT = 4            # octaves 480, 240, 120, 60: lattices of 2304, 576, 144, 36 sites


def _dims(O, **kw):
    return P.octave_dims(O, W, H, OCT, **kw)


def planted(O, request, seed=0, **kw):
    return P.Planted(_dims(O, **kw), request, seed=seed, sift_mode=kw.get("sift_mode", 0))


def oracle_on(O, pl, **kw):
    orc = O.Oracle(O.default_params(**P.params_kw(OCT, **kw)), threads=4)
    orc.run(np.zeros((H, W), np.uint8), keypoints=False)
    pl.load_oracle(orc)
    return orc


def device_on(hip, pl, debug=(), ctx=None, **kw):
    """a store_dog = 1 Context (new, or `ctx` again) with the planted planes, keypoint stages re-run on them"""
    if ctx is None:
        ctx = hip.Context(hip.default_params(store_dog=1, **P.params_kw(OCT, **kw)))
        for what, value in debug:
            ctx.debug_set(what, value)
        ctx.submit(np.zeros((H, W), np.uint8)).wait()
    pl.upload(ctx)
    return ctx.rerun_keypoint_stages()


def canon(feats, desc):
    f, d = sorted_features(feats, desc)
    return (f["debug_octave"].copy(), bits(f["xpos"]), bits(f["ypos"]), bits(f["sigma"]), f["num_ori"].copy(),
            bits(f["orientation"]), bits(d))


def same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def check(orc, ctx, pl=None, grid_mode=False):
    """the device against the oracle on the same planes; returns the device's result in canonical order"""
    n = orc.num_octaves
    eo, eh = orc.extrema(), ctx.extrema()
    key = lambda e: sorted(zip(e["octave"].tolist(), e["lpos"].tolist(), bits(e["xpos"]).tolist(), bits(e["ypos"]).tolist()))
    assert key(eo) == key(eh), "extrema: oracle %d, device %d" % (len(eo), len(eh))
    counts = orc.ext_counts()
    if pl is not None:
        assert counts == pl.counts
    rep = ctx.report()
    assert rep.num_octaves == n
    assert list(rep.ext_ct) == counts + [0] * (len(rep.ext_ct) - n), list(rep.ext_ct)
    fo, do = orc.fetch()
    fh, dh = ctx.fetch()
    ori_o = [int(fo["num_ori"][fo["debug_octave"] == o].sum()) for o in range(n)]
    ori_h = [int(fh["num_ori"][fh["debug_octave"] == o].sum()) for o in range(n)]
    # report().ori_ct is the device's own per-octave descriptor count, exactly
    assert list(rep.ori_ct) == ori_h + [0] * (len(rep.ori_ct) - n), (list(rep.ori_ct), ori_h)
    assert rep.ext_total == len(fo) == len(fh) and rep.ori_total == len(dh) == sum(ori_h)
    ok, msg, st = feature_parity(orc, fh, dh, grid_mode=grid_mode)
    assert ok, msg
    # ... and the oracle's, up to the features feature_parity lets differ in their number of orientations
    assert sum(abs(a - b) for a, b in zip(ori_o, ori_h)) <= 3 * st["num_ori_diff"], (ori_o, ori_h)
    assert len(do) == sum(ori_o)
    # layout contract of the reference: descriptors feature by feature, octaves ascending, indices contiguous
    idx = np.concatenate([f["desc_idx"][: int(f["num_ori"])] for f in fh]) if len(fh) else np.zeros(0, int)
    assert np.array_equal(idx, np.arange(len(dh)))
    assert np.all(np.diff(fh["debug_octave"]) >= 0)
    assert np.all(fh["desc_idx"][np.arange(4)[None, :] >= fh["num_ori"][:, None]] == -1)
    return canon(fh, dh)


def split(total):
    """a total spread over octaves 0 .. 2 (octave 0 holds the most)"""
    if total == 0:
        return {}
    k1, k2 = total // 5, total // 20
    return {0: total - k1 - k2, 1: k1, 2: k2}


SEAMS = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049]


@pytest.mark.parametrize("total", SEAMS)
def test_totals_across_the_launch_and_scan_seams(oracle_mod, gpu_hip, total):
    """every wave strides at KP_WAVES 32 and 64 (32 / 64 single-wave workgroups, 4 / 8 per XCD); the result must be the
    oracle's and bit-identical across the three launch sizes"""
    pl = planted(oracle_mod, split(total), seed=total)
    assert pl.total == total
    orc = oracle_on(oracle_mod, pl)
    res = []
    for waves in (None, 32, 64):
        debug = () if waves is None else ((gpu_hip.DEBUG_KP_WAVES, waves),)
        ctx = device_on(gpu_hip, pl, debug=debug)
        res.append(check(orc, ctx, pl))
        ctx.close()
    for r in res[1:]:
        assert same(r, res[0])


@pytest.mark.parametrize("layout", [{0: 63, 1: 2}, {0: 64, 1: 1}, {0: 255, 1: 3}, {0: 256, 1: 1, 2: 1},
                                    {0: 40, 1: 0, 2: 40}, {0: 30, 1: 0, 2: 0, 3: 30}, {1: 30, 2: 20, 3: 5},
                                    {0: 0, 1: 0, 2: 60}, {3: 20}, {0: 1, 3: 1}],
                         ids=lambda r: "-".join("%d:%d" % kv for kv in sorted(r.items())))
def test_octave_layouts(oracle_mod, gpu_hip, layout):
    """octave boundaries inside a 64- and a 256-extremum chunk, empty octaves between, before and after non-empty ones"""
    pl = planted(oracle_mod, layout, seed=7)
    orc = oracle_on(oracle_mod, pl)
    ctx = device_on(gpu_hip, pl)
    check(orc, ctx, pl)
    ctx.close()


def test_stale_counters_do_not_survive(oracle_mod, gpu_hip):
    """one context, three planted scale spaces in turn: a full one, one with empty octaves, and nothing at all"""
    ctx = None
    for k, layout in enumerate([{0: 300, 1: 100, 2: 40, 3: 12}, {0: 40, 1: 0, 2: 40, 3: 0}, {}, {3: 5}]):
        pl = planted(oracle_mod, layout, seed=20 + k)
        orc = oracle_on(oracle_mod, pl)
        ctx = device_on(gpu_hip, pl, ctx=ctx)
        check(orc, ctx, pl)
    ctx.close()


LAYOUT = {0: 300, 1: 120, 2: 40, 3: 9}


def _reference(O, hip, **kw):
    pl = planted(O, LAYOUT, seed=3, **kw)
    orc = oracle_on(O, pl, **kw)
    ctx = device_on(hip, pl, **kw)
    res = check(orc, ctx, pl)
    return pl, orc, ctx, res


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_orientation_histogram_capacity(oracle_mod, gpu_hip, delta):
    """OHIST_CAP = N - 1 / N / N + 1 for N extrema: hist_short flips at N (ctx.hip finish), and in the first pass the
    extremum at gc = hist_cap gets no orientation (k_scan_local)"""
    pl, orc, ref, res0 = _reference(oracle_mod, gpu_hip)
    n = pl.total
    ctx = device_on(gpu_hip, pl, debug=((gpu_hip.DEBUG_OHIST_CAP, n + delta),))
    assert same(check(orc, ctx, pl), res0)
    for c in (ctx, ref):
        c.close()


@pytest.mark.parametrize("delta", [0, -1])
def test_candidate_sub_queue_exactly_full(oracle_mod, gpu_hip, delta):
    """all candidates of octave 0 in one detection sub-queue's cell (k_detect: subq of an 8 x 8 grid over the octave,
    shared by all octaves); CAND_CAP = 64 x the fullest sub-queue: exactly full (no re-run), then one short (a re-run
    with a grown buffer).  Both must be the default run's result."""
    dims = _dims(oracle_mod)
    w, h = dims[0]
    rect = P.subq_rect(w, h, 18)
    k = P.capacity(w, h, rect=rect)
    pl = P.Planted(dims, {0: (k, rect), 1: 30, 2: 10}, seed=11)
    q = np.concatenate([P.subq_of(*dims[o], pl.bumps[o]["x"], pl.bumps[o]["y"]) for o in range(len(dims))])
    qmax = int(np.bincount(q, minlength=P.DET_SUBQ).max())
    assert qmax >= k >= 20
    orc = oracle_on(oracle_mod, pl)
    ref = device_on(gpu_hip, pl)
    res0 = check(orc, ref, pl)
    ctx = device_on(gpu_hip, pl, debug=((gpu_hip.DEBUG_CAND_CAP, P.DET_SUBQ * (qmax + delta)),))
    assert same(check(orc, ctx, pl), res0)
    for c in (ctx, ref):
        c.close()


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_max_extrema_at_the_fullest_octave(oracle_mod, gpu_hip, delta):
    """max_extrema = n_o - 1 / n_o / n_o + 1 for the fullest octave (300): at and above the need the result is the
    default run's bit for bit; one below, capped_parity"""
    pl, _, ref, res0 = _reference(oracle_mod, gpu_hip)
    full_ext = ref.extrema()
    full_dev = ref.fetch()
    cap = LAYOUT[0] + delta
    orc = oracle_on(oracle_mod, pl, max_extrema=cap)
    ctx = device_on(gpu_hip, pl, max_extrema=cap)
    if delta >= 0:
        assert same(check(orc, ctx, pl), res0)
    else:
        capped_parity(full_ext, cap, ctx, 0.0, orc=orc, full_dev=full_dev)
        assert list(ctx.report().ext_ct)[:4] == [cap, LAYOUT[1], LAYOUT[2], LAYOUT[3]]
    for c in (ctx, ref):
        c.close()


def test_descriptor_capacity_switch(gpu_hip):
    assert gpu_hip.DEBUG_DESC_CAP == 12
    ctx = gpu_hip.Context()
    ctx.debug_set(gpu_hip.DEBUG_DESC_CAP, 0)
    ctx.debug_set(gpu_hip.DEBUG_DESC_CAP, 17)
    ctx.close()


@pytest.mark.parametrize("where", ["t-1", "t", "t+1", "inside"])
def test_descriptor_capacity(oracle_mod, gpu_hip, where):
    """DESC_CAP = T - 1 / T / T + 1 for T descriptors (desc_short flips at T), and a cap that falls between the
    orientations of one multi-orientation keypoint (k_scan_apply: idx + q >= desc_cap drops the tail of its run)"""
    pl, orc, ref, res0 = _reference(oracle_mod, gpu_hip)
    t = ref.report().ori_total
    if where == "inside":
        fh, _ = ref.fetch()
        multi = fh[fh["num_ori"] >= 2]
        assert len(multi) > 0
        cap = int(multi[len(multi) // 2]["desc_idx"][0]) + 1     # its first descriptor fits, the second does not
    else:
        cap = t + {"t-1": -1, "t": 0, "t+1": 1}[where]
    ctx = device_on(gpu_hip, pl, debug=((gpu_hip.DEBUG_DESC_CAP, cap),))
    assert same(check(orc, ctx, pl), res0)
    for c in (ctx, ref):
        c.close()


FMAX = 500


@pytest.mark.parametrize("sorting", [1, 2])
@pytest.mark.parametrize("extra", [0, 1])
def test_grid_filter_ten_percent_rule(oracle_mod, gpu_hip, sorting, extra):
    """totals of exactly int(filter_max * 1.1) (not filtered) and one more (filtered): filter.hip's s_active"""
    total = int(FMAX * 1.1) + extra
    kw = dict(filter_max_extrema=FMAX, filter_sorting=sorting, filter_grid_size=2)
    pl = planted(oracle_mod, split(total), seed=40 + extra, **kw)
    orc = oracle_on(oracle_mod, pl, **kw)
    ctx = device_on(gpu_hip, pl, **kw)
    n = sum(orc.ext_counts())
    if extra:
        assert 0 < n < total
    else:
        assert n == total
    check(orc, ctx)
    ctx.close()


@pytest.mark.parametrize("desc_mode", [0, 1, 2, 3, 4])
def test_descriptor_modes_at_the_seams(oracle_mod, gpu_hip, desc_mode):
    for i, total in enumerate([1, 64, 65, 256, 257, 2049]):
        kw = dict(desc_mode=desc_mode, norm_mode=(desc_mode + i) % 2)
        pl = planted(oracle_mod, split(total), seed=60 + total)
        orc = oracle_on(oracle_mod, pl, **kw)
        ctx = device_on(gpu_hip, pl, **kw)
        check(orc, ctx, pl, grid_mode=desc_mode == 2)
        ctx.close()
