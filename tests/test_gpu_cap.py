"""What survives a BINDING max_extrema cap.  Which extrema survive is arrival order (atomicAdd, a guarded store, a clamp:
s_extrema.cu:541,558), so the survivor SET is not reproducible -- but three facts are, and util.capped_parity checks
them: every octave's count is min(uncapped count, cap); every survivor is, bit for bit, an extremum of the uncapped set,
none twice; every survivor's orientations and descriptors are the oracle's for the same list (run_from_extrema) and,
bit for bit, the uncapped device run's for the same keypoint.

The code that only works when the cap binds: the guarded store in k_refine, the min(ext_ct[o], max_extrema) of every
consumer, the clamp the scan writes back, the recount in finish(), and the descriptor / histogram buffers sized from
the cap, which a dense capped image outgrows (grow and re-run)."""
import os

import numpy as np
import pytest

import order_rule as R
from popsift_amd.synth import synth
from util import _feature_frame, _keys, bits, capped_parity, sorted_features

pytestmark = pytest.mark.gpu

THREADS = min(os.cpu_count() or 4, 16)
# octave counts under the default params (oracle): 3822, 563, 43, 13, 1 -- octaves 0 and 1 bind at a cap of 300
DENSE = synth(21, 400, 300)

_uncapped = {}


def uncapped(O, hip, img, name, **kw):
    """(extrema, octave counts, (features, descriptors)) of the UNCAPPED device run of `img`.  Its extrema are the oracle's
    (octave, lpos and position bit for bit, sigma within 1e-5: the device's powf), which pins the set the survivors are
    checked against; the identity check itself is against the device's own extrema, sigma bit for bit."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _uncapped:
        orc = O.Oracle(O.default_params(**kw), threads=THREADS).run(img)
        ctx = hip.Context(hip.default_params(**kw))
        dev = ctx.submit(img).fetch()
        e_h = ctx.extrema()
        ctx.close()
        same_set(orc.extrema(), e_h)
        counts = orc.ext_counts()
        assert max(counts) < orc.params.max_extrema
        _uncapped[key] = (e_h, counts, dev)
    return _uncapped[key]


def same_set(e_o, e_h):
    """the oracle's and the device's extrema: the same (octave, lpos, x, y) bit for bit, sigma within 1e-5"""
    so = np.lexsort((bits(e_o["ypos"]), bits(e_o["xpos"]), e_o["lpos"], e_o["octave"]))
    sh = np.lexsort((bits(e_h["ypos"]), bits(e_h["xpos"]), e_h["lpos"], e_h["octave"]))
    a, b = e_o[so], e_h[sh]
    assert len(a) == len(b), "uncapped extrema: oracle %d, device %d" % (len(a), len(b))
    for f in ("octave", "lpos", "xpos", "ypos"):
        assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), "uncapped extrema differ in " + f
    rel = np.abs(a["sigma"].astype(np.float64) - b["sigma"]) / a["sigma"]
    assert rel.max(initial=0.0) < 1e-5, rel.max()


def _canon(feats, desc):
    f, d = sorted_features(feats, desc)
    return (f["debug_octave"].copy(), bits(f["xpos"]), bits(f["ypos"]), bits(f["sigma"]), f["num_ori"].copy(),
            bits(f["orientation"]), bits(d))


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def _capped_run(O, hip, img, cap, debug=(), **kw):
    ctx = hip.Context(hip.default_params(max_extrema=cap, **kw))
    for what, value in debug:
        ctx.debug_set(what, value)
    ctx.submit(img)
    orc = O.Oracle(O.default_params(max_extrema=cap, **kw), threads=THREADS).run(img, keypoints=False)
    return ctx, orc


@pytest.mark.parametrize("which", ["1", "13", "43", "300", "c0-1", "c0", "c0+1"])
def test_cap_boundaries(oracle_mod, gpu_hip, which):
    """Caps of 1, two small primes (13 and 43: exactly octaves 3's and 2's counts), 300 and octave 0's count - 1 / +0 / +1:
    off-by-ones in idx < max_extrema, in the clamp and in the scan's chunk count show here.  A cap at or above every
    octave's count binds nowhere: the result is the uncapped run's, bit for bit."""
    full_ext, counts, full_dev = uncapped(oracle_mod, gpu_hip, DENSE, "dense")
    c0 = counts[0]
    assert c0 == max(counts) and counts[1] > 300 and counts[2] == 43 and counts[3] == 13
    cap = {"c0-1": c0 - 1, "c0": c0, "c0+1": c0 + 1}.get(which) or int(which)
    ctx, orc = _capped_run(oracle_mod, gpu_hip, DENSE, cap)
    capped_parity(full_ext, cap, ctx, 1.0, orc=orc, full_dev=full_dev)
    if cap >= c0:
        assert _same(_canon(*ctx.fetch()), _canon(*full_dev))
    ctx.close()


@pytest.mark.parametrize("norm_mode", [0, 1])
@pytest.mark.parametrize("desc_mode", [0, 1, 2, 3, 4])
def test_every_descriptor_mode_at_a_binding_cap(oracle_mod, gpu_hip, desc_mode, norm_mode):
    kw = dict(desc_mode=desc_mode, norm_mode=norm_mode)
    full_ext, counts, full_dev = uncapped(oracle_mod, gpu_hip, DENSE, "dense", **kw)
    ctx, orc = _capped_run(oracle_mod, gpu_hip, DENSE, 300, **kw)
    capped_parity(full_ext, 300, ctx, 1.0, orc=orc, full_dev=full_dev, grid_mode=desc_mode == 2)
    ctx.close()


@pytest.mark.parametrize("sorting", [0, 1, 2])
def test_grid_filter_over_a_binding_cap(oracle_mod, gpu_hip, sorting):
    """The filter thins the capped list (sum of min(count, 300) = 657 > 1.1 * 300): the survivors are checked against
    the uncapped, UNFILTERED set, their total against sum(min(count, cap)), their parity through run_from_extrema."""
    full_ext, counts, full_dev = uncapped(oracle_mod, gpu_hip, DENSE, "dense")
    kw = dict(filter_max_extrema=300, filter_grid_size=4, filter_sorting=sorting)
    ctx, orc = _capped_run(oracle_mod, gpu_hip, DENSE, 300, **kw)
    capped_parity(full_ext, 300, ctx, 1.0, orc=orc, full_dev=full_dev, filtered=True)
    assert 0 < ctx.report().ext_total < sum(min(c, 300) for c in counts)
    ctx.close()


def test_raster_order_over_a_binding_cap(oracle_mod, gpu_hip):
    """The ordering pass on lists that the cap cut: its kernels size every octave's list by min(ext_ct[o], cap) while
    ext_ct[o] itself still holds the uncapped count.  The survivors pass capped_parity (counts equal min(count, cap)), and
    the extrema and the fetched feature records are in the order tests/order_rule.py defines for that survivor list."""
    full_ext, counts, full_dev = uncapped(oracle_mod, gpu_hip, DENSE, "dense")
    ctx = gpu_hip.Context(gpu_hip.default_params(max_extrema=300, feature_order=gpu_hip.ORDER_RASTER))
    ctx.submit(DENSE)
    orc = oracle_mod.Oracle(oracle_mod.default_params(max_extrema=300), threads=THREADS).run(DENSE, keypoints=False)
    capped_parity(full_ext, 300, ctx, 1.0, orc=orc, full_dev=full_dev)
    ext, (feats, _) = ctx.extrema(), ctx.fetch()
    ctx.close()
    assert len(ext) == sum(min(c, 300) for c in counts)
    assert ext.tobytes() == R.sort(ext).tobytes()
    o, x, y, s = _feature_frame(ext, 1.0)
    assert _keys(feats["debug_octave"], feats["xpos"], feats["ypos"], feats["sigma"]) == _keys(o, x, y, s)


def _ekeys(ext):
    return _keys(ext["octave"], ext["lpos"].view(np.float32), ext["xpos"], ext["ypos"], ext["sigma"])


def test_keep_strongest_over_a_binding_cap(oracle_mod, gpu_hip):
    """The keep-strongest pass on lists that the cap cut (n = 200 of the sum of min(count, 300) = 657 records): which
    records the cap leaves is arrival order, so the kept set is not reproducible, but every kept record is bit for bit an
    extremum of the uncapped run, none twice, with the response an uncapped run that keeps everything hands out for it; at
    least n are kept and fewer than n lie strictly above the smallest kept response (the header's tie rule, which needs no
    sight of the dropped records); no octave keeps more than min(count, cap)."""
    from collections import Counter
    full_ext, counts, _ = uncapped(oracle_mod, gpu_hip, DENSE, "dense")
    n, cap = 200, 300
    assert n < sum(min(c, cap) for c in counts) == 657
    every = gpu_hip.Context(gpu_hip.default_params()).set_keep_strongest(2 ** 31 - 1).submit(DENSE)
    ext_all, resp_all = every.extrema(), every.fetch_responses()
    every.close()
    assert Counter(_ekeys(ext_all)) == Counter(_ekeys(full_ext)) and np.isfinite(resp_all).all()
    want = dict(zip(_ekeys(ext_all), bits(resp_all).tolist()))     # records with equal keys are byte-identical

    ctx = gpu_hip.Context(gpu_hip.default_params(max_extrema=cap)).set_keep_strongest(n).submit(DENSE)
    ext, resp, rep = ctx.extrema(), ctx.fetch_responses(), ctx.report()
    ctx.close()
    keys = _ekeys(ext)
    full_count = Counter(_ekeys(full_ext))
    bad = [k for k, m in Counter(keys).items() if m > full_count.get(k, 0)]
    assert not bad, "kept records that are not uncapped extrema (or are repeated): %s" % bad[:10]
    assert bits(resp).tolist() == [want[k] for k in keys]
    assert len(ext) == len(resp) >= n
    assert int((resp > resp.min()).sum()) < n
    kept = np.bincount(ext["octave"], minlength=len(counts))
    assert len(kept) == len(counts) and all(kept[o] <= min(counts[o], cap) for o in range(len(counts))), kept
    assert list(rep.ext_ct[:len(counts)]) == kept.tolist() and rep.ext_total == len(ext)


def test_binding_cap_through_the_slow_detection_pass(oracle_mod, gpu_hip):
    """A 4-entry detection queue sends almost every strip through the slow pass, which changes arrival order most."""
    full_ext, counts, full_dev = uncapped(oracle_mod, gpu_hip, DENSE, "dense")
    ctx, orc = _capped_run(oracle_mod, gpu_hip, DENSE, 300, debug=((gpu_hip.DEBUG_DET_QCAP, 4),))
    capped_parity(full_ext, 300, ctx, 1.0, orc=orc, full_dev=full_dev)
    ctx.close()


def test_binding_cap_through_grow_and_rerun(oracle_mod, gpu_hip):
    """A cap of 50: 157 survivors with more than 2 * 50 orientations outgrow the descriptor buffer, and small candidate /
    histogram buffers outgrow theirs, so finish() grows them and re-runs the keypoint stages under a binding cap.  The
    descriptors handed out must belong to the extrema handed out."""
    full_ext, counts, full_dev = uncapped(oracle_mod, gpu_hip, DENSE, "dense")
    debug = ((gpu_hip.DEBUG_CAND_CAP, 256), (gpu_hip.DEBUG_OHIST_CAP, 100))
    ctx, orc = _capped_run(oracle_mod, gpu_hip, DENSE, 50, debug=debug)
    capped_parity(full_ext, 50, ctx, 1.0, orc=orc, full_dev=full_dev)
    rep = ctx.report()
    assert rep.ext_total > 100 and rep.ori_total > 2 * 50
    again = ctx.submit(DENSE)                                   # the grown buffers are kept
    capped_parity(full_ext, 50, again, 1.0, full_dev=full_dev)
    ctx.close()


def test_batch_with_mixed_binding(oracle_mod, gpu_hip):
    """One launch of four images, two of which bind at 300 and two not (a low-contrast copy: 225, 128, 4, 1 extrema, and
    a flat image).  Images that do not bind equal their own single submit bit for bit; images that bind pass
    capped_parity through fetch_item against their own uncapped single submit."""
    imgs = [DENSE, (synth(21, 400, 300).astype(np.float32) * 0.25 + 96).round().astype(np.uint8), synth(22, 400, 300),
            np.full((300, 400), 128, np.uint8)]
    cap = 300
    ctx = gpu_hip.Context(gpu_hip.default_params(max_extrema=cap))
    ctx.submit_batch(imgs)
    single = gpu_hip.Context(gpu_hip.default_params(max_extrema=cap))
    lifted = gpu_hip.Context()
    binds = []
    for k, im in enumerate(imgs):
        got = ctx.fetch_item(k)
        full_dev = lifted.submit(im).fetch()
        full_ext = lifted.extrema()
        counts = np.bincount(full_ext["octave"]) if len(full_ext) else np.zeros(1, np.int64)
        binds.append(bool(counts.max() > cap))
        if not binds[-1]:
            assert _same(_canon(*got), _canon(*single.submit(im).fetch())), k
            assert _same(_canon(*got), _canon(*full_dev)), k
        else:
            orc = oracle_mod.Oracle(oracle_mod.default_params(max_extrema=cap), threads=THREADS).run(im, keypoints=False)
            capped_parity(full_ext, cap, got, 1.0, orc=orc, full_dev=full_dev)
    assert binds == [True, False, True, False]
    for c in (ctx, single, lifted):
        c.close()


@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch4"])
def test_bench_4k_leg_as_it_runs(gpu_hip, batch):
    """bench.py's config-3 leg: synth 3840 x 2160 at the default Config (cap 100 000, 2x upscale), alone and as one launch
    of 4 images.  Octave 0 binds; every octave must hold min(uncapped, 100 000), every survivor must be an extremum of
    the uncapped device run (max_extrema 400 000, pinned to the oracle by test_config3_4k_against_oracle) and
    bit-identical to it.  No oracle run at this size."""
    seeds = [3, 4, 103, 104] if batch else [3]
    imgs = [synth(s, 3840, 2160) for s in seeds]
    cap = 100000
    ctx = gpu_hip.Context()
    assert ctx.params.max_extrema == cap
    if batch:
        ctx.submit_batch(imgs)
    else:
        ctx.submit(imgs[0])
    lifted = gpu_hip.Context(gpu_hip.default_params(max_extrema=400000))
    for k, im in enumerate(imgs):
        full_dev = lifted.submit(im).fetch()
        full_ext = lifted.extrema()
        counts = np.bincount(full_ext["octave"])
        assert counts[0] > cap and counts.max() < 400000, counts
        got = ctx.fetch_item(k) if batch else ctx
        capped_parity(full_ext, cap, got, 1.0, full_dev=full_dev)
        if batch:
            assert int((got[0]["debug_octave"] == 0).sum()) == cap
        else:
            assert ctx.report().ext_ct[0] == cap
        del full_dev, full_ext, got
    ctx.close()
    lifted.close()
