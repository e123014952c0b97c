"""k_orientation walks the keypoint lists in GROUPS of 16 consecutive entries (keypoint.hip: KP_GROUP; one wave per group,
the peak search of the group's 16 histograms in one epilogue, four lanes per extremum, the group's Ext records and its
partial sum for k_scan_apply).  The counts and capacities at which a group is empty, partial, exactly full or split:

  - extremum counts 0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257 (one entry, one short of / exactly / one past one and two
    groups and one k_scan_apply chunk of 16 groups);
  - a group that holds the last entries of one octave and the first of the next, the boundary at positions 5 and 9;
  - DEBUG_OHIST_CAP inside a group, at a group's end and one past it: the first pass gives the entries from the cap on
    their record but no orientation (not visible from outside: finish() raises the cap and re-runs), the re-run's
    result is the uncapped run's;
  - DEBUG_KP_WAVES 32 and 64: eight waves, every one walks many groups;
  - a batch of two images with 17 and 256 entries;
  - the describe path with computed orientations and with given ones (k_frame_place writes the records and partial
    sums k_orientation would) at 15, 16 and 17 frames.
Planted scale spaces (tests/planted.py, 480 x 480, four octaves) against the oracle on the same planes as in
test_gpu_count_edges.py: extrema bit-exact, feature_parity, report() counts, the layout contract (`check`).  Planes can
be planted in image 0 of a context only, so the batch and the describe cases take their exact counts from caller-supplied
frames, the batch against single runs bit for bit, the describes against the extraction they came from bit for bit and
(computed orientations) against the oracle on the same extrema."""
import os

import numpy as np
import pytest

from popsift_amd.synth import synth
from test_gpu_count_edges import check, device_on, oracle_on, planted, same, split
from test_gpu_describe import _extract, _frames
from util import bits, feature_parity

pytestmark = pytest.mark.gpu

GROUP = 16          # keypoint_dev.h KP_GROUP
THREADS = min(os.cpu_count() or 4, 16)


@pytest.mark.parametrize("total", [0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257])
def test_counts_around_whole_groups(oracle_mod, gpu_hip, total):
    pl = planted(oracle_mod, split(total), seed=100 + total)
    assert pl.total == total
    orc = oracle_on(oracle_mod, pl)
    ctx = device_on(gpu_hip, pl)
    check(orc, ctx, pl)
    ctx.close()


@pytest.mark.parametrize("first", [5, 2 * GROUP + 9])
def test_a_group_across_an_octave_boundary(oracle_mod, gpu_hip, first):
    pl = planted(oracle_mod, {0: first, 1: 30, 2: 7}, seed=first)
    # the group that holds the boundary has entries of octave 0 below position `first % 16` and of octave 1 from there on
    assert pl.counts[0] % GROUP in (5, 9) and pl.counts[1] >= GROUP
    orc = oracle_on(oracle_mod, pl)
    ctx = device_on(gpu_hip, pl)
    check(orc, ctx, pl)
    ctx.close()


@pytest.fixture(scope="module")
def forty(oracle_mod, gpu_hip):
    """40 extrema (two and a half groups), the oracle on them and the device's uncapped result"""
    pl = planted(oracle_mod, {0: 28, 1: 12}, seed=40)
    assert pl.total == 40
    orc = oracle_on(oracle_mod, pl)
    ctx = device_on(gpu_hip, pl)
    res = check(orc, ctx, pl)
    ctx.close()
    return pl, orc, res


@pytest.mark.parametrize("cap", [8, 16, 17])
def test_orientation_capacity_inside_and_at_the_end_of_a_group(gpu_hip, forty, cap):
    pl, orc, res0 = forty
    assert cap < pl.total and {8: cap % GROUP != 0, 16: cap % GROUP == 0, 17: cap % GROUP == 1}[cap]
    ctx = device_on(gpu_hip, pl, debug=((gpu_hip.DEBUG_OHIST_CAP, cap),))
    assert same(check(orc, ctx, pl), res0)
    ctx.close()


def test_few_waves_walk_many_groups(oracle_mod, gpu_hip):
    total = 2049                          # 129 groups in nine chunks of 256: XCD 0 takes chunks 0 and 8
    pl = planted(oracle_mod, split(total), seed=9)
    assert pl.total == total
    orc = oracle_on(oracle_mod, pl)
    res = []
    for waves in (None, 32, 64):
        debug = () if waves is None else ((gpu_hip.DEBUG_KP_WAVES, waves),)
        ctx = device_on(gpu_hip, pl, debug=debug)
        res.append(check(orc, ctx, pl))
        ctx.close()
    assert same(res[1], res[0]) and same(res[2], res[0])


@pytest.fixture(scope="module")
def extracted(gpu_hip):
    """two images, their extraction, and one frame per feature (computed orientations) / per descriptor (given)"""
    out = []
    for seed in (5, 6):
        img = synth(seed, 320, 240)
        feats, desc, ext = _extract(gpu_hip, img)
        assert len(feats) >= 256 and len(np.unique(feats["debug_octave"])) >= 3
        out.append((img, feats, desc, ext))
    return out


def _spread(n_all, n):
    """n list positions spread over the whole list, so that the frames fall into several octaves"""
    return np.unique(np.linspace(0, n_all - 1, n).astype(int))


def test_a_batch_of_17_and_256(gpu_hip, extracted):
    hip = gpu_hip
    imgs, lists = [], []
    for (img, feats, desc, ext), n in zip(extracted, (17, 256)):
        pick = _spread(len(feats), n)
        assert len(pick) == n
        fr, _ = _frames(hip, feats[pick], ext[pick], False)
        assert len(fr) == n
        imgs.append(img)
        lists.append(fr)
    ctx = hip.Context(hip.default_params())
    got = ctx.describe_batch(imgs, lists, "compute")
    ctx.close()
    for k in range(2):
        one = hip.Context(hip.default_params())
        f, d = one.describe(imgs[k], lists[k], "compute")
        one.close()
        assert len(f) == len(lists[k]) and f["num_ori"].sum() == len(d) > 0
        for name in ("xpos", "ypos", "sigma", "orientation"):
            assert np.array_equal(bits(got[k][0][name]), bits(f[name])), (k, name)
        assert np.array_equal(got[k][0]["num_ori"], f["num_ori"]) and np.array_equal(got[k][0]["desc_idx"], f["desc_idx"])
        assert np.array_equal(bits(got[k][1]), bits(d)), k


@pytest.mark.parametrize("n", [15, 16, 17])
def test_describe_with_computed_orientations(gpu_hip, oracle_mod, extracted, n):
    hip, O = gpu_hip, oracle_mod
    img, feats, desc, ext = extracted[0]
    pick = _spread(len(feats), n)
    fr, _ = _frames(hip, feats[pick], ext[pick], False)
    assert len(fr) == n and len(np.unique(fr["octave"])) >= 2
    ctx = hip.Context(hip.default_params())
    cf, cd = ctx.describe(img, fr, "compute")
    e = ctx.extrema()
    assert len(cf) == n == len(e) == ctx.report().ext_total
    # the extraction the frames came from, bit for bit
    sel = feats[pick]
    assert np.array_equal(cf["num_ori"], sel["num_ori"])
    assert np.array_equal(bits(cf["orientation"]), bits(sel["orientation"]))
    for f, g in zip(cf, sel):
        k = int(f["num_ori"])
        assert np.array_equal(bits(cd[f["desc_idx"][:k]]), bits(desc[g["desc_idx"][:k]]))
    assert len(cd) == sel["num_ori"].sum()
    # the oracle on the same extrema
    orc = O.Oracle(O.default_params(), threads=THREADS).run(img, keypoints=False).run_from_extrema(e)
    ok, msg, _ = feature_parity(orc, cf, cd)
    assert ok, msg
    ctx.close()


@pytest.mark.parametrize("n", [15, 16, 17])
def test_describe_with_given_orientations(gpu_hip, extracted, n):
    """k_frame_place writes what k_orientation would: one descriptor per frame, idx_ori local to the group of 16"""
    hip = gpu_hip
    img, feats, desc, ext = extracted[0]
    fr_all, src_all = _frames(hip, feats, ext, True)
    pick = _spread(len(fr_all), n)
    fr, src = fr_all[pick], [src_all[i] for i in pick]
    assert len(fr) == n and len(np.unique(fr["octave"])) >= 2
    ctx = hip.Context(hip.default_params())
    df, dd = ctx.describe(img, fr, "given")
    assert len(df) == n == len(dd) and (df["num_ori"] == 1).all()
    assert np.array_equal(np.sort(df["desc_idx"][:, 0]), np.arange(n))
    assert np.array_equal(bits(df["orientation"][:, 0]), bits(fr["orientation"]))
    want = np.array([desc[feats[g]["desc_idx"][k]] for g, k in src])
    assert np.array_equal(bits(dd[df["desc_idx"][:, 0]]), bits(want))
    ctx.close()
