"""tests/strongest_rule.py on hand-made arrays and on the CPU oracle's output for the image the GPU tests use, and the
two new entry points' argument checks that need no GPU."""
import ctypes as C

import numpy as np
import pytest

import strongest_rule as S
from popsift_amd.synth import synth

NAN, INF = np.float32(np.nan), np.float32(np.inf)


def f32(*v):
    return np.array(v, np.float32)


# ------------------------------------------------------------------------------------------------------------ the rule

def test_keys():
    k = S.keys(f32(0.0, 1.0, 2.5, INF, NAN, 1e-45))
    assert k.dtype == np.uint32
    assert k[0] == 0 and k[4] == 0                      # NaN shares the lowest key with 0.0
    assert k[5] == 1                                    # the smallest denormal
    assert k[3] == 0x7f800000 and k[3] == k.max()       # +inf is the highest
    assert k[1] < k[2] < k[3]


def test_nan_goes_first_inf_last():
    r = f32(3.0, NAN, INF, 1.0)
    assert S.keep_mask(r, 1).tolist() == [False, False, True, False]
    assert S.keep_mask(r, 2).tolist() == [True, False, True, False]
    assert S.keep_mask(r, 3).tolist() == [True, False, True, True]


@pytest.mark.parametrize("total", [1, 2, 7, 64])
def test_counts_around_total(total):
    r = np.random.default_rng(total).permutation(total).astype(np.float32) + np.float32(1.0)   # distinct, positive
    assert S.keep_mask(r, 1).sum() == 1 and S.keep_mask(r, 1)[np.argmax(r)]
    if total > 1:
        m = S.keep_mask(r, total - 1)
        assert m.sum() == total - 1 and not m[np.argmin(r)]
    assert S.keep_mask(r, total).all()
    assert S.keep_mask(r, total + 1).all()
    assert S.keep_mask(r, S.INT32_MAX).all()


def test_threshold_zero_keeps_all():
    r = f32(5.0, 0.0, NAN, 0.0, 2.0)                    # the 3rd largest key is 0: every record has key >= 0
    assert S.keep_mask(r, 3).all()
    assert S.keep_mask(r, 2).tolist() == [True, False, False, False, True]


def test_tie_group_straddling_the_cut_is_kept_whole():
    r = f32(9.0, 4.0, 7.0, 4.0, 4.0, 1.0, 4.0)
    for n in (3, 4, 5, 6):                              # the cut falls inside the group of four 4.0
        assert S.keep_mask(r, n).tolist() == [True, True, True, True, True, False, True]
    assert S.keep_mask(r, 2).sum() == 2
    # the set does not depend on the order of the records
    p = np.random.default_rng(0).permutation(len(r))
    assert np.array_equal(S.keep_mask(r[p], 4), S.keep_mask(r, 4)[p])


def test_n_below_one_is_refused():
    with pytest.raises(ValueError):
        S.keep_mask(f32(1.0), 0)


def test_response_samples_and_clamps():
    w, h, levels = 6, 5, 3
    planes = [[np.arange(h * w, dtype=np.float32).reshape(h, w) * (1 if d % 2 else -1) + 100 * d for d in range(levels + 2)]]
    ext = np.zeros(7, [("xpos", np.float32), ("ypos", np.float32), ("lpos", np.int32), ("sigma", np.float32),
                       ("octave", np.int32), ("cell", np.int32)])
    ext["xpos"] = [2.49, 2.5, 0.0, 5.4, 9.0, NAN, 1.0]
    ext["ypos"] = [1.0, 1.5, 0.4, 3.6, -3.0, 1.0, INF]
    ext["lpos"] = [1, 2, 0, 4, 3, 1, 1]
    got = S.responses(planes, [(w, h)], ext, levels)
    D = lambda x, y, d: np.abs(planes[0][d][y, x])
    assert got[0] == D(2, 1, 1)
    assert got[1] == D(3, 2, 2)                         # halves round up: floor(v + 0.5)
    assert got[2] == D(0, 0, 1)                         # lpos 0 reads level 1
    assert got[3] == D(5, 4, 3)                         # lpos 4 reads level `levels`
    assert got[4] == D(5, 0, 3)                         # positions clamp to the plane
    assert np.isnan(got[5]) and np.isnan(got[6])
    assert got.dtype == np.float32 and (got[:5] >= 0).all()


# ---------------------------------------------------------------------------------------- the oracle on the test image

IMG = synth(21, 256, 192)
COUNTS = [1, 2, 63, 64, 65, 500, 1024, 1025, 1802]


@pytest.fixture(scope="module")
def oracle_run(oracle_mod):
    """(extrema, responses, DoG planes, Gaussian planes) of the oracle on IMG; never modified"""
    O = oracle_mod
    orc = O.Oracle(O.default_params()).run(IMG)
    n_oct, levels = orc.num_octaves, orc.params.levels
    dims = [orc.octave_dims(o) for o in range(n_oct)]
    dog = S.dog_planes(orc, n_oct, levels)
    gauss = [[orc.plane(o, 0, z) for z in range(levels + 3)] for o in range(n_oct)]
    ext = orc.extrema()
    resp = S.responses(dog, dims, ext, levels)
    orc.close()
    return ext, resp, dog, gauss


def test_oracle_population(oracle_run):
    ext, resp, dog, gauss = oracle_run
    assert len(ext) == 1803
    assert np.bincount(ext["octave"]).tolist()[:4] == [1543, 240, 14, 6] and ext["octave"].max() == 3
    assert np.isfinite(resp).all()
    assert 3.19 < resp.min() < 3.20 and 21.6 < resp.max() < 21.8, (resp.min(), resp.max())
    vals, n = np.unique(resp, return_counts=True)
    assert len(vals) == 1801 and n.max() == 2
    # the level clamp works on real records: refinement hands out lpos 0 and levels + 1
    assert ext["lpos"].min() == 0 and ext["lpos"].max() == 4
    assert int(((ext["lpos"] < 1) | (ext["lpos"] > 3)).sum()) == 25


def test_stored_dog_is_the_difference_of_its_neighbours(oracle_run):
    _, _, dog, gauss = oracle_run
    for o in range(len(dog)):
        for d in range(len(dog[o])):
            assert (gauss[o][d + 1] - gauss[o][d]).tobytes() == dog[o][d].tobytes(), (o, d)


@pytest.mark.parametrize("n", COUNTS)
def test_oracle_kept_count(oracle_run, n):
    _, resp, _, _ = oracle_run
    m = S.keep_mask(resp, n)
    assert int(m.sum()) == n                            # no natural tie sits on any of these cuts
    assert resp[m].min() > resp[~m].max()


# ------------------------------------------------------------------------------------------- argument checks, no GPU

def test_null_context_is_invalid(hip):
    L = hip.lib()
    assert L.popsift_hip_set_keep_strongest(None, 1) == hip.ERR_INVALID
    buf = (C.c_float * 4)()
    assert L.popsift_hip_fetch_responses_item(None, 0, buf, 4) == hip.ERR_INVALID
    p = C.c_void_p()
    assert L.popsift_hip_responses_dev_item(None, 0, C.byref(p)) == hip.ERR_INVALID
    assert hip.STRONGEST_CHUNK == 1024
