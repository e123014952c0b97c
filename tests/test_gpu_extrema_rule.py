"""k_detect and k_refine against the float64 rule, branch by branch: the planted cases of
tests/extrema_cases.py through BOTH detection routes -- store_dog = 1 with uploaded DoG planes (k_detect / k_refine with
FLY = false) and store_dog = 0 with uploaded Gaussian planes that subtract back to the same DoG planes bit for bit (FLY =
true, the default and benchmarked kernels) -- then rerun_keypoint_stages().  Per route: the extrema are the oracle's as
bits and the rule's within the measured bar, one to one; the two routes give the same bytes; report().ext_ct are the
rule's counts; fetch() returns one feature per extremum.  Nothing is asserted about orientations or descriptors."""
import numpy as np
import pytest

import extrema_cases as X
import extrema_rule as R
from extrema_cases import MODE_ID, MODES, POS_BAR, SET_ID, SETS, SIGMA_BAR, oracle_on
from util import bits

pytestmark = pytest.mark.gpu

ZERO = np.zeros((X.IMG_H, X.IMG_W), np.uint8)


def canon(e):
    """the extrema in a defined order (the device appends them in no fixed one)"""
    order = np.lexsort((bits(e["ypos"]), bits(e["xpos"]), e["lpos"], e["octave"]))
    return e[order]


def key(e):
    return list(zip(e["octave"].tolist(), e["lpos"].tolist(), bits(e["xpos"]).tolist(), bits(e["ypos"]).tolist(),
                    e["cell"].tolist()))


def context(hip, cs, store_dog, debug=(), batch=1):
    ctx = hip.Context(hip.default_params(store_dog=store_dog, **X.params_kw(cs.mode, cs.levels)))
    for what, value in debug:
        ctx.debug_set(what, value)
    if batch == 1:
        ctx.submit(ZERO).wait()
    else:
        ctx.submit_batch([ZERO] * batch).wait_batch()
    assert [tuple(ctx.octave_dims(o)) for o in range(ctx.report().num_octaves)] == cs.dims
    return ctx


def run_route(ctx, cs, store_dog):
    (cs.upload_dog_route if store_dog else cs.upload_gauss_route)(ctx)
    ctx.rerun_keypoint_stages()
    return canon(ctx.extrema())


def check_route(cs, eo, ctx, e, what):
    # 1. the oracle's, as bits
    assert key(e) == key(eo), "%s: oracle %d extrema, device %d" % (what, len(eo), len(e))
    assert np.all(np.abs(e["sigma"].astype(np.float64) - eo["sigma"]) <= SIGMA_BAR * eo["sigma"])
    # 2. the rule's, one to one under the measured bar
    bad, worst, worst_s = X.match(cs.extrema, e)
    print("%s: %d extrema, largest distance to the rule %.3e px, sigma %.3e" % (what, len(e), worst, worst_s))
    assert not bad, what + "\n" + "\n".join(bad[:20])
    assert worst <= POS_BAR and worst_s <= SIGMA_BAR, (what, worst, worst_s)
    # 4. the counts per octave
    rep = ctx.report()
    n = len(cs.dims)
    assert rep.num_octaves == n and list(rep.ext_ct) == cs.counts + [0] * (len(rep.ext_ct) - n), (what, list(rep.ext_ct))
    # 5. one feature per extremum
    feats, _ = ctx.fetch()
    assert len(feats) == len(e) == sum(cs.counts)


def both_routes(O, hip, cs, debug=(), what=""):
    eo = canon(oracle_on(O, cs).extrema())
    got = {}
    for store_dog in (1, 0):
        ctx = context(hip, cs, store_dog, debug)
        got[store_dog] = run_route(ctx, cs, store_dog)
        check_route(cs, eo, ctx, got[store_dog], "%s store_dog=%d" % (what, store_dog))
        ctx.close()
    # 3. the same bytes from the stored and the on-the-fly kernels
    assert got[0].tobytes() == got[1].tobytes()


@pytest.mark.parametrize("cset", SETS, ids=SET_ID)
def test_device_equals_rule_on_both_routes(oracle_mod, gpu_hip, cset):
    """levels 3: every family; levels 2 and 9 (another NP, another top plane): the random family and the top-plane guard"""
    both_routes(oracle_mod, gpu_hip, X.case_set(*cset), what=SET_ID(cset))


@pytest.mark.parametrize("mode", MODES, ids=MODE_ID)
def test_seams_through_the_slow_pass(oracle_mod, gpu_hip, mode):
    """DET_QCAP = 0: the fast pass may queue nothing, every strip that holds a candidate is redone by the SLOW pass"""
    cs = X.case_set(mode, "seams")
    both_routes(oracle_mod, gpu_hip, cs, debug=((gpu_hip.DEBUG_DET_QCAP, 0),), what=R.MODE_NAMES[mode] + " slow")


@pytest.mark.parametrize("store_dog", [1, 0])
def test_two_case_sets_in_turn_in_a_batch_context(oracle_mod, gpu_hip, store_dog):
    """A context that has run a batch of two: the upload hook reaches slot 0 only, so this slice runs on slot 0 -- two
    different case sets one after the other through the batch's launch shape (blockIdx.y = 2), the second over the first's
    counters and candidate lists; slot 1 stays the empty image it was."""
    ctx = None
    for kind in ("rare", "guards"):
        cs = X.case_set(R.POPSIFT, kind)
        eo = canon(oracle_on(oracle_mod, cs).extrema())
        if ctx is None:
            ctx = context(gpu_hip, cs, store_dog, batch=2)
        e = run_route(ctx, cs, store_dog)
        check_route(cs, eo, ctx, e, "batch %s store_dog=%d" % (kind, store_dog))
        assert ctx.wait_batch()[1] == (0, 0)
    ctx.close()
