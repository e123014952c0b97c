"""popsift_hip_set_keep_strongest on the GPU (strongest.hip), held to tests/strongest_rule.py byte for byte: the responses,
the selection at every count where a workgroup of the pass fills, planted ties at the cut, and the same bytes in every
batch slot, under the debug switches, through grow-and-rerun and after switching the setting on one context."""
import ctypes as C

import numpy as np
import pytest

import order_rule as R
import planted as P
import strongest_rule as S
from popsift_amd import _capi
from popsift_amd.synth import synth

pytestmark = pytest.mark.gpu

CHUNK = _capi.STRONGEST_CHUNK
ALL = S.INT32_MAX
REC = ["debug_octave", "xpos", "ypos", "sigma", "num_ori", "orientation"]   # a feature without its descriptor indices
IMG = synth(21, 256, 192)


def raster(hip, **kw):
    return hip.default_params(feature_order=hip.ORDER_RASTER, **kw)


def context(hip, params, n=0, debug=()):
    ctx = hip.Context(params)
    for what, value in debug:
        ctx.debug_set(what, value)
    return ctx.set_keep_strongest(n) if n else ctx


class Result:
    """everything a finished image hands out (image k of the batch in `ctx`)"""

    def __init__(self, ctx, k=0, responses=True):
        self.feats, self.desc = ctx.fetch_item(k)
        self.u8 = ctx.fetch_item(k, "u8")[1]
        self.resp = ctx.fetch_responses(k) if responses else None
        if k == 0:
            self.ext = ctx.extrema()
            self.ext_ct = list(ctx.report().ext_ct)

    def same_bytes(self, other, what=""):
        assert self.feats.tobytes() == other.feats.tobytes(), what
        assert self.desc.tobytes() == other.desc.tobytes(), what
        assert self.u8.tobytes() == other.u8.tobytes(), what
        if self.resp is not None and other.resp is not None:
            assert self.resp.tobytes() == other.resp.tobytes(), what
        if hasattr(self, "ext") and hasattr(other, "ext"):
            assert self.ext.tobytes() == other.ext.tobytes(), what
            assert self.ext_ct == other.ext_ct, what


def assert_thinned(full, mask, got, ordered=True):
    """`got` is `full` (a run that kept everything, with responses) with the records outside `mask` removed: extrema,
    feature records, descriptors through desc_idx, byte descriptors, responses and the per-octave counts.  ordered=False:
    `got` is in arrival order, so only the SET of extrema is compared (in the rule's order)."""
    n_oct = len(full.ext_ct)
    assert got.ext_ct == np.bincount(full.ext["octave"][mask], minlength=n_oct).tolist()
    assert len(got.ext) == len(got.feats) == len(got.resp) == int(mask.sum())
    if not ordered:
        assert R.sort(got.ext).tobytes() == full.ext[mask].tobytes()
        return
    assert got.ext.tobytes() == full.ext[mask].tobytes()
    assert got.resp.tobytes() == full.resp[mask].tobytes()
    for name in REC:
        assert got.feats[name].tobytes() == full.feats[name][mask].tobytes(), name
    iw, ig = full.feats["desc_idx"][mask], got.feats["desc_idx"]
    assert np.array_equal(iw >= 0, ig >= 0)
    assert np.array_equal(ig[ig >= 0], np.arange(len(got.desc)))        # contiguous in list order
    assert got.desc[ig[ig >= 0]].tobytes() == full.desc[iw[iw >= 0]].tobytes()
    assert got.u8[ig[ig >= 0]].tobytes() == full.u8[iw[iw >= 0]].tobytes()


# ------------------------------------------------------------------------------------------------------- 1. responses

@pytest.mark.parametrize("sift_mode", [0, 1, 2])
def test_responses(gpu_hip, sift_mode):
    hip = gpu_hip
    off = context(hip, raster(hip, sift_mode=sift_mode)).submit(IMG)
    plain = Result(off, responses=False)
    off.close()
    ctx = context(hip, raster(hip, sift_mode=sift_mode), ALL).submit(IMG)
    got = Result(ctx)
    got.same_bytes(plain, "n = INT32_MAX changes no result byte")
    rep = ctx.report()
    levels = ctx.params.levels
    dims = [ctx.octave_dims(o) for o in range(rep.num_octaves)]
    want = S.responses(S.dog_planes(ctx, rep.num_octaves, levels), dims, got.ext, levels)
    ctx.close()
    assert len(want) > 500 and np.isfinite(want).all()
    assert got.resp.tobytes() == want.tobytes()
    if sift_mode == 0:
        # the population tests/test_strongest_rule.py describes on the oracle: both level clamps occur
        assert len(got.ext) == 1803 and got.ext["lpos"].min() == 0 and got.ext["lpos"].max() == levels + 1


def test_responses_with_stored_dog(gpu_hip):
    hip = gpu_hip
    res = []
    for store in (0, 1):
        ctx = context(hip, raster(hip, store_dog=store), ALL).submit(IMG)
        res.append(Result(ctx))
        ctx.close()
    res[1].same_bytes(res[0], "stored DoG planes and the on-the-fly difference")


# ------------------------------------------------------------------------------------------------------- 2. selection

@pytest.fixture(scope="module")
def full(gpu_hip):
    """the raster run of IMG that keeps everything, with its responses; never modified"""
    ctx = context(gpu_hip, raster(gpu_hip), ALL).submit(IMG)
    r = Result(ctx)
    ctx.close()
    assert len(r.ext) == 1803
    return r


@pytest.fixture(scope="module")
def contexts(gpu_hip):
    c = {"raster": gpu_hip.Context(raster(gpu_hip)), "arrival": gpu_hip.Context(gpu_hip.default_params())}
    yield c
    for v in c.values():
        v.close()


TOTAL = 1803
COUNTS = [1, 2, 63, 64, 65, 500, 1024, 1025, TOTAL - 1, TOTAL, TOTAL + 1]


@pytest.mark.parametrize("n", COUNTS)
def test_selection(full, contexts, n):
    mask = S.keep_mask(full.resp, n)
    assert int(mask.sum()) == min(n, TOTAL)             # no natural tie on these cuts (tests/test_strongest_rule.py)
    assert_thinned(full, mask, Result(contexts["raster"].set_keep_strongest(n).submit(IMG)))
    assert_thinned(full, mask, Result(contexts["arrival"].set_keep_strongest(n).submit(IMG)), ordered=False)


# -------------------------------------------------------------------------------------------------- 3, 4. planted lists

W = H = 570         # octaves 570, 285, 143, 72: octave 0's lattice holds 56 x 56 = 3136 sites >= 3 * CHUNK + 1
OCT = 4


class PlantedContexts:
    """one store_dog context per feature order on the planted size, reused over the layouts"""

    def __init__(self, hip, O):
        self.hip, self.dims = hip, P.octave_dims(O, W, H, OCT)
        self.ctx = {}
        for name, order in (("raster", hip.ORDER_RASTER), ("arrival", hip.ORDER_ARRIVAL)):
            ctx = hip.Context(hip.default_params(store_dog=1, feature_order=order, **P.params_kw(OCT)))
            ctx.submit(np.zeros((H, W), np.uint8)).wait()
            self.ctx[name] = ctx

    def upload(self, pl):
        for ctx in self.ctx.values():
            pl.upload(ctx)

    def run(self, name, n):
        return Result(self.ctx[name].set_keep_strongest(n).rerun_keypoint_stages())

    def close(self):
        for c in self.ctx.values():
            c.close()


@pytest.fixture(scope="module")
def planted(gpu_hip, oracle_mod):
    p = PlantedContexts(gpu_hip, oracle_mod)
    yield p
    p.close()


GROUPS, PER_GROUP = 40, 30


def tie_table():
    """GROUPS x PER_GROUP bumps in octave 0: the bumps of a group share a sub-pixel offset triple (multiples of 1 / 32:
    every centre and every plane value is then exact in float64, whatever the site and level), so their responses
    A - 4 (dx^2 + dy^2 + dz^2) are one float32 value; the triples' squared lengths differ, so the groups' values do."""
    steps = [(a, b, c) for a in range(2, 10) for b in range(2, 10) for c in range(2, 10)]
    seen, triples = set(), []
    for a, b, c in steps:
        if a * a + b * b + c * c not in seen:
            seen.add(a * a + b * b + c * c)
            triples.append((a / 32.0, -b / 32.0, c / 32.0))
    assert len(triples) >= GROUPS
    sites = P.lattice(W, H)[:GROUPS * PER_GROUP]
    i = np.arange(len(sites))
    off = np.array([triples[g] for g in i // PER_GROUP])
    return P.bump_table(sites[:, 0], sites[:, 1], 1 + i % 3, off, np.where(i % 2, 1, -1))


def test_planted_ties(planted):
    pl = P.Planted.from_tables(planted.dims, {0: tie_table()}, seed=7)
    planted.upload(pl)
    full = planted.run("raster", ALL)
    # through the rule, before anything is built on it: 1200 extrema, 40 distinct responses in groups of 30
    want = S.responses([pl.dog[o] for o in range(OCT)], planted.dims, full.ext, P.LEVELS)
    assert full.resp.tobytes() == want.tobytes()
    assert len(full.ext) == GROUPS * PER_GROUP and set(full.ext["lpos"].tolist()) == {1, 2, 3}
    vals, n = np.unique(want, return_counts=True)
    assert len(vals) == GROUPS and (n == PER_GROUP).all()
    for g in (0, 1, 7, 20, GROUPS - 1):
        n = PER_GROUP * g + PER_GROUP // 2              # the cut falls inside the (g + 1)-th strongest group
        mask = S.keep_mask(full.resp, n)
        assert int(mask.sum()) == PER_GROUP * (g + 1), g
        assert_thinned(full, mask, planted.run("raster", n))
        assert_thinned(full, mask, planted.run("arrival", n), ordered=False)


EDGES = [0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 1]
LAYOUTS = [{0: c, 1: 70, 2: 9} for c in EDGES] + [{3: 1}]


def layout_id(i):
    return "-".join("%d:%d" % kv for kv in sorted(LAYOUTS[i].items()))


@pytest.mark.parametrize("i", range(len(LAYOUTS)), ids=layout_id)
def test_chunk_edges(planted, i):
    pl = P.Planted(planted.dims, LAYOUTS[i], seed=300 + i)
    planted.upload(pl)
    full = planted.run("raster", ALL)
    assert full.ext_ct[:OCT] == [LAYOUTS[i].get(o, 0) for o in range(OCT)]
    want = S.responses([pl.dog[o] for o in range(OCT)], planted.dims, full.ext, P.LEVELS)
    assert full.resp.tobytes() == want.tobytes()
    for n in sorted({max(pl.total // 2, 1), 1}):        # a total of 1 has no half: n = 0 would switch the pass off
        mask = S.keep_mask(full.resp, n)
        assert n <= int(mask.sum()) <= pl.total
        assert_thinned(full, mask, planted.run("raster", n))
        assert_thinned(full, mask, planted.run("arrival", n), ordered=False)


# ---------------------------------------------------------------------------------------------- 5. same bytes elsewhere

KEEP = 500


@pytest.fixture(scope="module")
def kept(gpu_hip, full):
    """the raster run of IMG with n = KEEP, checked against the rule; never modified"""
    ctx = context(gpu_hip, raster(gpu_hip), KEEP).submit(IMG)
    r = Result(ctx)
    ctx.close()
    assert_thinned(full, S.keep_mask(full.resp, KEEP), r)
    return r


def test_same_bytes_in_a_batch(gpu_hip, kept):
    imgs = [synth(30 + k, 256, 192) for k in range(16)]
    for k in (0, 7, 15):
        imgs[k] = IMG
    ctx = context(gpu_hip, raster(gpu_hip), KEEP).submit_batch(imgs)
    for k in (0, 7, 15):
        Result(ctx, k).same_bytes(kept, "slot %d" % k)
    ctx.close()


SWITCHES = {
    "det_qcap": ((_capi.DEBUG_DET_QCAP, 4),),
    "kp_waves": ((_capi.DEBUG_KP_WAVES, 32),),
    "blur_path": ((_capi.DEBUG_BLUR_PATH, 2),),
    "grow_rerun": ((_capi.DEBUG_CAND_CAP, 256), (_capi.DEBUG_OHIST_CAP, 100), (_capi.DEBUG_DESC_CAP, 64)),
}


@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_same_bytes_under_debug_switches(gpu_hip, kept, name):
    ctx = context(gpu_hip, raster(gpu_hip), KEEP, SWITCHES[name]).submit(IMG)
    Result(ctx).same_bytes(kept, name)
    ctx.close()


def test_same_bytes_after_rerun_and_switching(gpu_hip, full, kept):
    hip = gpu_hip
    ctx = context(hip, raster(hip), KEEP).submit(IMG)
    Result(ctx).same_bytes(kept, "first submit")
    Result(ctx.rerun_keypoint_stages()).same_bytes(kept, "rerun_keypoint_stages")
    # the setting is taken at the rerun, too
    assert_thinned(full, S.keep_mask(full.resp, 64), Result(ctx.set_keep_strongest(64).rerun_keypoint_stages()))
    assert_thinned(full, S.keep_mask(full.resp, 1025), Result(ctx.set_keep_strongest(1025).submit(IMG)))
    Result(ctx.set_keep_strongest(KEEP).submit(IMG)).same_bytes(kept, "back to KEEP")
    # off again: the plain run's bytes, and no responses
    plain = Result(ctx.set_keep_strongest(0).submit(IMG), responses=False)
    assert plain.feats.tobytes() == full.feats.tobytes() and plain.desc.tobytes() == full.desc.tobytes()
    assert plain.ext.tobytes() == full.ext.tobytes() and plain.ext_ct == full.ext_ct
    with pytest.raises(hip.PopsiftHipError) as e:
        ctx.fetch_responses()
    assert e.value.status == hip.ERR_STATE
    ctx.close()


# ------------------------------------------------------------------------------------------------ 6. errors and empties

def test_empty_image(gpu_hip):
    ctx = context(gpu_hip, raster(gpu_hip), 10).submit(np.zeros((96, 128), np.uint8))
    assert ctx.wait() == (0, 0)
    assert len(ctx.fetch_responses()) == 0 and len(ctx.extrema()) == 0
    ctx.close()


def test_setter_errors(gpu_hip):
    hip = gpu_hip
    ctx = hip.Context(hip.default_params())
    with pytest.raises(hip.PopsiftHipError) as e:
        ctx.set_keep_strongest(-1)
    assert e.value.status == hip.ERR_INVALID
    ctx.set_keep_strongest(2).submit(IMG)
    with pytest.raises(hip.PopsiftHipError) as e:       # not waited for: the batch is in flight
        ctx.set_keep_strongest(6)
    assert e.value.status == hip.ERR_STATE
    assert ctx.wait()[0] == 2
    ctx.set_keep_strongest(6)
    ctx.close()
    filt = hip.Context(hip.default_params(filter_max_extrema=100))
    with pytest.raises(hip.PopsiftHipError) as e:
        filt.set_keep_strongest(5)
    assert e.value.status == hip.ERR_INVALID
    filt.close()


def test_fetch_errors(gpu_hip, kept):
    hip = gpu_hip
    L = hip.lib()
    ctx = context(hip, raster(hip), KEEP).submit(IMG)
    nf = ctx.wait()[0]
    buf = np.zeros(nf, np.float32)
    assert L.popsift_hip_fetch_responses_item(ctx._h, 0, buf.ctypes.data, nf - 1) == hip.ERR_TOO_SMALL
    assert L.popsift_hip_fetch_responses_item(ctx._h, 1, buf.ctypes.data, nf) == hip.ERR_INVALID
    assert L.popsift_hip_fetch_responses_item(ctx._h, 0, buf.ctypes.data, nf) == hip.OK
    assert buf.tobytes() == kept.resp.tobytes()
    p = C.c_void_p()
    assert L.popsift_hip_responses_dev_item(ctx._h, 0, C.byref(p)) == hip.OK and p.value
    # a describe ignores the setting and has no responses
    fr = np.zeros(3, hip.FRAME_DTYPE)
    fr["xpos"], fr["ypos"], fr["sigma"] = [40, 90, 150], [30, 80, 120], [2.0, 3.0, 4.0]
    fr["octave"] = fr["level"] = -1
    f, d = ctx.describe(IMG, fr)
    assert len(f) == 3 and (f["num_ori"] > 0).all()
    assert L.popsift_hip_fetch_responses_item(ctx._h, 0, buf.ctypes.data, nf) == hip.ERR_STATE
    ctx.close()


def test_thinned_result_down_the_chain(gpu_hip, kept):
    hip = gpu_hip
    a = context(hip, raster(hip), KEEP).submit(IMG)
    b = context(hip, raster(hip), KEEP).submit(np.roll(IMG, (4, 8), axis=(0, 1)))
    A, B = a.clone_results(), b.clone_results()
    d, rev = A.download()
    assert d.tobytes() == kept.desc.tobytes()
    assert len(rev) == len(kept.desc) and 0 <= rev.min() and rev.max() < len(kept.feats)
    pairs = A.match_pairs(B, cross_check=True)
    assert len(pairs) > 50
    for x in (A, B, a, b):
        x.close()
