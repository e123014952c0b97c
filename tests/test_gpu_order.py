"""POPSIFT_HIP_ORDER_RASTER on the GPU (order.hip): the lists obey tests/order_rule.py, the result is the arrival-order
run's permuted accordingly, and its bytes repeat -- on every run, in every batch slot, under every debug switch, at the
counts where the pass's workgroups fill, with long buckets, with the grid filter, and down the match / verify chain."""
import numpy as np
import pytest

import order_rule as R
import planted as P
from popsift_amd import _capi
from popsift_amd.synth import synth

pytestmark = pytest.mark.gpu

CHUNK = _capi.ORDER_CHUNK
REC = ["debug_octave", "xpos", "ypos", "sigma", "num_ori", "orientation"]   # a feature without its descriptor indices


def raster(hip, **kw):
    return hip.default_params(feature_order=hip.ORDER_RASTER, **kw)


def run(hip, img, params, debug=()):
    ctx = hip.Context(params)
    for what, value in debug:
        ctx.debug_set(what, value)
    return ctx.submit(img)


def snapshot(ctx, k=0):
    """every result byte of image k: feature records, float descriptors, byte descriptors, the byte clone and its reverse
    map; for image 0 also the float clone and its reverse map"""
    feats, desc = ctx.fetch_item(k)
    feats8, desc8 = ctx.fetch_item(k, "u8")
    assert feats8.tobytes() == feats.tobytes()
    out = {"feats": feats.tobytes(), "desc": desc.tobytes(), "u8": desc8.tobytes()}
    b = ctx.clone_results_u8(k)
    d, rev = b.download()
    out["clone_u8"], out["rev_u8"] = d.tobytes(), rev.tobytes()
    b.close()
    if k == 0:
        c = ctx.clone_results()
        d, rev = c.download()
        out["clone"], out["rev"] = d.tobytes(), rev.tobytes()
        c.close()
    return out


def assert_same(a, b, what=""):
    for key in a:
        if key in b:
            assert a[key] == b[key], (what, key)


def assert_permuted(ext_a, fa, da, ext_r, fr, dr):
    """the raster run (ext_r, fr, dr) is the arrival run (ext_a, fa, da) in the rule's order, as bytes"""
    assert len(ext_a) == len(fa) and len(ext_r) == len(fr) == len(fa) and len(dr) == len(da)
    perm = R.permutation(ext_a)
    assert ext_r.tobytes() == ext_a[perm].tobytes()
    for name in REC:
        assert fr[name].tobytes() == fa[name][perm].tobytes(), name
    # descriptors through desc_idx; the raster run's own indices are contiguous in list order
    ia, ir = fa["desc_idx"][perm], fr["desc_idx"]
    assert np.array_equal(ia >= 0, ir >= 0)
    assert np.array_equal(ir[ir >= 0], np.arange(len(dr)))
    assert dr[ir[ir >= 0]].tobytes() == da[ia[ia >= 0]].tobytes()


# ---------------------------------------------------------------------------------------------------------------- 1, 2

IMG = synth(21, 256, 192)


@pytest.fixture(scope="module")
def reference(gpu_hip):
    """the raster run every other run is held to, with its extrema; never modified"""
    ctx = run(gpu_hip, IMG, raster(gpu_hip))
    ref = snapshot(ctx)
    ext = ctx.extrema()
    ctx.close()
    return ref, ext


def test_rule(gpu_hip, reference):
    hip = gpu_hip
    ref, ext_r = reference
    a = run(hip, IMG, hip.default_params())
    ext_a = a.extrema()
    fa, da = a.fetch()
    a.close()
    n0 = int((ext_a["octave"] == 0).sum())
    # 1803 extrema, 1543 of them in octave 0: two workgroups of the pass and seven 256-candidate refinement steps there
    # (the planted layouts below go to 3 * CHUNK + 1)
    assert len(ext_a) > 1500 and n0 > CHUNK + 256, (len(ext_a), n0)
    assert not R.is_ordered(ext_a)                                  # the arrival run is what the pass has to change
    assert R.is_ordered(ext_r)
    fr = np.frombuffer(ref["feats"], hip.FEATURE_DTYPE)
    dr = np.frombuffer(ref["desc"], np.float32).reshape(-1, 128)
    assert_permuted(ext_a, fa, da, ext_r, fr, dr)


def test_same_bytes_alone(gpu_hip, reference):
    hip = gpu_hip
    ref, _ = reference
    ctx = run(hip, IMG, raster(hip))
    assert_same(snapshot(ctx), ref, "second context")
    ctx.submit(synth(22, 256, 192)).wait()
    assert_same(snapshot(ctx.submit(IMG)), ref, "same context, after another image")
    ctx.close()


def test_same_bytes_in_a_batch(gpu_hip, reference):
    hip = gpu_hip
    ref, _ = reference
    imgs = [synth(30 + k, 256, 192) for k in range(16)]
    for k in (0, 7, 15):
        imgs[k] = IMG
    ctx = hip.Context(raster(hip)).submit_batch(imgs)
    for k in (0, 7, 15):
        assert_same(snapshot(ctx, k), ref, "slot %d" % k)
    ctx.close()


SWITCHES = {
    "det_qcap": ((_capi.DEBUG_DET_QCAP, 4),),
    "kp_waves": ((_capi.DEBUG_KP_WAVES, 32),),
    "blur_path": ((_capi.DEBUG_BLUR_PATH, 2),),
    "grow_rerun": ((_capi.DEBUG_CAND_CAP, 256), (_capi.DEBUG_OHIST_CAP, 100), (_capi.DEBUG_DESC_CAP, 64)),
    "coarse1": ((_capi.DEBUG_ORDER_COARSE, 1),),
    "coarse4": ((_capi.DEBUG_ORDER_COARSE, 4),),
    "coarse15": ((_capi.DEBUG_ORDER_COARSE, 15),),
}


@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_same_bytes_under_debug_switches(gpu_hip, reference, name):
    ref, _ = reference
    ctx = run(gpu_hip, IMG, raster(gpu_hip), SWITCHES[name])
    assert_same(snapshot(ctx), ref, name)
    ctx.close()


def test_order_coarse_range(gpu_hip):
    ctx = gpu_hip.Context(raster(gpu_hip))
    for v in (-1, 16):
        with pytest.raises(gpu_hip.PopsiftHipError) as e:
            ctx.debug_set(gpu_hip.DEBUG_ORDER_COARSE, v)
        assert e.value.status == gpu_hip.ERR_INVALID
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 3, 4

W = H = 570         # octaves 570, 285, 143, 72: octave 0's lattice holds 56 x 56 = 3136 sites >= 3 * CHUNK + 1
OCT = 4
COUNTS = [0, 1, 2, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 1]
LAYOUTS = [{0: n, 1: 70, 2: 9} for n in COUNTS] + [{3: 1}]


VARIANTS = [(_capi.ORDER_ARRIVAL, 0), (_capi.ORDER_RASTER, 0), (_capi.ORDER_RASTER, 3), (_capi.ORDER_RASTER, 15)]


class PlantedRuns:
    """one store_dog context per (order, ORDER_COARSE), reused over the layouts; a layout is planted once, run in all
    four contexts, and its results kept (never modified)"""

    def __init__(self, hip, O):
        self.hip, self.dims = hip, P.octave_dims(O, W, H, OCT)
        self.ctx, self.res = {}, {}

    def context(self, order, coarse):
        if (order, coarse) not in self.ctx:
            ctx = self.hip.Context(self.hip.default_params(store_dog=1, feature_order=order, **P.params_kw(OCT)))
            if coarse:
                ctx.debug_set(self.hip.DEBUG_ORDER_COARSE, coarse)
            ctx.submit(np.zeros((H, W), np.uint8)).wait()
            self.ctx[(order, coarse)] = ctx
        return self.ctx[(order, coarse)]

    def result(self, i, order, coarse=0):
        """(extrema, feats, desc, counts) of layout i"""
        if i not in self.res:
            pl = P.Planted(self.dims, LAYOUTS[i], seed=100 + i)
            self.res[i] = {}
            for v in VARIANTS:
                ctx = self.context(*v)
                pl.upload(ctx).rerun_keypoint_stages()
                feats, desc = ctx.fetch()
                self.res[i][v] = (ctx.extrema(), feats, desc, list(ctx.report().ext_ct)[:OCT])
        return self.res[i][(order, coarse)]

    def close(self):
        for c in self.ctx.values():
            c.close()


@pytest.fixture(scope="module")
def runs(gpu_hip, oracle_mod):
    r = PlantedRuns(gpu_hip, oracle_mod)
    yield r
    r.close()


def layout_id(i):
    return "-".join("%d:%d" % kv for kv in sorted(LAYOUTS[i].items()))


@pytest.mark.parametrize("i", range(len(LAYOUTS)), ids=layout_id)
def test_count_edges(gpu_hip, runs, i):
    want = [LAYOUTS[i].get(o, 0) for o in range(OCT)]
    ext_a, fa, da, ct_a = runs.result(i, gpu_hip.ORDER_ARRIVAL)
    ext_r, fr, dr, ct_r = runs.result(i, gpu_hip.ORDER_RASTER)
    assert ct_a == ct_r == want
    assert [int((ext_r["octave"] == o).sum()) for o in range(OCT)] == want
    assert R.is_ordered(ext_r)
    assert_permuted(ext_a, fa, da, ext_r, fr, dr)


@pytest.mark.parametrize("coarse", [3, 15])
@pytest.mark.parametrize("i", range(len(LAYOUTS)), ids=layout_id)
def test_ties_in_the_bucket_key(gpu_hip, runs, i, coarse):
    """ORDER_COARSE = 15: one bucket is the whole octave, the ranking loop alone orders it; 3: bands of 8 rows, where
    neighbouring bumps of different columns and levels share a bucket.  Both equal ORDER_COARSE = 0."""
    ext0, f0, d0, ct0 = runs.result(i, gpu_hip.ORDER_RASTER)
    ext, f, d, ct = runs.result(i, gpu_hip.ORDER_RASTER, coarse)
    assert ct == ct0
    assert ext.tobytes() == ext0.tobytes() and f.tobytes() == f0.tobytes() and d.tobytes() == d0.tobytes()


# ------------------------------------------------------------------------------------------------------------------- 5

FMAX = 1000


@pytest.mark.parametrize("sorting", [0, 1, 2], ids=["random", "largest_first", "smallest_first"])
def test_grid_filter(gpu_hip, reference, sorting):
    hip = gpu_hip
    kw = dict(filter_max_extrema=FMAX, filter_grid_size=3, filter_sorting=sorting)
    total = len(reference[1])
    assert int(FMAX * 1.1) < total          # the 10 % test passes: the filter thins
    ctx = run(hip, IMG, raster(hip, **kw))
    ref = snapshot(ctx)
    ext = ctx.extrema()
    ctx.close()
    assert 0 < len(ext) < total
    assert R.is_ordered(ext)
    again = run(hip, IMG, raster(hip, **kw))
    assert_same(snapshot(again), ref, "second run")
    assert again.extrema().tobytes() == ext.tobytes()       # the survivor set, RANDOM mode included
    again.close()
    batch = hip.Context(raster(hip, **kw)).submit_batch([synth(40, 256, 192), synth(41, 256, 192), IMG])
    assert_same(snapshot(batch, 2), ref, "batch slot 2")
    batch.close()
    if sorting != 0:
        a = run(hip, IMG, hip.default_params(**kw))
        ext_a = a.extrema()
        a.close()
        assert R.sort(ext_a).tobytes() == ext.tobytes()     # the scale orders pick the same members in either order


# ------------------------------------------------------------------------------------------------------------------- 6

def test_describe_ignores_the_order(gpu_hip):
    hip = gpu_hip
    img = synth(23, 160, 120)
    rng = np.random.default_rng(5)
    fr = np.zeros(300, hip.FRAME_DTYPE)
    fr["xpos"], fr["ypos"] = rng.uniform(5, 155, 300), rng.uniform(5, 115, 300)
    fr["sigma"] = rng.uniform(1.0, 6.0, 300)
    fr["octave"] = fr["level"] = -1
    got = []
    for order in (hip.ORDER_ARRIVAL, hip.ORDER_RASTER):
        ctx = hip.Context(hip.default_params(feature_order=order))
        f, d = ctx.describe(img, fr)
        got.append((f.tobytes(), d.tobytes()))
        ctx.close()
    assert len(got[0][0]) == 300 * hip.FEATURE_DTYPE.itemsize and got[0] == got[1]


# ------------------------------------------------------------------------------------------------------------------- 7

def test_chain_repeats(gpu_hip):
    """two independent extract -> match -> points -> RANSAC chains of one image pair: every byte equal"""
    hip = gpu_hip
    a = synth(95, 96, 72)
    b = np.roll(a, (4, 8), axis=(0, 1))
    v = hip.Verifier()
    chains = []
    for _ in range(2):
        A, B = run(hip, a, raster(hip)).clone_results(), run(hip, b, raster(hip)).clone_results()
        pairs = A.match_pairs(B, cross_check=True)
        pts = A.pair_points(B, pairs)
        res, mask = v.ransac(pts, "homography", 512, 1.0, 3)
        assert len(pairs) > 20 and res["n_inliers"] > len(pairs) // 2
        chains.append([pairs.tobytes(), pts.tobytes(), res.tobytes(), mask.tobytes()])
        A.close()
        B.close()
    v.close()
    assert len(chains[0][2]) == 52 and chains[0] == chains[1]
