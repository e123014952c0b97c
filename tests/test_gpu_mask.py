"""Extraction masks on the GPU (popsift_hip_submit_batch_masked; the masked instantiation of k_refine, extrema.hip), held to
tests/mask_rule.py byte for byte: a masked run is the unmasked raster run with the hidden records removed -- in every
refinement mode, with stored and on-the-fly DoG planes, for byte and float images and at every upscale factor -- and the
mask acts before the max_extrema cap, keep-strongest and the grid filter, in every batch slot and through every re-run.
The populations are those tests/test_mask_rule.py counts on the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import filter_rule as F
import mask_rule as M
import order_rule as R
import strongest_rule as S
from popsift_amd import _capi
from popsift_amd.synth import synth

pytestmark = pytest.mark.gpu

REC = ["debug_octave", "xpos", "ypos", "sigma", "num_ori", "orientation"]   # a feature without its descriptor indices
W, H = 256, 192
IMG = synth(21, W, H)
# upscale_factor -> (image size, total, visible under the checker, survivors of the planted mask): default parameters
POPULATION = {1: ((256, 192), 1803, 907, 915), 0: ((256, 192), 232, 112, 117), -1: ((640, 480), 145, 75, 73)}
CHECKER_CT = [782, 115, 7, 3]


def raster(hip, **kw):
    return hip.default_params(feature_order=hip.ORDER_RASTER, **kw)


def image(up, f32=False):
    (w, h) = POPULATION[up][0]
    img = IMG if (w, h) == (W, H) else synth(21, w, h)
    return img.astype(np.float32) / np.float32(256.0) if f32 else img


class Result:
    """everything a finished image hands out (image k of the batch in `ctx`)"""

    def __init__(self, ctx, k=0, responses=False):
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


def assert_filtered(full, keep, got, ordered=True):
    """`got` is `full` (the unmasked raster run) with the records outside `keep` removed: extrema, feature records,
    descriptors through desc_idx, byte descriptors, responses where both runs have them and the per-octave counts.
    ordered=False: `got` is in arrival order, so only the SET of extrema is compared (in the rule's order)."""
    assert len(got.feats) == int(keep.sum())
    if hasattr(got, "ext"):
        n_oct = len(full.ext_ct)
        assert got.ext_ct == np.bincount(full.ext["octave"][keep], minlength=n_oct).tolist()
        assert len(got.ext) == len(got.feats)
        if not ordered:
            assert R.sort(got.ext).tobytes() == full.ext[keep].tobytes()
            return
        assert got.ext.tobytes() == full.ext[keep].tobytes()
    if got.resp is not None and full.resp is not None:
        assert got.resp.tobytes() == full.resp[keep].tobytes()
    for name in REC:
        assert got.feats[name].tobytes() == full.feats[name][keep].tobytes(), name
    iw, ig = full.feats["desc_idx"][keep], got.feats["desc_idx"]
    assert np.array_equal(iw >= 0, ig >= 0)
    assert np.array_equal(ig[ig >= 0], np.arange(len(got.desc)))        # contiguous in list order
    assert got.desc[ig[ig >= 0]].tobytes() == full.desc[iw[iw >= 0]].tobytes()
    assert got.u8[ig[ig >= 0]].tobytes() == full.u8[iw[iw >= 0]].tobytes()


def planted_mask(full, w, h):
    """the planted mask of the unmasked raster run `full` (tests/mask_rule.py)"""
    return M.planted(full.feats["xpos"], full.feats["ypos"], full.feats["debug_octave"], w, h)[0]


@pytest.fixture(scope="module")
def ctx(gpu_hip):
    """a raster context with default parameters, shared by the tests that need nothing else"""
    c = gpu_hip.Context(raster(gpu_hip))
    yield c
    c.close()


@pytest.fixture(scope="module")
def full(ctx):
    """the unmasked raster run of IMG; never modified"""
    r = Result(ctx.submit(IMG))
    assert len(r.ext) == 1803 and r.ext_ct[:4] == [1543, 240, 14, 6]
    return r


@pytest.fixture(scope="module")
def masks(full):
    return {"checker": M.checker(W, H), "planted": planted_mask(full, W, H)}


# ------------------------------------------------------------------------------------------- 1. all, none, NULL

def test_all_visible_null_and_all_hidden(ctx, full):
    Result(ctx.submit(IMG, np.full((H, W), 255, np.uint8))).same_bytes(full, "all-255 mask")
    Result(ctx.submit(IMG, np.full((H, W), 1, np.uint8))).same_bytes(full, "all-1 mask")
    Result(ctx.submit_batch([IMG], [None])).same_bytes(full, "NULL mask")
    ctx.submit(IMG, np.zeros((H, W), np.uint8))
    assert ctx.wait() == (0, 0)
    f, d = ctx.fetch()
    assert len(f) == 0 and len(d) == 0 and len(ctx.extrema()) == 0
    assert not any(ctx.report().ext_ct)


# ------------------------------------------------------------------------------- 2. the six masked instantiations

@pytest.mark.parametrize("up", [1, 0, -1])
@pytest.mark.parametrize("f32", [False, True], ids=["u8", "f32"])
@pytest.mark.parametrize("store_dog", [0, 1])
@pytest.mark.parametrize("sift_mode", [0, 1, 2])
def test_checker_and_planted(gpu_hip, sift_mode, store_dog, f32, up):
    hip = gpu_hip
    (w, h), total, vis, survivors = POPULATION[up]
    img = image(up, f32)
    c = hip.Context(raster(hip, sift_mode=sift_mode, store_dog=store_dog, upscale_factor=float(up)))
    unmasked = Result(c.submit(img))
    counted = sift_mode == 0 and not f32        # the population the oracle counts (tests/test_mask_rule.py)
    if counted:
        assert len(unmasked.feats) == total
    # the rule from the feature records and from the extremum records is one rule
    x, y = M.image_xy(unmasked.ext, up)
    assert x.tobytes() == unmasked.feats["xpos"].tobytes() and y.tobytes() == unmasked.feats["ypos"].tobytes()
    for name, mask, want in (("checker", M.checker(w, h), vis), ("planted", planted_mask(unmasked, w, h), survivors)):
        keep = M.visible(unmasked.feats, mask)
        print(name, "sift_mode", sift_mode, "store_dog", store_dog, "f32", f32, "up", up, "visible", int(keep.sum()), "of",
              len(keep))
        assert 0 < keep.sum() < len(keep), name
        if counted:
            assert int(keep.sum()) == want, name
            if up == 1 and name == "checker":
                assert np.bincount(unmasked.ext["octave"][keep], minlength=4).tolist()[:4] == CHECKER_CT
        assert_filtered(unmasked, keep, Result(c.submit(img, mask)))
    c.close()


def test_planted_mask_holds_the_border_features(full, masks):
    mx, my = M.pixels(full.feats["xpos"], full.feats["ypos"], W, H)
    border = (mx == 0) | (mx == W - 1) | (my == 0) | (my == H - 1)
    assert int(border.sum()) == 3
    assert (masks["planted"][my[border], mx[border]] != 0).any()
    # a transposed or shifted read of the planted mask cannot return the planted survivors
    keep = M.visible(full.feats, masks["planted"])
    assert int(keep.sum()) == 915
    shifted = np.roll(masks["planted"], 1, axis=1)
    assert int(M.visible(full.feats, shifted).sum()) < 100


# -------------------------------------------------------------------------------------------------- 3. mask pitch

def padded(mask, pitch):
    buf = np.full((mask.shape[0], pitch), 255, np.uint8)
    buf[:, :mask.shape[1]] = mask
    return buf


def submit_raw(hip, c, kind, img_ptr, mask_ptr, pitch, mask_pitch):
    imgs, ms = (C.c_void_p * 1)(img_ptr), (C.c_void_p * 1)(mask_ptr)
    return hip.lib().popsift_hip_submit_batch_masked(c._h, imgs, ms, 1, kind, W, H, pitch, mask_pitch)


@pytest.mark.parametrize("where", ["host", "pinned", "device"])
def test_mask_pitch(gpu_hip, ctx, full, masks, where):
    hip = gpu_hip
    pitch = W + 37
    want = Result(ctx.submit(IMG, masks["planted"]))
    assert_filtered(full, M.visible(full.feats, masks["planted"]), want)
    buf = padded(masks["planted"], pitch)
    if where == "host":
        assert submit_raw(hip, ctx, hip.IMG_HOST_U8, IMG.ctypes.data, buf.ctypes.data, W, pitch) == hip.OK
        buf[:] = 0                                      # a pageable mask is copied before the call returns
        Result(ctx).same_bytes(want, where)
    elif where == "pinned":
        L = hip.lib()
        n_img, n_mask = W * H, H * pitch
        p = L.popsift_hip_host_alloc(n_img + n_mask)
        assert p
        try:
            C.memmove(p, IMG.ctypes.data, n_img)
            C.memmove(p + n_img, buf.ctypes.data, n_mask)
            assert submit_raw(hip, ctx, hip.IMG_PINNED_U8, p, p + n_img, W, pitch) == hip.OK
            Result(ctx).same_bytes(want, where)
        finally:
            L.popsift_hip_host_free(p)
    else:
        rt = C.CDLL("libamdhip64.so")              # the HIP runtime libpopsift_hip.so itself is linked against
        rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        rt.hipFree.argtypes = [C.c_void_p]
        d_img, d_mask = C.c_void_p(), C.c_void_p()
        assert rt.hipMalloc(C.byref(d_img), IMG.nbytes) == 0 and rt.hipMalloc(C.byref(d_mask), buf.nbytes) == 0
        try:
            assert rt.hipMemcpy(d_img, IMG.ctypes.data, IMG.nbytes, 1) == 0      # hipMemcpyHostToDevice
            assert rt.hipMemcpy(d_mask, buf.ctypes.data, buf.nbytes, 1) == 0
            ctx.submit_batch_dev([d_img.value], W, H, W, masks=[d_mask.value], mask_pitch=pitch)
            Result(ctx).same_bytes(want, where)
        finally:
            rt.hipFree(d_img)
            rt.hipFree(d_mask)


# ---------------------------------------------------------------------------------------- 4. the mask before the cap

def test_mask_acts_before_the_cap(gpu_hip, full, masks):
    hip = gpu_hip
    c = hip.Context(raster(hip, max_extrema=1000))
    c.submit(IMG).wait()
    assert c.report().ext_ct[0] == 1000                 # clamped from 1543: which 1000 is decided by arrival
    keep = M.visible(full.feats, masks["checker"])
    got = Result(c.submit(IMG, masks["checker"]))
    assert got.ext_ct[:4] == CHECKER_CT and len(got.feats) == 907
    assert_filtered(full, keep, got)                    # `full` ran with max_extrema = 100000
    c.close()


# ---------------------------------------------------------------------------------------------------------- 5. batch

def test_batch_of_mixed_masks_then_a_plain_submit(gpu_hip, ctx, full, masks):
    imgs = [IMG, synth(31, W, H), IMG, synth(32, W, H), IMG]
    ms = [masks["checker"], None, np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8), masks["planted"]]
    single = gpu_hip.Context(raster(gpu_hip))
    want = [Result(single.submit(im) if m is None else single.submit(im, m)) for im, m in zip(imgs, ms)]
    single.close()
    assert [len(r.feats) for r in want][0::2] == [907, 0, 915] and len(want[1].feats) > 500 and len(want[3].feats) > 500
    ctx.submit_batch(imgs, ms)
    for k in range(len(imgs)):
        Result(ctx, k).same_bytes(want[k], "slot %d" % k)
    # a plain submit clears the masks: every slot is unmasked again
    ctx.submit_batch([IMG] * 5)
    for k in range(5):
        Result(ctx, k).same_bytes(full, "plain slot %d" % k)


def test_describe_clears_the_mask(gpu_hip, ctx, full, masks):
    hip = gpu_hip
    assert ctx.submit(IMG, masks["checker"]).wait()[0] == 907
    fr = np.zeros(3, hip.FRAME_DTYPE)
    fr["xpos"], fr["ypos"], fr["sigma"] = [24, 90, 150], [30, 80, 120], [2.0, 3.0, 4.0]     # (24, 30) is a hidden pixel
    fr["octave"] = fr["level"] = -1
    f, _ = ctx.describe(IMG, fr)
    assert len(f) == 3 and (f["num_ori"] > 0).all()
    Result(ctx.submit(IMG)).same_bytes(full, "plain submit after a describe")


# --------------------------------------------------------------------------------------------------------- 6. chains

def test_masked_then_keep_strongest(gpu_hip, masks):
    hip = gpu_hip
    c = hip.Context(raster(hip)).set_keep_strongest(S.INT32_MAX)
    unmasked = Result(c.submit(IMG), responses=True)
    keep = M.visible(unmasked.feats, masks["checker"])
    masked = Result(c.submit(IMG, masks["checker"]), responses=True)
    assert_filtered(unmasked, keep, masked)             # responses included
    strong = S.keep_mask(masked.resp, 300)
    assert int(strong.sum()) == 300
    both = keep.copy()
    both[keep] = strong
    assert_filtered(unmasked, both, Result(c.set_keep_strongest(300).submit(IMG, masks["checker"]), responses=True))
    # the 300 strongest of the visible ones are not the visible ones among the 300 strongest of all
    assert int((S.keep_mask(unmasked.resp, 300) & keep).sum()) < 300
    c.close()


def test_masked_then_grid_filter(gpu_hip, full, masks):
    hip = gpu_hip
    kw = dict(filter_max_extrema=200, filter_sorting=F.LARGEST_FIRST, filter_grid_size=2)
    c = hip.Context(raster(hip, **kw))
    got = Result(c.submit(IMG, masks["checker"]))
    c.close()
    masked_list = full.ext[M.visible(full.feats, masks["checker"])]
    want, lim, act = F.expected_raster(masked_list, 2, 200, F.LARGEST_FIRST)
    assert act and lim != F.NO_LIMIT and 0 < len(want) < len(masked_list)
    assert got.ext.tobytes() == want.tobytes()
    # the budget is spent on the visible area: the filter of the unmasked list keeps other records
    unmasked_want, _, _ = F.expected_raster(full.ext, 2, 200, F.LARGEST_FIRST)
    vis = M.visible_ext(unmasked_want, masks["checker"], 1)
    assert int(vis.sum()) < len(want)


# -------------------------------------------------------------------------------------------------------- 7. re-runs

def test_rerun_keypoint_stages_applies_the_mask_again(ctx, full, masks):
    keep = M.visible(full.feats, masks["planted"])
    first = Result(ctx.submit(IMG, masks["planted"]))
    assert_filtered(full, keep, first)
    Result(ctx.rerun_keypoint_stages()).same_bytes(first, "rerun_keypoint_stages")


def test_grow_and_rerun_applies_the_mask_again(gpu_hip, full, masks):
    hip = gpu_hip
    c = hip.Context(raster(hip))
    for what, value in ((_capi.DEBUG_CAND_CAP, 256), (_capi.DEBUG_OHIST_CAP, 100), (_capi.DEBUG_DESC_CAP, 64)):
        c.debug_set(what, value)
    assert_filtered(full, M.visible(full.feats, masks["checker"]), Result(c.submit(IMG, masks["checker"])))
    c.close()


# -------------------------------------------------------------------------------------------------- 8. arrival order

def test_arrival_order_returns_the_same_set(gpu_hip, full, masks):
    c = gpu_hip.Context(gpu_hip.default_params())
    got = Result(c.submit(IMG, masks["checker"]))
    c.close()
    assert_filtered(full, M.visible(full.feats, masks["checker"]), got, ordered=False)


# ---------------------------------------------------------------------------------------------------------- 9. errors

def test_errors_leave_the_context_usable(gpu_hip, ctx, full, masks):
    hip = gpu_hip
    L = hip.lib()
    imgs = (C.c_void_p * 1)(IMG.ctypes.data)
    ms = (C.c_void_p * 1)(masks["checker"].ctypes.data)
    none = (C.c_void_p * 1)(None)
    assert L.popsift_hip_submit_batch_masked(ctx._h, imgs, None, 1, hip.IMG_HOST_U8, W, H, W, W) == hip.ERR_INVALID
    assert L.popsift_hip_submit_batch_masked(ctx._h, imgs, ms, 1, hip.IMG_HOST_U8, W, H, W, W - 1) == hip.ERR_INVALID
    assert L.popsift_hip_submit_batch_masked(ctx._h, imgs, ms, 0, hip.IMG_HOST_U8, W, H, W, W) == hip.ERR_INVALID
    assert L.popsift_hip_submit_batch_masked(ctx._h, imgs, ms, 1, hip.IMG_HOST_U8, W, H, W - 1, W) == hip.ERR_INVALID
    # without a mask the pitch of the masks is not looked at
    assert L.popsift_hip_submit_batch_masked(ctx._h, imgs, none, 1, hip.IMG_HOST_U8, W, H, W, 0) == hip.OK
    Result(ctx).same_bytes(full, "null entry, mask_pitch 0")
    assert_filtered(full, M.visible(full.feats, masks["checker"]), Result(ctx.submit(IMG, masks["checker"])))
