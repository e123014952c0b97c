"""tests/mask_rule.py on hand-made positions and on the CPU oracle's output for the images the GPU mask tests use
(tests/test_gpu_mask.py asserts the same counts on the device), and the argument check of the new entry point that needs
no GPU."""
import ctypes as C

import numpy as np
import pytest

import mask_rule as M
from popsift_amd.synth import synth

NAN, INF = np.float32(np.nan), np.float32(np.inf)
W, H = 256, 192

# (upscale_factor, image size) -> total, visible under the checker mask, survivors of the planted mask
POPULATION = {
    1: ((256, 192), 1803, 907, 915),
    0: ((256, 192), 232, 112, 117),
    -1: ((640, 480), 145, 75, 73),
}


# ------------------------------------------------------------------------------------------------------------ the rule

def test_pixels_of_hand_made_positions():
    v = np.array([-0.3, 0.49999997, 0.5, W - 1.5, W - 0.5, W + 7, NAN, INF, -INF], np.float32)
    # 0.49999997f, the float below 0.5: 0.49999997f + 0.5f is a tie that rounds to 1.0f, and the header's formula is
    # evaluated in float, so pixel 1 is its pixel.  w - 1.5 + 0.5 is w - 1 exactly.
    assert np.float32(0.49999997) < np.float32(0.5) and np.float32(0.49999997) + np.float32(0.5) == np.float32(1.0)
    want_x = [0, 1, 1, W - 1, W - 1, W - 1, 0, W - 1, 0]
    mx, my = M.pixels(v, np.zeros_like(v), W, H)
    assert mx.tolist() == want_x and (my == 0).all()
    u = np.array([-0.3, 0.49999997, 0.5, H - 1.5, H - 0.5, H + 7, NAN, INF, -INF], np.float32)
    want_y = [0, 1, 1, H - 1, H - 1, H - 1, 0, H - 1, 0]
    mx, my = M.pixels(np.zeros_like(u), u, W, H)
    assert my.tolist() == want_y and (mx == 0).all()
    assert mx.dtype == np.int64


def test_pixels_against_a_scalar_restatement():
    """the header's formula, one float32 operation at a time, on a spread of values"""
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.uniform(-3, W + 3, 500), np.arange(0, 40) + 0.5, np.arange(0, 40) + 0.49999]).astype(np.float32)
    mx, _ = M.pixels(v, v, W, H)
    for a, got in zip(v, mx):
        t = np.float32(np.floor(np.float32(a + np.float32(0.5))))
        t = min(max(t, np.float32(0.0)), np.float32(W - 1))
        assert int(t) == got, a


def test_visible_reads_row_my_column_mx():
    mask = np.zeros((H, W), np.uint8)
    mask[7, 100] = 1                                    # any non-zero value is visible
    f = np.zeros(4, [("xpos", np.float32), ("ypos", np.float32)])
    f["xpos"], f["ypos"] = [100.4, 7.0, 99.5, 100.5], [6.5, 100.0, 7.49, 7.0]
    assert M.visible(f, mask).tolist() == [True, False, True, False]


def test_image_xy_scales_by_an_exact_power_of_two():
    e = np.zeros(3, [("xpos", np.float32), ("ypos", np.float32), ("octave", np.int32)])
    e["xpos"], e["ypos"], e["octave"] = [10.3, 10.3, 10.3], [5.7, 5.7, 5.7], [0, 1, 3]
    x, y = M.image_xy(e, 1)
    assert x.dtype == np.float32
    assert x.tolist() == [np.float32(10.3) * np.float32(0.5), np.float32(10.3), np.float32(10.3) * np.float32(4)]
    x, _ = M.image_xy(e, -1)
    assert x.tolist() == [np.float32(10.3) * np.float32(2), np.float32(10.3) * np.float32(4), np.float32(10.3) * np.float32(16)]


def test_checker_and_planted_masks():
    c = M.checker(W, H)
    assert c[0, 0] == 255 and c[0, 16] == 0 and c[16, 0] == 0 and c[16, 16] == 255 and c[15, 15] == 255
    x = np.array([3.2, 3.4, 9.0, 1.0], np.float32)
    y = np.array([2.0, 2.1, 0.0, 0.0], np.float32)
    m, pix = M.planted(x, y, np.array([0, 0, 0, 1]), W, H)
    # sorted by (octave, my, mx): (0,0,9) (0,2,3) (0,2,3) (1,0,1) -> every second: (0, 9) and one of the twins at (2, 3)
    assert sorted(map(tuple, pix.tolist())) == [(0, 9), (2, 3)]
    assert int((m != 0).sum()) == 2 and m[0, 9] and m[2, 3]


# ---------------------------------------------------------------------------------------- the oracle on the test images

@pytest.fixture(scope="module", params=[1, 0, -1])
def oracle_run(request, oracle_mod):
    """(upscale, mask size, extrema of the oracle with default parameters); never modified"""
    O = oracle_mod
    up = request.param
    (w, h) = POPULATION[up][0]
    orc = O.Oracle(O.default_params(upscale_factor=float(up))).run(synth(21, w, h))
    ext = orc.extrema()
    orc.close()
    return up, w, h, ext


def test_oracle_checker_counts(oracle_run):
    up, w, h, ext = oracle_run
    _, total, vis, _ = POPULATION[up]
    assert len(ext) == total
    keep = M.visible_ext(ext, M.checker(w, h), up)
    assert int(keep.sum()) == vis
    if up == 1:
        assert np.bincount(ext["octave"], minlength=4).tolist()[:4] == [1543, 240, 14, 6]
        assert np.bincount(ext["octave"][keep], minlength=4).tolist()[:4] == [782, 115, 7, 3]


def test_oracle_planted_counts(oracle_run):
    up, w, h, ext = oracle_run
    _, total, _, survivors = POPULATION[up]
    x, y = M.image_xy(ext, up)
    mask, pix = M.planted(x, y, ext["octave"], w, h)
    keep = M.visible_ext(ext, mask, up)
    assert int(keep.sum()) == survivors
    assert len(pix) == (total + 1) // 2
    if up == 1:
        mx, my = M.pixels(x, y, w, h)
        # pixels shared by two or more features, features on a border row or column, and what the plant makes of them
        _, n = np.unique(my * w + mx, return_counts=True)
        assert int((n >= 2).sum()) == 22
        assert int(((mx == 0) | (mx == w - 1) | (my == 0) | (my == h - 1)).sum()) == 3
        # 902 features are planted and 13 further ones share a planted pixel; six of the planted ones share their pixel
        # with another planted one (of another octave, or the third of a triple), so 896 distinct pixels are set
        assert len(pix) == 902 and survivors - len(pix) == 13
        assert int((mask != 0).sum()) == 896


# ------------------------------------------------------------------------------------------- argument checks, no GPU

def test_null_context_is_invalid(hip):
    L = hip.lib()
    img = np.zeros((4, 4), np.uint8)
    imgs = (C.c_void_p * 1)(img.ctypes.data)
    masks = (C.c_void_p * 1)(img.ctypes.data)
    assert L.popsift_hip_submit_batch_masked(None, imgs, masks, 1, hip.IMG_HOST_U8, 4, 4, 4, 4) == hip.ERR_INVALID
