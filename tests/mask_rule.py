"""The extraction-mask rule of include/popsift_hip.h (popsift_hip_submit_batch_masked) restated in NumPy float32.

For a feature at (x, y) in input-image coordinates, as popsift_hip_feature reports it, and a w x h mask:
    mx = (int)fminf(fmaxf(floorf(x + 0.5f), 0.0f), (float)(w - 1))
    my = (int)fminf(fmaxf(floorf(y + 0.5f), 0.0f), (float)(h - 1))
    visible = mask[my, mx] != 0
fmaxf and fminf drop a NaN operand, so NaN lands on pixel 0 and +inf on the last column or row.

An extremum record (xpos, ypos in octave units, octave o) has x = xpos * 2^(o - up), up = (int)upscale_factor: a product
with a power of two, exact in float32."""
import numpy as np


def pixels(x, y, w, h):
    """-> (mx, my), int64 arrays"""
    def pix(v, n):
        v = np.asarray(v, np.float32)
        with np.errstate(invalid="ignore"):
            t = np.floor(v + np.float32(0.5)).astype(np.float32)
            t = np.fmax(t, np.float32(0.0))               # fmax / fmin: a NaN operand is dropped
            t = np.fmin(t, np.float32(n - 1))
        return t.astype(np.int64)
    return pix(x, w), pix(y, h)


def visible(feats, mask):
    """keep-mask over feature records (fields xpos, ypos in input-image coordinates) under the (h, w) uint8 mask"""
    h, w = mask.shape
    mx, my = pixels(feats["xpos"], feats["ypos"], w, h)
    return mask[my, mx] != 0


def image_xy(ext, up):
    """input-image coordinates of extremum records (xpos, ypos in octave units, octave), as the feature records hold them"""
    scl = np.exp2((ext["octave"].astype(np.int64) - int(up)).astype(np.float64)).astype(np.float32)
    return ext["xpos"].astype(np.float32) * scl, ext["ypos"].astype(np.float32) * scl


def visible_ext(ext, mask, up):
    h, w = mask.shape
    x, y = image_xy(ext, up)
    mx, my = pixels(x, y, w, h)
    return mask[my, mx] != 0


def checker(w, h, block=16):
    """((mx // block) + (my // block)) % 2 == 0 is visible"""
    my, mx = np.mgrid[0:h, 0:w]
    return ((((mx // block) + (my // block)) % 2 == 0) * 255).astype(np.uint8)


def planted(x, y, octave, w, h):
    """The planted mask of features at (x, y) of octaves `octave`: sort them by (octave, my, mx), set exactly the pixel of
    every second one (the first, third, ..), leave every other pixel zero -> (mask, the planted pixels as (my, mx) rows)"""
    mx, my = pixels(x, y, w, h)
    order = np.lexsort((mx, my, np.asarray(octave)))
    pick = order[::2]
    mask = np.zeros((h, w), np.uint8)
    mask[my[pick], mx[pick]] = 255
    return mask, np.stack([my[pick], mx[pick]], axis=1)
