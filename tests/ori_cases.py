"""Hard-edged images and the cases of the per-keypoint orientation check (tests/ori_rule.py), shared by its CPU and
GPU tests: step edges, binary and saturated planes, gradients of exactly 45 degrees, exact symmetries -- what
popsift_amd.synth.synth (low-passed noise plus smooth blobs) never produces."""
import functools

import numpy as np

from popsift_amd.synth import oxford_like_homographies, synth, warp

import ori_rule

W, H = 160, 120


def noise(block, seed):
    """0/255 noise in blocks of block x block pixels."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cells = rng.integers(0, 2, (-(-H // block), -(-W // block)), dtype=np.uint8) * np.uint8(255)
    return np.ascontiguousarray(np.kron(cells, np.ones((block, block), np.uint8))[:H, :W])


def checkerboard(period):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((((xx // period) + (yy // period)) & 1) * 255).astype(np.uint8)


def contrast6(seed):
    """synth(seed) with its contrast times six around 128, clipped: large areas saturated at 0 and at 255."""
    return np.clip((synth(seed, W, H).astype(np.float64) - 128.0) * 6.0 + 128.0, 0, 255).astype(np.uint8)


IMAGES = {
    # strong: at least 85 % of the keypoints decided, at least 100 keypoints
    "synth7": lambda: synth(7, W, H),
    "noise1": lambda: noise(1, 1),
    "noise2": lambda: noise(2, 22),
    "contrast6": lambda: contrast6(3),
    "checker8_warped": lambda: warp(checkerboard(8), oxford_like_homographies()[2]),
    # a float image whose maximum is exactly 1.0, the closed end of the documented [0, 1) range
    "synth7_float": lambda: synth(7, W, H).astype(np.float32) / np.float32(255.0),
    # open: mostly exact ties
    "checker7": lambda: checkerboard(7),
    "checker8": lambda: checkerboard(8),
    "noise4": lambda: noise(4, 104),
}
STRONG = ("synth7", "noise1", "noise2", "contrast6", "checker8_warped", "synth7_float")
OPEN = ("checker7", "checker8", "noise4")

PARAMS = {
    "default": dict(),
    "opencv": dict(sift_mode=1, gauss_mode=3),
    "vlfeat": dict(sift_mode=2),
    "no_upscale": dict(upscale_factor=0.0),
    "levels5": dict(levels=5),
}

# every image in the two modes whose pyramids differ most; the other parameter sets (other scales per level, other
# octave sizes) on one binary, one warped and one tied image -- without the up-scaling the binary noise leaves too few
# keypoints (24), so the smooth image stands in for it there
CASES = [(i, p) for p in ("default", "opencv") for i in STRONG + OPEN] + \
        [(i, p) for p in ("vlfeat", "levels5") for i in ("noise2", "checker8_warped", "checker8")] + \
        [(i, "no_upscale") for i in ("synth7", "checker8_warped", "checker8")]
CASE_IDS = ["%s-%s" % c for c in CASES]


@functools.lru_cache(maxsize=None)
def image(name):
    img = IMAGES[name]()
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def reference(O, image_name, param_name):
    """-> (the oracle after its run, its extrema, the rule of every extremum): computed once per case and shared; nobody
    changes it (tests that redo descriptors make an Oracle of their own)."""
    kw = PARAMS[param_name]
    orc = O.Oracle(O.default_params(**kw), threads=8).run(image(image_name))
    ext = orc.extrema()
    rules = ori_rule.analyse_all(lambda o, l: orc.plane(o, 0, l), ext, max(2, kw.get("levels", 3)) + 3)
    return orc, ext, rules
