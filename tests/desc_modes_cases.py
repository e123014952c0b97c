"""The cases of the per-descriptor check of the grid and interpolated descriptors (tests/desc_modes_rule.py), shared by
its CPU and GPU tests: the hard-edged images of tests/ori_cases.py and tests/desc_cases.py through extraction in every
descriptor mode, the crafted frames of desc_cases.crafted() through the describe path (sigma up to the largest accepted
one, angles of exactly +-0, pi/2, +-pi, a corner, x = w - 1 and y = h - 1, where the lattice lives on clamp addressing),
and frames on a vertical 0 -> 255 step, where all gradient of a descriptor falls into one bin.

A case is "<mode>-<image>-<parameters>"; a frame case "<mode>-frames_<image>-<norm>", the step case "<mode>-step".
Every descriptor of a case is checked.  The iloop rule costs about ten times notile's, so its cases are the small ones."""
import functools

import numpy as np

import desc_cases
import desc_modes_rule as R
from desc_cases import CLASSIC, crafted, image as _image

STRONG_IMAGES = desc_cases.STRONG_IMAGES
BORDER_IMAGE = "synth7_96x72"

# name -> (mode, image, parameters)
EXTRACTION = {}
for _i in STRONG_IMAGES:
    EXTRACTION["notile-%s-default" % _i] = ("notile", _i, dict())
for _i in ("noise2", "contrast6", "checker8_warped"):
    EXTRACTION["notile-%s-classic9" % _i] = ("notile", _i, CLASSIC)
EXTRACTION["igrid-synth7-default"] = ("igrid", "synth7", dict())
for _i in ("synth7", "noise2", "checker8_warped"):
    EXTRACTION["grid-%s-default" % _i] = ("grid", _i, dict())
EXTRACTION["grid-noise2-classic9"] = ("grid", "noise2", CLASSIC)
STRONG_CASES = list(EXTRACTION)                 # at least 400 descriptors each and a sharpness bar
BORDER_CASES = ["%s-%s-default" % (m, BORDER_IMAGE) for m in ("notile", "grid", "iloop")]
for _c in BORDER_CASES:
    EXTRACTION[_c] = (_c.split("-")[0], BORDER_IMAGE, dict())
EXTRACTION["iloop-noise1-default"] = ("iloop", "noise1", dict())
EXTRACTION_CASES = list(EXTRACTION)

# name -> (mode, image, parameters, frames)
FRAMES = {
    "notile-frames_noise2-rootsift": ("notile", "noise2", dict(), "crafted"),
    "notile-frames_noise2-classic9": ("notile", "noise2", CLASSIC, "crafted"),
    "igrid-frames_noise2-rootsift": ("igrid", "noise2", dict(), "crafted"),
    "grid-frames_noise2-rootsift": ("grid", "noise2", dict(), "crafted"),
    "iloop-frames_noise2-rootsift": ("iloop", "noise2", dict(), "crafted"),
    "iloop-frames_noise2-classic9": ("iloop", "noise2", CLASSIC, "crafted"),
    "notile-step": ("notile", "step", dict(), "step"),
    "iloop-step": ("iloop", "step", dict(), "step"),
}
FRAME_CASES = list(FRAMES)
STEP_CASES = ["notile-step", "iloop-step"]
ALL_CASES = EXTRACTION_CASES + FRAME_CASES

_FRAME_DT = [("xpos", np.float32), ("ypos", np.float32), ("sigma", np.float32), ("orientation", np.float32), ("level", np.int32)]


@functools.lru_cache(maxsize=None)
def image(name):
    if name == "step":                          # columns 0 .. 79 black, 80 .. 159 white
        img = np.zeros((120, 160), np.uint8)
        img[:, 80:] = 255
        img.setflags(write=False)
        return img
    return _image(name)


def step_frames():
    """Frames ON the edge, in OCTAVE units of octave 0 (320 x 240; the edge lies between columns 159 and 160 of its
    level-0 plane): sigma 1 and 8, angles +0 and pi / 4, on the edge, half a pixel and a quarter pixel beside it."""
    rows = [(x, y, s, a, 1 + k % 3) for s in (1.0, 8.0) for a in (0.0, np.float32(np.pi / 4))
            for k, (x, y) in enumerate(((159.5, 120.0), (160.0, 100.5), (159.25, 140.25), (159.5, 30.0)))]
    fr = np.zeros(len(rows), _FRAME_DT)
    for i, r in enumerate(rows):
        fr[i] = r
    return fr


def mode_of(case):
    return case.split("-")[0]


def params_of(case):
    """the parameters without desc_mode (what desc_cases.params_of returns)"""
    return (EXTRACTION[case] if case in EXTRACTION else FRAMES[case])[2]


def image_of(case):
    return image((EXTRACTION[case] if case in EXTRACTION else FRAMES[case])[1])


def frames_of(case):
    return crafted() if FRAMES[case][3] == "crafted" else step_frames()


def describe_frames(case, frame_dtype, upscale=1):
    """the frames of a frame case as the describe path takes them: image units (octave units halved, exactly), octave 0"""
    c = frames_of(case)
    fr = np.zeros(len(c), frame_dtype)
    for n in ("xpos", "ypos", "sigma"):
        fr[n] = np.ldexp(c[n], -upscale)
    fr["orientation"], fr["octave"], fr["level"] = c["orientation"], 0, c["level"]
    return fr


def norm_of(case):
    kw = params_of(case)
    return kw.get("norm_mode", 0), kw.get("norm_multi", 0)


class Reference:
    """orc: the oracle after its run in the case's descriptor mode (nobody changes it); rows: per descriptor (octave,
    lpos, x, y, sigma, angle) in the order of desc; desc / raw: the oracle's descriptors and raw histograms; samples:
    desc_modes_rule.samples of every row."""

    def __init__(self, case, orc, rows, desc, raw):
        self.case, self.orc, self.rows, self.desc, self.raw = case, orc, rows, desc, raw
        self.norm = norm_of(case)
        self.lattice = R.LATTICE[mode_of(case)]
        self._rules = {}
        self.planes = {}
        self.samples = []
        for o, l, x, y, s, a in rows:
            if (o, l) not in self.planes:
                self.planes[(o, l)] = orc.plane(o, 0, l)
            self.samples.append(R.samples(self.lattice, self.planes[(o, l)], x, y, s, a))

    def plane(self, row):
        return self.planes[(row[0], row[1])]

    def rules(self, device=True):
        if device not in self._rules:
            self._rules[device] = [R.evaluate(p, *self.norm, device=device) for p in self.samples]
        return self._rules[device]

    def name(self, i):
        return "%s descriptor %d, octave %d level %d" % ((self.case, i) + tuple(self.rows[i][:2]))


@functools.lru_cache(maxsize=None)
def reference(O, case):
    """computed once per case and shared"""
    kw = dict(params_of(case), desc_mode=R.DESC_MODE[mode_of(case)])
    n_planes = kw.get("levels", 3) + 3
    if case in EXTRACTION:
        orc = O.Oracle(O.default_params(**kw), threads=8).run(image_of(case))
        ext = orc.extrema()
        feats, desc = orc.fetch()
        rows = [None] * len(desc)
        for e, f in zip(ext, feats):
            for k in range(int(f["num_ori"])):
                rows[f["desc_idx"][k]] = (int(e["octave"]), min(max(int(e["lpos"]), 0), n_planes - 1), e["xpos"], e["ypos"],
                                          e["sigma"], f["orientation"][k])
        return Reference(case, orc, rows, desc, orc.raw_descriptors())
    c = frames_of(case)
    ext = np.zeros(len(c), O.EXTREMUM_DTYPE)
    ext["xpos"], ext["ypos"], ext["sigma"], ext["lpos"], ext["cell"] = c["xpos"], c["ypos"], c["sigma"], c["level"], np.arange(len(c))
    orc = O.Oracle(O.default_params(**kw), threads=8).run(image_of(case), keypoints=False).run_from_extrema(ext)
    feats, _ = orc.fetch()
    assert (feats["num_ori"] >= 1).all()          # redo_descriptors keeps the number of orientations
    ori = np.zeros((len(c), 4), np.float32)
    ori[:] = c["orientation"][:, None]
    feats, desc = orc.redo_descriptors(ori).fetch()
    first = feats["desc_idx"][:, 0]
    rows = [(0, int(f["level"]), f["xpos"], f["ypos"], f["sigma"], f["orientation"]) for f in c]
    return Reference(case, orc, rows, desc[first], orc.raw_descriptors()[first])
