"""The cases of the per-descriptor check of k_descriptor (tests/desc_rule.py), shared by its CPU and GPU tests: the
hard-edged images of tests/ori_cases.py through extraction, and crafted frames through the describe path -- orientations
of exactly +-0 (the only way into the inv_s == 0 branch of k_descriptor's row spans), patches at the largest accepted
scale (about 170 rows, several passes, fbits 10), positions in a corner and on the right border."""
import functools

import numpy as np

from popsift_amd.synth import synth

import desc_rule
import ori_cases

CLASSIC = dict(norm_mode=1, norm_multi=9)
# name -> (image, parameters)
# the strong cases: at least 400 descriptors each and a sharpness bar (tests/test_desc_rule.py).  The 160 x 120 1 px noise
# of ori_cases gives 216 descriptors, so the strong 1 px noise is a 240 x 180 one; the small one stays a case without bars.
STRONG_IMAGES = tuple("noise1_240x180" if i == "noise1" else i for i in ori_cases.STRONG)
EXTRACTION = {("%s-default" % i): (i, dict()) for i in STRONG_IMAGES}
EXTRACTION.update({("%s-classic9" % i): (i, CLASSIC) for i in ("noise2", "contrast6", "checker8_warped")})
STRONG_CASES = list(EXTRACTION)
BORDER_CASE = "synth7_96x72-default"            # the border cuts more than half of its patches
EXTRACTION[BORDER_CASE] = ("synth7_96x72", dict())
EXTRACTION["noise1-default"] = ("noise1", dict())
EXTRACTION_CASES = list(EXTRACTION)
FRAME_CASES = ["frames_%s-%s" % (i, n) for i in ("noise2", "synth7") for n in ("rootsift", "classic9")]

PI32 = np.float32(np.pi)
FRAME_SIGMAS = (1.0, 6.5, 8.0)                  # octave units; 8 is POPSIFT_HIP_FRAME_SIGMA_MAX
FRAME_ANGLES = np.array([0.0, -0.0, np.float32(np.pi / 2), PI32, -PI32, 0.7, -2.1, np.float32(np.pi / 4)], np.float32)
# octave 0 of a 160 x 120 image is 320 x 240: the centre, three more inside, integer coordinates, a corner, the right
# border (x = w - 1, the largest valid one) and the bottom border
FRAME_POSITIONS = ((160.3, 120.6), (100.5, 90.25), (220.75, 130.5), (150.0, 100.0), (61.3, 170.8), (3.5, 2.25),
                   (319.0, 120.5), (140.5, 239.0))


@functools.lru_cache(maxsize=None)
def image(name):
    if name == "synth7_96x72":
        img = synth(7, 96, 72)
    elif name == "noise1_240x180":              # 0/255 noise, every pixel its own
        img = np.random.Generator(np.random.PCG64(1)).integers(0, 2, (180, 240), dtype=np.uint8) * np.uint8(255)
    else:
        return ori_cases.image(name)
    img.setflags(write=False)
    return img


def params_of(case):
    if case in EXTRACTION:
        return EXTRACTION[case][1]
    return CLASSIC if case.endswith("classic9") else dict()


def norm_of(case):
    kw = params_of(case)
    return kw.get("norm_mode", 0), kw.get("norm_multi", 0)


def crafted():
    """the 192 frames in OCTAVE units of octave 0: (x, y, sigma, angle, level) float32 / int"""
    rows = [(x, y, s, a, 1 + k % 3) for s in FRAME_SIGMAS for a in FRAME_ANGLES for k, (x, y) in enumerate(FRAME_POSITIONS)]
    fr = np.zeros(len(rows), [("xpos", np.float32), ("ypos", np.float32), ("sigma", np.float32), ("orientation", np.float32),
                              ("level", np.int32)])
    for i, r in enumerate(rows):
        fr[i] = r
    return fr


def describe_frames(frame_dtype, upscale=1):
    """the crafted frames as the describe path takes them: image units (octave units halved, exactly), octave hint 0"""
    c = crafted()
    fr = np.zeros(len(c), frame_dtype)
    for n in ("xpos", "ypos", "sigma"):
        fr[n] = np.ldexp(c[n], -upscale)
    fr["orientation"], fr["octave"], fr["level"] = c["orientation"], 0, c["level"]
    return fr


class Reference:
    """orc: the oracle after its run (nobody changes it); rows: per descriptor (octave, lpos, x, y, sigma, angle) in the
    order of desc; desc / raw: the oracle's descriptors and raw histograms; patches: desc_rule.samples of every row."""

    def __init__(self, case, orc, rows, desc, raw):
        self.case, self.orc, self.rows, self.desc, self.raw = case, orc, rows, desc, raw
        self.norm = norm_of(case)
        self._rules = {}
        planes = {}
        self.patches = []
        for o, l, x, y, s, a in rows:
            if (o, l) not in planes:
                planes[(o, l)] = orc.plane(o, 0, l)
            self.patches.append(desc_rule.samples(planes[(o, l)], x, y, s, a))
        self.planes = planes

    def plane(self, row):
        return self.planes[(row[0], row[1])]

    def rules(self, **kw):
        """the rule of every descriptor under desc_rule.evaluate(**kw): computed once per set of terms"""
        key = tuple(sorted(kw.items()))
        if key not in self._rules:
            self._rules[key] = [desc_rule.evaluate(p, *self.norm, **kw) for p in self.patches]
        return self._rules[key]

    def name(self, i):
        return "%s descriptor %d, octave %d level %d" % ((self.case, i) + tuple(self.rows[i][:2]))


@functools.lru_cache(maxsize=None)
def reference(O, case):
    """computed once per case and shared"""
    kw = params_of(case)
    n_planes = kw.get("levels", 3) + 3
    if case in EXTRACTION:
        orc = O.Oracle(O.default_params(**kw), threads=8).run(image(EXTRACTION[case][0]))
        ext = orc.extrema()
        feats, desc = orc.fetch()
        rows = [None] * len(desc)
        for e, f in zip(ext, feats):
            for k in range(int(f["num_ori"])):
                rows[f["desc_idx"][k]] = (int(e["octave"]), min(max(int(e["lpos"]), 0), n_planes - 1), e["xpos"], e["ypos"],
                                          e["sigma"], f["orientation"][k])
        return Reference(case, orc, rows, desc, orc.raw_descriptors())
    c = crafted()
    ext = np.zeros(len(c), O.EXTREMUM_DTYPE)
    ext["xpos"], ext["ypos"], ext["sigma"], ext["lpos"], ext["cell"] = c["xpos"], c["ypos"], c["sigma"], c["level"], np.arange(len(c))
    orc = O.Oracle(O.default_params(**kw), threads=8).run(image(case.split("-")[0][len("frames_"):]), keypoints=False).run_from_extrema(ext)
    feats, _ = orc.fetch()
    assert (feats["num_ori"] >= 1).all()          # redo_descriptors keeps the number of orientations
    ori = np.zeros((len(c), 4), np.float32)
    ori[:] = c["orientation"][:, None]
    feats, desc = orc.redo_descriptors(ori).fetch()
    first = feats["desc_idx"][:, 0]
    rows = [(0, int(f["level"]), f["xpos"], f["ypos"], f["sigma"], f["orientation"]) for f in c]
    return Reference(case, orc, rows, desc[first], orc.raw_descriptors()[first])
