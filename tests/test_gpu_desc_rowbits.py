"""k_descriptor finds the patch row of a sample from row-end bits: the rows' column intervals of a pass lie end to end
as one flat list, a bit marks the last position of every row, and the row of a position is the number of bits below it.
A pass ends after DESC_ROWS rows or DESC_LIST list positions, whichever comes first -- in the second case inside a
row, and the next pass takes the rest of that row.  The histogram sums are integers, so where the passes are cut must
not show in a single bit of a descriptor; and patches that the image border cuts (rows without a sample at the start
or the end of a pass, intervals clamped on either side) must come out as the oracle's."""
import numpy as np
import pytest

from popsift_amd.synth import synth
from util import bits, feature_parity, sorted_features

pytestmark = pytest.mark.gpu

DESC_MAGNIFY = 3.0


def extract(hip, img, rows=None, lst=None):
    ctx = hip.Context(hip.default_params())
    if rows:
        ctx.debug_set(hip.DEBUG_DESC_ROWS, rows)
    if lst:
        ctx.debug_set(hip.DEBUG_DESC_LIST, lst)
    ctx.submit(img)
    f, d = ctx.fetch()
    ctx.close()
    return f, d


def clipped_boxes(orc):
    """Per descriptor of the oracle's features: is the bounding box of its patch (the union of the 16 rotated cell boxes,
    2.5 * (|cos| + |sin|) * 3 sigma around the keypoint, in the pixels of its octave) cut by the plane's border, i.e.
    does it reach beyond the pixels 1 .. w - 2, 1 .. h - 2 that have a gradient."""
    fo, _ = orc.fetch()
    up = int(orc.params.upscale_factor)
    out = []
    for f in fo:
        o = int(f["debug_octave"])
        w, h = orc.octave_dims(o)[:2]
        scl = 2.0 ** (o - up)
        x, y, s = float(f["xpos"]) / scl, float(f["ypos"]) / scl, float(f["sigma"]) / scl
        for k in range(int(f["num_ori"])):
            a = float(f["orientation"][k])
            r = 2.5 * (abs(np.cos(a)) + abs(np.sin(a))) * DESC_MAGNIFY * s
            out.append(np.floor(x - r) < 1 or np.floor(y - r) < 1 or np.floor(x + r) + 1 > w - 2 or np.floor(y + r) + 1 > h - 2)
    return np.array(out, bool)


def test_pass_splits_are_invisible(gpu_hip):
    """synth(7, 320, 240), default parameters: 2749 features, 3385 descriptors, patches of 586 .. 5175 list positions
    (the largest take two passes at the default capacity).  Passes of 8 rows; of 64 positions (every pass is one step);
    of 65 (a pass ends one position into its second step); of 19 rows or 200 positions, whichever comes first; and a
    list size beyond the capacity, which clamps to it: all bit for bit the default's descriptors."""
    img = synth(7, 320, 240)
    f0, d0 = sorted_features(*extract(gpu_hip, img))
    assert len(d0) > 2000
    for rows, lst in ((8, None), (None, 64), (None, 65), (19, 200), (None, 4096)):
        f, d = sorted_features(*extract(gpu_hip, img, rows, lst))
        assert np.array_equal(bits(f["xpos"]), bits(f0["xpos"])), (rows, lst)
        assert np.array_equal(bits(d), bits(d0)), (rows, lst)


@pytest.fixture(scope="module")
def border_case(oracle_mod, gpu_hip):
    img = synth(7, 96, 72)
    orc = oracle_mod.Oracle(oracle_mod.default_params(), threads=8).run(img)
    return img, orc, extract(gpu_hip, img)


def test_patches_cut_by_every_border(border_case):
    """synth(7, 96, 72), default parameters: the oracle gives 223 features and 268 descriptors, and the image is so small
    that the bounding boxes of more than half of the patches are cut by the border of their plane.  The parent of this
    change passes the same bars on this image, so seed and size are the first choice."""
    img, orc, (fh, dh) = border_case
    clipped = clipped_boxes(orc)
    assert len(clipped) >= 200 and 3 * int(clipped.sum()) >= len(clipped), (len(clipped), int(clipped.sum()))
    ok, msg, _ = feature_parity(orc, fh, dh)
    assert ok, msg


def test_cut_patches_in_short_passes(gpu_hip, border_case):
    """The same image in passes of 8 rows or 64 positions: bit for bit the result of the default passes."""
    img, _, (fh, dh) = border_case
    f0, d0 = sorted_features(fh, dh)
    f, d = sorted_features(*extract(gpu_hip, img, 8, 64))
    assert len(d0) >= 200
    assert np.array_equal(bits(f["xpos"]), bits(f0["xpos"]))
    assert np.array_equal(bits(d), bits(d0))
