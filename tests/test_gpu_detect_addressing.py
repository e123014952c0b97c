"""k_detect and k_refine address the planes as a scalar base plus 32-bit byte offsets: per wave the octave's record,
the row base and the plane bases, per lane three column offsets that hold for a whole strip (extrema.hip).  These are
the shapes at which that can go wrong, each compared with the CPU oracle bit for bit like the parity tests:

  widths  65, 66, 127, 129, 130 -- one and two strips of 64 columns, the last strip's clamped centre and right column,
          w - 2 on both sides of a multiple of 64;
  heights 34, 35, 66, 67 -- the clamp of a strip's last row, the fetch of the row below it by the last load group, one
          and three load groups of four rows;
  up-scaling on and off, two and three octaves -- plane stride and pitch differ from octave to octave, pitch != width
          (up-scaled, it is octave 1 that has the size named here);
  the three SIFT modes -- the OpenCV mode leaves out a border of 5 rows and columns.

A batch takes its slot, and with it its arena, from blockIdx.y; the SLOW instance of k_detect walks the same strips row
by row."""
import numpy as np
import pytest

from popsift_amd.synth import synth
from test_gpu_parity import assert_keypoints_match
from util import bits, sorted_features

pytestmark = pytest.mark.gpu

WIDTHS = (65, 66, 127, 129, 130)
HEIGHTS = (34, 35, 66, 67)
MODES = {"popsift": 0, "opencv": 1, "vlfeat": 2}


def ext_key(e, sigma=True):
    """device against device: every field bit for bit.  Against the oracle without sigma, which goes through powf (an
    ulp between the two libraries; the parity tests compare octave, level and position as well)"""
    cols = [e["octave"].tolist(), e["lpos"].tolist(), bits(e["xpos"]).tolist(), bits(e["ypos"]).tolist()]
    return sorted(zip(*(cols + ([bits(e["sigma"]).tolist()] if sigma else []))))


@pytest.mark.parametrize("octaves", [2, 3])
@pytest.mark.parametrize("upscale", [1.0, 0.0], ids=["upscaled", "plain"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_strip_and_row_edges_match_the_oracle(oracle_mod, gpu_hip, mode, upscale, octaves):
    kw = dict(sift_mode=MODES[mode], upscale_factor=upscale, octaves=octaves)
    ctx = gpu_hip.Context(gpu_hip.default_params(**kw))       # one context: every size lays the planes out anew
    total = 0
    for w in WIDTHS:
        for h in HEIGHTS:
            img = synth(1000 + 7 * w + h, w, h)
            orc = oracle_mod.Oracle(oracle_mod.default_params(**kw), threads=4).run(img)
            ctx.submit(img)
            assert ctx.report().num_octaves == orc.num_octaves == octaves
            assert ctx.octave_dims(octaves - 1) == orc.octave_dims(octaves - 1)
            try:
                assert_keypoints_match(orc, ctx)
            except AssertionError as e:
                raise AssertionError("%d x %d %s: %s" % (w, h, kw, e))
            total += len(orc.extrema())
    ctx.close()
    # the comparison is of something (the oracle finds 330 .. 3448 extrema over the twenty images of a case)
    assert total >= 300, total


@pytest.mark.parametrize("mode", sorted(MODES))
def test_batch_slots_equal_single_submits(oracle_mod, gpu_hip, mode):
    kw = dict(sift_mode=MODES[mode], octaves=3)
    for w, h in ((129, 67), (66, 35)):
        imgs = [synth(2000 + 3 * w + k, w, h) for k in range(3)]
        single = gpu_hip.Context(gpu_hip.default_params(**kw))
        want = []
        for im in imgs:
            f, d = sorted_features(*single.submit(im).fetch())
            want.append((ext_key(single.extrema()), bits(f["xpos"]), bits(f["ypos"]), bits(f["sigma"]), bits(d)))
        assert len({tuple(x[0]) for x in want}) == 3 and min(len(x[0]) for x in want) > 0   # three different results
        ctx = gpu_hip.Context(gpu_hip.default_params(**kw))
        ctx.submit_batch(imgs)
        assert len(ctx.wait_batch()) == 3
        for k in range(3):
            f, d = sorted_features(*ctx.fetch_item(k))
            got = (bits(f["xpos"]), bits(f["ypos"]), bits(f["sigma"]), bits(d))
            assert all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got, want[k][1:])), (w, h, k)
        # image 0 of the batch against the oracle as well (the debug views show slot 0)
        orc = oracle_mod.Oracle(oracle_mod.default_params(**kw), threads=4).run(imgs[0])
        assert ext_key(ctx.extrema()) == want[0][0]
        assert ext_key(ctx.extrema(), sigma=False) == ext_key(orc.extrema(), sigma=False)
        ctx.close()
        single.close()


@pytest.mark.parametrize("mode", sorted(MODES))
def test_slow_instance_finds_the_fast_path_s_extrema(gpu_hip, mode):
    """A dense small image (no contrast threshold) with the fast pass's candidate queue cut to 4 entries and to none:
    (nearly) every strip is handed to the SLOW instance, which must find the same set."""
    for w, h in ((130, 67), (127, 34)):
        img = synth(77 + w, w, h)
        kw = dict(sift_mode=MODES[mode], octaves=3, threshold=0.0)
        fast = gpu_hip.Context(gpu_hip.default_params(**kw))
        e0 = ext_key(fast.submit(img).extrema())
        assert len(e0) > 100, len(e0)                 # the oracle finds 134 .. 320
        for qcap in (4, 0):
            ctx = gpu_hip.Context(gpu_hip.default_params(**kw))
            ctx.debug_set(gpu_hip.DEBUG_DET_QCAP, qcap)
            assert ext_key(ctx.submit(img).extrema()) == e0, (w, h, qcap)
            ctx.close()
        fast.close()


def test_an_arena_of_4_gib_is_refused_by_submit(gpu_hip):
    """the planning failure reaches the caller through the ordinary error path, and the context stays usable"""
    ctx = gpu_hip.Context()
    small = synth(3, 129, 67)
    want = ext_key(ctx.submit(small).extrema())
    assert gpu_hip.plan_arena(7680, 4320)[0] == gpu_hip.ERR_INVALID
    with pytest.raises(gpu_hip.PopsiftHipError) as e:
        ctx.submit(np.zeros((4320, 7680), np.uint8))
    assert e.value.status == gpu_hip.ERR_INVALID
    assert b"4 GiB" in gpu_hip.lib().popsift_hip_last_error(ctx._h)
    assert ext_key(ctx.submit(small).extrema()) == want
    ctx.close()
