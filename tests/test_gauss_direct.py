"""The vlfeat-direct Gauss mode (Config::VLFeat_Relative_All) without a GPU: the C ABI accepts it, and the CPU
restatement the GPU tests compare with (tests/gauss_direct_ref.c) reproduces the oracle's default-mode pyramid bit for
bit, which pins its order of arithmetic."""
import ctypes as C

import numpy as np
import pytest

from gauss_direct import Ref
from popsift_amd.synth import synth
from util import bits


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return Ref(tmp_path_factory.mktemp("gauss_direct_ref"))


def test_context_creation_accepts_vlfeat_direct(hip):
    lib = hip.lib()
    h = C.c_void_p()
    p = hip.default_params(gauss_mode=hip.GAUSS_VLFEAT_RELATIVE_ALL)
    rc = lib.popsift_hip_ctx_create(0, C.byref(p), C.byref(h))
    try:
        assert rc == (hip.OK if hip.device_count() > 0 else hip.ERR_NO_DEVICE), rc
    finally:
        if rc == hip.OK:
            lib.popsift_hip_ctx_destroy(h)
    # vlfeat-hw-interpolated (texture-unit blending), fixed9 and fixed15 stay rejected
    for mode in (hip.GAUSS_VLFEAT_RELATIVE, hip.GAUSS_FIXED9, hip.GAUSS_FIXED15):
        p = hip.default_params(gauss_mode=mode)
        assert lib.popsift_hip_ctx_create(0, C.byref(p), C.byref(h)) == hip.ERR_INVALID, mode
    assert lib.popsift_hip_get_gauss_table_abs0(None, None, None, None, None) == hip.ERR_INVALID
    assert hip.DEBUG_DIRECT_PATH == 11


@pytest.mark.parametrize("kw", [dict(), dict(levels=2, sigma=2.0), dict(levels=5), dict(assume_initial_blur=0),
                                dict(upscale_factor=0.0, sigma=1.3), dict(gauss_mode=3, sift_mode=1)])
def test_tables(ref, oracle_mod, kw):
    """inc equals the oracle's table; abs_o0 level 0 equals inc level 0; abs_o0 spans follow the VLFeat rule, the top
    level of (sigma 2, 2 levels) reaching the 31-tap cap (a halo of 30)"""
    O = oracle_mod
    f, span, sig = O.Oracle(O.default_params(**kw)).gauss_table()
    t = ref.tables(O.default_params(**kw))
    assert np.array_equal(bits(t["inc"][0]), bits(f)) and np.array_equal(t["inc"][1], span)
    assert np.array_equal(bits(t["inc"][2]), bits(sig))
    af, aspan, asig = t["abs0"]
    assert np.array_equal(bits(af[0]), bits(f[0])) and aspan[0] == span[0] and asig[0] == sig[0]
    assert np.all(np.diff(asig) > 0) and np.all(aspan <= 31) and np.all(aspan >= 2)
    for l in range(len(aspan)):
        assert aspan[l] == min(int(np.ceil(np.float32(4.0) * asig[l]) + 1), 31)
        assert af[l, aspan[l]:].max(initial=0) == 0
        assert abs(float(af[l, 0]) + 2 * float(af[l, 1:aspan[l]].sum()) - 1.0) < 1e-5
    if kw == dict(levels=2, sigma=2.0):
        assert aspan[-1] == 31


@pytest.mark.parametrize("name,kw,shape,f32", [
    ("default_96x64", dict(), (96, 64), False),
    ("upscale0_odd_101x77", dict(upscale_factor=0.0), (101, 77), False),
    ("opencv_down_150x130", dict(upscale_factor=-1.0, sift_mode=1, gauss_mode=3), (150, 130), False),
    ("f32_levels4_80x60", dict(levels=4, sigma=1.3), (80, 60), True),
])
def test_restatement_reproduces_oracle_default_pyramid(ref, oracle_mod, name, kw, shape, f32):
    O = oracle_mod
    w, h = shape
    img = synth(40 + len(name), w, h)
    if f32:
        img = img.astype(np.float32) / 256.0
    p = O.default_params(**kw)
    orc = O.Oracle(p, threads=4).run(img, keypoints=False)
    dims = [orc.octave_dims(o) for o in range(orc.num_octaves)]
    planes = ref.pyramid(img, p, dims, direct=0)
    L = len(planes[0])
    for o in range(len(dims)):
        for l in range(L):
            assert np.array_equal(bits(planes[o][l]), bits(orc.plane(o, 0, l))), (name, o, l)


def test_direct_pyramid_shares_level0_and_the_incremental_octaves(ref, oracle_mod):
    """vlfeat-direct against the default mode on the restatement: octave 0 level 0 is the same plane, the other
    octave-0 levels differ (and are blurrier), and octave 1 starts from every second pixel of octave 0's level L-3"""
    O = oracle_mod
    img = synth(5, 120, 90)
    p = O.default_params()
    orc = O.Oracle(p).run(img, keypoints=False)
    dims = [orc.octave_dims(o) for o in range(orc.num_octaves)]
    d = ref.pyramid(img, p, dims, direct=1)
    s = ref.pyramid(img, p, dims, direct=0)
    L = len(d[0])
    assert np.array_equal(bits(d[0][0]), bits(s[0][0]))
    for l in range(1, L):
        assert not np.array_equal(d[0][l], s[0][l])
        assert np.abs(np.diff(d[0][l], axis=1)).mean() < np.abs(np.diff(d[0][l - 1], axis=1)).mean()
    assert np.array_equal(bits(d[1][0]), bits(d[0][L - 3][::2, ::2][:dims[1][1], :dims[1][0]]))
