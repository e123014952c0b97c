"""The ScaleDirect scaling mode (Config::ScaleDirect, params.scale_direct = 1) without a GPU: the C ABI accepts it,
rejects what stays unsupported, and the CPU restatement the GPU tests compare with (tests/scale_direct_ref.c) reproduces
the oracle's default-mode pyramid bit for bit, which pins its order of arithmetic."""
import ctypes as C

import numpy as np
import pytest

from popsift_amd.synth import synth
from scale_direct import MAX_OCT, Ref
from util import bits


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return Ref(tmp_path_factory.mktemp("scale_direct_ref"))


def test_context_creation_accepts_scale_direct(hip):
    lib = hip.lib()
    h = C.c_void_p()
    assert (hip.SCALE_DEFAULT, hip.SCALE_DIRECT) == (0, 1)
    assert hip.default_params().scale_direct == hip.SCALE_DEFAULT
    for gauss_mode in (hip.GAUSS_VLFEAT_COMPUTE, hip.GAUSS_VLFEAT_RELATIVE_ALL, hip.GAUSS_OPENCV_COMPUTE):
        p = hip.default_params(scale_direct=hip.SCALE_DIRECT, gauss_mode=gauss_mode)
        rc = lib.popsift_hip_ctx_create(0, C.byref(p), C.byref(h))
        try:
            assert rc == (hip.OK if hip.device_count() > 0 else hip.ERR_NO_DEVICE), (gauss_mode, rc)
        finally:
            if rc == hip.OK:
                lib.popsift_hip_ctx_destroy(h)


def test_rejections(hip):
    lib = hip.lib()
    h = C.c_void_p()
    for v in (2, -1, 7):
        p = hip.default_params(scale_direct=v)
        assert lib.popsift_hip_ctx_create(0, C.byref(p), C.byref(h)) == hip.ERR_INVALID, v
    # vlfeat-hw-interpolated, fixed9 and fixed15 stay rejected in this mode too
    for mode in (hip.GAUSS_VLFEAT_RELATIVE, hip.GAUSS_FIXED9, hip.GAUSS_FIXED15):
        p = hip.default_params(scale_direct=1, gauss_mode=mode)
        assert lib.popsift_hip_ctx_create(0, C.byref(p), C.byref(h)) == hip.ERR_INVALID, mode
    assert lib.popsift_hip_get_gauss_table_dd(None, None, None, None, None) == hip.ERR_INVALID
    assert hip.DEBUG_SCALE_PATH == 13 and hip.DEBUG_DIRECT_PATH == 11
    assert C.sizeof(hip.Params) == 19 * 4 + 4  # the struct keeps its size: scale_direct took one reserved word


@pytest.mark.parametrize("kw", [dict(), dict(levels=2, sigma=2.0), dict(levels=5), dict(assume_initial_blur=0),
                                dict(upscale_factor=0.0, sigma=1.3), dict(upscale_factor=-1.0),
                                dict(gauss_mode=3, sift_mode=1), dict(gauss_mode=2), dict(sigma=0.5)])
def test_dd_table(ref, oracle_mod, kw):
    """dd against its closed form, dd[0] equal to inc[0] bit for bit, the mode's span rule, normalised rows; inc is the
    oracle's table"""
    O = oracle_mod
    p = O.default_params(**kw)
    # the oracle takes Gauss modes 0 and 3; mode 2's inc table and span rule are mode 0's
    f, span, sig = O.Oracle(O.default_params(**dict(kw, gauss_mode=0 if p.gauss_mode == 2 else p.gauss_mode))).gauss_table()
    t = ref.tables(p)
    assert np.array_equal(bits(t["inc"][0]), bits(f)) and np.array_equal(t["inc"][1], span)
    df, dspan, dsig = t["dd"]
    assert df.shape == (MAX_OCT, 32)
    f32 = np.float32
    ib = f32(p.initial_blur) * f32(2.0) ** f32(p.upscale_factor) if p.assume_initial_blur else f32(0.0)
    for o in range(MAX_OCT):
        s = np.ldexp(f32(p.sigma), o).astype(f32)
        want = np.ldexp(np.sqrt(np.abs(f32(s * s) - f32(ib * ib))).astype(f32), -o).astype(f32)
        assert bits(dsig[o:o + 1])[0] == bits(np.array([want], f32))[0], (o, dsig[o], want)
        if p.gauss_mode == 3:
            want_span = min(((int(np.round(f32(8.0) * dsig[o] + f32(1.0))) | 1) >> 1) + 1, 31)
        else:
            want_span = min(int(np.ceil(f32(4.0) * dsig[o])) + 1, 31)
        assert dspan[o] == want_span, (o, dspan[o], want_span)
        assert df[o, dspan[o]:].max(initial=0) == 0
        assert abs(float(df[o, 0]) + 2 * float(df[o, 1:dspan[o]].sum()) - 1.0) < 1e-5
    # octave 0 is the default mode's: dd[0] is inc[0] bit for bit
    assert np.array_equal(bits(df[0]), bits(f[0])) and dspan[0] == span[0] and bits(dsig[:1])[0] == bits(sig[:1])[0]
    # the blur approaches sigma0 (in octave pixels) as the assumed input blur shrinks against sigma0 * 2^o
    assert abs(float(dsig[-1]) - p.sigma) < 1e-5


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
    planes = ref.pyramid(img, p, dims, scale_direct=0)
    L = len(planes[0])
    for o in range(len(dims)):
        for l in range(L):
            assert np.array_equal(bits(planes[o][l]), bits(orc.plane(o, 0, l))), (name, o, l)


@pytest.mark.parametrize("kw", [dict(), dict(upscale_factor=0.0, sift_mode=1), dict(gauss_mode=3, levels=2, sigma=2.0)])
def test_scale_direct_octave0_is_the_oracles(ref, oracle_mod, kw):
    """ScaleDirect on the restatement: octave 0 is the oracle's (default-mode) octave 0, every level; the later octaves
    start from the input image, not from level L-3 of the octave before, so they differ"""
    O = oracle_mod
    img = synth(5, 120, 90)
    p = O.default_params(**kw)
    orc = O.Oracle(p).run(img, keypoints=False)
    dims = [orc.octave_dims(o) for o in range(orc.num_octaves)]
    d = ref.pyramid(img, p, dims, scale_direct=1)
    L = len(d[0])
    for l in range(L):
        assert np.array_equal(bits(d[0][l]), bits(orc.plane(0, 0, l))), l
    assert len(dims) >= 2
    for o in range(1, len(dims)):
        assert not np.array_equal(d[o][0], orc.plane(o, 0, 0)), o
        # still a smoothed copy of the same image at the same scale
        assert np.abs(d[o][0] - orc.plane(o, 0, 0)).mean() < 0.1 * np.abs(orc.plane(o, 0, 0)).mean() + 1.0
