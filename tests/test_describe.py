"""Describe caller-supplied keypoints (popsift_hip_describe_batch), the parts that need no GPU: the frame record's
layout against the binding, argument checks, and the numpy restatement of the octave / level rule the GPU tests
(tests/test_gpu_describe.py) hold the device to."""
import ctypes as C
import os
import subprocess

import numpy as np

from describe_rule import SIGMA_MAX, derive, level, octave_dims, resolve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frame_layout_matches_the_header(hip, tmp_path):
    src = tmp_path / "frame.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "popsift_hip.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu %d %d %.9g\n", sizeof(popsift_hip_frame), offsetof(popsift_hip_frame, xpos),
           offsetof(popsift_hip_frame, ypos), offsetof(popsift_hip_frame, sigma), offsetof(popsift_hip_frame, orientation),
           offsetof(popsift_hip_frame, octave), offsetof(popsift_hip_frame, level), POPSIFT_HIP_ORI_COMPUTE,
           POPSIFT_HIP_ORI_GIVEN, (double)POPSIFT_HIP_FRAME_SIGMA_MAX);
    return 0;
}
""")
    exe = str(tmp_path / "frame.bin")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    v = subprocess.check_output([exe], text=True).split()
    d = hip.FRAME_DTYPE
    assert [int(x) for x in v[:7]] == [d.itemsize] + [d.fields[n][1] for n in d.names] == [24, 0, 4, 8, 12, 16, 20]
    assert (int(v[7]), int(v[8])) == (hip.ORI_COMPUTE, hip.ORI_GIVEN)
    assert float(v[9]) == float(hip.FRAME_SIGMA_MAX) == float(SIGMA_MAX)


def test_describe_rejects_bad_arguments_without_a_gpu(hip):
    L = hip.lib()
    img = np.zeros((32, 32), np.uint8)
    fr = np.zeros(3, hip.FRAME_DTYPE)
    imgs = (C.c_void_p * 1)(img.ctypes.data)
    frs = (C.c_void_p * 1)(fr.ctypes.data)
    nulls = (C.c_void_p * 1)(None)
    cnt = lambda *v: (C.c_int * len(v))(*v)
    call = lambda ctx, f, n, nb, mode: L.popsift_hip_describe_batch(ctx, imgs, f, n, nb, hip.IMG_HOST_U8, 32, 32, 32, mode)
    assert call(None, frs, cnt(3), 1, hip.ORI_COMPUTE) == hip.ERR_INVALID        # NULL context
    assert call(None, frs, cnt(3), 0, hip.ORI_COMPUTE) == hip.ERR_INVALID        # n < 1
    assert call(None, frs, cnt(-1), 1, hip.ORI_COMPUTE) == hip.ERR_INVALID       # n_frames < 0
    assert call(None, nulls, cnt(3), 1, hip.ORI_GIVEN) == hip.ERR_INVALID        # NULL frame list with frames
    assert call(None, None, None, 1, hip.ORI_GIVEN) == hip.ERR_INVALID           # no lists at all
    assert call(None, frs, cnt(3), 1, 2) == hip.ERR_INVALID                      # bad ori_mode
    assert call(None, frs, cnt(3), 1, -1) == hip.ERR_INVALID


def _sigma(o, sn, sigma0=1.6, levels=3, up=1):
    """the input-image sigma of a keypoint refinement puts at scale sn of octave o"""
    return np.float32(np.ldexp(np.float32(sigma0 * 2.0 ** (sn / levels)), o - up))


def test_rule_inverts_refinement_inside_the_band():
    """sn in [0.5, levels + 0.5) of octave o resolves to octave o and lpos = roundf(sn), for every octave and both
    upscale settings"""
    for up, levels in ((1, 3), (0, 3), (-1, 3), (1, 2), (1, 5)):
        L, n_oct = levels + 3, 6
        sn = np.linspace(0.5 + 1e-3, levels + 0.5 - 1e-3, 97)
        for o in range(n_oct):
            s = np.array([_sigma(o, v, 1.6, levels, up) for v in sn], np.float32)
            oo, dist = derive(s, 1.6, levels, up, n_oct)
            assert (oo == o).all(), (up, levels, o, sn[oo != o])
            so = np.ldexp(s, up - oo).astype(np.float32)
            lp, _ = level(so, 1.6, levels, L)
            want = np.floor(sn + 0.5).astype(np.int32)
            assert (lp == want).all(), (up, levels, o)


def test_rule_boundaries_and_clamps():
    levels, up, n_oct, L = 3, 1, 5, 6
    # sn = 0.5 exactly: octave o (t - 0.5 / levels lands on the integer), lpos roundf(0.5) = 1 -- half away from zero
    s = np.float32(np.ldexp(np.float32(1.6) * np.float32(2.0 ** (0.5 / 3)), 2 - up))
    o, dist = derive([s], 1.6, levels, up, n_oct)
    assert dist[0] < 1e-5  # a boundary case: the device's log2f may take either side
    # just inside and just outside the band of octave 2
    lo = _sigma(2, 0.5 + 1e-3)
    hi = _sigma(2, 3.5 - 1e-3)
    out_lo = _sigma(2, 0.5 - 1e-3)   # = octave 1, sn 3.499
    out_hi = _sigma(2, 3.5 + 1e-3)   # = octave 3, sn 0.501
    o, _ = derive([lo, hi, out_lo, out_hi], 1.6, levels, up, n_oct)
    assert list(o) == [2, 2, 1, 3]
    so = np.ldexp(np.array([lo, hi, out_lo, out_hi], np.float32), up - o).astype(np.float32)
    assert list(level(so, 1.6, levels, L)[0]) == [1, 3, 3, 1]
    # tiny sigma: octave 0, level 0; huge sigma: the last octave, the last level
    o, _ = derive([1e-6, 1e6], 1.6, levels, up, n_oct)
    assert list(o) == [0, n_oct - 1]
    so = np.ldexp(np.array([1e-6, 1e6], np.float32), up - o).astype(np.float32)
    assert list(level(so, 1.6, levels, L)[0]) == [0, L - 1]


def test_rule_validity():
    levels, up = 3, 1
    dims = octave_dims(64, 48, 1.0, 4)
    assert dims == [(128, 96), (64, 48), (32, 24), (16, 12)]
    fr = np.zeros(14, np.dtype([("xpos", "f4"), ("ypos", "f4"), ("sigma", "f4"), ("orientation", "f4"),
                                ("octave", "i4"), ("level", "i4")]))
    fr["xpos"], fr["ypos"], fr["sigma"], fr["octave"], fr["level"] = 10.0, 10.0, 2.0, -1, -1
    fr["xpos"][1] = np.nan
    fr["sigma"][2] = 0.0
    fr["sigma"][3] = -1.0
    fr["xpos"][4:6], fr["octave"][4:6] = 63.5, 0  # x_oct 127 in octave 0 = w_0 - 1: still inside ...
    fr["xpos"][5] = np.nextafter(np.float32(63.5), np.float32(100))  # ... one ulp more is not
    fr["ypos"][6] = -0.0                      # -0 >= 0
    fr["octave"][7] = 4                       # n_oct = 4
    fr["octave"][8] = -2
    fr["level"][9] = 6                        # L = 6
    fr["orientation"][10] = np.inf            # invalid only with given orientations
    fr["octave"][11], fr["sigma"][11] = 0, np.ldexp(SIGMA_MAX, -up)                   # sigma_oct at the cap
    fr["octave"][12], fr["sigma"][12] = 0, np.nextafter(np.ldexp(SIGMA_MAX, -up), np.float32(1e9))
    fr["octave"][13], fr["level"][13] = 2, 0  # hints are taken as given
    o, lp, x, y, s = resolve(fr, 1.6, levels, up, dims)
    assert list(o >= 0) == [True, False, False, False, True, False, True, False, False, False, True, True, False, True]
    assert (o[13], lp[13], x[13]) == (2, 0, np.float32(5.0))
    assert s[11] == SIGMA_MAX
    o, *_ = resolve(fr, 1.6, levels, up, dims, given=True)
    assert o[10] == -1
