"""popsift_hip_ransac_many without a GPU: the layout and the defaults of its options through the binding, the defines, and
the ERR_INVALID cases that are answered before a verifier is looked at."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layout_defines_and_defaults(hip, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "popsift_hip.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(popsift_hip_ransac_many_opts), offsetof(popsift_hip_ransac_many_opts, kind),
           offsetof(popsift_hip_ransac_many_opts, hypotheses), offsetof(popsift_hip_ransac_many_opts, max_err),
           offsetof(popsift_hip_ransac_many_opts, seed), offsetof(popsift_hip_ransac_many_opts, reserved),
           sizeof(popsift_hip_ransac_result), POPSIFT_HIP_RANSAC_MANY_GROUP, POPSIFT_HIP_RANSAC_MANY_SEGMENT);
    return 0;
}
""")
    exe = str(tmp_path / "layout.bin")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = list(map(int, subprocess.check_output([exe], text=True).split()))
    O = hip.RansacManyOpts
    assert got == [C.sizeof(O), O.kind.offset, O.hypotheses.offset, O.max_err.offset, O.seed.offset, O.reserved.offset,
                   hip.RANSAC_RESULT_DTYPE.itemsize, hip.RANSAC_MANY_GROUP, hip.RANSAC_MANY_SEGMENT]
    assert got[:7] == [32, 0, 4, 8, 12, 16, 52]
    o = O()
    C.memset(C.byref(o), 0x55, C.sizeof(o))
    hip.lib().popsift_hip_default_ransac_many_opts(C.byref(o))
    assert (o.kind, o.hypotheses, o.max_err, o.seed, list(o.reserved)) == (hip.REFIT_HOMOGRAPHY, 2048, 2.0, 0, [0, 0, 0, 0])
    hip.lib().popsift_hip_default_ransac_many_opts(None)            # tolerated
    # the one numbering of the kinds
    assert [hip.ransac_many_opts(k).kind for k in ("homography", "affine", "epipolar")] == [0, 1, 2]
    o = hip.ransac_many_opts("epipolar", 77, 1.5, 9)
    assert (o.kind, o.hypotheses, o.max_err, o.seed) == (2, 77, 1.5, 9)


def test_invalid_arguments_are_rejected_without_a_verifier(hip):
    lib = hip.lib()
    pts, res = np.zeros((8, 4), np.float32), np.zeros(2, hip.RANSAC_RESULT_DTYPE)
    good = hip.ransac_many_opts(hypotheses=8, max_err=1.0)
    for off in ([0, 3, 8], [1, 3, 8], [0, 5, 4], [0, -1, 8], [0, 8, (1 << 24) + 1]):
        o = np.array(off, np.int32)
        assert lib.popsift_hip_ransac_many(None, pts.ctypes.data, o.ctypes.data, 2, C.byref(good), res.ctypes.data, None) == \
            hip.ERR_INVALID, off
        assert lib.popsift_hip_ransac_many_trace(None, pts.ctypes.data, o.ctypes.data, 2, C.byref(good), None, None, None, None,
                                                 None) == hip.ERR_INVALID, off
    assert not res.view(np.uint8).any()
    assert lib.popsift_hip_verifier_debug_set_group(None, 0) == hip.ERR_INVALID
