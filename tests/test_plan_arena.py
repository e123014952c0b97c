"""popsift_hip_plan_arena: the pyramid's geometry without a device.  Detection and refinement address a plane element
as the arena's base plus an unsigned 32-bit byte offset, so a pyramid whose arena reaches 4 GiB is refused where it is
planned -- before anything is allocated, which is why this can be tested on a machine without a GPU."""
import math

import pytest

PITCH = 64  # floats: rows start on 256 B (data layout)


def arena_bytes(bw, bh, n_oct, levels=3, store_dog=0):
    """the layout of DESIGN.md: per octave L Gaussian planes (+ L-1 DoG planes when stored), else one scratch plane"""
    L = levels + 3
    total, w, h, first = 0, bw, bh, None
    for _ in range(n_oct):
        plane = (w + PITCH - 1) // PITCH * PITCH * h
        first = plane if first is None else first
        total += plane * (L if not store_dog else 2 * L - 1)
        w, h = math.ceil(w / 2), math.ceil(h / 2)
    if not store_dog:
        total += first
    return 4 * total


@pytest.mark.parametrize("w,h,n_oct", [(1920, 1080, 9), (3840, 2160, 10), (640, 480, 7)])
def test_plan_of_the_benchmark_sizes(hip, w, h, n_oct):
    rc, octaves, nbytes = hip.plan_arena(w, h)
    assert rc == hip.OK and octaves == n_oct
    assert nbytes == arena_bytes(2 * w, 2 * h, n_oct)
    rc, octaves, nbytes = hip.plan_arena(w, h, hip.default_params(store_dog=1, upscale_factor=0.0, octaves=4, levels=5))
    assert rc == hip.OK and octaves == 4 and nbytes == arena_bytes(w, h, 4, levels=5, store_dog=1)


def test_arena_of_4_gib_is_refused_exactly_at_4_gib(hip):
    # one octave, no up-scaling: 7 planes of 16384 x h floats = 458752 * h bytes; 2^32 / 458752 = 9362.3
    p = hip.default_params(upscale_factor=0.0, octaves=1)
    assert arena_bytes(16384, 9362, 1) < 2 ** 32 <= arena_bytes(16384, 9363, 1)
    assert hip.plan_arena(16384, 9362, p) == (hip.OK, 1, arena_bytes(16384, 9362, 1))
    assert hip.plan_arena(16384, 9363, p) == (hip.ERR_INVALID, 1, arena_bytes(16384, 9363, 1))
    # exactly 2^32 bytes: 8 planes (levels = 4) of 16384 x 8192
    p = hip.default_params(upscale_factor=0.0, octaves=1, levels=4)
    assert arena_bytes(16384, 8192, 1, levels=4) == 2 ** 32
    assert hip.plan_arena(16384, 8192, p) == (hip.ERR_INVALID, 1, 2 ** 32)
    assert hip.plan_arena(16384, 8191, p)[0] == hip.OK
    # the default configuration up-scales by two: an 8K image has a 15360 x 8640 base plane and 4.8 GB of planes
    rc, octaves, nbytes = hip.plan_arena(7680, 4320)
    assert rc == hip.ERR_INVALID and nbytes == arena_bytes(15360, 8640, octaves) >= 2 ** 32
    assert hip.plan_arena(7680, 4320, hip.default_params(upscale_factor=0.0))[0] == hip.OK


def test_plan_refuses_what_a_submit_refuses(hip):
    assert hip.plan_arena(0, 10)[0] == hip.ERR_INVALID
    assert hip.plan_arena(20000, 100)[0] == hip.ERR_INVALID                       # 40000 pixels wide after up-scaling
    assert hip.plan_arena(100, 100, hip.default_params(sigma=2.5))[0] == hip.ERR_INVALID
    assert hip.lib().popsift_hip_plan_arena(None, 10, 10, None, None) == hip.ERR_INVALID
    import ctypes as C
    p = hip.default_params()
    assert hip.lib().popsift_hip_plan_arena(C.byref(p), 320, 240, None, None) == hip.OK
