"""The case generator of the randomised differential test (tests/fuzz_cases.py), checked without a GPU: the default
draws are the ones the fixed-seed slices of tests/test_gpu_fuzz.py were cut from, and the wide draws reach the whole
accepted parameter range."""
import hashlib

import numpy as np

import fuzz_cases


def _digest(seed, n, **kw):
    rng = np.random.default_rng(seed)
    h = hashlib.sha256()
    for case in range(n):
        k, img = fuzz_cases.random_case(rng, case, **kw)
        h.update(repr(sorted(k.items())).encode())
        h.update(repr((img.shape, str(img.dtype))).encode())
    h.update(repr(rng.bit_generator.state["state"]).encode())
    return h.hexdigest()[:16]


def test_default_stream_is_unchanged():
    """parameters, sizes, image types and the generator state after the slices of tests/test_gpu_fuzz.py, as they were
    before random_case took its `wide` option"""
    assert _digest(20261004, 60, max_w=420, max_h=320) == "059c9971281b447b"
    assert _digest(50505, 110) == "6efed4bdae395c4c"
    assert _digest(50505, 110, wide=False) == "6efed4bdae395c4c"


def test_wide_draws_cover_the_accepted_range():
    rng = np.random.default_rng(7)
    cases = [fuzz_cases.random_case(rng, c, max_w=60, max_h=40, wide=True)[0] for c in range(400)]
    assert {k["levels"] for k in cases} == set(range(10))
    assert {k["upscale_factor"] for k in cases} == {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert {k["sift_mode"] for k in cases} == {0, 1, 2}
    sig = [k["sigma"] for k in cases]
    assert 0.4 <= min(sig) < 0.5 and 1.9 < max(sig) <= 2.0
