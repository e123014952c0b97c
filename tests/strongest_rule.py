"""The keep-strongest rule of include/popsift_hip.h (popsift_hip_set_keep_strongest) in numpy: the response of a refined
extremum and which records of an image stay.  tests/test_strongest_rule.py holds it to hand-made cases and to the CPU
oracle's output, tests/test_gpu_strongest.py holds the device to it, bit for bit."""
import numpy as np

INT32_MAX = 2 ** 31 - 1


def dog_planes(src, n_oct, levels):
    """planes[o][d], d = 0 .. levels + 1, of anything with plane(octave, kind, level) (an Oracle or a Context)"""
    return [[src.plane(o, 1, d) for d in range(levels + 2)] for o in range(n_oct)]


def responses(planes, dims, extrema, levels):
    """float32 response per record of `extrema` (xpos, ypos, lpos, octave): |D| at the sample nearest to the refined
    position, level clamped to the search levels; NaN for a non-finite position.  planes[o][d]: DoG plane d of octave o
    as an (h, w) float32 array; dims[o] = (w, h)."""
    out = np.full(len(extrema), np.nan, np.float32)
    for i, e in enumerate(extrema):
        x, y = np.float32(e["xpos"]), np.float32(e["ypos"])
        if not (np.isfinite(x) and np.isfinite(y)):
            continue
        w, h = dims[int(e["octave"])]
        xi = min(max(int(np.floor(x + np.float32(0.5))), 0), w - 1)
        yi = min(max(int(np.floor(y + np.float32(0.5))), 0), h - 1)
        di = min(max(int(e["lpos"]), 1), levels)
        out[i] = np.abs(np.float32(planes[int(e["octave"])][di][yi, xi]))
    return out


def keys(resp):
    """uint32 selection keys: 0 for NaN, else the bit pattern (responses are >= 0, so bit order is numeric order)"""
    r = np.ascontiguousarray(resp, np.float32)
    return np.where(np.isnan(r), np.uint32(0), r.view(np.uint32)).astype(np.uint32)


def keep_mask(resp, n):
    """bool per record: with more than n records, those whose key is at least the n-th largest key (every tie with the
    n-th included); otherwise all"""
    k = keys(resp)
    if n < 1:
        raise ValueError("n >= 1")
    if len(k) <= n:
        return np.ones(len(k), bool)
    t = np.sort(k)[len(k) - n]
    return k >= t
