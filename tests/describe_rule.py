"""numpy restatement of how popsift_hip_describe_batch places a frame (include/popsift_hip.h): octave and level derived
from sigma when the hints are -1, the frame scaled into its octave, and the validity rules.  float32 throughout, as on the
device; log2 may differ from the device's log2f in the last bit, which moves a result only next to a .5 boundary."""
import numpy as np

SIGMA_MAX = np.float32(8.0)  # POPSIFT_HIP_FRAME_SIGMA_MAX


def derive(sigma, sigma0, levels, up, n_oct):
    """(octave, the boundary distance of t - 0.5 / levels) for frames with octave = -1"""
    f32 = np.float32
    sigma = np.asarray(sigma, f32)
    with np.errstate(all="ignore"):
        t = np.log2(sigma / f32(sigma0)) + f32(up)
        u = t - f32(0.5) / f32(levels)
        o = np.clip(np.floor(u), 0, n_oct - 1)
    o = np.where(np.isfinite(o), o, 0).astype(np.int32)
    return o, np.abs(u - np.round(u))


def level(sigma_oct, sigma0, levels, L):
    """(lpos, the distance of sn from a .5 boundary) for frames with level = -1: roundf(levels * log2f(sigma_oct / sigma0))"""
    f32 = np.float32
    with np.errstate(all="ignore"):
        sn = f32(levels) * np.log2(np.asarray(sigma_oct, f32) / f32(sigma0))
        r = np.where(np.abs(sn - np.trunc(sn)) == f32(0.5), np.trunc(sn) + np.sign(sn), np.round(sn))  # roundf: half away from 0
        lp = np.clip(r, 0, L - 1)
    lp = np.where(np.isfinite(lp), lp, 0).astype(np.int32)
    return lp, np.abs(np.abs(sn - np.floor(sn)) - f32(0.5))


def resolve(frames, sigma0, levels, up, dims, given=False):
    """-> (octave, lpos, x_oct, y_oct, sigma_oct) per frame; octave = -1 marks an invalid frame.  dims: (w, h) per octave."""
    f32 = np.float32
    n_oct, L = len(dims), levels + 3
    fr = np.asarray(frames)
    x, y, s = fr["xpos"].astype(f32), fr["ypos"].astype(f32), fr["sigma"].astype(f32)
    ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(s) & (s > 0)
    if given:
        ok &= np.isfinite(fr["orientation"])
    ho, hl = fr["octave"].astype(np.int64), fr["level"].astype(np.int64)
    ok &= (ho >= -1) & (ho < n_oct) & (hl >= -1) & (hl < L)
    o_der, _ = derive(np.where(ok, s, f32(1)), sigma0, levels, up, n_oct)
    o = np.where(ho >= 0, ho, o_der).astype(np.int32)
    o = np.where(ok, o, 0)
    sh = (up - o).astype(np.int32)
    xo, yo, so = np.ldexp(x, sh).astype(f32), np.ldexp(y, sh).astype(f32), np.ldexp(s, sh).astype(f32)
    w = np.array([d[0] for d in dims], np.int64)[o]
    h = np.array([d[1] for d in dims], np.int64)[o]
    with np.errstate(invalid="ignore"):
        ok &= (xo >= 0) & (xo <= (w - 1).astype(f32)) & (yo >= 0) & (yo <= (h - 1).astype(f32))
        ok &= (so > 0) & (so <= SIGMA_MAX)
    l_der, _ = level(np.where(ok, so, f32(sigma0)), sigma0, levels, L)
    lp = np.where(hl >= 0, hl, l_der).astype(np.int32)
    return np.where(ok, o, -1).astype(np.int32), lp, xo, yo, so


def octave_dims(w, h, upscale, n_oct):
    """the octave sizes the library plans for a w x h image (plan_dims, popsift.cpp:89-120)"""
    bw, bh = int(np.ceil(w * 2.0 ** upscale)), int(np.ceil(h * 2.0 ** upscale))
    dims = []
    for _ in range(n_oct):
        dims.append((bw, bh))
        bw, bh = int(np.ceil(bw / 2.0)), int(np.ceil(bh / 2.0))
    return dims
