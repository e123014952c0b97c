"""The raster feature order (include/popsift_hip.h, POPSIFT_HIP_ORDER_RASTER) restated in NumPy, for extrema records
(EXTREMUM_DTYPE of popsift_amd/_capi.py or of oracle/oracle.py: xpos, ypos in octave units, lpos, sigma, octave, cell).

Octave-major; within an octave ascending in the tuple
    ( iy, ix, lpos, bits(ypos), bits(xpos), bits(sigma) )
with iy = pix(ypos), ix = pix(xpos), pix(v) = 0 for NaN and v <= 0, 32767 for v >= 32767, else trunc(v); lpos as int32;
bits() the float's pattern as uint32.  Records that tie under the whole tuple are byte-identical, so any stable or
unstable sort gives the same bytes."""
import numpy as np


def pix(v):
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        pos = v > 0                                     # False for NaN
        big = v >= np.float32(32767.0)
        t = np.where(pos & ~big, v, np.float32(0.0)).astype(np.int64)   # truncation, on values that are in range
    return np.where(big, 32767, np.where(pos, t, 0)).astype(np.int64)


def bits(v):
    return np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.int64)


def columns(ext):
    """the tuple's columns, most significant first, with the octave in front"""
    return (np.asarray(ext["octave"], np.int64), pix(ext["ypos"]), pix(ext["xpos"]), np.asarray(ext["lpos"], np.int64),
            bits(ext["ypos"]), bits(ext["xpos"]), bits(ext["sigma"]))


def keys(ext):
    """(n, 7) int64: one row per record, comparable lexicographically"""
    return np.stack(columns(ext), 1) if len(ext) else np.zeros((0, 7), np.int64)


def permutation(ext):
    """indices that put the records into raster order (stable)"""
    return np.lexsort(columns(ext)[::-1])


def sort(ext):
    return ext[permutation(ext)]


def is_ordered(ext):
    """every record's key >= its predecessor's"""
    k = keys(ext)
    for a, b in zip(k[:-1].tolist(), k[1:].tolist()):
        if a > b:
            return False
    return True
