"""ctypes front of tests/scale_direct_ref.c, the CPU restatement of the Gaussian pyramid in both scaling modes."""
import ctypes as C
import os
import subprocess

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "scale_direct_ref.c")
GA = 32
MAX_OCT = 20


class Ref:
    """Built with gcc -O2 -ffp-contract=off into `build_dir`: numpy cannot reproduce the fmaf chains bit for bit."""

    def __init__(self, build_dir):
        so = os.path.join(str(build_dir), "libscale_direct_ref.so")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, SRC, "-lm"])
        self.lib = C.CDLL(so)
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
        self.lib.sdr_tables.restype = C.c_int
        self.lib.sdr_tables.argtypes = [C.c_float, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, fp, ip, fp, fp, ip, fp]
        self.lib.sdr_pyramid.restype = C.c_int
        self.lib.sdr_pyramid.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, fp, ip, fp,
                                         ip, C.c_int, C.c_int, ip, ip, fp]

    def tables(self, p):
        """{"inc": (filter[L, 32], span[L], sigma[L]), "dd": (filter[20, 32], span[20], sigma[20])} of the params p"""
        levels = max(2, int(p.levels))
        L = levels + 3
        t = {k: (np.zeros((n, GA), np.float32), np.zeros(n, np.int32), np.zeros(n, np.float32))
             for k, n in (("inc", L), ("dd", MAX_OCT))}
        ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_float) if a.dtype == np.float32 else C.POINTER(C.c_int))
        n = self.lib.sdr_tables(p.sigma, levels, p.assume_initial_blur, p.initial_blur, p.upscale_factor, p.gauss_mode,
                                *[ptr(a) for a in t["inc"]], *[ptr(a) for a in t["dd"]])
        assert n == L
        return t

    def pyramid(self, img, p, dims, scale_direct):
        """Gaussian planes [octave][level] ((h, w) float32) for the octave sizes dims = [(w, h), ...]; scale_direct = 1:
        every octave's level 0 from the input image (ScaleDirect), 0: the default mode's pyramid"""
        t = self.tables(p)
        L = len(t["inc"][1])
        img = np.ascontiguousarray(img)
        assert img.dtype in (np.uint8, np.float32) and img.ndim == 2
        h, w = img.shape
        shift = np.float32(0.5)
        if p.sift_mode in (0, 2):  # PopSift / VLFeat sift mode
            shift = np.float32(0.5) * np.float32(2.0) ** np.float32(p.upscale_factor)
        ow = np.array([d[0] for d in dims], np.int32)
        oh = np.array([d[1] for d in dims], np.int32)
        out = np.zeros(int(sum(L * a * b for a, b in dims)), np.float32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        u8 = img.ctypes.data if img.dtype == np.uint8 else None
        f32 = img.ctypes.data if img.dtype == np.float32 else None
        rc = self.lib.sdr_pyramid(u8, f32, w, h, w, float(shift), L, fp(t["inc"][0]), ip(t["inc"][1]), fp(t["dd"][0]),
                                  ip(t["dd"][1]), int(scale_direct), len(dims), ip(ow), ip(oh), fp(out))
        assert rc == 0
        planes, off = [], 0
        for a, b in dims:
            planes.append([out[off + l * a * b: off + (l + 1) * a * b].reshape(b, a) for l in range(L)])
            off += L * a * b
        return planes
