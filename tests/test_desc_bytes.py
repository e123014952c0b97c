"""Descriptors as bytes (popsift_hip_fetch*_u8, include/popsift_hip.h) without a GPU: the exports, the argument checks
that need no device, and the host reference of the byte rule that the GPU tests hold the kernel to
(tests/test_gpu_desc_bytes.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "popsift_amd")

U8_SYMBOLS = ("popsift_hip_fetch_item_u8", "popsift_hip_fetch_u8", "popsift_hip_fetch_begin_item_u8",
              "popsift_hip_fetch_begin_u8", "popsift_hip_results_dev_item_u8", "popsift_hip_devfeatures_download_u8")

# (value, q(value)): roundf ties away from zero, saturation at 255, NaN and everything <= 0 to 0
EDGES = [(0.49999997, 0), (0.5, 1), (1.5, 2), (2.5, 3), (254.49998, 254), (254.5, 255), (255.0, 255), (1e30, 255),
         (np.inf, 255), (np.nan, 0), (-0.0, 0), (1e-30, 0)]


def test_byte_symbols_are_exported_and_bound(hip):
    lib = hip.lib()
    bound = {n for n, _, _ in hip.SYMBOLS}
    for n in U8_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in bound, n


def test_null_context_and_null_set_are_invalid(hip):
    lib = hip.lib()
    buf = np.zeros(128, np.uint8)
    feats = np.zeros(1, hip.FEATURE_DTYPE)
    p = C.c_void_p()
    assert lib.popsift_hip_fetch_u8(None, feats.ctypes.data, 1, buf.ctypes.data, 128) == hip.ERR_INVALID
    assert lib.popsift_hip_fetch_item_u8(None, 0, feats.ctypes.data, 1, buf.ctypes.data, 128) == hip.ERR_INVALID
    assert lib.popsift_hip_fetch_begin_u8(None, feats.ctypes.data, 1, buf.ctypes.data, 128) == hip.ERR_INVALID
    assert lib.popsift_hip_fetch_begin_item_u8(None, 0, feats.ctypes.data, 1, buf.ctypes.data, 128) == hip.ERR_INVALID
    assert lib.popsift_hip_results_dev_item_u8(None, 0, C.byref(p), C.byref(p)) == hip.ERR_INVALID
    assert lib.popsift_hip_devfeatures_download_u8(None, buf.ctypes.data) == hip.ERR_INVALID


def test_reference_rule_on_the_edges(hip):
    v = np.array([e[0] for e in EDGES], np.float32)
    assert hip.quantize_u8(v).tolist() == [e[1] for e in EDGES]
    # the traps the rule names: floor(d + 0.5) and banker's rounding differ from it here
    assert np.floor(np.float32(0.49999997) + np.float32(0.5)) == 1.0 and hip.quantize_u8([0.49999997])[0] == 0
    assert np.round(np.float32(2.5)) == 2.0 and hip.quantize_u8([2.5])[0] == 3
    assert hip.quantize_u8([-np.inf, -1.0, -0.5, 0.0])[0:4].tolist() == [0, 0, 0, 0]


def test_reference_rule_against_c_roundf(hip, tmp_path):
    """quantize_u8 agrees with the C expression the rule is written in, on every float of [0, 256] that ends in .5 or
    lies one ulp either side of it, and on a random sample"""
    src = tmp_path / "q.c"
    src.write_text(r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
int main(int argc, char** argv)
{
    FILE* f = fopen(argv[1], "rb");
    FILE* g = fopen(argv[2], "wb");
    float d;
    while (fread(&d, 4, 1, f) == 1) {
        uint8_t q = (isnan(d) || d <= 0.0f) ? 0 : d >= 255.0f ? 255 : (uint8_t)roundf(d);
        fwrite(&q, 1, 1, g);
    }
    fclose(f);
    fclose(g);
    return 0;
}
""")
    exe = str(tmp_path / "q.bin")
    subprocess.check_call(["gcc", "-O1", str(src), "-o", exe, "-lm"])
    half = np.arange(0, 257, dtype=np.float32) + np.float32(0.5)
    v = np.concatenate([half, np.nextafter(half, np.float32(0)), np.nextafter(half, np.float32(1e9)),
                        np.random.default_rng(5).uniform(-10, 300, 100000).astype(np.float32),
                        np.array([e[0] for e in EDGES], np.float32)]).astype(np.float32)
    (tmp_path / "in.bin").write_bytes(v.tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    want = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.uint8)
    assert np.array_equal(hip.quantize_u8(v), want)


def test_cpp_config_carries_the_descriptor_format():
    """popsift::Config::DescriptorFormat: float by default, part of equal(); FeaturesHost in the byte format"""
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host")], stdout=subprocess.DEVNULL)
    out = subprocess.check_output(["nm", "-DC", "--defined-only", os.path.join(PKG, "libpopsift.so")], text=True)
    for sym in ("popsift::FeaturesHost::resetBytes(int, int)", "popsift::FeaturesHost::descriptorBytes(int, int) const"):
        assert sym in out, sym
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "host_desc_bytes_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "host_desc_bytes_cpu.bin")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DDESC_BYTES_CPU_ONLY", "-I", os.path.join(ROOT, "include"), src,
                           os.path.join(PKG, "host", "pgmread.cpp"), "-o", exe, "-L", PKG, "-lpopsift", "-lpopsift_hip",
                           "-pthread", "-Wl,-rpath," + PKG])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host_desc_bytes cpu ok" in r.stdout
