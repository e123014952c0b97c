"""PopSift::enqueue(w, h, img, frames) of the C++ layer (tests/cpp/host_describe_test.cpp) against the C ABI's
popsift_hip_describe_batch, byte for byte, with one job per submit and with describe jobs batched four at a time
between extraction jobs."""
import os
import subprocess

import numpy as np
import pytest

from popsift_amd.synth import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "popsift_amd")


@pytest.mark.parametrize("batch", [1, 4])
@pytest.mark.parametrize("mode", ["compute", "given"])
def test_cpp_describe_equals_c_abi(gpu_hip, tmp_path, batch, mode):
    hip = gpu_hip
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host")], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "host_describe_test.bin")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "host_describe_test.cpp"), "-o", exe, "-L", PKG,
                           "-lpopsift", "-lpopsift_hip", "-pthread", "-Wl,-rpath," + PKG])
    w, h, n, rep = 240, 180, 1500, 7
    img = synth(61, w, h)
    rng = np.random.default_rng(2)
    fr = np.zeros(n, hip.FRAME_DTYPE)
    fr["xpos"], fr["ypos"] = rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)
    fr["sigma"] = np.exp2(rng.uniform(-1, 5, n))
    fr["orientation"] = rng.uniform(-np.pi, np.pi, n)
    fr["octave"], fr["level"] = -1, -1
    fr["xpos"][::50] = np.nan  # a few invalid frames
    img.tofile(str(tmp_path / "img.u8"))
    fr.tofile(str(tmp_path / "frames.bin"))
    env = dict(os.environ, POPSIFT_BATCH=str(batch), POPSIFT_CONTEXTS_PER_DEVICE="1")
    r = subprocess.run([exe, str(tmp_path), str(w), str(h), str(n), "1" if mode == "compute" else "0", str(rep)],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    assert "host_describe_test ok" in r.stdout
    ctx = hip.Context(hip.default_params())
    for j in range(rep):
        nj = n - j * n // (2 * rep)
        f, d = ctx.describe(img, fr[:nj], mode)
        got_f = np.fromfile(str(tmp_path / ("job%d.feat" % j)), hip.FEATURE_DTYPE)
        got_d = np.fromfile(str(tmp_path / ("job%d.desc" % j)), np.float32).reshape(-1, 128)
        assert len(got_f) == nj
        assert got_f.tobytes() == f.tobytes() and got_d.tobytes() == d.tobytes(), j
    ctx.close()
