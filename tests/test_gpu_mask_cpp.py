"""PopSift::enqueueMasked of the C++ layer (tests/cpp/host_mask_test.cpp) and popsift-demo --mask against the C ABI's
popsift_hip_submit_batch_masked, byte for byte: byte and float images, one job per submit and masked and unmasked jobs
batched four at a time; a mask of another size ends the demo before any extraction."""
import os
import subprocess

import numpy as np
import pytest

import mask_rule as M
from popsift_amd.synth import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "popsift_amd")
DEMO = os.path.join(PKG, "popsift-demo")
W, H = 256, 192
IMG = synth(21, W, H)
MASK = M.checker(W, H)


def write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host")], stdout=subprocess.DEVNULL)
    path = str(tmp_path_factory.mktemp("mask_cpp") / "host_mask_test.bin")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "host_mask_test.cpp"), "-o", path, "-L", PKG,
                           "-lpopsift", "-lpopsift_hip", "-pthread", "-Wl,-rpath," + PKG])
    return path


@pytest.mark.parametrize("batch", [1, 4])
@pytest.mark.parametrize("is_float", [0, 1])
def test_cpp_masked_equals_c_abi(gpu_hip, exe, tmp_path, batch, is_float):
    hip = gpu_hip
    rep = 7
    img = IMG.astype(np.float32) / np.float32(256.0) if is_float else IMG
    img.tofile(str(tmp_path / ("img.f32" if is_float else "img.u8")))
    MASK.tofile(str(tmp_path / "mask.u8"))
    env = dict(os.environ, POPSIFT_BATCH=str(batch), POPSIFT_CONTEXTS_PER_DEVICE="1")
    r = subprocess.run([exe, str(tmp_path), str(W), str(H), str(is_float), str(rep)], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    assert "host_mask_test ok" in r.stdout
    ctx = hip.Context(hip.default_params(feature_order=hip.ORDER_RASTER))
    want = {True: ctx.submit(img, MASK).fetch(), False: ctx.submit(img).fetch()}
    ctx.close()
    assert 0 < len(want[True][0]) < len(want[False][0])
    if not is_float:
        assert (len(want[True][0]), len(want[False][0])) == (907, 1803)
    for j in range(rep):
        f, d = want[j % 3 != 1]
        got_f = np.fromfile(str(tmp_path / ("job%d.feat" % j)), hip.FEATURE_DTYPE)
        got_d = np.fromfile(str(tmp_path / ("job%d.desc" % j)), np.float32).reshape(-1, 128)
        assert got_f.tobytes() == f.tobytes() and got_d.tobytes() == d.tobytes(), j


def demo(*args):
    return subprocess.run([DEMO] + list(args), capture_output=True, text=True, timeout=300)


def test_demo_mask_writes_the_masked_features(gpu_hip, tmp_path):
    hip = gpu_hip
    pgm, mpgm, full, masked = (str(tmp_path / n) for n in ("img.pgm", "m.pgm", "full.txt", "masked.txt"))
    write_pgm(pgm, IMG)
    write_pgm(mpgm, MASK)
    ctx = hip.Context(hip.default_params(feature_order=hip.ORDER_RASTER))
    f_all, _ = ctx.submit(IMG).fetch()
    f_vis, d_vis = ctx.submit(IMG, MASK).fetch()
    ctx.close()
    keep = M.visible(f_all, MASK)
    assert len(f_vis) == int(keep.sum()) == 907

    r = demo("-i", pgm, "--feature-order", "raster", "--output-file", full)
    assert r.returncode == 0, r.stdout + r.stderr
    r = demo("-i", pgm, "--feature-order", "raster", "--mask", mpgm, "--output-file", masked)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Number of feature points: %d number of feature descriptors: %d" % (len(f_vis), len(d_vis)) in r.stderr
    with open(full) as f:
        full_rows = f.read().splitlines()
    with open(masked) as f:
        masked_rows = f.read().splitlines()
    # the feature file has one row per descriptor, in feature order: the masked file is the rows of the visible features
    per_row = np.repeat(keep, f_all["num_ori"])
    assert len(full_rows) == len(per_row)
    assert masked_rows == [row for row, k in zip(full_rows, per_row) if k]


def test_demo_refuses_a_mask_of_another_size(gpu_hip, tmp_path):
    pgm, mpgm, out = (str(tmp_path / n) for n in ("img.pgm", "m.pgm", "never.txt"))
    write_pgm(pgm, IMG)
    write_pgm(mpgm, M.checker(W + 1, H))
    r = demo("-i", pgm, "--mask", mpgm, "--output-file", out)
    assert r.returncode != 0 and "--mask" in r.stderr, r.stderr
    assert "Number of feature points" not in r.stderr and not os.path.exists(out)
    r = demo("-i", pgm, "--mask", str(tmp_path / "missing.pgm"), "--output-file", out)
    assert r.returncode != 0 and "--mask" in r.stderr, r.stderr
    assert not os.path.exists(out)
