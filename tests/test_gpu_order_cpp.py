"""Config::setFeatureOrder through the C++ layer's programs: popsift-demo and popsift-match with --feature-order raster
write the same bytes on every run, and an unknown order is a usage error."""
import os
import subprocess

import numpy as np
import pytest

from popsift_amd.synth import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "popsift_amd")
DEMO, MATCH, BENCH = (os.path.join(PKG, n) for n in ("popsift-demo", "popsift-match", "popsift-bench"))


def write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


@pytest.fixture(scope="module")
def pair(gpu_hip, tmp_path_factory):
    d = tmp_path_factory.mktemp("order_cpp")
    a = synth(95, 240, 180)
    pa, pb = str(d / "l.pgm"), str(d / "r.pgm")
    write_pgm(pa, a)
    write_pgm(pb, np.roll(a, (8, 16), axis=(0, 1)))
    return pa, pb


def test_demo_writes_the_same_file_twice(pair, tmp_path):
    outs = []
    for k in range(2):
        out = str(tmp_path / ("features%d.txt" % k))
        r = subprocess.run([DEMO, "-i", pair[0], "--feature-order", "raster", "--output-file", out], capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        with open(out, "rb") as f:
            outs.append(f.read())
    assert len(outs[0]) > 100000 and outs[0] == outs[1]
    # the same features as the default order writes, line for line in another order
    out = str(tmp_path / "arrival.txt")
    r = subprocess.run([DEMO, "-i", pair[0], "--feature-order=arrival", "--output-file", out], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(out, "rb") as f:
        assert sorted(f.read().splitlines()) == sorted(outs[0].splitlines())


def test_match_prints_the_same_twice(pair):
    outs = []
    for _ in range(2):
        r = subprocess.run([MATCH, "-l", pair[0], "-r", pair[1], "--pairs", "--cross-check", "--verify", "homography",
                            "--feature-order", "raster"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout)
    lines = outs[0].splitlines()
    assert lines[-5] == "Model (homography):" and len(lines) > 50, lines[-6:]
    assert outs[0] == outs[1]


def test_unknown_order_is_a_usage_error(pair, tmp_path):
    for cmd in ([DEMO, "-i", pair[0], "--feature-order", "sorted", "--output-file", str(tmp_path / "never.txt")],
                [MATCH, "-l", pair[0], "-r", pair[1], "--feature-order", "sorted"]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "--feature-order" in r.stderr and "Usage:" in r.stderr, r.stderr
    assert not os.path.exists(str(tmp_path / "never.txt"))
    r = subprocess.run([BENCH, "--images", "1", "--feature-order", "sorted"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--feature-order" in r.stderr
