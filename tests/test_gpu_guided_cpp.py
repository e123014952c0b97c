"""FeaturesDev::matchGuided / matchGuidedRows / fromHostPoints of the C++ layer (tests/cpp/host_guided_test.cpp) against
the C calls, and popsift-match --pairs --verify MODEL --guided on an image pair."""
import os
import re
import subprocess

import numpy as np
import pytest

import guided_rule as G
from popsift_amd.synth import synth
from test_gpu_verify_cpp import parse_verification, write_pgm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "popsift_amd")


@pytest.mark.parametrize("model", ["homography", "epipolar"])
def test_cpp_guided_matching_gives_the_bytes_of_the_c_calls(gpu_hip, tmp_path, model):
    hip = gpu_hip
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host")], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "host_guided_test.bin")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "host_guided_test.cpp"), "-o", exe, "-L", PKG,
                           "-lpopsift", "-lpopsift_hip", "-pthread", "-Wl,-rpath," + PKG])
    s, Hm = G.scene(200, 1000)
    M = Hm if model == "homography" else G.scene_F()
    scene, out = str(tmp_path / "scene.bin"), str(tmp_path / "result.out")
    with open(scene, "wb") as f:
        f.write(np.array([200, 1000, hip.GUIDES[model]], np.int32).tobytes() + M.astype(np.float32).tobytes() +
                np.float32(2.0).tobytes() + s["l"].tobytes() + s["lxy"].tobytes() + s["r"].tobytes() + s["rxy"].tobytes())
    r = subprocess.run([exe, scene, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host_guided ok: " in r.stdout, r.stdout + r.stderr
    L = hip.DevFeatures.from_host_points(s["l"], s["lxy"])
    R = hip.DevFeatures.from_host_points(s["r"], s["rxy"])
    plain = L.match_pairs_guided(R, model, M, 2.0)
    crossed = L.match_pairs_guided(R, model, M, 2.0, cross_check=True)
    # the scene's pairs follow the homography; under the cameras' F a band holds the true partner only by chance
    assert len(crossed) > (20 if model == "homography" else 0)
    want = (L.match_guided(R, model, M, 2.0).tobytes() + np.int32(len(plain)).tobytes() + plain.tobytes() +
            np.int32(len(crossed)).tobytes() + crossed.tobytes())
    assert open(out, "rb").read() == want


def test_the_match_program_matches_again_under_the_model(gpu_hip, tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host")], stdout=subprocess.DEVNULL)
    a = synth(95, 240, 180)
    b = np.roll(a, (8, 16), axis=(0, 1))
    pa, pb = str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm")
    write_pgm(pa, a)
    write_pgm(pb, b)
    match = os.path.join(PKG, "popsift-match")

    def run(*args):
        o = subprocess.run([match, "-l", pa, "-r", pb, "--pairs", "--cross-check"] + list(args), capture_output=True,
                           text=True, timeout=300)
        assert o.returncode == 0, o.stderr
        return o.stdout.splitlines()

    plain = run()
    verified = run("--verify", "affine")
    # without --guided the output is what it was: the pair lines of the plain run (two extractions list the features in
    # arrival order: the head, the number of lines and the count are compared, as tests/test_gpu_verify_cpp.py does), then
    # the model block
    assert len(verified) == len(plain) + 5 and verified[:5] == plain[:5] and verified[-6] == plain[-1]
    _, inliers, n_pairs = parse_verification(verified, "affine")
    for model, extra in (("affine", []), ("homography", ["--guided-err", "3"]), ("epipolar", [])):
        base = run("--verify", model)
        lines = run("--verify", model, "--guided", *extra)
        _, k, n = parse_verification(base, model)
        m = re.match(r"Number of guided pairs: (\d+)$", lines[-1])
        assert m, lines[-3:]
        n_guided = int(m.group(1))
        # the verified block is unchanged, the guided pair lines follow it in the pair format
        assert len(lines) == len(base) + n_guided + 1 and lines[:5] == base[:5]
        assert parse_verification(lines[:len(base)], model)[1:] == (k, n)
        assert all(re.match(r"pair feat +\d+ \[ *\d+\] matches feat +\d+ \[ *\d+\] dist \d+\.\d{3}$", x) for x in lines[len(base):-1])
        # every verified pair is found again (tests/test_gpu_guided.py proves it pair by pair)
        assert n_guided >= k, (model, n_guided, k, n)
    assert inliers > n_pairs // 2
    # the combinations that make no sense name the option
    for args in (["--pairs", "--guided"], ["--guided"], ["--pairs", "--verify", "affine", "--guided", "--bytes", "--norm-multi", "9"]):
        o = subprocess.run([match, "-l", pa, "-r", pb] + args, capture_output=True, text=True, timeout=300)
        assert o.returncode != 0 and "--guided" in o.stderr, args
