"""popsift::Verifier::epipolar of the C++ layer (tests/cpp/host_epipolar_test.cpp) against the C call, and popsift-match
--pairs --verify epipolar on an image pair."""
import os
import subprocess

import numpy as np
import pytest

import epipolar_rule as E
from popsift_amd.synth import synth
from test_gpu_verify_cpp import parse_verification, write_pgm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "popsift_amd")


def test_cpp_epipolar_gives_the_bytes_of_the_c_call(gpu_hip, tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host")], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "host_epipolar_test.bin")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "host_epipolar_test.cpp"), "-o", exe, "-L", PKG,
                           "-lpopsift", "-lpopsift_hip", "-pthread", "-Wl,-rpath," + PKG])
    pts, inl, _ = E.two_view(1000, 1)
    scene, out = str(tmp_path / "scene.bin"), str(tmp_path / "result.out")
    with open(scene, "wb") as f:
        f.write(np.int32(len(pts)).tobytes() + pts.tobytes() + inl.tobytes())
    r = subprocess.run([exe, scene, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host_epipolar ok: 600 " in r.stdout, r.stdout + r.stderr
    v = gpu_hip.Verifier()
    res, mask = v.epipolar(pts, 1500, 0.5, 0)
    v.close()
    want = res["H"].tobytes() + np.array([res["n_inliers"], res["hypothesis"], res["n_valid"]], np.int32).tobytes() + mask.tobytes()
    assert open(out, "rb").read() == want


def test_the_match_program_verifies_epipolar(gpu_hip, tmp_path):
    hip = gpu_hip
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

    A, B = hip.Context().submit(a).clone_results(), hip.Context().submit(b).clone_results()
    pairs = A.match_pairs(B, cross_check=True)
    pts = A.pair_points(B, pairs)
    plain = run()
    lines = run("--verify", "epipolar", "--max-err", "0.75", "--seed", "9")
    # the pair lines as without --verify (two extractions list the features in arrival order: the head, the number of lines
    # and the count are compared, as tests/test_gpu_verify_cpp.py does), then the model block
    assert len(lines) == len(plain) + 5 and lines[:5] == plain[:5] and lines[-6] == plain[-1]
    assert plain[-1] == "Number of pairs:       %d" % len(pairs)
    F, k, n = parse_verification(lines, "epipolar")
    assert n == len(pts) and k > n // 2
    assert np.abs(F).max() == 1.0
    # The program prints no points and its pairs come in its own extraction's order, so its F is held to the C call's points
    # of the same pairs (the same set of rows): the printed count lies between the numbers of rows whose distance to the
    # epipolar constraint under the printed F -- the Sampson distance, which is what the rule bounds by max_err -- is
    # within max_err -+ 1e-3 px, computed in float64.
    d = E.sampson(F, pts)
    assert (d <= 0.75 - 1e-3).sum() <= k <= (d <= 0.75 + 1e-3).sum(), (k, np.sort(d)[max(k - 3, 0):k + 3])
    # the sibling's words stay what they were
    for args in (["--pairs", "--verify", "fundamental"], ["--verify", "epipolar"]):
        o = subprocess.run([match, "-l", pa, "-r", pb] + args, capture_output=True, text=True, timeout=300)
        assert o.returncode != 0 and "--verify" in o.stderr
