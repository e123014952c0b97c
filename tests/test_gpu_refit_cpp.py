"""popsift::Verifier::refit of the C++ layer (tests/cpp/host_refit_test.cpp) on the points of an image pair against the C
calls, and popsift-match --pairs --verify MODEL --refit [--guided] on the rolled pair."""
import os
import re
import subprocess

import numpy as np
import pytest

from popsift_amd.synth import synth
from test_gpu_verify_cpp import parse_verification, write_pgm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "popsift_amd")
SHIFT = (8, 16)   # rows, columns: the rolled 96 x 72 pair of tests/test_gpu_ransac.py


@pytest.fixture(scope="module")
def rolled_pair(tmp_path_factory):
    d = tmp_path_factory.mktemp("refit_pair")
    a = synth(95, 96, 72)
    b = np.roll(a, SHIFT, axis=(0, 1))
    pa, pb = str(d / "l.pgm"), str(d / "r.pgm")
    write_pgm(pa, a)
    write_pgm(pb, b)
    return pa, pb, d


def test_cpp_refit_gives_the_bytes_of_the_c_call(gpu_hip, rolled_pair):
    hip = gpu_hip
    pa, pb, d = rolled_pair
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host")], stdout=subprocess.DEVNULL)
    exe, out = str(d / "host_refit_test.bin"), str(d / "result.out")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "host_refit_test.cpp"),
                           os.path.join(PKG, "host", "pgmread.cpp"), "-o", exe, "-L", PKG,
                           "-lpopsift", "-lpopsift_hip", "-pthread", "-Wl,-rpath," + PKG])
    r = subprocess.run([exe, pa, pb, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "host_refit ok: " in r.stdout, r.stdout + r.stderr
    raw = open(out, "rb").read()
    n = int(np.frombuffer(raw, np.int32, 1)[0])
    pts = np.frombuffer(raw, np.float32, 4 * n, 4).reshape(n, 4)
    at = 4 + 16 * n
    v = hip.Verifier()
    for kind in ("homography", "affine", "epipolar"):
        start = np.frombuffer(raw, np.float32, 9, at)
        win = (v.epipolar(pts) if kind == "epipolar" else v.ransac(pts, kind))[0]
        assert start.tobytes() == win["H"].tobytes()
        res, mask = v.refit(pts, kind, start, 2.0, 4)
        assert raw[at + 36:at + 36 + 52] == res.tobytes(), (kind, res)
        assert raw[at + 88:at + 88 + n] == mask.tobytes()
        assert res["n_inliers"] >= res["n_start"] == win["n_inliers"] > n // 2
        at += 88 + n
    assert at == len(raw)
    v.close()


def parse_refit(lines):
    """the five lines --refit appends -> (M as 9 float32, start, inliers, pairs, rounds, reason)"""
    assert lines[-5] == "Refitted model:", lines[-5:]
    M = np.array([float(x) for row in lines[-4:-1] for x in row.split()], np.float32)
    m = re.match(r"Refit inliers:         (\d+) -> (\d+) of (\d+), (\d+) rounds \(([a-z ]+)\)$", lines[-1])
    assert len(M) == 9 and m, lines[-5:]
    return (M,) + tuple(int(m.group(i)) for i in (1, 2, 3, 4)) + (m.group(5),)


def test_the_match_program_refits_and_guides_with_the_refitted_model(gpu_hip, rolled_pair):
    pa, pb, _ = rolled_pair
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host")], stdout=subprocess.DEVNULL)
    match = os.path.join(PKG, "popsift-match")

    def run(*args):
        # raster order: every run extracts the same lists, so every run's RANSAC sees the same pairs and returns the same
        # winner, and a run with --refit differs from one without it by the refit alone
        o = subprocess.run([match, "-l", pa, "-r", pb, "--pairs", "--cross-check", "--feature-order", "raster"] + list(args),
                           capture_output=True, text=True, timeout=300)
        assert o.returncode == 0, o.stderr
        return o.stdout.splitlines()

    count = lambda ls: int(re.match(r"Number of guided pairs: (\d+)$", ls[-1]).group(1))
    base = run("--verify", "affine")
    lines = run("--verify", "affine", "--refit")
    # the RANSAC block is what it was, the refit block follows
    assert lines[:-5] == base
    Hm, k, n = parse_verification(base, "affine")
    assert parse_verification(lines[:-5], "affine")[1:] == (k, n) and k > n // 2
    M, start, inliers, pairs, rounds, why = parse_refit(lines)
    assert start == k and inliers >= k and pairs == n and 0 <= rounds <= 4
    assert why in ("all rounds ran", "converged", "no more inliers")
    # the planted shift: more than half of the pairs are displaced by the roll exactly and an inlier lies within
    # max_err = 2 px of its image under M, so M moves a point among them -- the image centre -- by the roll to within 2 px
    # (measured: 0.0017 px on 175 inliers of 196 pairs)
    assert M[6] == 0.0 and M[7] == 0.0 and M[8] == 1.0
    off = np.hypot(*(M.astype(np.float64).reshape(3, 3)[:2] @ [47.5, 35.5, 1.0] - [47.5 + SHIFT[1], 35.5 + SHIFT[0]]))
    print("affine: %d -> %d of %d pairs, %d rounds (%s); the image centre moves %.4f px off the roll" %
          (start, inliers, pairs, rounds, why, off))
    assert off <= 2.0
    assert parse_refit(run("--verify", "affine", "--refit", "--refit-rounds", "1"))[4] <= 1
    # with --guided the refitted model is the guide, and finds at least the pairs the minimal-sample model finds
    for model in ("affine", "homography", "epipolar"):
        guided, refitted = run("--verify", model, "--guided"), run("--verify", model, "--refit", "--guided")
        print("%s: guided pairs %d, under the refitted model %d" % (model, count(guided), count(refitted)))
        assert count(refitted) >= count(guided)
        k = parse_verification(guided[:-count(guided) - 1], model)[1]
        assert parse_refit(refitted[:-count(refitted) - 1])[1] == k
    # --refit without --verify, and rounds outside 1 .. 16: refused
    for args in (["--pairs", "--refit"], ["--refit"]):
        o = subprocess.run([match, "-l", pa, "-r", pb] + args, capture_output=True, text=True, timeout=300)
        assert o.returncode != 0 and "--refit" in o.stderr, args
    o = subprocess.run([match, "-l", pa, "-r", pb, "--pairs", "--verify", "affine", "--refit", "--refit-rounds", "17"],
                       capture_output=True, text=True, timeout=300)
    assert o.returncode != 0
