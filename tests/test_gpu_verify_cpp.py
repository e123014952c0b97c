"""popsift::Verifier and FeaturesDev::pairPoints of the C++ layer (tests/cpp/host_verify_test.cpp) on the planted scene and
on an image pair, against the C ABI; and popsift-match --pairs --verify against the same."""
import os
import re
import subprocess

import numpy as np
import pytest

import ransac_rule as R
from popsift_amd.synth import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "popsift_amd")


def write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


def parse_verification(lines, model):
    """the five lines --verify appends -> (H as 9 float32, inliers, pairs)"""
    assert lines[-5] == "Model (%s):" % model, lines[-5:]
    Hm = np.array([float(x) for row in lines[-4:-1] for x in row.split()], np.float32)
    m = re.match(r"Number of inliers:     (\d+) of (\d+)$", lines[-1])
    assert len(Hm) == 9 and m, lines[-5:]
    return Hm, int(m.group(1)), int(m.group(2))


def test_cpp_verifier_pair_points_and_the_match_program(gpu_hip, tmp_path):
    hip = gpu_hip
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host")], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "host_verify_test.bin")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "host_verify_test.cpp"),
                           os.path.join(PKG, "host", "pgmread.cpp"), "-o", exe, "-L", PKG,
                           "-lpopsift", "-lpopsift_hip", "-pthread", "-Wl,-rpath," + PKG])
    pts, inl, _ = R.planted(1000, 1)
    scene = str(tmp_path / "scene.bin")
    with open(scene, "wb") as f:
        f.write(np.int32(len(pts)).tobytes() + pts.tobytes() + inl.tobytes())
    a = synth(95, 240, 180)
    b = np.roll(a, (8, 16), axis=(0, 1))
    pa, pb, out = str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm"), str(tmp_path / "points.out")
    write_pgm(pa, a)
    write_pgm(pb, b)
    r = subprocess.run([exe, scene, pa, pb, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"host_verify ok: (\d+) (\d+)((?: \S+){9})$", r.stdout, re.M)
    assert m, r.stdout

    # The same through the C ABI.  Two extractions of one image hold the same features but not in the same order (the
    # lists are compacted in arrival order), so the two sets of points are compared as sorted rows, and the C++ model
    # against the C ABI's verifier on the C++ program's own points.
    A, B = hip.Context().submit(a).clone_results(), hip.Context().submit(b).clone_results()
    pairs = A.match_pairs(B, cross_check=True)
    want = A.pair_points(B, pairs)
    got = np.fromfile(out, np.float32).reshape(-1, 4)
    rows = lambda p: p[np.lexsort(p.T[::-1])].tobytes()
    assert int(m.group(1)) == len(pairs) == len(got) and rows(got) == rows(want)
    v = hip.Verifier()
    res, _ = v.ransac(got, "affine")
    assert int(m.group(2)) == res["n_inliers"] > len(pairs) // 2
    assert np.array([float(x) for x in m.group(3).split()], np.float32).tobytes() == res["H"].tobytes()

    # the program: the pair lines as without --verify, then the model and its inliers
    match = os.path.join(PKG, "popsift-match")

    def run(*args):
        o = subprocess.run([match, "-l", pa, "-r", pb, "--pairs", "--cross-check"] + list(args), capture_output=True,
                           text=True, timeout=300)
        assert o.returncode == 0, o.stderr
        return o.stdout.splitlines()

    def check(lines, model, max_err, pts):
        """The program prints no points and its pairs come in its own extraction's order, so its model is held to the C
        ABI's points of the same pairs: its inlier count is the number of rows within max_err of their image, computed
        in float64; rows within 1e-3 px of the limit may fall on either side (the float32 scoring of coordinates below
        256 with coefficients near 1 is exact to about 1e-4 px)."""
        Hm, k, n = parse_verification(lines, model)
        assert n == len(pts) and k > n // 2
        err = np.hypot(*(R.project(Hm.astype(np.float64).reshape(3, 3), pts[:, :2]) - pts[:, 2:]).T)
        assert (err <= max_err - 1e-3).sum() <= k <= (err <= max_err + 1e-3).sum(), (k, np.sort(err)[k - 3:k + 3])

    plain = run()
    lines = run("--verify", "affine")
    assert len(lines) == len(plain) + 5 and lines[:5] == plain[:5] and lines[-6] == plain[-1]
    assert plain[-1] == "Number of pairs:       %d" % len(pairs)
    check(lines, "affine", 2.0, want)
    check(run("--verify=homography", "--hypotheses", "500", "--max-err", "0.75", "--seed", "9"), "homography", 0.75, want)
    # --bytes: the pairs of the byte matcher, their points from the float sets
    lines = run("--bytes", "--norm-multi", "9", "--verify", "affine")
    p9 = hip.default_params(norm_multi=9)
    A9, B9 = hip.Context(p9).submit(a).clone_results(), hip.Context(p9).submit(b).clone_results()
    bp = hip.ByteFeatures.from_set(A9).match_pairs(hip.ByteFeatures.from_set(B9), cross_check=True)
    check(lines, "affine", 2.0, A9.pair_points(B9, bp))
    # --verify without --pairs, and an unknown model: refused
    for args in (["--verify", "affine"], ["--pairs", "--verify", "fundamental"]):
        o = subprocess.run([match, "-l", pa, "-r", pb] + args, capture_output=True, text=True, timeout=300)
        assert o.returncode != 0 and "--verify" in o.stderr
