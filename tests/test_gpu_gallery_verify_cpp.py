"""A gallery verified through the C++ layer (tests/cpp/host_gallery_verify_test.cpp: Gallery::add(FeaturesDev*),
Gallery::pairPoints, Verifier::ransacMany against the per-member calls) and popsift-match --gallery-verify against the
binding."""
import os
import re
import subprocess

import numpy as np
import pytest

from popsift_amd.synth import synth
from test_gpu_match_pairs_cpp import write_pgm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "popsift_amd")


def test_cpp_gallery_verification_and_the_match_program(gpu_hip, tmp_path):
    hip = gpu_hip
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host")], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "host_gallery_verify_test.bin")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "host_gallery_verify_test.cpp"),
                           os.path.join(PKG, "host", "pgmread.cpp"), "-o", exe, "-L", PKG,
                           "-lpopsift", "-lpopsift_hip", "-pthread", "-Wl,-rpath," + PKG])
    q = synth(95, 240, 180)
    imgs = [q, np.roll(q, (2, 4), axis=(0, 1)), synth(23, 240, 180)]
    paths = [str(tmp_path / n) for n in ("q.pgm", "a.pgm", "b.pgm")]
    for p, img in zip(paths, imgs):
        write_pgm(p, img)
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"host_gallery_verify ok: (\d+) (\d+)", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) > int(m.group(2)) and int(m.group(1)) >= 30

    # the program against the binding, both with the features in raster order: the same bytes on every run
    p9 = hip.default_params(norm_multi=9, feature_order=hip.ORDER_RASTER)
    Q, A, B = (hip.Context(p9).submit(img).clone_results() for img in imgs)
    Qb = hip.ByteFeatures.from_set(Q)
    v = hip.Verifier()
    match = [os.path.join(PKG, "popsift-match"), "-l", paths[0], "--norm-multi", "9", "--feature-order", "raster"]
    for order, sets in (((1, 2), (A, B)), ((2, 1), (B, A))):
        g = hip.Gallery()
        for s in sets:
            g.add_set(s)
        pairs, off = g.match_pairs(Qb, cross_check=True)
        for kind, T, seed in (("homography", 300, 5), ("epipolar", 700, 1)):
            res, _ = v.ransac_many(g.pair_points(Q, pairs, off), off, kind, T, 1.5, seed)
            cmd = match + [x for k in order for x in ("--gallery", paths[k])] + [
                "--cross-check", "--gallery-verify", kind, "--hypotheses", str(T), "--max-err", "1.5", "--seed", str(seed)]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            assert out.returncode == 0, out.stderr
            lines = out.stdout.splitlines()
            heads = [i for i, x in enumerate(lines) if re.match(r"gallery \d+ .*: \d+ pairs$", x)]
            assert len(heads) == 2
            got = []
            for k, i in enumerate(heads):
                n = int(lines[i].split()[-2])
                assert n == off[k + 1] - off[k]
                block = lines[i + 1 + n:i + 1 + n + 5]           # under the image's pair lines
                assert block[0] == "Model (%s):" % kind, block
                H = np.array([[float(x) for x in row.split()] for row in block[1:4]], np.float32)
                assert H.tobytes() == res[k]["H"].reshape(3, 3).tobytes()          # %.9g round-trips a float
                inl = re.match(r"Number of inliers: +(\d+) of (\d+)$", block[4])
                assert inl and int(inl.group(2)) == n, block[4]
                got.append(int(inl.group(1)))
            assert got == res["n_inliers"].tolist()
            total = [i for i, x in enumerate(lines) if x.startswith("Number of pairs:")]
            assert len(total) == 1 and int(lines[total[0]].split()[-1]) == off[-1]
            rank = sorted(range(2), key=lambda k: -got[k])
            assert lines[total[0] + 1] == "Ranking by inliers:   " + "".join(" %d (%d)" % (k, got[k]) for k in rank)
            assert lines[total[0] + 1] == lines[-1]
            if kind == "homography":
                assert got[order.index(1)] > got[order.index(2)] and rank[0] == order.index(1)      # the shifted copy wins
    v.close()
    # what the program refuses, and what its help says
    out = subprocess.run(match + ["-r", paths[1], "--gallery-verify", "homography"], capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "--gallery" in out.stderr
    out = subprocess.run(match + ["--gallery", paths[1], "--gallery-verify", "circle"], capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "--gallery-verify" in out.stderr
    assert "--gallery-verify" in subprocess.run([match[0], "--help"], capture_output=True, text=True).stdout
