"""popsift::Gallery of the C++ layer (tests/cpp/host_gallery_test.cpp) against the per-pair C++ calls and the binding, and
popsift-match --gallery against the binding."""
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


def test_cpp_gallery_and_the_match_program(gpu_hip, tmp_path):
    hip = gpu_hip
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host")], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "host_gallery_test.bin")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "host_gallery_test.cpp"),
                           os.path.join(PKG, "host", "pgmread.cpp"), "-o", exe, "-L", PKG,
                           "-lpopsift", "-lpopsift_hip", "-pthread", "-Wl,-rpath," + PKG])
    q = synth(95, 240, 180)
    imgs = [q, np.roll(q, (2, 4), axis=(0, 1)), synth(23, 240, 180)]
    paths = [str(tmp_path / n) for n in ("q.pgm", "a.pgm", "b.pgm")]
    for p, img in zip(paths, imgs):
        write_pgm(p, img)
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"host_gallery ok: (\d+) (\d+) (\d+)", r.stdout)
    assert m, r.stdout
    cpp_counts = [int(x) for x in m.groups()]

    # the binding on the same images
    p9 = hip.default_params(norm_multi=9)
    Q, A, B = (hip.Context(p9).submit(img).clone_results_u8() for img in imgs)
    g = hip.Gallery()
    g.add(A)
    g.add(np.zeros((0, 128), np.uint8))
    g.add(B)
    assert g.counts(Q, cross_check=True).tolist() == cpp_counts
    assert cpp_counts[1] == 0 and cpp_counts[0] > 50 and cpp_counts[0] > cpp_counts[2]

    # the program: a and b as the gallery, in both orders
    match = [os.path.join(PKG, "popsift-match"), "-l", paths[0], "--norm-multi", "9"]
    pat = re.compile(r"pair feat +(\d+) \[ *(\d+)\] matches feat +(\d+) \[ *(\d+)\] dist ([0-9.]+)$")

    def run(files, *args):
        cmd = match + [x for f in files for x in ("--gallery", f)] + list(args)
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert lines[0] == "%s <-> %d gallery images" % (paths[0], len(files))
        body = lines[1 + 2 * (1 + len(files)):]                      # two count lines per image
        assert body[-1].startswith("Number of pairs:")
        per_image, k = [], -1
        for x in body[:-1]:
            head = re.match(r"gallery (\d+) (.*): (\d+) pairs$", x)
            if head:
                k += 1
                assert int(head.group(1)) == k and head.group(2) == files[k]
                per_image.append([int(head.group(3)), []])
            else:
                row = pat.match(x)
                assert row, x
                per_image[-1][1].append((int(row.group(2)), int(row.group(4))))
        assert len(per_image) == len(files)
        for n, rows in per_image:
            assert n == len(rows)
        assert int(body[-1].split()[-1]) == sum(n for n, _ in per_image)
        return per_image

    two = hip.Gallery()
    two.add(A)
    two.add(B)
    for args, kw in ((["--cross-check"], dict(cross_check=True)), ([], dict()), (["--ratio=0.6"], dict(ratio=0.6)),
                     (["--max-dist=40", "--cross-check"], dict(max_dist2=1600.0, cross_check=True))):
        pairs, off = two.match_pairs(Q, **kw)
        got = run(paths[1:], *args)
        for k in range(2):
            want = pairs[off[k]:off[k + 1]]
            assert got[k][0] == len(want)                             # the features' order differs from run to run
            left = [l for l, _ in got[k][1]]
            assert left == sorted(left) and len(set(left)) == len(left)
            if kw.get("cross_check"):
                assert len({r for _, r in got[k][1]}) == len(left)   # one left per right descriptor
    back = run(paths[:0:-1], "--cross-check")
    assert [n for n, _ in back] == [cpp_counts[2], cpp_counts[0]]
    # what the program refuses, and what its help says
    for bad in (["--pairs", "--verify", "homography"], ["--guided"], ["-r", paths[2]]):
        out = subprocess.run(match + ["--gallery", paths[1]] + bad, capture_output=True, text=True, timeout=300)
        assert out.returncode != 0 and "--gallery" in out.stderr, (bad, out.stderr)
    out = subprocess.run(match, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "--right" in (out.stderr + out.stdout)
    assert "--gallery" in subprocess.run([match[0], "--help"], capture_output=True, text=True).stdout
