"""FeaturesDev::matchPairs of the C++ layer (tests/cpp/host_match_pairs_test.cpp) against matchAndGet in both directions
filtered on the host, and popsift-match --pairs against it."""
import os
import re
import subprocess

import numpy as np
import pytest

from popsift_amd.synth import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "popsift_amd")


def write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


def test_cpp_match_pairs_and_the_match_program(gpu_hip, tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host")], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "host_match_pairs_test.bin")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "host_match_pairs_test.cpp"),
                           os.path.join(PKG, "host", "pgmread.cpp"), "-o", exe, "-L", PKG,
                           "-lpopsift", "-lpopsift_hip", "-pthread", "-Wl,-rpath," + PKG])
    a = synth(95, 240, 180)
    b = np.roll(a, (2, 4), axis=(0, 1))
    pa, pb = str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm")
    write_pgm(pa, a)
    write_pgm(pb, b)
    r = subprocess.run([exe, pa, pb], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"host_match_pairs ok: (\d+)", r.stdout)
    assert m, r.stdout
    n_pairs = int(m.group(1))
    assert n_pairs > 50

    # the program: as many pair lines as matchPairs returns, then the count; the lines before are today's
    r = subprocess.run([os.path.join(PKG, "popsift-match"), "-l", pa, "-r", pb, "--pairs", "--cross-check"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == pa + " <-> " + pb and lines[1].startswith("Number of features:")
    pat = re.compile(r"pair feat +(\d+) \[ *(\d+)\] matches feat +(\d+) \[ *(\d+)\] dist ([0-9.]+)$")
    rows = [pat.match(x) for x in lines[5:-1]]
    assert all(rows) and len(rows) == n_pairs
    assert lines[-1] == "Number of pairs:       %d" % n_pairs
    left = [int(x.group(2)) for x in rows]
    assert left == sorted(left) and len(set(left)) == len(left)
    assert len({int(x.group(4)) for x in rows}) == len(rows)        # cross-checked: one left per right descriptor
    # --ratio and --max-dist reach the matcher: the counts are the C ABI's for the same options (a rolled image repeats
    # many descriptors bit for bit, so a tiny distance still keeps pairs -- fewer than no cap keeps)
    A, B = gpu_hip.Context().submit(a).clone_results(), gpu_hip.Context().submit(b).clone_results()

    def count(*args):
        out = subprocess.run([os.path.join(PKG, "popsift-match"), "-l", pa, "-r", pb, "--pairs"] + list(args),
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        n = int(lines[-1].split()[-1])
        assert len(lines) == 6 + n
        return n

    d = np.float32(1e-6)
    assert count("--cross-check") == n_pairs == len(A.match_pairs(B, cross_check=True))
    assert count("--cross-check", "--ratio", "0") == len(A.match_pairs(B, ratio=0.0, cross_check=True)) > n_pairs
    assert count("--ratio=0.6") == len(A.match_pairs(B, ratio=0.6))
    assert count("--max-dist=1e-6") == len(A.match_pairs(B, max_dist2=float(d * d))) < count() == len(A.match_pairs(B))
