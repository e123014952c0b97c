"""FeaturesDevBytes of the C++ layer (tests/cpp/host_match_bytes_test.cpp) against the C calls field by field, and
popsift-match --bytes against the binding."""
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


def test_cpp_byte_sets_and_the_match_program(gpu_hip, tmp_path):
    hip = gpu_hip
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host")], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "host_match_bytes_test.bin")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "host_match_bytes_test.cpp"),
                           os.path.join(PKG, "host", "pgmread.cpp"), "-o", exe, "-L", PKG,
                           "-lpopsift", "-lpopsift_hip", "-pthread", "-Wl,-rpath," + PKG])
    a = synth(95, 240, 180)
    b = np.roll(a, (2, 4), axis=(0, 1))
    pa, pb = str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm")
    write_pgm(pa, a)
    write_pgm(pb, b)
    r = subprocess.run([exe, pa, pb], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"host_match_bytes ok: (\d+)", r.stdout)
    assert m, r.stdout
    n_pairs = int(m.group(1))
    assert n_pairs > 50

    # the program, against the binding on the same images
    p9 = hip.default_params(norm_multi=9)
    A, B = hip.Context(p9).submit(a).clone_results_u8(), hip.Context(p9).submit(b).clone_results_u8()
    match = [os.path.join(PKG, "popsift-match"), "-l", pa, "-r", pb, "--norm-multi", "9", "--bytes"]

    def count(*args):
        out = subprocess.run(match + ["--pairs"] + list(args), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        n = int(lines[-1].split()[-1])
        assert lines[-1].startswith("Number of pairs:") and len(lines) == 6 + n
        return n, lines[5:-1]

    n, lines = count("--cross-check")
    assert n == n_pairs == len(A.match_pairs(B, cross_check=True))
    pat = re.compile(r"pair feat +(\d+) \[ *(\d+)\] matches feat +(\d+) \[ *(\d+)\] dist ([0-9.]+)$")
    rows = [pat.match(x) for x in lines]
    assert all(rows)
    left = [int(x.group(2)) for x in rows]
    assert left == sorted(left) and len(set(left)) == len(left)
    assert len({int(x.group(4)) for x in rows}) == len(rows)        # cross-checked: one left per right descriptor
    assert count("--cross-check", "--ratio", "0")[0] == len(A.match_pairs(B, ratio=0.0, cross_check=True)) > n_pairs
    assert count("--ratio=0.6")[0] == len(A.match_pairs(B, ratio=0.6))
    assert count("--max-dist=40")[0] == len(A.match_pairs(B, max_dist2=1600.0)) < count()[0] == len(A.match_pairs(B))
    # without --pairs: a line per left descriptor, from the byte matcher's rows
    out = subprocess.run(match, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    body = out.stdout.splitlines()[5:]
    rows = A.match(B)
    assert len(body) == len(rows)
    assert sum(x.startswith("accept") for x in body) == int((rows["accept"] == 1).sum())
    assert "--bytes" in subprocess.run([match[0], "--help"], capture_output=True, text=True).stdout
