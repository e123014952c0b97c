"""popsift::Gallery over links in the C++ layer (tests/cpp/host_links_test.cpp) against the per-pair C++ calls and the
binding, and popsift-match --all-pairs / --sequential against the binding."""
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


def test_cpp_links_and_the_match_program(gpu_hip, tmp_path):
    hip = gpu_hip
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host")], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "host_links_test.bin")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "host_links_test.cpp"),
                           os.path.join(PKG, "host", "pgmread.cpp"), "-o", exe, "-L", PKG,
                           "-lpopsift", "-lpopsift_hip", "-pthread", "-Wl,-rpath," + PKG])
    a = synth(95, 240, 180)
    imgs = [a, np.roll(a, (2, 4), axis=(0, 1)), synth(23, 240, 180)]
    paths = [str(tmp_path / n) for n in ("a.pgm", "b.pgm", "c.pgm")]
    for p, img in zip(paths, imgs):
        write_pgm(p, img)
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"host_links ok: (\d+) (\d+) (\d+)", r.stdout)
    assert m, r.stdout
    cpp_counts = [int(x) for x in m.groups()]

    # the binding on the same images
    p9 = hip.default_params(norm_multi=9)
    g = hip.Gallery()
    for img in imgs:
        g.add_set(hip.Context(p9).submit(img).clone_results())
    links = hip.all_links(3)
    assert g.link_counts(links, cross_check=True).tolist() == cpp_counts
    assert cpp_counts[0] > 50 and cpp_counts[0] > cpp_counts[1] and cpp_counts[0] > cpp_counts[2]

    # the program: one line per link, then the totals
    match = [os.path.join(PKG, "popsift-match"), "--norm-multi", "9"] + [x for f in paths for x in ("--gallery", f)]
    head = re.compile(r"link (\d+) (\d+): (\d+) pairs(?:, (\d+) inliers, (\w+)((?: [-+0-9.eEinfa]+){9}))?$")

    def run(*args):
        out = subprocess.run(match + list(args), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert lines[0] == "3 gallery images <-> each other"
        body = lines[1 + 2 * 3:]                                      # two count lines per image
        assert body[-2].startswith("Number of links:") and body[-1].startswith("Number of pairs:")
        rows = [head.match(x) for x in body[:-2]]
        assert all(rows), body
        assert int(body[-2].split()[-1]) == len(rows) and int(body[-1].split()[-1]) == sum(int(x.group(3)) for x in rows)
        return rows

    for args, want_links, kw in ((["--all-pairs", "--cross-check"], links, dict(cross_check=True)),
                                 (["--all-pairs", "--ratio=0.6"], links, dict(ratio=0.6)),
                                 (["--sequential", "1"], hip.sequential_links(3, 1), dict()),
                                 (["--sequential=2", "--max-dist=40", "--cross-check"], hip.sequential_links(3, 2),
                                  dict(max_dist2=1600.0, cross_check=True))):
        rows = run(*args)
        assert [(int(x.group(1)), int(x.group(2))) for x in rows] == want_links.tolist()
        assert [int(x.group(3)) for x in rows] == g.link_counts(want_links, **kw).tolist()   # the features' order differs
        assert all(x.group(4) is None for x in rows)

    # verified: the binding's three calls on the same links.  Raster order makes the sets, and so the sampler's input, the
    # same in both processes
    pr = hip.default_params(norm_multi=9, feature_order=hip.ORDER_RASTER)
    gr = hip.Gallery()
    for img in imgs:
        gr.add_set(hip.Context(pr).submit(img).clone_results())
    pairs, off = gr.match_pairs_links(links, cross_check=True)
    v = hip.Verifier()
    res, _ = v.ransac_many(gr.link_points(links, pairs, off), off, "homography", 512, 2.0, 3)
    v.close()
    rows = run("--all-pairs", "--cross-check", "--feature-order", "raster", "--gallery-verify", "homography",
               "--hypotheses", "512", "--max-err", "2", "--seed", "3")
    assert [int(x.group(3)) for x in rows] == np.diff(off).tolist()
    assert [int(x.group(4)) for x in rows] == res["n_inliers"].tolist() and rows[0].group(5) == "homography"
    assert int(rows[0].group(4)) >= 30 and int(rows[0].group(4)) > max(int(rows[1].group(4)), int(rows[2].group(4)))
    for x, rec in zip(rows, res):
        assert np.array([float(t) for t in x.group(6).split()], np.float32).tobytes() == rec["H"].tobytes()

    # what the program refuses, and what its help says
    for bad in (["--all-pairs", "-l", paths[0]], ["--all-pairs", "--sequential", "2"], ["--sequential", "0"]):
        out = subprocess.run(match + bad, capture_output=True, text=True, timeout=300)
        assert out.returncode != 0 and ("--all-pairs" in out.stderr or "--sequential" in out.stderr), (bad, out.stderr)
    out = subprocess.run([match[0], "--all-pairs", "-l", paths[0], "-r", paths[1]], capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "--gallery" in out.stderr
    out = subprocess.run(match, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "--left" in (out.stderr + out.stdout)
    text = subprocess.run([match[0], "--help"], capture_output=True, text=True).stdout
    assert "--all-pairs" in text and "--sequential" in text
