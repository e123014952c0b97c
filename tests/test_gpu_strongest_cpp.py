"""Config::setKeepStrongest through the C++ layer's programs: popsift-demo --keep-strongest N writes the features the C ABI
keeps, as a subsequence of what it writes without the option, and their responses; popsift-match takes the option; a
negative N is a usage error."""
import os
import subprocess

import numpy as np
import pytest

from popsift_amd.synth import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "popsift_amd")
DEMO, MATCH = (os.path.join(PKG, n) for n in ("popsift-demo", "popsift-match"))
IMG = synth(21, 256, 192)
KEEP = 500


def write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


def demo(*args):
    return subprocess.run([DEMO] + list(args), capture_output=True, text=True, timeout=300)


def is_subsequence(part, whole):
    it = iter(whole)
    return all(row in it for row in part)


def test_demo_keeps_the_strongest(gpu_hip, tmp_path):
    hip = gpu_hip
    pgm, full, kept, resp = (str(tmp_path / n) for n in ("img.pgm", "full.txt", "kept.txt", "r.txt"))
    write_pgm(pgm, IMG)
    ctx = hip.Context(hip.default_params(feature_order=hip.ORDER_RASTER)).set_keep_strongest(KEEP).submit(IMG)
    nf, nd = ctx.wait()
    want = ctx.fetch_responses()
    ctx.close()
    assert nf == KEEP and nd >= nf

    r = demo("-i", pgm, "--feature-order", "raster", "--output-file", full)
    assert r.returncode == 0, r.stdout + r.stderr
    r = demo("-i", pgm, "--feature-order", "raster", "--keep-strongest", str(KEEP), "--write-responses", resp, "--output-file", kept)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Number of feature points: %d number of feature descriptors: %d" % (nf, nd) in r.stderr
    with open(full) as f:
        full_rows = f.read().splitlines()
    with open(kept) as f:
        kept_rows = f.read().splitlines()
    assert len(kept_rows) == nd < len(full_rows)
    assert is_subsequence(kept_rows, full_rows)
    with open(resp) as f:
        got = np.array([np.float32(x) for x in f.read().split()], np.float32)
    assert got.tobytes() == want.tobytes()          # %.9g round-trips a float32


def test_match_takes_the_option(gpu_hip, tmp_path):
    pa, pb = str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm")
    write_pgm(pa, IMG)
    write_pgm(pb, np.roll(IMG, (4, 8), axis=(0, 1)))
    counts = []
    for extra in ([], ["--keep-strongest", str(KEEP)]):
        r = subprocess.run([MATCH, "-l", pa, "-r", pb, "--pairs", "--feature-order", "raster"] + extra, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        counts.append(len(r.stdout.splitlines()))
    assert 50 < counts[1] < counts[0]


def test_negative_count_is_a_usage_error(gpu_hip, tmp_path):
    pgm = str(tmp_path / "img.pgm")
    write_pgm(pgm, IMG)
    r = demo("-i", pgm, "--keep-strongest", "-1", "--output-file", str(tmp_path / "never.txt"))
    assert r.returncode != 0 and "--keep-strongest" in r.stderr and "Usage:" in r.stderr, r.stderr
    assert not os.path.exists(str(tmp_path / "never.txt"))
    r = subprocess.run([MATCH, "-l", pgm, "-r", pgm, "--keep-strongest", "-1"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--keep-strongest" in r.stderr, r.stderr
    # the responses file needs the option that produces them
    r = demo("-i", pgm, "--write-responses", str(tmp_path / "r.txt"), "--output-file", str(tmp_path / "never.txt"))
    assert r.returncode != 0 and "--keep-strongest" in r.stderr, r.stderr
