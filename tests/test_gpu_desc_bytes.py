"""Descriptors as bytes on the GPU (popsift_hip_fetch*_u8, desc_bytes.hip): every byte equals the rule of
include/popsift_hip.h applied to the float result of the same finished image (quantize_u8, tests/test_desc_bytes.py),
the feature records are those of the float fetch, and the byte buffer survives the download overlap protocol."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from popsift_amd.synth import synth
from test_desc_bytes import EDGES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "popsift_amd")


def rows(feats, desc):
    """(features, descriptors) -> one row per orientation (x, y, sigma, num_ori, k, angle bits, descriptor bytes), sorted:
    equal for two runs of one image whatever order the compaction gave their features"""
    out = []
    for k in range(4):
        sel = feats[feats["num_ori"] > k]
        if len(sel) == 0:
            continue
        head = np.stack([sel["xpos"].view(np.uint32), sel["ypos"].view(np.uint32), sel["sigma"].view(np.uint32),
                         sel["num_ori"].astype(np.uint32), np.full(len(sel), k, np.uint32),
                         np.ascontiguousarray(sel["orientation"][:, k]).view(np.uint32)], 1)
        body = np.ascontiguousarray(desc[sel["desc_idx"][:, k]]).view(np.uint32).reshape(len(sel), -1)
        out.append(np.concatenate([head, body], 1))
    if not out:
        return np.zeros((0, 38), np.uint32)
    a = np.concatenate(out, 0)
    return a[np.lexsort(a.T[::-1])]


def same_image(hip, f32, u8):
    """the byte fetch of an image against q() of a float result of the same image (any run)"""
    assert np.array_equal(rows(u8[0], u8[1]), rows(f32[0], hip.quantize_u8(f32[1])))


def parity(hip, ctx):
    """float fetch, then byte fetch of the SAME finished image: records byte-identical, bytes = q(floats)"""
    ff, fd = ctx.fetch()
    bf, bd = ctx.fetch(fmt="u8")
    assert bd.dtype == np.uint8 and bd.shape == fd.shape
    assert ff.tobytes() == bf.tobytes()
    assert np.array_equal(bd, hip.quantize_u8(fd))
    return ff, fd, bd


def test_planted_values_through_the_kernel(gpu_hip):
    edge = np.zeros(128, np.float32)
    extra = [-np.inf, -1.0, -1e-30, 0.0, 254.999, 255.00002, 3.4028235e38, 0.50000006, 127.5, 128.5, 253.5, 7.49999952]
    vals = [e[0] for e in EDGES] + extra
    edge[:len(vals)] = vals
    rnd = np.random.default_rng(7).uniform(0, 300, 7813 * 128).astype(np.float32)   # 10^6 values and a few more
    # every .5 of [0, 256) and one ulp either side of it
    half = np.arange(0, 256, dtype=np.float32) + np.float32(0.5)
    ties = np.concatenate([half, np.nextafter(half, np.float32(0)), np.nextafter(half, np.float32(1e9))])
    ties = np.concatenate([ties, np.zeros((-len(ties)) % 128, np.float32)])
    planted = np.concatenate([edge, rnd, ties]).reshape(-1, 128)
    s = gpu_hip.DevFeatures.from_host(planted)
    got = s.download_u8()
    s.close()
    want = gpu_hip.quantize_u8(planted)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert got[0, :len(EDGES)].tolist() == [e[1] for e in EDGES]
    # an empty set
    e = gpu_hip.DevFeatures.from_host(np.zeros((0, 128), np.float32))
    assert e.download_u8().shape == (0, 128)
    e.close()


CONFIGS = {
    "default": {},
    "rootsift_nm9": dict(norm_multi=9),
    "classic_nm9": dict(norm_mode=1, norm_multi=9),
    "classic_nm12": dict(norm_mode=1, norm_multi=12),
    "grid": dict(desc_mode=2, norm_multi=9),
    "igrid": dict(desc_mode=3, norm_multi=9),
    "notile": dict(desc_mode=4, norm_multi=9),
    "iloop": dict(desc_mode=1, norm_multi=9),
    "no_upscale": dict(upscale_factor=0.0, norm_multi=9),
    "grid_filter": dict(filter_max_extrema=300, filter_grid_size=4, norm_multi=9),
}


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_extraction_parity(gpu_hip, name):
    ctx = gpu_hip.Context(gpu_hip.default_params(**CONFIGS[name]))
    ff, fd, bd = parity(gpu_hip, ctx.submit(synth(61, 480, 360)))
    assert len(fd) > 100
    if name == "default":
        assert bd.max() <= 1                         # norm_multi 0: every byte is 0 or 1
    if name == "classic_nm12":
        assert (bd == 255).mean() > 0.01             # heavy saturation
    ctx.close()


def test_f32_image_and_odd_pitch(gpu_hip):
    ctx = gpu_hip.Context(gpu_hip.default_params(norm_multi=9))
    img = synth(62, 333, 257)
    parity(gpu_hip, ctx.submit(img.astype(np.float32) / np.float32(256.0)))
    pitch = 347                                      # odd, larger than the width
    padded = np.zeros((257, pitch), np.uint8)
    padded[:, :333] = img
    ctx._chk(gpu_hip.lib().popsift_hip_submit_u8(ctx._h, padded.ctypes.data, 333, 257, pitch), "submit_u8")
    parity(gpu_hip, ctx)
    ctx.close()


def test_dense_1080p(gpu_hip):
    ctx = gpu_hip.Context(gpu_hip.default_params(norm_multi=9))
    ff, fd, bd = parity(gpu_hip, ctx.submit(synth(100, 1920, 1080)))
    assert len(fd) > 50000
    ctx.close()


def test_descriptor_capacity_regrowth(gpu_hip):
    ctx = gpu_hip.Context(gpu_hip.default_params(norm_multi=9))
    ctx.debug_set(gpu_hip.DEBUG_DESC_CAP, 64)
    img = synth(63, 640, 480)
    bf, bd = ctx.submit(img).fetch(fmt="u8")        # the byte buffer is first sized after the grow-and-rerun
    ff, fd = ctx.fetch()
    assert len(fd) > 64 and ff.tobytes() == bf.tobytes() and np.array_equal(bd, gpu_hip.quantize_u8(fd))
    # a larger image grows the slab again: the byte buffer follows
    parity(gpu_hip, ctx.submit(synth(64, 1280, 960)))
    ctx.close()


def test_flat_image_has_no_features(gpu_hip):
    ctx = gpu_hip.Context(gpu_hip.default_params(norm_multi=9))
    ctx.submit(np.full((240, 320), 128, np.uint8))
    bf, bd = ctx.fetch(fmt="u8")
    assert len(bf) == 0 and bd.shape == (0, 128)
    ctx.close()


def test_batch_of_16_overlapped(gpu_hip):
    params = gpu_hip.default_params(norm_multi=9)
    a = [synth(200 + i, 320, 240) for i in range(16)]
    b = [synth(300 + i, 320, 240) for i in range(16)]
    ref = gpu_hip.Context(params)
    want_a = [ref.submit(im).fetch() for im in a]
    want_b = [ref.submit(im).fetch() for im in b]
    ctx = gpu_hip.Context(params)
    ctx.submit_batch(a)
    ctx.wait_batch()
    pend = [ctx.fetch_begin_item(k, fmt="u8") for k in range(16)]
    ctx.submit_batch(b)                              # its kernels run under the downloads of a
    got_a = [p.result() for p in pend]               # the first result() is the one fetch_end; the others have landed
    for k in range(16):
        same_image(gpu_hip, want_a[k], got_a[k])
    for k in range(16):
        same_image(gpu_hip, want_b[k], ctx.fetch_item(k, fmt="u8"))
    # float and byte downloads alternating on consecutive images
    seq = a[:6]
    pend, got = None, []
    for i, im in enumerate(seq):
        ctx.submit(im)
        if pend is not None:
            got.append(pend.result())
        pend = ctx.fetch_begin(fmt="u8" if i % 2 else "f32")
    got.append(pend.result())
    for i in range(len(seq)):
        if i % 2:
            same_image(gpu_hip, want_a[i], got[i])
        else:
            assert np.array_equal(rows(*got[i]), rows(*want_a[i]))
    ctx.close()
    ref.close()


def test_pending_byte_download_and_synchronous_fetch(gpu_hip):
    """fetch_begin_u8 of image N, submit N+1, synchronous fetch_u8 of N+1, only then fetch_end: the synchronous pass must
    not overwrite the byte buffer the pending download still reads"""
    params = gpu_hip.default_params(norm_multi=9)
    n0, n1 = synth(71, 1280, 720), synth(72, 1280, 720)
    ref = gpu_hip.Context(params)
    w0, w1 = ref.submit(n0).fetch(), ref.submit(n1).fetch()
    ctx = gpu_hip.Context(params)
    for _ in range(2):
        p = ctx.submit(n0).fetch_begin(fmt="u8")
        ctx.submit(n1)
        g1 = ctx.fetch(fmt="u8")
        g0 = p.result()                              # fetch_end: still pending, still completes
        same_image(gpu_hip, w0, g0)
        same_image(gpu_hip, w1, g1)
    # and the device pointer of N+1 while N's byte download is pending
    p = ctx.submit(n0).fetch_begin(fmt="u8")
    ctx.submit(n1).wait()
    fp, dp = ctx.results_dev_item(0, fmt="u8")
    same_image(gpu_hip, w0, p.result())
    ctx.close()
    ref.close()


def _hip_rt():
    rt = C.CDLL("libamdhip64.so")
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rt.hipMemcpy.restype = C.c_int
    return rt


def test_results_dev_item_u8(gpu_hip):
    ctx = gpu_hip.Context(gpu_hip.default_params(norm_multi=9))
    ctx.submit_batch([synth(81, 400, 300), synth(82, 400, 300)])
    rt = _hip_rt()
    for k in range(2):
        feats, desc = ctx.fetch_item(k, fmt="u8")
        fp, dp = ctx.results_dev_item(k, fmt="u8")
        assert fp and dp
        got = np.zeros_like(desc)
        assert rt.hipMemcpy(got.ctypes.data, dp, got.nbytes, 2) == 0            # hipMemcpyDeviceToHost
        gf = np.zeros_like(feats)
        assert rt.hipMemcpy(gf.ctypes.data, fp, gf.nbytes, 2) == 0
        assert np.array_equal(got, desc) and gf.tobytes() == feats.tobytes()
        _, fdesc = ctx.fetch_item(k)
        assert np.array_equal(got, gpu_hip.quantize_u8(fdesc))
    ctx.close()


def test_errors(gpu_hip):
    lib = gpu_hip.lib()
    ctx = gpu_hip.Context(gpu_hip.default_params(norm_multi=9))
    ctx.submit(synth(91, 320, 240))
    nf, nd = ctx.wait()
    feats = np.zeros(nf, gpu_hip.FEATURE_DTYPE)
    desc = np.zeros((nd, 128), np.uint8)
    f, d = feats.ctypes.data, desc.ctypes.data
    assert lib.popsift_hip_fetch_u8(ctx._h, f, nf, d, nd * 128 - 1) == gpu_hip.ERR_TOO_SMALL
    assert lib.popsift_hip_fetch_u8(ctx._h, f, nf - 1, d, nd * 128) == gpu_hip.ERR_TOO_SMALL
    assert lib.popsift_hip_fetch_begin_u8(ctx._h, f, nf, d, nd * 128 - 1) == gpu_hip.ERR_TOO_SMALL
    assert lib.popsift_hip_fetch_u8(ctx._h, f, nf, None, nd * 128) == gpu_hip.ERR_INVALID
    for k in (-1, 1, 16):
        assert lib.popsift_hip_fetch_item_u8(ctx._h, k, f, nf, d, nd * 128) == gpu_hip.ERR_INVALID
        assert lib.popsift_hip_fetch_begin_item_u8(ctx._h, k, f, nf, d, nd * 128) == gpu_hip.ERR_INVALID
        p = C.c_void_p()
        assert lib.popsift_hip_results_dev_item_u8(ctx._h, k, C.byref(p), C.byref(p)) == gpu_hip.ERR_INVALID
    pend = ctx.fetch_begin(fmt="u8")
    assert lib.popsift_hip_fetch_u8(ctx._h, f, nf, d, nd * 128) == gpu_hip.ERR_STATE
    assert lib.popsift_hip_fetch_begin_u8(ctx._h, f, nf, d, nd * 128) == gpu_hip.ERR_STATE
    p = C.c_void_p()
    assert lib.popsift_hip_results_dev_item_u8(ctx._h, 0, C.byref(p), C.byref(p)) == gpu_hip.ERR_STATE
    pf, pd = pend.result()
    assert pd.dtype == np.uint8 and len(pd) == nd
    fresh = gpu_hip.Context()
    assert lib.popsift_hip_fetch_u8(fresh._h, f, nf, d, nd * 128) == gpu_hip.ERR_STATE   # nothing submitted
    fresh.close()
    ctx.close()


@pytest.mark.parametrize("orientation", ["compute", "given"])
def test_describe(gpu_hip, orientation):
    """caller frames, including frames on a flat region (the normalisation of a patch without gradient)"""
    img = synth(95, 480, 360)
    img[:, :160] = 90                                # flat left third
    rng = np.random.default_rng(3)
    fr = np.zeros(400, gpu_hip.FRAME_DTYPE)
    fr["xpos"] = rng.uniform(10, 470, 400)
    fr["xpos"][:100] = rng.uniform(20, 120, 100)     # on the flat region
    fr["ypos"] = rng.uniform(10, 350, 400)
    fr["sigma"] = rng.uniform(1.0, 6.0, 400)
    fr["orientation"] = rng.uniform(-3, 3, 400)
    fr["octave"] = -1
    fr["level"] = -1
    params = gpu_hip.default_params(norm_multi=9)
    ctx = gpu_hip.Context(params)
    ctx.describe_batch_async([img], [fr], orientation)
    ff, fd = ctx.fetch_item(0)
    bf, bd = ctx.fetch_item(0, fmt="u8")
    assert ff.tobytes() == bf.tobytes() and np.array_equal(bd, gpu_hip.quantize_u8(fd))
    flat = np.concatenate([ff["desc_idx"][:100][ff["num_ori"][:100] > k][:, k] for k in range(4)])
    assert len(flat) > 0
    # a constant image: every patch is without gradient
    ctx.describe_batch_async([np.full((240, 320), 77, np.uint8)], [fr[fr["xpos"] < 300][:50]], orientation)
    ff, fd = ctx.fetch_item(0)
    bf, bd = ctx.fetch_item(0, fmt="u8")
    assert ff.tobytes() == bf.tobytes() and np.array_equal(bd, gpu_hip.quantize_u8(fd))
    print("constant image, %s: %d descriptors, %d NaN elements, bytes %s" %
          (orientation, len(fd), int(np.isnan(fd).sum()), np.unique(bd).tolist()))
    ctx.close()


def _write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())


@pytest.mark.parametrize("batch", [1, 4])
def test_cpp_api_byte_format(tmp_path, batch):
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host")], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "tests", "cpp", "host_desc_bytes_test.bin")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "host_desc_bytes_test.cpp"),
                           os.path.join(PKG, "host", "pgmread.cpp"), "-o", exe, "-L", PKG,
                           "-lpopsift", "-lpopsift_hip", "-pthread", "-Wl,-rpath," + PKG])
    paths = []
    for i in range(6):
        p = str(tmp_path / ("img%d.pgm" % i))
        _write_pgm(p, synth(400 + i, 640, 480))
        paths.append(p)
    env = dict(os.environ, POPSIFT_BATCH=str(batch), POPSIFT_CONTEXTS_PER_DEVICE="2")
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host_desc_bytes ok" in r.stdout


def test_demo_desc_bytes(tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host")], stdout=subprocess.DEVNULL)
    demo = os.path.join(PKG, "popsift-demo")
    img = str(tmp_path / "in.pgm")
    _write_pgm(img, synth(97, 640, 480))
    outs = {}
    for name, flags in (("uchar", ["--write-as-uchar"]), ("bytes", ["--desc-bytes"])):
        out = str(tmp_path / (name + ".txt"))
        r = subprocess.run([demo, "-i", img, "--norm-multi", "9", "--output-file", out] + flags, capture_output=True,
                           text=True, timeout=300, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr
        outs[name] = np.loadtxt(out, ndmin=2)
    a, b = outs["uchar"], outs["bytes"]
    assert a.shape == b.shape and a.shape[1] == 133 and len(a) > 100
    key = lambda m: m[np.lexsort(m.T[::-1])]
    want = a.copy()
    want[:, 5:] = np.minimum(want[:, 5:], 255)
    assert np.array_equal(key(b), key(want))
