"""The device-resident sets through the C ABI (sets.hip, and the two clone calls of ctx.hip): every constructor at sizes
around one 256-thread block of k_clone_features / k_desc_bytes, the argument errors, the clones of a small and of an empty
result, and a set's release after every call that parks scratch in it.  Every comparison is exact.

Asserted elsewhere and not repeated here: clone_results().download() against fetch() on a 320 x 240 image
(test_gpu_match.py::test_cloned_results_and_image_to_image_matching) and clone_results_u8 / from_set / download_u8
against fetch(fmt="u8") on the same image (test_gpu_match_bytes.py::test_sets_from_extraction)."""
import ctypes as C

import numpy as np
import pytest

import desc_cases

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 3, 257)              # 257: one past a 256-thread block


def floats(n, seed=5):
    """n descriptors over the byte rule's whole range: negatives, halves, values past 255"""
    d = np.random.default_rng(seed).uniform(-20, 300, (n, 128)).astype(np.float32)
    d[:, ::7] = np.floor(d[:, ::7]) + np.float32(0.5)
    return d


def points(n):
    return np.stack([np.arange(n, dtype=np.float32) * 3 + 1, np.arange(n, dtype=np.float32) % 17 + 2], 1)


def ptrs(hip, s):
    p = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
    assert hip.lib().popsift_hip_devfeatures_ptrs(s._h, *map(C.byref, p)) == hip.OK
    return [x.value for x in p]


def alloc(hip, n_feat, n_desc):
    h = C.c_void_p()
    assert hip.lib().popsift_hip_devfeatures_alloc(0, n_feat, n_desc, C.byref(h)) == hip.OK and h.value
    return hip.DevFeatures(h)


def free(hip, s):
    """the free call's own status; the wrapper forgets the handle"""
    fn = hip.lib().popsift_hip_devfeatures_free if isinstance(s, hip.DevFeatures) else hip.lib().popsift_hip_bytefeatures_free
    h, s._h = s._h, None
    return fn(h)


@pytest.mark.parametrize("n", SIZES)
def test_every_constructor(gpu_hip, n):
    hip = gpu_hip
    d, xy = floats(n), points(n)
    q = hip.quantize_u8(d)
    assert n == 0 or (q.min() == 0 and q.max() == 255)
    H = hip.DevFeatures.from_host(d)
    P = hip.DevFeatures.from_host_points(d, xy)
    A = alloc(hip, n + 2, n)
    assert H.info() == (0, 0, n) and P.info() == (0, n, n) and A.info() == (0, n + 2, n)
    for s in (H, P, A):
        assert all(ptrs(hip, s)), n
    got, rev = H.download()
    assert got.tobytes() == d.tobytes() and got.shape == (n, 128) and (rev == -1).all() and rev.shape == (n,)
    got, rev = P.download()
    assert got.tobytes() == d.tobytes() and np.array_equal(rev, np.arange(n))
    got, rev = A.download()
    assert not got.any() and not rev.any() and got.shape == (n, 128)
    for s, want_rev in ((H, np.full(n, -1)), (P, np.arange(n))):
        B = hip.ByteFeatures.from_set(s)
        assert B.info() == (0, n)
        b, rev = B.download()
        assert np.array_equal(b, q) and np.array_equal(rev, want_rev)
        assert np.array_equal(s.download_u8(), q)
        assert free(hip, B) == hip.OK
    B = hip.ByteFeatures.from_host(q)
    b, rev = B.download()
    assert B.info() == (0, n) and np.array_equal(b, q) and (rev == -1).all() and rev.shape == (n,)
    for s in (H, P, A, B):
        assert free(hip, s) == hip.OK


def test_argument_errors(gpu_hip):
    hip, L = gpu_hip, gpu_hip.lib()
    d, xy, q = floats(3), points(3), hip.quantize_u8(floats(3))
    dp, xp, qp = d.ctypes.data, xy.ctypes.data, q.ctypes.data
    S = hip.DevFeatures.from_host(d)
    bad = hip.device_count()
    # (call, arguments before `out`): out == NULL first, then each bad argument with an out that must come back NULL
    calls = [
        (L.popsift_hip_devfeatures_alloc, [(0, 3, 3)], [(0, -1, 3), (0, 3, -1), (bad, 3, 3), (-1, 3, 3)]),
        (L.popsift_hip_devfeatures_from_host, [(0, dp, 3)], [(0, dp, -1), (0, None, 3), (bad, dp, 3)]),
        (L.popsift_hip_devfeatures_from_host_points, [(0, dp, xp, 3)],
         [(0, dp, xp, -1), (0, None, xp, 3), (0, dp, None, 3), (bad, dp, xp, 3)]),
        (L.popsift_hip_bytefeatures_from_host, [(0, qp, 3)], [(0, qp, -1), (0, None, 3), (bad, qp, 3)]),
        (L.popsift_hip_bytefeatures_from_set, [(S._h,)], [(None,)]),
    ]
    for fn, good, bads in calls:
        for args in good:
            assert fn(*args, None) == hip.ERR_INVALID, (fn.__name__, args)
        for args in bads:
            # a refused device index clears the handle; the other argument errors return before they touch it
            h = C.c_void_p(0xdead if args[0] in (bad, -1) else None)
            assert fn(*args, C.byref(h)) == hip.ERR_INVALID, (fn.__name__, args)
            assert not h.value, (fn.__name__, args)
    # null inputs are fine where nothing is read
    for fn, args in ((L.popsift_hip_devfeatures_from_host, (0, None, 0)),
                     (L.popsift_hip_devfeatures_from_host_points, (0, None, None, 0)),
                     (L.popsift_hip_bytefeatures_from_host, (0, None, 0))):
        h = C.c_void_p()
        assert fn(*args, C.byref(h)) == hip.OK and h.value
        assert (L.popsift_hip_bytefeatures_free if "byte" in fn.__name__ else L.popsift_hip_devfeatures_free)(h) == hip.OK
    assert L.popsift_hip_devfeatures_free(None) == hip.OK and L.popsift_hip_bytefeatures_free(None) == hip.OK
    assert L.popsift_hip_devfeatures_info(None, None, None, None) == hip.ERR_INVALID
    assert L.popsift_hip_devfeatures_ptrs(None, None, None, None) == hip.ERR_INVALID
    assert L.popsift_hip_devfeatures_download(None, None, None) == hip.ERR_INVALID
    assert L.popsift_hip_bytefeatures_info(None, None, None) == hip.ERR_INVALID
    assert L.popsift_hip_bytefeatures_download(None, None, None) == hip.ERR_INVALID
    assert L.popsift_hip_devfeatures_download_u8(S._h, None) == hip.ERR_INVALID
    assert free(hip, S) == hip.OK


@pytest.mark.parametrize("image", ("synth7_96x72", "flat"))
def test_clones(gpu_hip, image):
    hip = gpu_hip
    img = desc_cases.image(image) if image != "flat" else np.full((72, 96), 100, np.uint8)
    ctx = hip.Context(hip.default_params(norm_multi=9)).submit(img)
    nf, nd = ctx.wait()
    assert (nf, nd) == (0, 0) if image == "flat" else nd >= nf > 100
    feats, desc = ctx.fetch()
    _, desc8 = ctx.fetch(fmt="u8")
    assert hip.lib().popsift_hip_clone_results(ctx._h, None) == hip.ERR_INVALID
    assert hip.lib().popsift_hip_clone_results_u8(ctx._h, 0, None) == hip.ERR_INVALID
    F, B = ctx.clone_results(), ctx.clone_results_u8(0)
    assert F.info() == (0, nf, nd) and B.info() == (0, nd)
    assert all(ptrs(hip, F))
    got, rev = F.download()
    want_rev = np.repeat(np.arange(nf), feats["num_ori"])
    assert got.tobytes() == desc.tobytes() and got.shape == (nd, 128) and np.array_equal(rev, want_rev)
    got8, rev8 = B.download()
    assert np.array_equal(got8, desc8) and got8.shape == (nd, 128) and np.array_equal(rev8, want_rev)
    assert np.array_equal(desc8, hip.quantize_u8(desc))
    assert nd == 0 or desc8.max() > 100
    # the context still has its results after the clones
    assert ctx.fetch()[1].tobytes() == desc.tobytes()
    assert free(hip, F) == hip.OK and free(hip, B) == hip.OK
    ctx.close()


def test_a_used_left_set_is_freed_and_its_successor_works(gpu_hip):
    """every call that keeps scratch in its left set, then free; a second set of the same size gives the same answers"""
    hip = gpu_hip
    n, m = 257, 130
    d, xy = floats(n, 11), points(n)
    R = hip.DevFeatures.from_host_points(d[:m] + np.float32(0.25), xy[:m])
    RB = hip.ByteFeatures.from_set(R)
    I3 = np.eye(3, dtype=np.float32)

    def use(L, LB):
        out = [L.match(R).tobytes()]
        assert hip.lib().popsift_hip_match_set_path(hip.MATCH_SCREEN) == hip.OK
        try:
            out.append(L.match(R).tobytes())                                    # the screened path: norms and the redo list
            assert L.debug_redo_count() >= 0
        finally:
            assert hip.lib().popsift_hip_match_set_path(hip.MATCH_AUTO) == hip.OK
        pairs = L.match_pairs(R, ratio=0.0, cross_check=True)
        assert len(pairs) == m
        out += [pairs.tobytes(), L.match_guided(R, "homography", I3, 2.0).tobytes(),
                L.match_pairs_guided(R, "homography", I3, 2.0, ratio=0.0, cross_check=True).tobytes()]
        pts = L.pair_points(R, pairs)
        assert np.array_equal(pts[:, :2], xy[pairs["l"]]) and np.array_equal(pts[:, 2:], xy[pairs["r"]])
        out += [pts.tobytes(), LB.match(RB).tobytes(), LB.match_pairs(RB, ratio=0.0, cross_check=True).tobytes()]
        return out

    L = hip.DevFeatures.from_host_points(d, xy)
    LB = hip.ByteFeatures.from_set(L)
    first = use(L, LB)
    assert free(hip, L) == hip.OK and free(hip, LB) == hip.OK
    L = hip.DevFeatures.from_host_points(d, xy)
    LB = hip.ByteFeatures.from_set(L)
    assert use(L, LB) == first
    for s in (L, LB, R, RB):
        assert free(hip, s) == hip.OK
