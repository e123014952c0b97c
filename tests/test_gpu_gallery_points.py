"""Positions in a gallery: popsift_hip_gallery_add_set and popsift_hip_gallery_pair_points against the per-pair calls
(popsift_hip_bytefeatures_from_set, popsift_hip_pair_points), and a gallery verified end to end with
popsift_hip_ransac_many."""
import ctypes as C

import numpy as np
import pytest

from popsift_amd.synth import synth

pytestmark = pytest.mark.gpu

SHIFT = (4.0, 2.0)    # (x, y) of np.roll(q, (2, 4), axis=(0, 1))


@pytest.fixture(scope="module")
def sets(gpu_hip):
    """three 240 x 180 images: a query, its shifted copy, an unrelated one -> their float sets and byte sets"""
    hip = gpu_hip
    q = synth(95, 240, 180)
    imgs = [q, np.roll(q, (2, 4), axis=(0, 1)), synth(23, 240, 180)]
    p9 = hip.default_params(norm_multi=9)
    floats = [hip.Context(p9).submit(img).clone_results() for img in imgs]
    return floats, [hip.ByteFeatures.from_set(f) for f in floats]


def test_add_set_is_from_set_plus_positions(gpu_hip, sets):
    hip = gpu_hip
    (Q, A, B), (Qb, Ab, Bb) = sets
    by_set, by_bytes = hip.Gallery(), hip.Gallery()
    assert [by_set.add_set(A), by_set.add_set(B)] == [0, 1] and [by_bytes.add(Ab), by_bytes.add(Bb)] == [0, 1]
    for m, b in enumerate((Ab, Bb)):
        assert by_set.download(m).tobytes() == b.download()[0].tobytes() and by_set.member(m) == by_bytes.member(m)
    assert by_set.info() == by_bytes.info()
    # the matchers do not see how the members were added
    assert by_set.match(Qb).tobytes() == by_bytes.match(Qb).tobytes()
    for kw in (dict(cross_check=True), dict(ratio=0.7)):
        p1, o1 = by_set.match_pairs(Qb, **kw)
        p2, o2 = by_bytes.match_pairs(Qb, **kw)
        assert p1.tobytes() == p2.tobytes() and o1.tobytes() == o2.tobytes() and len(p1) > 50
    # the points of the CSR are the per-member points
    pairs, off = by_set.match_pairs(Qb, cross_check=True)
    pts = by_set.pair_points(Q, pairs, off)
    assert pts.shape == (len(pairs), 4)
    for m, f in enumerate((A, B)):
        assert off[m + 1] > off[m]
        assert pts[off[m]:off[m + 1]].tobytes() == Q.pair_points(f, pairs[off[m]:off[m + 1]]).tobytes(), m


def test_members_without_positions_and_bad_arguments(gpu_hip, sets):
    hip, lib = gpu_hip, gpu_hip.lib()
    (Q, A, B), (Qb, Ab, Bb) = sets
    g = hip.Gallery()
    # a member without positions in between, an empty one with positions at the end: every index as in a byte gallery
    assert [g.add_set(A), g.add(Bb.download()[0]), g.add_set(B), g.add(Ab), g.add_set(hip.DevFeatures.from_host_points(
        np.zeros((0, 128), np.float32), np.zeros((0, 2), np.float32)))] == [0, 1, 2, 3, 4]
    plain = hip.Gallery()
    for b in (Ab, Bb, Bb, Ab, hip.ByteFeatures.from_host(np.zeros((0, 128), np.uint8))):
        plain.add(b)
    assert [g.member(m) for m in range(5)] == [plain.member(m) for m in range(5)]
    pairs, off = g.match_pairs(Qb, cross_check=True)
    p2, o2 = plain.match_pairs(Qb, cross_check=True)
    assert pairs.tobytes() == p2.tobytes() and off.tobytes() == o2.tobytes()
    assert off[2] > off[1] and off[4] > off[3] and off[5] == off[4]

    def call(l, gal, prs, offs, out):
        return lib.popsift_hip_gallery_pair_points(l, gal, prs.ctypes.data if prs is not None else None,
                                                   offs.ctypes.data if offs is not None else None,
                                                   out.ctypes.data if out is not None else None)

    out = np.full((len(pairs), 4), 7.0, np.float32)
    assert call(Q._h, g._h, pairs, off, out) == hip.ERR_INVALID and (out == 7.0).all()     # pairs lie in members 1 and 3
    # without the lists of members 1 and 3: the points of the others
    keep = np.r_[np.arange(off[0], off[1]), np.arange(off[2], off[3])]
    kp, ko = pairs[keep], np.array([0, off[1], off[1], off[1] + off[3] - off[2]] + [len(keep)] * 2, np.int32)
    pts = g.pair_points(Q, kp, ko)
    assert pts[:ko[1]].tobytes() == Q.pair_points(A, kp[:ko[1]]).tobytes()
    assert pts[ko[2]:].tobytes() == Q.pair_points(B, kp[ko[2]:]).tobytes()
    # a pair index outside the query or outside its member: nothing is written
    for field, value, where in (("l", Q.info()[2], 0), ("l", -1, 3), ("r", A.info()[2], 0), ("r", B.info()[2], ko[2]),
                                ("r", -1, len(kp) - 1)):
        bad = kp.copy()
        bad[field][where] = value
        out = np.full((len(kp), 4), 7.0, np.float32)
        assert call(Q._h, g._h, bad, ko, out) == hip.ERR_INVALID and (out == 7.0).all(), (field, value, where)
    # NULLs and offsets
    out = np.zeros((len(kp), 4), np.float32)
    assert call(Q._h, g._h, kp, ko, out) == hip.OK
    assert call(None, g._h, kp, ko, out) == hip.ERR_INVALID
    assert call(Q._h, None, kp, ko, out) == hip.ERR_INVALID
    assert call(Q._h, g._h, kp, None, out) == hip.ERR_INVALID
    assert call(Q._h, g._h, None, ko, out) == hip.ERR_INVALID
    assert call(Q._h, g._h, kp, ko, None) == hip.ERR_INVALID
    for bad in (ko + 1, np.array([0, 5, 4, 4, 4, 4], np.int32)):
        assert call(Q._h, g._h, kp, bad, out) == hip.ERR_INVALID
    assert lib.popsift_hip_gallery_add_set(None, A._h, None) == hip.ERR_INVALID
    assert lib.popsift_hip_gallery_add_set(g._h, None, None) == hip.ERR_INVALID
    # a query without features behind its descriptors: found on the GPU, as popsift_hip_pair_points
    bare = hip.DevFeatures.from_host(Q.download()[0])
    out = np.full((len(kp), 4), 7.0, np.float32)
    assert call(bare._h, g._h, kp, ko, out) == hip.ERR_INVALID and (out == 7.0).all()
    # a member whose map names no feature is refused and the gallery stays as it was
    before = g.info()
    assert lib.popsift_hip_gallery_add_set(g._h, bare._h, None) == hip.ERR_INVALID and g.info() == before
    # only members without positions: an all-empty CSR is accepted
    assert plain.pair_points(Q, np.zeros(0, hip.PAIR_DTYPE), np.zeros(6, np.int32)).shape == (0, 4)
    assert call(Q._h, plain._h, p2, o2, np.zeros((len(p2), 4), np.float32)) == hip.ERR_INVALID


def test_a_gallery_verified_end_to_end(gpu_hip, sets):
    hip = gpu_hip
    (Q, A, B), (Qb, _, _) = sets
    g = hip.Gallery()
    g.add_set(A)
    g.add_set(B)
    pairs, off = g.match_pairs(Qb, cross_check=True)
    pts = g.pair_points(Q, pairs, off)
    v = hip.Verifier()
    max_err = 2.0
    res, mask = v.ransac_many(pts, off, "homography", 512, max_err, 3)
    # the per-list call on the per-pair points of the shifted copy: the same record and mask
    one, one_mask = v.ransac(Q.pair_points(A, pairs[:off[1]]), "homography", 512, max_err, 3)
    assert res[0].tobytes() == one.tobytes() and mask[:off[1]].tobytes() == one_mask.tobytes()
    v.close()
    assert res[0]["hypothesis"] >= 0 and res[0]["n_inliers"] > res[1]["n_inliers"] and res[0]["n_inliers"] >= 30
    assert res[0]["n_inliers"] == mask[:off[1]].sum() and res[1]["n_inliers"] == mask[off[1]:].sum()
    # translation-like: an inlier's image under H lies within max_err of its right point (the inlier rule, here in
    # float64), and the typical right point is the left point moved by the shift
    inl = pts[:off[1]][mask[:off[1]] == 1].astype(np.float64)
    Hm = res[0]["H"].astype(np.float64).reshape(3, 3)
    q = np.c_[inl[:, :2], np.ones(len(inl))] @ Hm.T
    img = q[:, :2] / q[:, 2:3]
    assert (np.hypot(*(img - inl[:, 2:]).T) <= max_err * (1 + 1e-4)).all()
    assert np.median(np.hypot(*(img - (inl[:, :2] + SHIFT)).T)) <= max_err
    assert np.allclose(np.median(inl[:, 2:] - inl[:, :2], axis=0), SHIFT, atol=0.05)
