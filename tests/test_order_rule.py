"""The raster feature order without a GPU: tests/order_rule.py on the oracle's extrema and on hand-made records, the
params field, and what popsift_hip_ctx_create refuses before it touches a device."""
import ctypes as C

import numpy as np

import order_rule as R
from popsift_amd.synth import synth


def test_pix_and_bits_define_every_value():
    f = np.float32
    v = np.array([np.nan, -np.inf, -1.0, -0.0, 0.0, 0.99, 1.0, 17.75, 32766.9, 32767.0, 1e9, np.inf], f)
    assert R.pix(v).tolist() == [0, 0, 0, 0, 0, 0, 1, 17, 32766, 32767, 32767, 32767]
    # bits(): numeric order on the non-negative finite values, -0.0 after every positive value
    pos = np.array([0.0, 1e-30, 0.5, 0.5000001, 3.0, 1e9], f)
    assert np.all(np.diff(R.bits(pos)) > 0)
    assert R.bits(np.array([-0.0], f))[0] > R.bits(np.array([np.inf], f))[0]


def test_hand_made_records(hip):
    e = np.zeros(8, hip.EXTREMUM_DTYPE)
    #            xpos  ypos  lpos sigma octave
    rows = [(5.5, 2.2, 1, 2.0, 1),      # octave 1 goes last
            (9.1, 3.9, 2, 2.0, 0),
            (9.7, 3.1, 1, 2.0, 0),      # same pixel (9, 3), lower level: before the record above
            (9.7, 3.1, 1, 1.5, 0),      # same but a smaller sigma: before
            (9.2, 3.1, 1, 9.0, 0),      # same pixel and level, same ypos, smaller xpos: before
            (2.0, 3.99, 3, 2.0, 0),     # same row, an earlier column
            (30.0, 2.0, 3, 2.0, 0),     # an earlier row
            (9.7, 3.1, 1, 1.5, 0)]      # a byte-identical twin of row 3
    for i, (x, y, l, s, o) in enumerate(rows):
        e[i] = (x, y, l, s, o, 0)
    p = R.permutation(e)
    assert p.tolist() in ([6, 5, 4, 3, 7, 2, 1, 0], [6, 5, 4, 7, 3, 2, 1, 0])
    assert R.is_ordered(R.sort(e)) and not R.is_ordered(e)


def test_oracle_extrema_sorted_by_the_rule(oracle_mod):
    O = oracle_mod
    orc = O.Oracle(O.default_params(), threads=4).run(synth(5, 128, 96))
    ext = orc.extrema()
    assert len(ext) > 100 and len(np.unique(ext["octave"])) >= 3
    s = R.sort(ext)
    assert sorted(s.tobytes()[i:i + 24] for i in range(0, 24 * len(s), 24)) == \
        sorted(ext.tobytes()[i:i + 24] for i in range(0, 24 * len(ext), 24))
    k = R.keys(s).tolist()
    for i in range(1, len(s)):
        assert k[i - 1] <= k[i], i
        if k[i - 1] == k[i]:        # a tie under the whole tuple: the same record twice
            assert s[i - 1].tobytes() == s[i].tobytes(), i
    assert np.all(np.diff(s["octave"]) >= 0)
    # what refinement lets through (the header's remark on the key's domain)
    for o in range(orc.num_octaves):
        w, h = orc.octave_dims(o)
        m = ext[ext["octave"] == o]
        assert np.all((m["xpos"] >= 0) & (m["xpos"] <= w - 1) & (m["ypos"] >= 0) & (m["ypos"] <= h - 1))
    assert np.all(np.isfinite(ext["sigma"]) & (ext["sigma"] > 0) & (ext["lpos"] >= 0))


def test_params_field(hip):
    assert C.sizeof(hip.Params) == 80
    assert hip.Params.feature_order.offset == 76 and hip.Params.feature_order.size == 4
    assert (hip.ORDER_ARRIVAL, hip.ORDER_RASTER) == (0, 1)
    assert hip.default_params().feature_order == hip.ORDER_ARRIVAL
    assert hip.DEBUG_ORDER_COARSE == 14 and hip.ORDER_CHUNK == 1024


def test_ctx_create_validates_the_order_before_any_device_call(hip):
    lib = hip.lib()
    h = C.c_void_p()
    for v in (-1, 2):
        p = hip.default_params(feature_order=v)
        assert lib.popsift_hip_ctx_create(0, C.byref(p), C.byref(h)) == hip.ERR_INVALID, v
    for v in (hip.ORDER_ARRIVAL, hip.ORDER_RASTER):
        p = hip.default_params(feature_order=v)
        rc = lib.popsift_hip_ctx_create(0, C.byref(p), C.byref(h))
        try:
            assert rc == (hip.OK if hip.device_count() > 0 else hip.ERR_NO_DEVICE), (v, rc)
        finally:
            if rc == hip.OK:
                lib.popsift_hip_ctx_destroy(h)
