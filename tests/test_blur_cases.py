"""The case list of tests/blur_cases.py reaches every 64-row instance of the tile kernels (no GPU: the list and the
restated dispatch are checked, not the library).  The spans are the oracle's gauss_table(), level 0 first."""
import pytest

from blur_cases import BUCKETS, CASES, case_instances, level0_fast2x, oracle_kw, tile_instance


@pytest.fixture(scope="module")
def spans(oracle_mod):
    out = {}
    for name, kw, spec in CASES:
        orc = oracle_mod.Oracle(oracle_mod.default_params(**oracle_kw(kw)))
        out[name] = [int(s) for s in orc.gauss_table()[1]]
        orc.close()
    return out


def test_case_names_are_unique():
    assert len({c[0] for c in CASES}) == len(CASES)


def test_halos_of_the_parameter_sets(spans):
    """the halos (span - 1) the cases were chosen by"""
    halos = {n: [s - 1 for s in v] for n, v in spans.items()}
    assert halos["default_400x300"] == [5, 5, 7, 8, 10, 13]
    assert halos["levels5_sigma1p3"] == [4, 3, 4, 4, 5, 6, 6, 7]
    assert halos["levels2_sigma2"] == [7, 8, 12, 16, 23]
    assert halos["levels2_sigma1p8"] == [6, 8, 11, 15, 21]
    assert halos["no_upscale_257x129"] == [7, 5, 7, 8, 10, 13]
    assert halos["initial_blur4_sigma2"] == [30, 7, 8, 10, 13, 16]
    assert halos["initial_blur2p5_sigma2_opencv"] == [19, 6, 8, 10, 13, 16]


def test_the_dispatch_restated():
    assert [tile_instance(0, 64, h, False) for h in (0, 4, 5, 10)] == [("k_blur_tile", b, 512) for b in (4, 4, 5, 10)]
    assert [tile_instance(0, 64, h, False) for h in (11, 12, 13)] == [("k_blur_tile64_lp", 13, 512)] * 3
    assert [tile_instance(0, 64, h, True) for h in (11, 13)] == [("k_blur_tile", 13, 256)] * 2
    assert [tile_instance(m, 64, 12, False) for m in (1, 2)] == [("k_blur_tile", 13, 256)] * 2
    assert [tile_instance(0, 64, h, False) for h in (14, 16, 17, 22, 23, 30)] == [("k_blur_tile", b, 256) for b in (16, 16, 22, 22, 30, 30)]
    assert all(tile_instance(m, 32, h, d) == ("k_blur_tile", next(b for b in BUCKETS if h <= b), 256)
               for m in (0, 1, 2) for h in range(31) for d in (False, True))
    with pytest.raises(ValueError):
        tile_instance(0, 64, 31, False)
    with pytest.raises(ValueError):
        tile_instance(0, 48, 5, False)
    assert level0_fast2x(dict(), 400, False) == 2 and level0_fast2x(dict(), 333, False) == 1
    assert level0_fast2x(dict(), 400, True) == 1 and level0_fast2x(dict(sift_mode=2), 400, False) == 2
    assert level0_fast2x(dict(sift_mode=1), 400, False) == 0 and level0_fast2x(dict(upscale_factor=0.0), 400, False) == 0


def test_the_cases_reach_every_64_row_instance(spans):
    seen = set()
    for name, kw, spec in CASES:
        seen.update(case_instances(name, kw, spec, spans[name], 64))
    tile, lp13 = "k_blur_tile", ("k_blur_tile64_lp", 13, 512)
    want = []
    # mode 0, DoG on the fly
    want += [(0, False, None, (tile, b, 512)) for b in (4, 5, 6, 7, 8, 10)]
    want += [(0, False, None, lp13)]
    want += [(0, False, None, (tile, b, 256)) for b in (16, 22, 30)]
    # mode 0, stored DoG
    want += [(0, True, None, (tile, b, 256)) for b in (13, 16, 30)]
    missing = [w for w in want if w not in seen]
    assert not missing, missing
    assert any(m == 0 and dog and inst[2] == 512 for m, dog, _, inst in seen), "stored DoG at 512 lanes"
    # level 0: from u8 with each fast2x at some lane count and both lane counts, from f32 both lane counts
    assert {f for m, _, f, _ in seen if m == 1} == {0, 1, 2}
    for mode in (1, 2):
        assert {inst[2] for m, _, _, inst in seen if m == mode} == {256, 512}, mode
    # nothing of mode 0 on the fly may claim the plain 13-bucket: those launches are lp13's
    assert (0, False, None, (tile, 13, 256)) not in seen and (0, False, None, (tile, 13, 512)) not in seen
