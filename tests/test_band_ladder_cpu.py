"""The band ladder of the line tests (tests/band_ladder.py) and its restatement of the library's band rules, without a device."""
import numpy as np
import pytest

import band_ladder as B
from pinocchio_amd import synth


def test_restated_hess_band_gives_the_production_bands():
    """the five pruned radii of the 1024^3 benchmark step and the R = 6 radius of the 2048^3 configuration"""
    bands = [B.hess_band(1024, float(r)) for r in synth.radii_ladder(12)]
    assert bands[:5] == [93, 132, 186, 261, 372] == list(B.PRODUCTION_1024)
    assert all(b >= 512 for b in bands[5:])                  # the other seven radii: every mode
    assert B.hess_band(2048, 6.0) == 496 == B.PRODUCTION_2048[0]
    assert [B.hess_band(128, r) for r in (16.0, 8.0, 4.0, 2.0)] == [12, 24, 47, 1 << 30]   # tests/test_gpu_parity.py
    assert B.hess_band(1024, 0.0) == 1 << 30 and B.hess_band(1024, 16.0, eps=0.0) == 1 << 30
    # the largest band it can return is n / 2 - 1, and radius_of_band inverts it over the whole range
    for n in (40, 64, 96, 128, 1024, 2048):
        for band in range(1, n // 2):
            assert B.hess_band(n, B.radius_of_band(n, band)) == band
        top = B.radius_of_band(n, n // 2 - 1)                                     # its cut-off lies at n / 2 - 1.5 ...
        assert B.hess_band(n, top * (n // 2 - 1.5) / (n // 2 - 0.99)) == 1 << 30  # ... and a cut-off beyond n / 2 - 1 prunes nothing


def test_restated_compact_pitch():
    for fb, m in ((8, 8), (4, 16)):
        nzp = 528
        assert B.band_zpitch(1024, fb, 1 << 30, nzp) == nzp and B.band_zpitch(1024, fb, 512, nzp) == nzp
        for band in range(1, 512):
            zp = B.band_zpitch(1024, fb, band, nzp)
            assert zp % m == 0 and band + 1 <= zp < band + 1 + m and zp <= nzp
        assert B.band_zpitch(1024, fb, m - 1, nzp) == m and B.band_zpitch(1024, fb, m, nzp) == 2 * m


@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("n", B.LADDER_SIZES)
def test_ladder_holds_every_required_class(n, fb):
    lad = B.band_ladder(n, fb)
    half = n // 2
    assert lad == sorted(set(lad)) and lad[0] >= 1 and lad[-1] == half
    assert len(lad) <= B.CAP or len(lad) == B.OVER_CAP[(n, fb)]
    assert (len(lad) > B.CAP) == ((n, fb) in B.OVER_CAP)
    for b in (1, 2, 3, half - 2, half - 1, half):
        assert b in lad or not 1 <= b <= half
    # the granules, stated here once more and independently of band_ladder.granules
    gran = {8 if fb == 8 else 16, 64}
    gran.add(n // 16 if n & (n - 1) == 0 else (n // 2) // (8 if (n // 2) % 8 == 0 else 4))   # threads of a z-pass line
    gran.discard(0)
    if fb == 4 and n in (1024, 2048):
        gran.add(128)
    assert set(B.granules(n, fb)) == gran
    for g in gran:
        mult = [k * g for k in range(1, half) if k * g < half]
        for kg in mult[:2] + mult[-1:]:
            for b in (kg - 2, kg - 1, kg, kg + 1):
                assert b in lad or not 1 <= b <= half, (n, fb, g, kg, b)
    if n == 1024:
        assert set(B.PRODUCTION_1024) <= set(lad)
    if n == 2048:
        assert 496 in lad
    # a band + 1 that is exactly a whole number of 128-byte lines, and its two neighbours: what the compact pitch turns on
    m = B.line_granule(fb)
    if m < half:
        assert {m - 2, m - 1, m} <= set(lad) or m - 2 < 1


def test_ladder_sizes_reach_every_kernel_family():
    s = set(B.LADDER_SIZES)
    assert {16, 64, 256} <= s                 # the plain radix-8 plans
    assert {128, 1024} <= s                   # paired radix-16 first stage (fp64; 1024 fp32: k_strided_pk8)
    assert {2048, 512} <= s                   # k_strided16 (fp32) / four-column fp64 tiles; the invariant z-pass with reducing waves
    assert {24, 40} <= s and all(n < 96 for n in (24, 40))              # run-time mixed plans
    assert {96, 200, 768, 1000} <= s                                    # mixed plans compiled in
    assert np.all(np.array(sorted(s)) % 8 == 0)
