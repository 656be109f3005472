"""CPU-side checks of what tests/test_gpu_shells_production.py stands on: the fast shell restatements (tests/np_shells_fast.py) return
the bits of the slow ones on every kind of case the small-grid device tests use -- math.fsum is exact, so the order of the terms
cannot matter and equality of bits is asserted, not closeness --; the grouping rules restated in tests/shell_passes.py give the rows
that profiles/corr_notes.md and profiles/multipole_notes.md state, carry every sum exactly once within 64 KB for every grid up to
2048, and split no pair of the correlation's signs; and the windows and the ragged shape of tests/shell_production_cases.py are what
they are meant to be."""
import numpy as np
import pytest

import corr_cases as cc
import multipole_cases as mc
import np_corr as npc
import np_matter as npm
import np_multipoles as npl
import np_power as npp
import np_shells_fast as fast
import power_cases as pc
import shell_passes as sp
import shell_production_cases as spc

SPECTRUM_WINDOWS = lambda n: ((0, n), (0, n // 2), (n // 2, n // 2), (3, 5))
RADII = (4.0, 2.0, 1.0, 0.0)


def same_bits(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        elif isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
            assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint64), np.ascontiguousarray(b[k]).view(np.uint64)), k
        else:
            assert type(a[k]) is type(b[k]) and a[k] == b[k], k
    return True


def spectra_for(n):
    a, b = mc.random_spectra(n, 70 + n)
    a[3, 2, 1] = np.nan
    a[0, 0, n // 2] = np.inf
    b[2, 1, 0] = -np.inf
    return a, b


# ------------------------------------------------------------------------------------------------------------ 1. the fast restatement
@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("n", [16, 24])
def test_power_is_the_slow_restatement_bit_for_bit(n, fb):
    boxes = [spectra_for(n)[0], pc.random_box(5, n)] + ([s for _, s, _ in pc.cases()] if n == pc.N else [])
    for spec in boxes:
        for y0, nyl in SPECTRUM_WINDOWS(n):
            for radii in (RADII, (), tuple(np.linspace(0.0, 3.25, 14))):
                assert same_bits(fast.power(spec[y0:y0 + nyl], y0, radii, fb), npp.power(spec[y0:y0 + nyl], y0, radii, fb))


@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("n", [16, 24])
def test_matter_shells_are_the_slow_restatement_bit_for_bit(n, fb):
    a, b = spectra_for(n)
    m = pc.random_box(31, n)
    for sa, sb in ((a, b), (m, 0.7 * m + 0.5 * pc.random_box(32, n))):
        for y0, nyl in SPECTRUM_WINDOWS(n):
            for ngp, dec in spc.FLAGS:
                for lin in (sb[y0:y0 + nyl], None):
                    assert same_bits(fast.matter_shells(sa[y0:y0 + nyl], lin, y0, fb, ngp, dec), npm.shells(sa[y0:y0 + nyl], lin, y0, fb, ngp, dec))
    want = npm.shells(a, b, 0, fb)
    assert want["nonfinite_modes"] == 4 and np.count_nonzero(want["cross_neg"]) > n // 4            # (the cases are not empty ones)


@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("n", [16, 24])
def test_multipole_shells_are_the_slow_restatement_bit_for_bit(n, fb):
    a, b = spectra_for(n)
    for los in range(3):
        for y0, nyl in SPECTRUM_WINDOWS(n):
            for ngp, dec in spc.FLAGS:
                for lin in (b[y0:y0 + nyl], None):
                    assert same_bits(fast.multipole_shells(a[y0:y0 + nyl], lin, y0, fb, ngp, dec, los), npl.shells(a[y0:y0 + nyl], lin, y0, fb, ngp, dec, los))
    assert np.count_nonzero(npl.shells(a, b, 0, fb, los=1)["parts"][10]) > n // 4


@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("n", [16, 24])
def test_corr_shells_are_the_slow_restatement_bit_for_bit(n, fb):
    f = cc.random_field(n, 5 + n)
    f[3, 2, 1] = np.inf
    f[n - 1, 0, 5] = np.nan
    for los in range(3):
        for wins in cc.x_windows(n):
            for x0, nxl in wins:
                assert same_bits(fast.corr_shells(f[x0:x0 + nxl], x0, fb, los), npc.shells(f[x0:x0 + nxl], x0, fb, los))
        for g in (cc.on_los(n, los, 3), cc.across_los(n, los, n // 2), cc.one_cell(n, (0, 0, 0), -2.0), -np.ones((n, n, n))):
            assert same_bits(fast.corr_shells(g, 0, fb, los), npc.shells(g, 0, fb, los))
    assert np.count_nonzero(npc.shells(f, 0, fb, 0)["parts"][5]) > n // 4


def test_the_production_fields_through_both_restatements():
    """the generators of the production cases at a size the slow restatement can take: the same bits, and what they plant is there"""
    n = 24
    for y0, nyl in ((0, 1), (n // 2, 1), (n - 1, 1), (n // 2 - 1, 3)):
        a, b = spc.spectra(n, y0, nyl)
        for fb in (8, 4):
            assert same_bits(fast.power(a, y0, spc.RADII13, fb), npp.power(a, y0, spc.RADII13, fb))
            assert same_bits(fast.matter_shells(a, b, y0, fb, False, True), npm.shells(a, b, y0, fb, False, True))
            want = npl.shells(a, b, y0, fb, True, True, 1)
            assert same_bits(fast.multipole_shells(a, b, y0, fb, True, True, 1), want) and want["nonfinite_modes"] == 2
            f = spc.field(n, y0, nyl)
            want = npc.shells(f, y0, fb, 2)
            assert same_bits(fast.corr_shells(f, y0, fb, 2), want) and want["nonfinite_cells"] == 1
        t = npp.terms(a)
        t = t[np.isfinite(t) & (t > 0)]
        assert t.max() / t.min() > 1e30 and np.any(f > 0) and np.any(f < 0)                            # many decades, both signs


# ------------------------------------------------------------------------------------------------------------ 2. the grouping
def test_the_rows_the_notes_state():
    """profiles/corr_notes.md and profiles/multipole_notes.md: shells, sums per launch, and the LDS of the longest launch in KB"""
    kb = lambda b: round(b / 1000.0)
    assert [npp.bins(n) for n in (256, 512, 1024, 1536, 2048)] == [223, 444, 888, 1331, 1775]
    rows = {n: sp.corr(npp.bins(n)) for n in spc.GRIDS}
    assert [(sp.lengths(r["scans"]), sp.lengths(r["accs"])) for r in rows.values()] == [((6,), (4, 2)), ((6,), (2, 2, 2)), ((4, 2), (1,) * 6), ((2, 2, 2), (1,) * 6)]
    assert [(kb(rows[n]["lds_scan"]), kb(rows[n]["lds_acc"])) for n in (512, 1024, 2048)] == [(28, 50), (57, 50), (57, 50)]
    assert rows[512]["accs"] == [[0, 1, 2, 3], [4, 5]] and rows[2048]["scans"] == [[0, 1], [2, 3], [4, 5]]
    rows = {n: sp.multipoles(npp.bins(n)) for n in (256, 1024, 2048)}
    assert [(sp.lengths(r["scans"]), sp.lengths(r["accs"])) for r in rows.values()] == [((11,), (5, 6)), ((5, 6), (1, 2, 2, 2, 2, 2)), ((1, 2, 2, 2, 2, 2), (1,) * 11)]
    assert [(kb(r["lds_scan"]), kb(r["lds_acc"])) for r in rows.values()] == [(23, 37), (57, 50), (57, 50)]
    assert rows[1024]["accs"] == [[0], [1, 2], [3, 4], [5, 6], [7, 8], [9, 10]]
    assert [sp.form(sp.multipoles(npp.bins(n))) for n in spc.GRIDS] == [(1, 3), (2, 6), (3, 11), (6, 11)]
    # one sum per launch (PF_*_SCAN_EACH=1), and every small grid in one launch
    assert sp.form(sp.corr(888, each=True)) == (6, 6) and sp.form(sp.multipoles(888, each=True)) == (11, 11) and sp.form(sp.multipoles(888, 5, each=True)) == (5, 5)
    assert sp.form(sp.corr(npp.bins(64))) == (1, 1) == sp.form(sp.multipoles(npp.bins(64)))
    # the matter scan is fused up to 1890, and the column groups of the power walk
    assert [sp.matter(npp.bins(n))["fused"] for n in (16, 1024, 1536, 1890, 1892, 2048)] == [True, True, True, True, False, False]
    assert sp.lengths(sp.matter(1775)["scans"]) == (1, 1, 1) and sp.lengths(sp.matter(1775, two=False)["scans"]) == (1,) and sp.lengths(sp.matter(16, each=True)["scans"]) == (1, 1, 1)
    assert [sp.power(n, npp.bins(n))["cg"] for n in (16, 512, 514, 1024, 1026, 1536, 2048)] == [1, 1, 2, 2, 4, 4, 4]
    assert sp.power(1024, 888, 13)["batches"] == 2 and sp.power(1024, 888, 0)["batches"] == 1 == sp.power(1024, 888, 12)["batches"]


def test_every_sum_rides_once_within_the_lds_for_every_grid():
    seen = set()
    for n in range(2, 2049):
        nb = npp.bins(n)
        for each in (False, True):
            plans = [(sp.corr(nb, each), sp.CORR_SUMS), (sp.multipoles(nb, sp.MULTIPOLE_SUMS, each), sp.MULTIPOLE_SUMS),
                     (sp.multipoles(nb, sp.MULTIPOLE_SUMS_AUTO, each), sp.MULTIPOLE_SUMS_AUTO), (sp.matter(nb, True, each), 3), (sp.matter(nb, False, each), 1)]
            for p, total in plans:
                for key, per_sum, extra in (("scans", sp.TABLE, 2), ("accs", sp.ACC, 0)):
                    assert sorted(s for launch in p[key] for s in launch) == list(range(total)), (n, each, key)                  # every sum exactly once
                    assert all(launch == list(range(launch[0], launch[0] + len(launch))) for launch in p[key]), (n, each, key)      # in runs
                    assert (max(len(launch) for launch in p[key]) + extra) * per_sum * nb <= p["lds_" + key[:-1]] <= sp.LDS, (n, each, key, total)
            for key in ("scans", "accs"):                    # no pair (2k, 2k + 1) is split: a launch carries whole pairs, or, where there is room for one sum only, one
                ls = plans[0][0][key]
                assert sp.lengths(ls) == (1,) * 6 or all(launch[0] % 2 == 0 and len(launch) % 2 == 0 for launch in ls), (n, each, key)
                assert sp.lengths(ls) != (1,) * 6 or each or 2 * (sp.ACC if key == "accs" else sp.TABLE) * nb + (0 if key == "accs" else 2 * sp.TABLE * nb) > sp.LDS, (n, key)
            seen.add((sp.form(plans[0][0]), sp.form(plans[1][0]), sp.form(plans[2][0])))
        pw = sp.power(n, nb, 13)
        assert max(pw["lds_scan"], pw["lds_acc"]) <= sp.LDS
    assert len(seen) >= 8                                                                                                            # (the rule has that many shapes)


# ------------------------------------------------------------------------------------------------------------ 3. the shapes of the cases
@pytest.mark.parametrize("n", spc.GRIDS)
def test_planes_0_and_half_reach_every_shell(n):
    nb = npp.bins(n)
    assert spc.windows(n)[:2] == [(0, 1), (n // 2, 1)]
    modes = sum(np.bincount(npp.geometry(n, y0, 1)[1].ravel(), minlength=nb) for y0 in (0, n // 2))
    r2 = npp.signed(np.arange(n), n)[:, None] ** 2 + npp.signed(np.arange(n), n)[None, :] ** 2
    cells = sum(np.bincount(npp.shell_of(r2 + s * s).ravel(), minlength=nb) for s in (0, n // 2))
    assert modes.shape == cells.shape == (nb,) and np.all(modes > 0) and np.all(cells > 0)
    top = np.bincount(npp.geometry(n, n // 2, 1)[1].ravel(), minlength=nb)
    assert top[nb - 1] > 0 and npp.geometry(n, 0, 1)[1].max() == npp.shell_of(2 * (n // 2) ** 2)


def test_the_lines_of_sight_and_widths_of_the_cases():
    cases = spc.cases()
    for n in spc.GRIDS:
        mine = [c for c in cases if c[0] == n]
        assert {los for c in mine for los in c[4]} == {0, 1, 2}, n
        assert [c[1:4] for c in mine if c[3] == 4] == [(0, 1, 4)] and {c[1:3] for c in mine if c[3] == 8} == set(spc.windows(n))
        assert all(planes * n * n <= 4 << 20 for _, _, planes, _, _ in mine)
    assert len({spc.case_id(c) for c in cases}) == len(cases)
    assert (512 // 2 - 1, 3) in spc.windows(512) and (1023, 1) in spc.windows(1024) and len(spc.windows(1536)) == len(spc.windows(2048)) == 2


def test_the_ragged_shape_is_ragged():
    n = spc.RAGGED
    assert sp.rows(n * n) == (3, 6166, 1)                                # every tap without radii: a last workgroup of one row where the others have three
    assert sp.rows(n * n, sp.MAXWG_RADII) == (10, 1850, 6)               # the power tap with radii
    # and the thin windows give every workgroup one row, but the three planes of 1024 under radii two: the carried root of the power walk
    assert sp.rows(2048 * 1)[0] == 1 and sp.rows(1024 * 3, sp.MAXWG_RADII) == (2, 1536, 2)
