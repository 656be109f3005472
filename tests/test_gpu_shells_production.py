"""The four shell-sum passes of pinocchio_amd/csrc/pf_power.hip (k_power_*, k_matter_*, k_multipole_*, k_corr_*) and their launchers
at production shell counts: every case is one tap on one thin window of a grid of 512, 1024, 1536 or 2048
(tests/shell_production_cases.py), whose shell count, LDS tables, grouping of the sums, column groups and strides are those of the
full box.  What ran is held against tests/shell_passes.py: the (scans, accumulations) the taps report are the production shapes -- 1 +
(4, 2), 1 + (2, 2, 2), (4, 2) + 6 x 1, (2, 2, 2) + 6 x 1 for the correlation; 1 + 3, 2 + 6, 3 + 11, 6 + 11 for the multipoles; the
unfused matter scan at 2048; CG = 2 at 1024 and 4 above by the rule of power_device.

The assertions are those of the small-grid tests (tests/test_gpu_power.py, test_gpu_matter.py, test_gpu_multipoles.py,
test_gpu_corr.py) against the fast restatement (tests/np_shells_fast.py, the bits of the slow one: tests/test_shells_fast_cpu.py):
integer columns equal; positive sums within TOL_POWER of math.fsum by npp.rel; signed outputs within TOL_POWER times the sum of
their two parts; xi the bits of the difference of the returned parts; the variances within TOL_VARIANCE.  No tolerance is new.  The
radii stay at or below two cells: on plane n/2 the argument of the window is then at most 3 pi^2 R^2 = 118, and what TOL_VARIANCE
allows for the rounding of the argument (|x| 2^-53 per exponential, tests/test_gpu_power.py) stays below 3e-14."""
import os
import subprocess
import sys

import numpy as np
import pytest

import np_matter as npm
import np_power as npp
import np_shells_fast as fast
import shell_passes as sp
import shell_production_cases as spc
from test_gpu_power import TOL_POWER, TOL_VARIANCE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = spc.cases()
# the power tap also takes three planes of 1024 under radii: two rows per workgroup, so the root of k2 is carried from row to row
POWER_CASES = CASES + [(1024, 1024 // 2 - 1, 3, 8, ())]


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


@pytest.fixture(scope="module")
def wanted():
    """the restatements, each computed once"""
    return {}


def once(cache, key, make):
    if key not in cache:
        cache[key] = make()
    return cache[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def flags_of(case):
    return spc.FLAGS[(CASES.index(case) if case in CASES else 0) % len(spc.FLAGS)]


def within(got, want, absum):
    return bool(np.all(np.abs(got - want) <= TOL_POWER * absum))


# ------------------------------------------------------------------------------------------------------------ 1. power and variances
def check_power(got, want, radii_index, what):
    assert np.array_equal(got["nmodes"], want["nmodes"]) and np.array_equal(got["k2sum"], want["k2sum"]), what
    assert (got["modes"], got["nonfinite"]) == (want["modes"], want["nonfinite"]), what
    rp, rv = npp.rel(got["power"], want["power"]), npp.rel(got["variance"], want["variance"][radii_index])
    print(what, "power rel", rp, "of", TOL_POWER, "variance rel", rv, "of", TOL_VARIANCE)
    assert rp <= TOL_POWER and rv <= TOL_VARIANCE, (what, rp, rv)


@pytest.mark.parametrize("case", POWER_CASES, ids=spc.case_id)
def test_power_tap(api, wanted, case):
    n, y0, nyl, fb, _ = case
    nb = npp.bins(n)
    assert sp.power(n, nb)["cg"] == {512: 1, 1024: 2, 1536: 4, 2048: 4}[n]
    spec, _ = spc.spectra(n, y0, nyl)
    all_radii = spc.RADII13 if n == 1024 else spc.RADII3
    want = once(wanted, ("power",) + case[:4], lambda: fast.power(spec, y0, all_radii, fb))
    assert want["nonfinite"] == 2 and int(want["nmodes"].sum()) == nyl * n * n
    runs = [((), []), (spc.RADII3, [12, 6, 0]), (spc.RADII13, list(range(13)))] if n == 1024 and nyl == 1 else [(spc.RADII3, [12, 6, 0] if n == 1024 else [0, 1, 2])]
    for radii, index in runs:
        got = api.debug_power_spectrum(spec, y0, fb, radii)
        check_power(got, want, index, (spc.case_id(case), len(radii), "radii"))
        assert np.array_equal(got["power"] == 0, want["power"] == 0)          # untouched shells are exactly 0
        if y0 == n // 2:
            assert got["nmodes"][nb - 1] > 0 and got["power"][nb - 1] > 0     # the top shell
    if nyl == 3:
        assert sp.rows(n * nyl, sp.MAXWG_RADII)[0] == 2 or n == 512


# ------------------------------------------------------------------------------------------------------------ 2. two spectra
def check_matter(got, want, what):
    assert np.array_equal(got["nmodes"], want["nmodes"]) and np.array_equal(got["k2sum"], want["k2sum"]), what
    assert (got["modes"], got["nonfinite_modes"]) == (want["modes"], want["nonfinite_modes"]), what
    r = {k: npp.rel(got[k], want[k]) for k in ("power", "cross_pos", "cross_neg")}
    print(what, "rel", r, "of", TOL_POWER)
    assert all(v <= TOL_POWER for v in r.values()), (what, r)       # each part, not only the difference
    assert within(got["cross"], want["cross"], want["cross_pos"] + want["cross_neg"]), what


@pytest.mark.parametrize("case", CASES, ids=spc.case_id)
def test_matter_tap(api, wanted, case):
    n, y0, nyl, fb, _ = case
    nb = npp.bins(n)
    ngp, dec = flags_of(case)
    m, lin = spc.spectra(n, y0, nyl)
    want = once(wanted, ("matter",) + case[:4], lambda: fast.matter_shells(m, lin, y0, fb, ngp, dec))
    assert want["nonfinite_modes"] == 2 and min(np.count_nonzero(want[k]) for k in ("power", "cross_pos", "cross_neg")) > nb // 4
    assert "PF_MATTER_SCAN_EACH" not in os.environ
    plan = sp.matter(nb)
    assert plan["fused"] == (n < 2048)
    got = api.debug_matter_shells(m, lin, y0, fb, ngp, dec)
    assert api.matter_form()[1] == len(plan["scans"]) == (3 if n == 2048 else 1)
    # the two parts of cross, each from a run of its own on a masked second spectrum
    pos, neg = npm.cross_masks(m, lin, y0, fb, ngp, dec)
    got["cross_pos"] = api.debug_matter_shells(m, pos, y0, fb, ngp, dec)["cross"]
    got["cross_neg"] = -api.debug_matter_shells(m, neg, y0, fb, ngp, dec)["cross"]
    check_matter(got, want, (spc.case_id(case), ngp, dec))
    only = api.debug_matter_shells(m, None, y0, fb, ngp, dec)
    assert only["cross"] is None and np.array_equal(bits(only["power"]), bits(got["power"])) and api.matter_form()[1] == 1
    if y0 == n // 2:
        assert got["power"][nb - 1] > 0


# ------------------------------------------------------------------------------------------------------------ 3. multipoles
def check_multipoles(got, want, what):
    assert np.array_equal(got["nmodes"], want["nmodes"]) and np.array_equal(got["k2sum"], want["k2sum"]), what
    assert (got["modes"], got["nonfinite_modes"]) == (want["modes"], want["nonfinite_modes"]), what
    r = npp.rel(got["parts"], want["parts"])
    print(what, "parts rel", r, "of", TOL_POWER)
    assert r <= TOL_POWER, (what, r)
    P = want["parts"]
    assert within(got["power"], want["power"], np.stack([P[0], P[1] + P[2], P[3] + P[4]])), what
    if want["cross"] is not None:
        assert within(got["cross"], want["cross"], np.stack([P[5] + P[6], P[7] + P[8], P[9] + P[10]])), what
    else:
        assert got["cross"] is None and not np.any(got["parts"][5:]), what


@pytest.mark.parametrize("case", CASES, ids=spc.case_id)
def test_multipole_tap(api, wanted, case):
    n, y0, nyl, fb, lines = case
    nb = npp.bins(n)
    ngp, dec = flags_of(case)
    m, lin = spc.spectra(n, y0, nyl)
    assert "PF_MULTIPOLE_SCAN_EACH" not in os.environ
    for los in lines:
        want = once(wanted, ("multipoles",) + case[:4] + (los, 2), lambda: fast.multipole_shells(m, lin, y0, fb, ngp, dec, los))
        assert want["nonfinite_modes"] == 2 and np.count_nonzero(want["parts"][0]) > nb // 4 and np.count_nonzero(want["parts"]) > 2 * nb        # (a plane across the line of sight has mu = 0: one sign per order)
        got = api.debug_multipole_shells(m, lin, y0, fb, ngp, dec, los)
        form = api.multipole_form()
        print(spc.case_id(case), "los", los, "scans, accumulations", form)
        assert form == sp.form(sp.multipoles(nb)) == {512: (1, 3), 1024: (2, 6), 1536: (3, 11), 2048: (6, 11)}[n]
        check_multipoles(got, want, (spc.case_id(case), los, ngp, dec))
        if y0 == n // 2:
            assert got["nmodes"][nb - 1] > 0 and got["parts"][0, nb - 1] > 0                                       # the top shell
            # without a second spectrum: five sums, grouped anew
            want5 = once(wanted, ("multipoles",) + case[:4] + (los, 1), lambda: fast.multipole_shells(m, None, y0, fb, ngp, dec, los))
            got5 = api.debug_multipole_shells(m, None, y0, fb, ngp, dec, los)
            assert api.multipole_form() == sp.form(sp.multipoles(nb, sp.MULTIPOLE_SUMS_AUTO))
            check_multipoles(got5, want5, (spc.case_id(case), los, "auto alone"))
            assert np.array_equal(bits(got5["parts"][:5]), bits(got["parts"][:5]))


EACH_CHILD = """
import sys
import numpy as np
from pinocchio_amd import api
data = np.load(sys.argv[1])
out = {}
for two in (1, 0):
    got = api.debug_multipole_shells(data["m"], data["lin"] if two else None, int(data["y0"]), 8, False, True, int(data["los"]))
    for k in ("nmodes", "k2sum", "power", "parts"):
        out["%s_%d" % (k, two)] = got[k]
    out["form_%d" % two] = np.array(api.multipole_form())
np.savez(sys.argv[2], **out)
"""


@pytest.mark.parametrize("n", spc.GRIDS)
def test_the_grouping_of_the_multipole_sums_changes_no_bit(api, n, tmp_path):
    """plane n/2 with one sum per launch (PF_MULTIPOLE_SCAN_EACH=1) in a fresh child process: the passes that ran, and the bits of the
    production grouping in every column"""
    nb, y0, los = npp.bins(n), n // 2, spc.GRIDS.index(n) % 3
    m, lin = spc.spectra(n, y0, 1)
    np.savez(tmp_path / "in.npz", m=m, lin=lin, y0=y0, los=los)
    env = dict(os.environ, PF_MULTIPOLE_SCAN_EACH="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", EACH_CHILD, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=env, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    each = np.load(tmp_path / "out.npz")
    for two, total in ((1, 11), (0, 5)):
        here = api.debug_multipole_shells(m, lin if two else None, y0, 8, False, True, los)
        assert api.multipole_form() == sp.form(sp.multipoles(nb, total)) and each["form_%d" % two].tolist() == [total, total]
        assert api.multipole_form() != (total, total)
        for k in ("nmodes", "k2sum", "power", "parts"):
            assert np.array_equal(bits(here[k]), bits(each["%s_%d" % (k, two)])), (n, two, k)


# ------------------------------------------------------------------------------------------------------------ 4. separation space
def check_corr(got, want, what):
    assert np.array_equal(got["ncells"], want["ncells"]) and np.array_equal(got["r2sum"], want["r2sum"]) and got["nonfinite_cells"] == want["nonfinite_cells"] == 1, what
    rp = npp.rel(got["parts"], want["parts"])
    print(what, "positive sums against fsum", rp, "of", TOL_POWER)
    assert rp <= TOL_POWER, (what, rp)
    assert within(got["xi"], want["xi"], want["parts"][0::2] + want["parts"][1::2]), what
    assert np.array_equal(bits(got["xi"]), bits(got["parts"][0::2] - got["parts"][1::2])), what


@pytest.mark.parametrize("case", CASES, ids=spc.case_id)
def test_corr_tap(api, wanted, case, monkeypatch):
    n, x0, nxl, fb, lines = case
    nb = npp.bins(n)
    f = spc.field(n, x0, nxl)
    assert "PF_CORR_SCAN_EACH" not in os.environ
    for los in lines:
        want = once(wanted, ("corr",) + case[:4] + (los,), lambda: fast.corr_shells(f, x0, fb, los))
        assert min(np.count_nonzero(want["parts"][s]) for s in (0, 1)) > nb // 4 and np.count_nonzero(want["parts"]) > 2 * nb and int(want["ncells"].sum()) == nxl * n * n
        got = api.debug_corr_shells(f, x0, fb, los)
        passes = api.corr_passes()
        print(spc.case_id(case), "los", los, "scans, accumulations", passes)
        assert passes == sp.form(sp.corr(nb)) == {512: (1, 2), 1024: (1, 3), 1536: (2, 6), 2048: (3, 6)}[n]
        check_corr(got, want, (spc.case_id(case), los))
        if x0 == n // 2:
            assert got["ncells"][nb - 1] > 0 and np.any(got["parts"][:, nb - 1] > 0)                              # the top shell: the corner of the cube
        # one sum per launch (PF_CORR_SCAN_EACH, tests only): the grouping changes no bit
        monkeypatch.setenv("PF_CORR_SCAN_EACH", "1")
        each = api.debug_corr_shells(f, x0, fb, los)
        monkeypatch.delenv("PF_CORR_SCAN_EACH")
        assert api.corr_passes() == (6, 6)
        assert all(np.array_equal(bits(each[k]), bits(got[k])) for k in ("ncells", "r2sum", "xi", "parts")) and each["nonfinite_cells"] == 1


# ------------------------------------------------------------------------------------------------------------ 5. a ragged last workgroup
@pytest.mark.parametrize("tap", ["power", "matter", "multipoles", "corr"])
def test_rows_that_do_not_divide_among_the_workgroups(api, tap):
    """a full box of 136: 18496 rows over at most 8192 workgroups are three rows each and a last workgroup of one (under radii: ten
    each and a last one of six)"""
    n = spc.RAGGED
    assert sp.rows(n * n)[2] not in (0, sp.rows(n * n)[0]) and sp.rows(n * n, sp.MAXWG_RADII)[2] not in (0, sp.rows(n * n, sp.MAXWG_RADII)[0])
    if tap == "corr":
        f = spc.field(n, 0, n)
        for los in (0, 2):
            got = api.debug_corr_shells(f, 0, 8, los)
            assert api.corr_passes() == (1, 1)
            check_corr(got, fast.corr_shells(f, 0, 8, los), ("ragged corr", los))
        return
    m, lin = spc.spectra(n, 0, n)
    if tap == "power":
        want = fast.power(m, 0, spc.RADII3, 8)
        check_power(api.debug_power_spectrum(m, 0, 8, spc.RADII3), want, [0, 1, 2], "ragged power, radii")
        check_power(api.debug_power_spectrum(m, 0, 8, ()), want, [], "ragged power")
    elif tap == "matter":
        got = api.debug_matter_shells(m, lin, 0, 8, False, True)
        pos, neg = npm.cross_masks(m, lin, 0, 8, False, True)
        got["cross_pos"] = api.debug_matter_shells(m, pos, 0, 8, False, True)["cross"]
        got["cross_neg"] = -api.debug_matter_shells(m, neg, 0, 8, False, True)["cross"]
        check_matter(got, fast.matter_shells(m, lin, 0, 8, False, True), "ragged matter")
    else:
        got = api.debug_multipole_shells(m, lin, 0, 8, False, True, 1)
        assert api.multipole_form() == (1, 1)
        check_multipoles(got, fast.multipole_shells(m, lin, 0, 8, False, True, 1), "ragged multipoles")
