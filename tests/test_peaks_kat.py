"""The peak totals the reference logged in count_peaks (src/fragment.c:605-706), reproduced on the CPU: the oracle's Fmax of the
run + the numpy restatement of the reference's loop (tests/np_peaks.py) against tests/golden/peaks_kat.json.

The peak count depends on the ORDER of Fmax between neighbouring cells, cell by cell -- a sharper pin on the reference than the
histogram of the KAT tests.  Bound: a cell that crosses Flast adds or removes at most one peak, so |d peaks| <= |d collapsed| + order
flips between neighbours; the tests allow what the collapsed-cell check of the same run allows (5, 8, 8, 100) and print the difference.
Measured here: +1 (HMF_Validation, the one extra cell the oracle collapses), 0, 0, 0.

These tests need no device: they pin the restatement the GPU tests (tests/test_gpu_peaks.py) compare the kernel with.  The f(R) run
(two minutes of table integrations on the CPU) is left to the GPU test.
"""
import json
import os

import numpy as np
import pytest

import ic_oracle
import np_peaks
import oracle_lib

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _load(name):
    with open(os.path.join(GOLD, name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def logged():
    kat = _load("peaks_kat.json")
    assert kat["Flast"] == 1.0
    return {r["run"]: r for r in kat["runs"]}


def _box(p):
    return p["BoxSize_h100"] / p["Hubble100"]   # true Mpc


def _oracle_fmax(kat, dk, splines=None):
    p = kat["params"]
    n = p["GridSize"]
    o = oracle_lib.Oracle(n, 0)
    o.set_density(dk)
    if splines is None:
        x, y = ic_oracle.growth_table_lcdm(p["Omega0"])
        o.set_invgrow(x, y)
    else:
        for i in range(len(kat["radii_Mpc"])):
            o.set_invgrow_radius(i, *splines)
    o.compute_fmax(np.array(kat["radii_Mpc"]) / (_box(p) / n), do_lpt=False)
    return np.ascontiguousarray(o.products()["Fmax"]).reshape(n, n, n)


def _check(run, fmax, bound):
    peaks, good = np_peaks.count_peaks(fmax, 1.0)
    print(run["run"], "peaks", peaks, "logged", run["total_peaks"], "difference", peaks - run["total_peaks"])
    assert good == peaks                                   # the whole periodic box has no border and no safety layer
    assert abs(peaks - run["total_peaks"]) <= bound, (peaks, run["total_peaks"])
    return peaks


@pytest.fixture(scope="module")
def hmf_fmax():
    kat = _load("hmf_validation_kat.json")
    p = kat["params"]
    return _oracle_fmax(kat, ic_oracle.genic(p["GridSize"], _box(p), p["RandomSeed"], kat["PkNorm"], p))


def test_fixture_holds_the_log_lines(logged):
    assert len(logged) == 6 and logged["RECOMPUTE_DISPLACEMENTS_LCDM"]["total_peaks"] == logged["SCALE_DEP_LCDM"]["total_peaks"]
    for r in logged.values():
        assert "Total number of peaks: %d" % r["total_peaks"] in r["log_line"]
        if r["tasks"] == 1:
            assert r["task0_peaks"] == r["task0_well_resolved"] == r["total_peaks"]


def test_hmf_validation_peaks(logged, hmf_fmax):
    _check(logged["HMF_Validation"], hmf_fmax, 5)          # measured: 114 994 against 114 993 (collapsed: 1 230 387 against 1 230 386)


def test_example_log_peaks(logged):
    kat = _load("example_kat.json")
    p = kat["params"]
    fmax = _oracle_fmax(kat, ic_oracle.genic(p["GridSize"], _box(p), p["RandomSeed"], kat["PkNorm"], p))
    _check(logged["example"], fmax, 8)                     # measured: 107 684, as logged (four tasks: the sum of their well resolved counts)


def test_lcdm_256_peaks(logged):
    kat = _load("hmf256_kat.json")
    p = kat["params"]
    fmax = _oracle_fmax(kat, ic_oracle.genic(p["GridSize"], _box(p), p["RandomSeed"], kat["PkNorm"], p, fixed=bool(p["FixedIC"])))
    _check(logged["RECOMPUTE_DISPLACEMENTS_LCDM"], fmax, 8)  # measured: 967 337, as logged
    _check(logged["SCALE_DEP_LCDM"], fmax, 8)


def test_read_pk_table_256_peaks(logged):
    kat = _load("readpk256_kat.json")
    p = kat["params"]
    t = np.array(kat["camb_z0_k_hMpc_P"])
    pk_table = (np.log10(t[:, 0] * p["Hubble100"]), np.log10(t[:, 0] ** 3 * t[:, 1]))
    g = np.array(kat["scaledep_a_D1"])
    dk = ic_oracle.genic(p["GridSize"], _box(p), p["RandomSeed"], 1.0, p, fixed=True, pk_table=pk_table)
    fmax = _oracle_fmax(kat, dk, splines=(np.log10(g[:, 1]), np.log10(g[:, 0])))
    _check(logged["READ_PK_TABLE_and_SCALE_DEP"], fmax, 100)  # measured: 986 905, as logged


def tiling(n, parts, boundary):
    """the reference's sub-boxes: the box cut into parts[d] pieces per direction, each with a boundary layer of `boundary` cells
    on both sides of a direction that is cut (safe = boundary); a direction that is not cut spans the box and is periodic"""
    regions = []
    for ix in range(parts[0]):
        for iy in range(parts[1]):
            for iz in range(parts[2]):
                start, length, safe = [], [], []
                for d, i in enumerate((ix, iy, iz)):
                    if parts[d] == 1:
                        start.append(0); length.append(n); safe.append(0)
                    else:
                        core = n // parts[d]
                        start.append((i * core - boundary) % n); length.append(core + 2 * boundary); safe.append(boundary)
                regions.append((start, length, safe))
    return regions


@pytest.mark.parametrize("parts", [(2, 2, 1), (2, 2, 2)])
@pytest.mark.parametrize("boundary", [1, 2, 3])
def test_well_resolved_peaks_of_a_tiling_add_up_to_the_box(hmf_fmax, parts, boundary):
    """what the four-task example log shows: the total is the sum of the tasks' well resolved counts"""
    n = hmf_fmax.shape[0]
    whole, _ = np_peaks.count_peaks(hmf_fmax, 1.0)
    got = [np_peaks.count_peaks(hmf_fmax, 1.0, rg) for rg in tiling(n, parts, boundary)]
    assert sum(g[1] for g in got) == whole
    # (a boundary of one cell is the border layer itself, which is never examined: all peaks of such a sub-box are well resolved)
    assert all(g[0] >= g[1] for g in got) and (sum(g[0] for g in got) > whole) == (boundary > 1)


def test_restatement_on_hand_made_fields():
    f = np.zeros((4, 4, 4), dtype=np.float32)
    f[1, 2, 3] = 2.0
    assert np_peaks.count_peaks(f, 1.0) == (1, 1)
    assert np_peaks.count_peaks(f, 0.0) == (1, 1)          # every cell stored: the zeros are equal to their neighbours, no peaks
    f[1, 2, 0] = 2.0                                       # a stored neighbour across the periodic edge, equal: both are no peak
    assert np_peaks.count_peaks(f, 1.0) == (0, 0)
    f[1, 2, 0] = np.nan                                    # NaN is not stored and vetoes nothing
    assert np_peaks.count_peaks(f, 1.0) == (1, 1)
    # a sub-box that is not periodic in z: the cell at its border is skipped
    assert np_peaks.count_peaks(f, 1.0, ((0, 0, 3), (4, 4, 3), (0, 0, 0))) == (0, 0)
    assert np_peaks.count_peaks(f, 1.0, ((0, 0, 2), (4, 4, 3), (0, 0, 1))) == (1, 1)
    assert np_peaks.count_peaks(f, 1.0, ((0, 0, 1), (4, 4, 4), (0, 0, 1))) == (1, 1)   # periodic again; local z = 2
    assert np_peaks.count_peaks(f, 1.0, ((0, 0, 0), (4, 4, 4), (0, 0, 1))) == (1, 0)   # local z = 3 lies in the safety layer
