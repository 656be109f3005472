"""count_peaks on the device (pf_count_peaks, pf_select_peaks, pf_debug_peaks; csrc/pf_peaks.hip) against the numpy restatement
of the reference's loop (tests/np_peaks.py, pinned on the CPU by tests/test_peaks_kat.py).  Counts are integers: every
comparison with the restatement is exact.  The last part repeats the reference's five logged totals on the device."""
import json
import os

import numpy as np
import pytest

import ic_oracle
import np_peaks
from pinocchio_amd import synth
from test_gpu_multirank import run_ranks

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
RADII = np.array([2.0, 1.0, 0.5, 0.0])
FLASTS = (0.0, 0.5, 1.0, 1.3, 3.0)


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


def _swept(api, n, seed=5, **kw):
    f = api.Fmax(n, **kw)
    f.set_density(synth.make_density(n, seed=seed))
    f.set_invgrow(*synth.invgrow_table("lcdm"))
    f.sweep(RADII)
    return f


def random_regions(n, count, seed):
    """seeded regions: wrapping starts, len == n in none, one, two or three directions, safe 0..3, one and two cells thick ones"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        start = [int(v) for v in rng.integers(-n, 2 * n, 3)]
        length, safe = [], []
        full = [int(d) for d in rng.permutation(3)[:k % 4]]  # 0, 1, 2, 3 periodic directions in turn
        thin = int(rng.integers(0, 3)) if k % 5 == 2 else -1
        for d in range(3):
            if d in full:
                L = n
            elif d == thin:
                L = int(rng.integers(1, 3))                 # one or two cells thick: nothing is examined
            else:
                L = int(rng.integers(3, n + 1))
            length.append(L)
            safe.append(int(rng.integers(0, min(3, L // 2) + 1)))
        out.append((start, length, safe))
    return out


# 16: power-of-two passes, 24: mixed radix, 36: the general (chirp-z) path, 200: mixed radix with a last column of partial rows
@pytest.mark.parametrize("n", [16, 24, 36, 128, 200])
def test_count_peaks_equals_the_restatement(api, n):
    with _swept(api, n) as f:
        fmax = f.block("FMAX").reshape(n, n, n)
        assert (fmax >= 1.0).sum() > n ** 3 // 50
        for flast in FLASTS:
            want = np_peaks.count_peaks(fmax, flast)
            got = f.count_peaks(flast)
            print(n, flast, got, want)
            assert got == want
        assert f.count_peaks(1.0)[0] > 0
        # region form
        for rg in random_regions(n, 20, seed=n):
            assert f.count_peaks(1.0, rg) == np_peaks.count_peaks(fmax, 1.0, rg), rg
        # the reference's own sub-boxes: the well resolved peaks of a tiling add up to the box
        whole = f.count_peaks(1.0)[0]
        core = n // 2
        tiles = [((ix * core - 2, iy * core - 2, 0), (core + 4, core + 4, n), (2, 2, 0)) for ix in range(2) for iy in range(2)]
        assert sum(f.count_peaks(1.0, rg)[1] for rg in tiles) == whole


@pytest.mark.parametrize("n", [16, 64])
def test_count_peaks_with_fp32_fields(api, n):
    with _swept(api, n, field_bytes=4) as f:
        fmax = f.block("FMAX").reshape(n, n, n)
        for flast in FLASTS:
            assert f.count_peaks(flast) == np_peaks.count_peaks(fmax, flast)


@pytest.mark.parametrize("n", [16, 64])
def test_count_peaks_with_double_products(api, n):
    """a -DDOUBLE_PRECISION_PRODUCTS context: the count compares the fp64 column (pf_select_peaks, fp32 by definition, refuses)"""
    with _swept(api, n, double_products=True) as f:
        fmax = np.ascontiguousarray(f.products()["Fmax"])
        assert fmax.dtype == np.float64
        for flast in FLASTS:
            assert f.count_peaks(flast) == np_peaks.count_peaks(fmax, flast)
        for rg in random_regions(n, 10, seed=3):
            assert f.count_peaks(1.0, rg) == np_peaks.count_peaks(fmax, 1.0, rg), rg
        with pytest.raises(api.PinfmaxError, match="pf_select_peaks: fp32 Fmax only"):
            f.select_peaks(1.0)


def test_errors_in_the_house_format(api, capfd):
    n = 16
    with api.Fmax(n) as f:
        with pytest.raises(api.PinfmaxError, match="pf_count_peaks: products not computed"):
            f.count_peaks(1.0)
        with pytest.raises(api.PinfmaxError, match="pf_select_peaks: products not computed"):
            f.select_peaks(1.0)
        f.set_density(synth.make_density(n, seed=5))
        f.set_invgrow(*synth.invgrow_table("lcdm"))
        f.sweep(RADII)
        for bad, text in ((((0, 0, 0), (n, n + 1, n), (0, 0, 0)), r"len\[1\] = 17 outside \[1, 16\]"),
                          (((0, 0, 0), (0, n, n), (0, 0, 0)), r"len\[0\] = 0 outside \[1, 16\]"),
                          (((0, 0, 0), (n, n, 5), (0, 0, 3)), r"safe\[2\] = 3, 2 \* safe > len\[2\] = 5")):
            with pytest.raises(api.PinfmaxError, match="pf_count_peaks: region does not fit the box: " + text):
                f.count_peaks(1.0, bad)
        assert f.count_peaks(1.0, ((0, 0, 0), (n, n, 6), (0, 0, 3)))[1] == 0     # 2 * safe == len: allowed, nothing is well resolved
    assert "ERROR on task 0: pf_count_peaks: region does not fit the box" in capfd.readouterr().out
    with pytest.raises(api.PinfmaxError, match="pf_debug_peaks: region does not fit the box"):
        api.debug_peaks(np.zeros((4, 4, 4), dtype=np.float32), 1.0, ((0, 0, 0), (5, 4, 4), (0, 0, 0)))


def _constructed_fields():
    rng = np.random.default_rng(11)
    n = 12
    base = rng.random((n, n, n)).astype(np.float32) * 3.0
    out = {}
    f = base.copy(); f[3, 4, 5] = f[3, 4, 6] = 9.0; f[0, 0, 0] = f[n - 1, 0, 0] = 8.0; f[2, 0, 7] = f[2, n - 1, 7] = 8.5
    out["equal neighbours, across the periodic edges too"] = f
    f = base.copy(); f[4:8, 4:8, 4:8] = 7.0
    out["a plateau"] = f
    f = base.copy(); f[rng.random((n, n, n)) < 0.1] = np.nan
    out["NaN cells and NaN neighbours"] = f
    f = base.copy(); f[1, 1, 1] = np.inf; f[5, 5, 5] = f[5, 5, 6] = np.inf; f[8, 8, 8] = -np.inf; f[9, 1, 1] = np.inf; f[9, 1, 2] = np.nan
    out["infinities"] = f
    i, j, k = np.indices((n, n, n))
    out["a checkerboard: a peak on every other cell"] = np.where((i + j + k) % 2 == 0, 2.0, 1.5).astype(np.float32)
    out["all cells below flast"] = (base * 0.1).astype(np.float32)
    out["a constant field"] = np.full((n, n, n), 2.0, dtype=np.float32)
    # sizes whose rows are not a multiple of four cells take the one-cell-per-lane form of the kernel
    out["n = 10"] = rng.random((10, 10, 10)).astype(np.float32) * 3.0
    out["n = 6"] = rng.random((6, 6, 6)).astype(np.float32) * 3.0
    out["n = 4"] = rng.random((4, 4, 4)).astype(np.float32) * 3.0
    out["n = 72, rows longer than a wavefront's 256 cells are not needed to wrap inside one"] = rng.random((72, 72, 72)).astype(np.float32) * 3.0
    return out


@pytest.mark.parametrize("name", sorted(_constructed_fields()))
def test_debug_peaks_on_constructed_fields(api, name):
    f = _constructed_fields()[name]
    n = f.shape[0]
    for flast in (1.0, 0.0, 1.75, -np.inf, np.inf, 2.0):
        assert api.debug_peaks(f, flast) == np_peaks.count_peaks(f, flast), (name, flast)
    for rg in random_regions(n, 12, seed=n + len(name)):
        assert api.debug_peaks(f, 1.0, rg) == np_peaks.count_peaks(f, 1.0, rg), (name, rg)
    if name.startswith("a checkerboard"):
        assert api.debug_peaks(f, 1.0) == (n ** 3 // 2, n ** 3 // 2)
        assert api.debug_peaks(f, 1.75) == (n ** 3 // 2, n ** 3 // 2)      # the low cells are not stored: no change
    if name.startswith(("all cells below", "a constant")):
        assert api.debug_peaks(f, 1.0) == (0, 0)


def test_flast_is_compared_as_a_double(api):
    """outputs.Flast is a double: a cell of 1.0f is stored for flast = 1 and not for the next double above 1"""
    f = np.zeros((8, 8, 8), dtype=np.float32)
    f[2, 2, 2] = 1.0
    f[5, 5, 5] = np.nextafter(np.float32(1.0), np.float32(2.0))
    assert api.debug_peaks(f, 1.0) == (2, 2)
    assert api.debug_peaks(f, float(np.nextafter(1.0, 2.0))) == (1, 1) == np_peaks.count_peaks(f, float(np.nextafter(1.0, 2.0)))
    assert api.debug_peaks(f, float(np.nextafter(np.float64(f[5, 5, 5]), 2.0))) == (0, 0)


@pytest.mark.parametrize("n", [24, 64, 128])
def test_select_peaks(api, n):
    with _swept(api, n) as f:
        fmax = f.block("FMAX").reshape(n, n, n)
        for flast in (1.0, 0.5, 3.0):
            idx, val = f.select_peaks(flast)
            widx, wval = np_peaks.sorted_peaks(fmax, flast)
            assert len(idx) == f.count_peaks(flast)[0] == len(widx)
            assert np.array_equal(idx, widx) and np.array_equal(val, wval)
            # ... which is the sorted selection filtered by the peak mask
            sidx, sval = f.select_sorted(flast)
            keep = np_peaks.peak_mask(fmax, flast).ravel()[sidx]
            assert np.array_equal(idx, sidx[keep]) and np.array_equal(val, sval[keep])
        idx, val = f.select_peaks(1e9)
        assert len(idx) == 0 and len(val) == 0


@pytest.mark.parametrize("n,P", [(64, 2), (64, 4), (64, 8), (16, 16), (96, 3)])
def test_slabs_equal_the_single_rank(api, n, P):
    """slabs on one GPU through the in-process fabric: the planes next to a slab come from the neighbouring ranks (with
    n / P == 1 both of them); summed counts, concatenated lists and region counts equal the single-rank result"""
    dk = synth.make_density(n, seed=17 + P)
    x, y = synth.invgrow_table("lcdm")
    nxl = n // P
    regions = random_regions(n, 6, seed=P)
    with api.Fmax(n) as f1:
        f1.set_density(dk); f1.set_invgrow(x, y); f1.sweep(RADII)
        fmax = f1.block("FMAX").reshape(n, n, n)
        want = [f1.count_peaks(fl) for fl in (1.0, 0.5)]
        want_rg = [f1.count_peaks(1.0, rg) for rg in regions]
        widx, wval = f1.select_peaks(1.0)
    assert want[0] == np_peaks.count_peaks(fmax, 1.0) and want[0][0] > 0

    def body(f, r):
        f.set_density(dk[r * nxl:(r + 1) * nxl]); f.set_invgrow(x, y); f.sweep(RADII)
        return f.block("FMAX"), [f.count_peaks(fl) for fl in (1.0, 0.5)], [f.count_peaks(1.0, rg) for rg in regions], f.select_peaks(1.0)

    res = run_ranks(api, n, P, body)
    assert np.array_equal(np.concatenate([r[0] for r in res]).reshape(n, n, n), fmax)
    for r in range(P):
        assert res[r][1] == want and res[r][2] == want_rg, r                        # all-reduced: the same on every rank
        idx, val = res[r][3]
        assert np.all(val[:-1] >= val[1:])
    # concatenated lists (local index + slab offset): the same set, each slab's part in the global order
    gidx = np.concatenate([res[r][3][0].astype(np.int64) + r * nxl * n * n for r in range(P)])
    gval = np.concatenate([res[r][3][1] for r in range(P)])
    order = np.lexsort((gidx, -gval.astype(np.float64)))
    assert np.array_equal(gidx[order], widx) and np.array_equal(gval[order], wval)
    for r in range(P):
        mine = (widx >= r * nxl * n * n) & (widx < (r + 1) * nxl * n * n)
        assert np.array_equal(res[r][3][0].astype(np.int64) + r * nxl * n * n, widx[mine])


# ------------------------------------------------------------------------------------------------------------------------
# The reference's logs on the device: the five committed runs, set up as the test_hip_path_reproduces_* / test_hmf_validation_run_on_gpu
# tests of the same runs do; count_peaks(1.0) against the logged "Total number of peaks" within the bound of the collapsed-cell
# check of the same run (tests/test_peaks_kat.py has the derivation).
# Measured on the device: HMF_Validation 114 994 (logged 114 993: the one extra cell that collapses), example 107 684, LCDM 256^3
# 967 337, READ_PK 986 905, f(R) 931 084 -- the last four as logged.
def _kat(name):
    with open(os.path.join(GOLD, name)) as fh:
        return json.load(fh)


def _logged(run):
    return [r for r in _kat("peaks_kat.json")["runs"] if r["run"] == run][0]["total_peaks"]


def _box(p):
    return p["BoxSize_h100"] / p["Hubble100"]


def _report(run, f, bound):
    got = f.count_peaks(1.0)
    want = _logged(run)
    print(run, "device peaks", got[0], "logged", want, "difference", got[0] - want)
    assert got[0] == got[1]
    assert abs(got[0] - want) <= bound, (got, want)


def test_device_reproduces_the_logged_peaks_of_hmf_validation(api):
    kat = _kat("hmf_validation_kat.json")
    p = kat["params"]
    n = p["GridSize"]
    with api.Fmax(n) as f:
        f.set_density(ic_oracle.genic(n, _box(p), p["RandomSeed"], kat["PkNorm"], p))
        f.set_invgrow(*ic_oracle.growth_table_lcdm(p["Omega0"]))
        f.sweep(np.array(kat["radii_Mpc"]) / (_box(p) / n))
        _report("HMF_Validation", f, 5)


def test_device_reproduces_the_logged_peaks_of_the_example(api):
    kat = _kat("example_kat.json")
    p = kat["params"]
    n = p["GridSize"]
    with api.Fmax(n) as f:
        f.genic_density(p["RandomSeed"], _box(p), p["Omega0"], p["OmegaBaryon"], p["Hubble100"], p["PrimordialIndex"], pknorm=kat["PkNorm"])
        f.set_invgrow(*ic_oracle.growth_table_lcdm(p["Omega0"]))
        f.sweep(np.array(kat["radii_Mpc"]) / (_box(p) / n))
        _report("example", f, 8)
        # four tasks: the logged total is the sum of the tasks' well resolved peaks
        core = n // 2
        tiles = [((ix * core - 3, iy * core - 3, 0), (core + 6, core + 6, n), (3, 3, 0)) for ix in range(2) for iy in range(2)]
        assert sum(f.count_peaks(1.0, rg)[1] for rg in tiles) == f.count_peaks(1.0)[0]


def test_device_reproduces_the_logged_peaks_of_the_lcdm_256_runs(api):
    kat = _kat("hmf256_kat.json")
    p = kat["params"]
    n = p["GridSize"]
    with api.Fmax(n) as f:
        f.genic_density(p["RandomSeed"], _box(p), p["Omega0"], p["OmegaBaryon"], p["Hubble100"], p["PrimordialIndex"], pknorm=kat["PkNorm"], fixed=True)
        f.set_invgrow(*ic_oracle.growth_table_lcdm(p["Omega0"]))
        f.sweep(np.array(kat["radii_Mpc"]) / (_box(p) / n))
        _report("RECOMPUTE_DISPLACEMENTS_LCDM", f, 8)
        _report("SCALE_DEP_LCDM", f, 8)


def test_device_reproduces_the_logged_peaks_of_the_read_pk_table_run(api):
    kat = _kat("readpk256_kat.json")
    p = kat["params"]
    n = p["GridSize"]
    t = np.array(kat["camb_z0_k_hMpc_P"])
    g = np.array(kat["scaledep_a_D1"])
    with api.Fmax(n) as f:
        f.genic_density(p["RandomSeed"], _box(p), p["Omega0"], p["OmegaBaryon"], p["Hubble100"], p["PrimordialIndex"], pknorm=1.0, fixed=True,
                        pk_table=(np.log10(t[:, 0] * p["Hubble100"]), np.log10(t[:, 0] ** 3 * t[:, 1])))
        for i in range(len(kat["radii_Mpc"])):
            f.set_invgrow(np.log10(g[:, 1]), np.log10(g[:, 0]), ismooth=i)
        f.sweep(np.array(kat["radii_Mpc"]) / (_box(p) / n))
        _report("READ_PK_TABLE_and_SCALE_DEP", f, 100)


def test_device_reproduces_the_logged_peaks_of_the_f_of_R_run(api):
    mg = _kat("mg256_kat.json")
    p = mg["params"]
    n = p["GridSize"]
    a0, d0 = mg["growth_first_rows_a_D1"][0]
    radii = np.array(mg["radii_Mpc"])
    size = radii.copy()
    size[-1] = size[-2]
    with api.Fmax(n) as f:
        f.genic_density(p["RandomSeed"], _box(p), p["Omega0"], p["OmegaBaryon"], p["Hubble100"], p["PrimordialIndex"], pknorm=mg["PkNorm"], fixed=True)
        f.set_invgrow(*ic_oracle.growth_table_lcdm(p["Omega0"]))
        f.set_collapse_model(1, cosmo=(p["Omega0"], p["OmegaLambda"], 0.0, 0.0), d_in=np.full(len(radii), d0 * (1e-5 / a0) ** mg["dlnD_dlna_first_row"]))
        f.set_modified_gravity(p["FR0"], 100.0 / 299792.458, size=size)
        f.set_tabulated_ct(np.array(mg["variance"]))
        f.sweep(radii / (_box(p) / n))
        _report("MOD_GRAV_and_SCALE_DEP", f, 40)
