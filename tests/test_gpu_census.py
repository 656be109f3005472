"""The arithmetic of the solve as a run-time setting, and the census of a sweep under both flavours, on the device.

The census kernels (pinocchio_amd/csrc/pf_census.hip) are pinned by the tap on planted columns against the numpy restatement
(tests/np_census.py): every field and every record equal.  The full path is held against two independent contexts created under
PF_EXACT_LIBM=0 / 1 whose products are compared on the host with the same restatement; the setting against contexts created under
the matching environment value, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import census_cases as cc
import np_census as npc
from pinocchio_amd import synth

pytestmark = pytest.mark.gpu

RADII3 = np.array([2.0, 1.0, 0.0])
RADII4 = np.array([3.0, 1.5, 0.75, 0.0])


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


def _ctx(api, n, dk, monkeypatch, env=None, **kw):
    """a context with the density and the tables set, created with PF_EXACT_LIBM = env (None: unset)"""
    if env is None:
        monkeypatch.delenv("PF_EXACT_LIBM", raising=False)
    else:
        monkeypatch.setenv("PF_EXACT_LIBM", env)
    f = api.Fmax(n, **kw)
    monkeypatch.delenv("PF_EXACT_LIBM", raising=False)
    f.set_density(dk)
    f.set_invgrow(*synth.invgrow_table("lcdm"))
    f.set_growth(synth.growth_multipliers())
    return f


def _same_products(a, b):
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------- the kernels, through the tap ----
def _tap_twice(api, f, e, rf, re, first, cap):
    a = api.debug_census(f, rf, e, re, first_cell=first, capacity=cap)
    b = api.debug_census(f, rf, e, re, first_cell=first, capacity=cap)
    assert npc.same(a[0], b[0]) is None and npc.same_records(a[1], b[1]), "two calls differ"
    return a


PLANTED = [(np.dtype(T).name, c[0]) for T in cc.DTYPES for c in cc.cases(T)]


@pytest.mark.parametrize("tname,name", PLANTED)
def test_tap_on_the_planted_columns(api, tname, name):
    _, f, e, rf, re, first = next(c for c in cc.cases(np.dtype(tname).type) if c[0] == name)
    want, wrec = npc.census(f, e, rf, re, first)
    got, rec = _tap_twice(api, f, e, rf, re, first, len(f))
    print(name, tname, {k: got[k] for k in npc.COUNTS}, got["max_abs"], got["max_ulps"], got["max_abs_cell"])
    assert npc.same(got, want) is None, npc.same(got, want)
    assert npc.same_records(rec, wrec)
    npc.invariants(got)
    for cap in sorted({0, want["outliers"] // 2, want["outliers"] + 3}):
        got, rec = _tap_twice(api, f, e, rf, re, first, cap)
        assert npc.same(got, want) is None and npc.same_records(rec, wrec[:cap]), cap


@pytest.mark.parametrize("tname", ["float32", "float64"])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 256, 257, 4099, 2 ** 20 + 3])
def test_tap_at_counts_around_the_wave_the_workgroup_and_the_tile(api, tname, count):
    f, e, rf, re = cc.for_count(np.dtype(tname).type, count)
    first = 2 ** 33 + 1 if count == 4099 else 0
    want, wrec = npc.census(f, e, rf, re, first)
    assert want["outliers"] > 0 or count == 1
    got, rec = _tap_twice(api, f, e, rf, re, first, count)
    assert npc.same(got, want) is None, npc.same(got, want)
    assert npc.same_records(rec, wrec)
    npc.invariants(got)
    cap = want["outliers"] // 3
    got, rec = _tap_twice(api, f, e, rf, re, first, cap)
    assert npc.same(got, want) is None and npc.same_records(rec, wrec[:cap])


def test_tap_of_no_cells(api):
    z = np.zeros(0, np.float32)
    got, rec = api.debug_census(z, np.zeros(0, np.int32), z, np.zeros(0, np.int32))
    assert got["cells"] == 0 and got["outliers"] == 0 and not got["hist"].any() and got["max_abs_cell"] == npc.NOCELL and len(rec) == 0


# --------------------------------------------------------------------------------------------------------------- the setting ----
@pytest.mark.parametrize("n", [32, 24])
def test_set_arithmetic_round_trip_equals_contexts_of_the_environment(api, n, monkeypatch):
    dk = synth.make_density(n, seed=synth.SEED + n)
    hess = np.random.default_rng(n).standard_normal((4096, 6)) * np.array([1.0, 1.0, 1.0, 0.4, 0.4, 0.4])
    want = {}
    for env, name in (("1", "exact"), ("0", "fast")):
        with _ctx(api, n, dk, monkeypatch, env) as f:
            assert f.arithmetic == name
            tv = f.sweep(RADII3)
            want[name] = (tv, f.products(), f.collapse_cells(hess), f.L.pf_invgrow_table_status(f.h, -1, None))
    assert not _same_products(want["exact"][1], want["fast"][1]) or not np.array_equal(want["exact"][2], want["fast"][2]), "the flavours cannot be told apart here"
    with _ctx(api, n, dk, monkeypatch, None) as a:
        assert a.arithmetic == "fast"
        for name in ("exact", "fast", "exact", "fast"):
            a.set_arithmetic(name)
            assert a.arithmetic == name
            tv = a.sweep(RADII3)
            assert np.array_equal(tv, want[name][0]), name
            assert _same_products(a.products(), want[name][1]), name
            assert a.collapse_cells(hess).tobytes() == want[name][2].tobytes(), name
            assert a.L.pf_invgrow_table_status(a.h, -1, None) == want[name][3], name
        with pytest.raises(ValueError):
            a.set_arithmetic("quick")
        assert a.L.pf_set_arithmetic(a.h, 2) != 0 and b"pf_set_arithmetic: flavour 2" in a.L.pf_last_error() and a.arithmetic == "fast"
    assert want["fast"][3] == 1 and want["exact"][3] == 0


def test_a_table_built_on_the_device_follows_the_setting_and_a_loaded_one_stays(api, monkeypatch):
    n = 32
    dk = synth.make_density(n, seed=5)
    var = 1.7
    tabs, fm = {}, {}
    for env, name in (("1", "exact"), ("0", "fast")):
        with _ctx(api, n, dk, monkeypatch, env) as f:
            tabs[name] = f.ct_build(0, var)
            f.compute_second_derivatives(1.0)
            f.compute_collapse_times(0)
            fm[name] = f.products()["Fmax"].copy()
    with _ctx(api, n, dk, monkeypatch, None) as a:
        assert a.ct_build(0, var).tobytes() == tabs["fast"].tobytes()
        a.compute_second_derivatives(1.0)
        a.set_arithmetic("exact")       # the fast table in place is no longer this context's
        a.compute_collapse_times(0)     # ... so the pass rebuilds it
        assert a.products()["Fmax"].tobytes() == fm["exact"].tobytes()
        assert a.ct_build(0, var).tobytes() == tabs["exact"].tobytes()
        a.ct_load(0, var, tabs["fast"])  # data: stays through a change of the setting
        a.set_arithmetic("fast")
        a.set_arithmetic("exact")
        a.compute_collapse_times(0)
        with _ctx(api, n, dk, monkeypatch, "1") as b:
            b.ct_load(0, var, tabs["fast"])
            b.compute_second_derivatives(1.0)
            b.compute_collapse_times(0)
            assert a.products()["Fmax"].tobytes() == b.products()["Fmax"].tobytes()


# ------------------------------------------------------------------------------------------------------------- the full path ----
FULL = {   # name: (n, field_bytes, double_products, radii, differing bits demanded)
    "n64_fp64_4radii": (64, 8, False, RADII4 * 2.0, False),
    "n64_fp32": (64, 4, False, RADII3 * 2.0, False),
    "n24": (24, 8, False, RADII3, False),
    "n36_chirpz": (36, 8, False, RADII3, False),
    "n32_double_products": (32, 8, True, RADII3, True),
    "n128_ladder5": (128, 8, False, None, False),
}


@pytest.mark.parametrize("name", list(FULL))
def test_full_path_census_equals_two_contexts_compared_on_the_host(api, name, monkeypatch):
    n, fb, dp, radii, must_differ = FULL[name]
    if radii is None:    # the input of test_gpu_parity.py::test_full_path_exact_libm_outliers_are_bit_explained
        radii = synth.radii_ladder(5) * (n / 128.0)
        radii[-1] = 0.0
    dk = synth.make_density(n, seed=synth.SEED)
    prod = {}
    for env, flav in (("0", "fast"), ("1", "exact")):
        with _ctx(api, n, dk, monkeypatch, env, field_bytes=fb, double_products=dp) as f:
            tv = f.sweep(radii)
            prod[flav] = (tv, f.products())
    col = lambda flav, k: np.ascontiguousarray(prod[flav][1][k]).reshape(-1)
    want, wrec = npc.census(col("fast", "Fmax"), col("exact", "Fmax"), col("fast", "Rmax"), col("exact", "Rmax"))
    with _ctx(api, n, dk, monkeypatch, None, field_bytes=fb, double_products=dp) as f:
        if name == "n36_chirpz":
            assert f.L.pf_transform_path(f.h) == 2
        tv, got, rec = f.flavour_census(radii, capacity=n ** 3)
        p = f.products()
        assert f.arithmetic == "fast"
    print(name, {k: got[k] for k in npc.COUNTS}, "max_abs %.3e max_ulps %.3e cell %d" % (got["max_abs"], got["max_ulps"], got["max_abs_cell"]),
          "bins", {int(k): int(got["hist"][k]) for k in np.flatnonzero(got["hist"])})
    assert npc.same(got, want) is None, npc.same(got, want)
    assert npc.same_records(rec, wrec)
    npc.invariants(got)
    assert got["cells"] == n ** 3 and np.array_equal(tv, prod["fast"][0]) and _same_products(p, prod["fast"][1])
    if must_differ:    # double products keep what float products round away: the census is not one of zeros here
        assert got["differing_bits"] > 0


# ------------------------------------------------------------------------------------------------------ the state afterwards ----
@pytest.mark.parametrize("flavour", ["fast", "exact"])
@pytest.mark.parametrize("sources", [1, 0])
def test_the_context_is_left_as_a_plain_sweep_leaves_it(api, flavour, sources, monkeypatch):
    n = 32
    dk = synth.make_density(n, seed=21)
    with _ctx(api, n, dk, monkeypatch, "1" if flavour == "exact" else "0") as fresh:
        tv0 = fresh.compute_fmax(RADII4, do_lpt=True)
        p0, pdf0, bytes0 = fresh.products(), fresh.Fmax_PDF(), fresh.device_bytes
    with _ctx(api, n, dk, monkeypatch, None) as f:
        f.set_arithmetic(flavour)
        assert f.L.pf_set_sources_in_sweep(f.h, sources) == 0
        before = f.device_bytes
        tv, cen, rec = f.flavour_census(RADII4, capacity=16)
        assert f.device_bytes == before and f.arithmetic == flavour
        assert f.L.pf_set_sources_in_sweep(f.h, 0) == 0
        assert np.array_equal(tv, tv0)
        assert np.array_equal(f.Fmax_PDF(), pdf0)
        f.compute_displacements(1, 0)
        assert _same_products(f.products(), p0)
        assert f.device_bytes == bytes0
        assert np.array_equal(f.Fmax_PDF(), pdf0)
        npc.invariants(cen)
        # ... and fast / exact mean the flavours, whichever ran last: the census does not depend on the context's own flavour
        with _ctx(api, n, dk, monkeypatch, None) as g:
            g.set_arithmetic("exact" if flavour == "fast" else "fast")
            _, cen2, rec2 = g.flavour_census(RADII4, capacity=16)
        assert npc.same(cen, cen2) is None and npc.same_records(rec, rec2)


# ----------------------------------------------------------------------------------------------------------------- two ranks ----
def test_two_ranks_sum_to_the_one_rank_census(api, monkeypatch):
    from test_gpu_multirank import run_ranks
    monkeypatch.delenv("PF_EXACT_LIBM", raising=False)
    n, P = 32, 2
    nxl = n // P
    dk = synth.make_density(n, seed=19)
    x, y = synth.invgrow_table("lcdm")
    g = synth.growth_multipliers()
    radii = RADII4
    # double products: the census has something to count at this size
    with api.Fmax(n, double_products=True) as f1:
        f1.set_density(dk)
        f1.set_invgrow(x, y)
        f1.set_growth(g)
        tv1, cen1, rec1 = f1.flavour_census(radii, capacity=n ** 3)

    class Dp:    # run_ranks creates its contexts through api.Fmax: the same fabric with double products
        @staticmethod
        def Fmax(*a, **kw):
            return api.Fmax(*a, double_products=True, **kw)

    def body(f, r):
        f.set_density(dk[r * nxl:(r + 1) * nxl])
        f.set_invgrow(x, y)
        f.set_growth(g)
        return f.flavour_census(radii, capacity=n ** 3)

    res = run_ranks(Dp, n, P, body)
    assert cen1["differing_bits"] > 0
    assert all(res[r][1]["cells"] == nxl * n * n for r in range(P))
    tot = api.census_sum([res[r][1] for r in range(P)])
    assert npc.same(tot, cen1) is None, npc.same(tot, cen1)
    recs = []
    for r in range(P):
        q = res[r][2].copy()
        q["cell"] += np.uint64(r * nxl * n * n)    # x_local -> x
        recs.append(q)
    assert npc.same_records(np.concatenate(recs), rec1)
    for r in range(P):
        assert np.allclose(res[r][0], tv1, rtol=1e-13)


# -------------------------------------------------------------------------------------------------------------------- errors ----
def test_refused_calls_leave_the_context_as_it_was(api, monkeypatch, capfd):
    n = 32
    monkeypatch.delenv("PF_EXACT_LIBM", raising=False)
    from pinocchio_amd import _lib
    with api.Fmax(n) as f:    # no density yet
        f.set_arithmetic("exact")
        with pytest.raises(api.PinfmaxError, match="pf_flavour_census: density not set"):
            f.flavour_census(RADII3)
        assert f.arithmetic == "exact"
    dk = synth.make_density(n, seed=3)
    with _ctx(api, n, dk, monkeypatch, None) as f:
        f.set_arithmetic("exact")
        f.sweep(RADII3)
        p0, bytes0 = f.products(), f.device_bytes
        out = _lib.Census()
        r = np.ascontiguousarray(RADII3)
        rp = r.ctypes.data_as(C.POINTER(C.c_double))
        capfd.readouterr()
        for call, msg in ((lambda: f.L.pf_flavour_census(f.h, 0, rp, None, C.byref(out), 0, None), b"pf_flavour_census: Nsmooth 0"),
                          (lambda: f.L.pf_flavour_census(f.h, 3, rp, None, None, 0, None), b"pf_flavour_census: null argument"),
                          (lambda: f.L.pf_flavour_census(f.h, 3, None, None, C.byref(out), 0, None), b"pf_flavour_census: null argument"),
                          (lambda: f.L.pf_flavour_census(f.h, 3, rp, None, C.byref(out), 5, None), b"pf_flavour_census: null argument")):
            assert call() != 0
            assert msg in f.L.pf_last_error()
            assert "ERROR on task 0: " + msg.decode() in capfd.readouterr().out
            assert f.arithmetic == "exact" and f.device_bytes == bytes0 and _same_products(f.products(), p0)
        with pytest.raises(api.PinfmaxError):
            f.flavour_census([])
        assert f.arithmetic == "exact" and _same_products(f.products(), p0)
