"""The power-spectrum call on the device (include/pinfmax.h: pf_power_spectrum, pf_debug_power_spectrum) against the numpy restatement
of its definitions (tests/np_power.py): planted spectra through the tap, resident spectra on every transform path and field width,
the variances against what the sweep reports for the same radii (Parseval), the generator's own spectrum against the analytic one,
slabs against one rank, the LPT source spectra, and the refusals.

Where the two tolerances come from.  Every term is positive and carries at most three roundings of half an ulp (two products, one
sum); the weight is a power of two and 1 / N^6 is applied once to a shell's sum.  A sum of positive terms inherits the per-term
relative error, so `power` lies within about 5e-16 of the exact sum.  TOL_POWER = 1e-14 leaves a factor of ten for a different order
of the additions and for what the fixed-point form drops below 2^-95 of a shell's largest term.  TOL_VARIANCE = 1e-13: the window
adds the exp itself (1-2 ulp on the device, by the project's test of its elementary functions) and the rounding of its argument,
|x| 2^-53 with |x| <~ 40 for every term that still contributes.  Neither figure is measured on the code under test.

fp32 fields, Parseval against the sweep (printed by test_variances_against_the_sweep, not asserted -- the difference is the error of
the fp32 transforms): see profiles/power_notes.md for the largest ratio seen."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import np_power as npp
import power_cases as pc
from pinocchio_amd import synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_POWER, TOL_VARIANCE = 1e-14, 1e-13
RADII = (4.0, 2.0, 1.0, 0.0)


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


def raw_debug(spec, y0, fb, radii):
    """pf_debug_power_spectrum with a guard element behind every output array -> the dict of api.debug_power_spectrum"""
    from pinocchio_amd import _lib
    L = _lib.load()
    spec = np.ascontiguousarray(spec, dtype=np.complex128)
    nyl, n = spec.shape[:2]
    nb = L.pf_power_bins(n)
    r = np.ascontiguousarray(radii, dtype=np.float64)
    nm, ks = np.zeros(nb + 1, np.uint64), np.zeros(nb + 1, np.uint64)
    pw, var = np.zeros(nb + 1), np.zeros(len(r) + 1)
    nm[-1] = ks[-1] = 0xABCDEF
    pw[-1] = var[-1] = 123.5
    info = (_lib.PowerInfo * 2)()
    info[1].modes = info[1].nonfinite = 0xABCDEF
    up, dp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_ulonglong))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double)))
    assert L.pf_debug_power_spectrum(fb, n, y0, nyl, dp(spec.view(np.float64)), len(r), dp(r), up(nm), up(ks), dp(pw), dp(var), info) == 0, L.pf_last_error()
    assert nm[-1] == ks[-1] == 0xABCDEF and pw[-1] == var[-1] == 123.5 and info[1].modes == info[1].nonfinite == 0xABCDEF
    return {"nmodes": nm[:-1], "k2sum": ks[:-1], "power": pw[:-1], "variance": var[:-1], "modes": int(info[0].modes), "nonfinite": int(info[0].nonfinite)}


def check(got, want, what, ints_only=False):
    assert np.array_equal(got["nmodes"], want["nmodes"]) and np.array_equal(got["k2sum"], want["k2sum"]), what
    assert (got["modes"], got["nonfinite"]) == (want["modes"], want["nonfinite"]), what
    rp, rv = npp.rel(got["power"], want["power"]), npp.rel(got["variance"], want["variance"])
    print(what, "power", rp, "variance", rv)
    assert rp <= TOL_POWER and rv <= TOL_VARIANCE, (what, rp, rv)


def same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.uint64), np.asarray(b[k]).view(np.uint64)) for k in ("nmodes", "k2sum", "power", "variance")) and \
        (a["modes"], a["nonfinite"]) == (b["modes"], b["nonfinite"])


@pytest.fixture(scope="module")
def wanted():
    """the restatement of every planted case, computed once: (name, fb) -> whole box, two slabs"""
    out = {}
    for name, spec, _ in pc.cases():
        for fb in (8, 4):
            out[name, fb] = (npp.power(spec, 0, RADII, fb), [npp.power(spec[a:a + 8], a, RADII, fb) for a in (0, 8)])
    return out


@pytest.mark.parametrize("fb", [8, 4])
def test_planted_cases_through_the_tap(api, wanted, fb):
    for name, spec, expect in pc.cases():
        whole, slabs = wanted[name, fb]
        got = raw_debug(spec, 0, fb, RADII)
        check(got, whole, (name, fb))
        assert int(got["nmodes"].sum()) == pc.N ** 3 == got["modes"]
        assert np.array_equal(got["power"] == 0, whole["power"] == 0)          # untouched shells are exactly 0
        if expect is not None:
            exp = np.zeros(npp.bins(pc.N))
            exp[expect[0]] = expect[1] * expect[3] / float(pc.N ** 6)
            assert np.array_equal(got["power"], exp), name
        parts = [raw_debug(spec[a:a + 8], a, fb, RADII) for a in (0, 8)]
        for p, w in zip(parts, slabs):
            check(p, w, (name, fb, "slab"))
            assert int(p["nmodes"].sum()) == 8 * pc.N * pc.N == p["modes"]
        both = npp.add(parts)
        assert np.array_equal(both["nmodes"], got["nmodes"]) and np.array_equal(both["k2sum"], got["k2sum"]) and both["nonfinite"] == got["nonfinite"]
        assert same_bits(got, api.debug_power_spectrum(spec, 0, fb, RADII)), name   # the binding, and the same bits from run to run
    assert raw_debug(pc.cases()[0][1], 0, fb, ())["variance"].size == 0             # ns = 0 with null radii and variance
    # more radii than one pair of launches takes: the batches of the radii
    spec, many = pc.random_box(8), np.linspace(0.0, 3.25, 14)
    check(raw_debug(spec, 0, fb, many), npp.power(spec, 0, many, fb), ("14 radii", fb))


@pytest.mark.parametrize("n,fb,path", [(16, 8, 0), (16, 4, 0), (64, 8, 0), (64, 4, 0), (48, 8, 1), (48, 4, 1), (36, 8, 2)])
def test_resident_density_on_every_transform_path(api, n, fb, path):
    with api.Fmax(n, field_bytes=fb) as f:
        assert f.L.pf_transform_path(f.h) == path
        f.synth_density(seed=40 + n)
        f.set_invgrow(*synth.invgrow_table("lcdm"))
        f.sweep(np.array([2.0]))      # products exist: the call must leave them alone
        state = (f.device_bytes, f.arithmetic, f.L.pf_replicated_spectrum(f.h))
        dk = f.density()
        prod = f.products()
        got = f.power_spectrum("density", RADII, box=100.0)
        again = f.power_spectrum(0, RADII)
        assert same_bits(got, again)
        assert state == (f.device_bytes, f.arithmetic, f.L.pf_replicated_spectrum(f.h))
        after = f.products()
        assert prod.tobytes() == after.tobytes()
        assert np.array_equal(dk, f.density())
    want = npp.power(npp.from_x_slab(dk), 0, RADII, 8)    # (the export widens the fields exactly)
    check(got, want, (n, fb, path))
    assert int(got["nmodes"].sum()) == n ** 3 == got["modes"] and got["nonfinite"] == 0 and np.count_nonzero(got["power"]) > n // 4
    nz = got["nmodes"] > 0
    nm = got["nmodes"][nz].astype(np.float64)
    assert np.array_equal(got["k"][nz], (2.0 * np.pi / 100.0) * np.sqrt(got["k2sum"][nz].astype(np.float64) / nm))
    assert np.array_equal(got["pk"][nz], got["power"][nz] / nm * 100.0 ** 3)


@pytest.mark.parametrize("n", [32, 48])
def test_variances_against_the_sweep(api, n):
    """Parseval: the windowed sum is the TrueVariance the sweep reports for the radius.  1e-12 is the figure the project holds
    TrueVariance to against the oracle; asserted with fp64 fields, printed with fp32 fields"""
    radii = np.array([4.0, 2.0, 1.0, 0.0])
    x, y = synth.invgrow_table("lcdm")
    for fb in (8, 4):
        with api.Fmax(n, field_bytes=fb) as f:
            f.synth_density(seed=3 + n)
            f.set_invgrow(x, y)
            var = f.power_spectrum("density", radii)["variance"]
            tv = f.sweep(radii)
            assert np.array_equal(var, f.power_spectrum("density", radii)["variance"])   # the sweep leaves delta(k) as it was
        ratio = np.abs(var - tv) / tv
        print("n", n, "field_bytes", fb, "variance", var, "true_variance", tv, "relative difference", ratio)
        if fb == 8:
            assert np.all(ratio <= 1e-12), ratio


def _params():
    with open(os.path.join(HERE, "golden", "hmf_validation_kat.json")) as fh:
        return json.load(fh)["params"]


@pytest.mark.parametrize("tabulated", [False, True])
def test_the_generators_spectrum_on_the_device(api, tabulated):
    """pf_genic_density with FixedIC: power[b] is the shell sum of PkNorm P(k) / Box^3 over the modes the generator leaves non-zero --
    Eisenstein & Hu, or the spline values of a table"""
    import ic_oracle
    from test_power_cpu import analytic_shell_sums, eh_of
    p = _params()
    n, pkn = 32, 1.7e7
    box = float(n) / p["Hubble100"]
    table = None
    pk = eh_of(p)
    if tabulated:
        lk = np.linspace(-3.0, 1.5, 40)
        lp = 3.0 * lk + np.log10([pkn * pk(10.0 ** v) for v in lk])     # log10(k^3 P) of a spectrum of the same shape
        table, pkn = (lk, lp), 1.0
        L = ic_oracle._lib()
        dp = C.POINTER(C.c_double)
        coef = np.zeros(len(lk))
        L.orc_cspline_coeffs.argtypes = [dp, dp, C.c_int, dp]
        L.orc_my_spline_eval.restype = C.c_double
        L.orc_my_spline_eval.argtypes = [dp, dp, dp, C.c_int, C.c_double]
        assert L.orc_cspline_coeffs(lk.ctypes.data_as(dp), lp.ctypes.data_as(dp), len(lk), coef.ctypes.data_as(dp)) == 0
        pk = lambda k: 10.0 ** L.orc_my_spline_eval(lk.ctypes.data_as(dp), lp.ctypes.data_as(dp), coef.ctypes.data_as(dp), len(lk), math.log10(k)) / k / k / k
    with api.Fmax(n) as f:
        f.genic_density(5, box, p["Omega0"], p["OmegaBaryon"], p["Hubble100"], p["PrimordialIndex"], pknorm=pkn, fixed=True, pk_table=table)
        got = f.power_spectrum("density", box=box)
        dk = f.density()
    want = analytic_shell_sums(n, box, pkn, dk != 0, pk)
    r = npp.rel(got["power"], want)
    print("tabulated" if tabulated else "E&H", "power against the analytic shell sums:", r)
    assert np.count_nonzero(want) >= 16 and r <= 1e-12


@pytest.mark.parametrize("n,P,fb", [(32, 2, 8), (64, 4, 8), (48, 3, 8), (64, 8, 8), (64, 4, 4)])
@pytest.mark.parametrize("replicate", [0, 1])
def test_slabs_return_the_boxs_numbers(api, n, P, fb, replicate, monkeypatch):
    from test_gpu_multirank import run_ranks
    monkeypatch.setenv("PF_REPLICATE_DK", str(replicate))
    with api.Fmax(n, field_bytes=fb) as f1:
        f1.synth_density(seed=9)
        one = f1.power_spectrum("density", RADII)

    def body(f, r):
        f.synth_density(seed=9)
        return f.power_spectrum("density", RADII), f.L.pf_replicated_spectrum(f.h)

    res = run_ranks(api, n, P, body, field_bytes=fb)
    for r in range(P):
        got, rep = res[r]
        assert rep == replicate
        assert same_bits(got, res[0][0]), r
        check(got, one, (n, P, fb, replicate, r))     # integers exactly, doubles to the two tolerances


def test_source_spectra(api):
    n = 32
    x, y = synth.invgrow_table("lcdm")
    with api.Fmax(n) as f:
        f.synth_density(seed=21)
        for which in (1, 2, 3):
            with pytest.raises(api.PinfmaxError, match="pf_power_spectrum: LPT sources not computed"):
                f.power_spectrum(which)
        f.set_invgrow(x, y)
        f.set_growth(synth.growth_multipliers())
        f.sweep(np.array([2.0, 0.0]))
        f.compute_displacements(1, 0)
        for which, name in ((1, "kvector_2LPT"), (2, "kvector_3LPT_1"), (3, "kvector_3LPT_2")):
            got = f.power_spectrum(name, (1.0, 0.0))
            want = npp.power(npp.from_x_slab(f.kvector(which - 1)), 0, (1.0, 0.0), 8)
            check(got, want, name)
            assert same_bits(got, f.power_spectrum(which, (1.0, 0.0)))
            assert np.count_nonzero(got["power"]) > 8


def test_refusals_on_a_live_context(api, capfd):
    from pinocchio_amd import _lib
    n = 16
    with api.Fmax(n) as f:
        with pytest.raises(api.PinfmaxError, match="pf_power_spectrum: density not set"):
            f.power_spectrum()
        f.synth_density(seed=1)
        L, nb = f.L, api.power_bins(n)
        nm, ks = (C.c_ulonglong * nb)(), (C.c_ulonglong * nb)()
        pw, var = (C.c_double * nb)(), (C.c_double * (_lib.MAX_SMOOTH + 1))()
        info = _lib.PowerInfo()
        r = (C.c_double * (_lib.MAX_SMOOTH + 1))()
        call = lambda **k: L.pf_power_spectrum(f.h, k.get("which", 0), k.get("ns", 2), k.get("r", r), k.get("nm", nm), k.get("ks", ks), k.get("pw", pw),
                                               k.get("var", var), k.get("info", C.byref(info)))
        before = f.device_bytes
        for kw, what in (({"which": -1}, b"not in 0..3"), ({"which": 4}, b"not in 0..3"), ({"ns": -1}, b"radii not in"), ({"ns": _lib.MAX_SMOOTH + 1}, b"radii not in"),
                         ({"r": (C.c_double * 2)(1.0, -1.0)}, b"negative or not finite"), ({"r": (C.c_double * 2)(float("nan"), 0.0)}, b"negative or not finite"),
                         ({"r": None}, b"null radius_cells or variance"), ({"var": None}, b"null radius_cells or variance"), ({"nm": None}, b"null argument"),
                         ({"ks": None}, b"null argument"), ({"pw": None}, b"null argument"), ({"info": None}, b"null argument")):
            assert call(**kw) != 0, kw
            assert what in L.pf_last_error() and b"pf_power_spectrum" in L.pf_last_error(), (kw, L.pf_last_error())
        assert "ERROR on task 0: pf_power_spectrum" in capfd.readouterr().out
        assert call(ns=0, r=None, var=None) == 0 and call(ns=_lib.MAX_SMOOTH) == 0      # the two ends of the range are served
        assert before == f.device_bytes
