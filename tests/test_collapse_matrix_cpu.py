"""The harness of the collapse matrix (tests/collapse_matrix.py) proven without a GPU: the host compilation of the per-cell header
(tests/cpu_emul/collapse_emul.cpp: emul_collapse, emul_collapse_fast, emul_ct, emul_ell_sng) with a numpy running maximum stands
where the device stands in tests/test_gpu_collapse_matrix.py -- the same ladder, the same injection of the Hessian into the oracle,
the same noise spread, per-cell contract and caps, Route C's Rmax expectations, Route D's share check.  The mutant of the last test
(the running maximum compared in product precision) lives here, not in product code."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import collapse_matrix as cm
import oracle_lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emul", "collapse_emul.cpp")
SO = os.path.join(HERE, "cpu_emul", "libcollapse_emul.so")
dp = C.POINTER(C.c_double)


def _dp(a):
    return a.ctypes.data_as(dp)


@pytest.fixture(scope="module")
def emul():
    hdrs = [os.path.join(HERE, "..", "pinocchio_amd", "csrc", h) for h in ("pf_collapse_core.h", "pf_sng_core.h")]
    if (not os.path.exists(SO)) or os.path.getmtime(SO) < max([os.path.getmtime(SRC)] + [os.path.getmtime(h) for h in hdrs]):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-o", SO, SRC])
    L = C.CDLL(SO)
    L.emul_collapse.argtypes = [dp, dp, C.c_int, dp, C.c_long, dp, dp]
    L.emul_collapse_fast.argtypes = [dp, dp, C.c_int, dp, C.c_long, dp, dp, C.c_int]
    L.emul_ct.argtypes = [dp, C.c_double, dp, C.c_long, dp, dp, C.c_int]
    L.emul_ell_sng.argtypes = [dp, C.c_long, C.c_double, dp, dp]
    L.emul_ell_sng.restype = None
    return L


_hess = {}
_orc = {}


def _hessian(n, radius, field_bytes):
    """the oracle's own second derivatives; fp32 fields: rounded to fp32 as the device's transforms store them"""
    key = (n, float(radius), field_bytes)
    if key not in _hess:
        if n not in _orc:
            _orc[n] = oracle_lib.Oracle(n, 0)
            _orc[n].set_density(cm.density(n))
        H = _orc[n].second_derivatives(radius)
        if field_bytes == 4:
            H = [h.astype(np.float32).astype(np.float64) for h in H]
        for h in H:
            h.setflags(write=False)
        _hess[key] = H
    return _hess[key]


class EmulSide:
    """pf_collapse_body restated: the per-cell functions of the header compiled for the host, and the running maximum in numpy --
    the stored PRODFLOAT compared after promotion, (double)fold < Fnew (quirk Q2); product_precision=True is the mutant that
    compares fold < (PRODFLOAT)Fnew"""

    def __init__(self, L, n, field_bytes, double_products, variant, arithmetic, product_precision=False):
        self.L, self.n, self.fb, self.variant, self.fast = L, n, field_bytes, variant, arithmetic == "fast"
        self.pr = np.float64 if double_products else np.float32
        self.mutant = product_precision
        self.x, self.y = cm.invgrow()
        self.H = None
        self.tab = None
        self.F = self.R = None

    def hessian(self, ismooth, radius):
        self.H = _hessian(self.n, radius, self.fb)
        return self.H

    def load_table(self, ismooth, variance, table):
        self.tab = (np.ascontiguousarray(table, dtype=np.float64), float(np.sqrt(variance)))

    def collapse(self, ismooth):
        d = np.ascontiguousarray(np.stack([h.ravel() for h in self.H], axis=1))
        m = len(d)
        Fnew, lam = np.empty(m), np.zeros((m, 3))
        if self.fast:
            assert self.L.emul_collapse_fast(_dp(self.x), _dp(self.y), len(self.x), _dp(d), m, _dp(Fnew), _dp(lam), 1) in (0, 2)
        else:
            assert self.L.emul_collapse(_dp(self.x), _dp(self.y), len(self.x), _dp(d), m, _dp(Fnew), _dp(lam)) == 0
        have_lam = Fnew != -10.0
        if self.variant.startswith("tab"):
            table, ampl = self.tab
            delta, Ft = np.empty(100), np.empty(m)
            assert self.L.emul_ct(_dp(table), ampl, _dp(lam), m, _dp(delta), _dp(Ft), cm.flavour_of(self.variant)) == 0
            Fnew = np.where(have_lam, Ft, -10.0)
        elif self.variant == "sng":
            cosmo = np.array(list(cm.SNG_COSMO) + [0.0, 100.0 / 299792.458, 0.0])
            bc = np.empty(m)
            self.L.emul_ell_sng(_dp(lam), m, cm.SNG_DIN, _dp(cosmo), _dp(bc))
            Fnew = np.where(have_lam, np.where(bc > 0.0, 1.0 / np.where(bc > 0.0, bc, 1.0), 0.0), -10.0)
        if ismooth == 0:
            self.F, self.R = np.full(m, -10.0, dtype=self.pr), np.full(m, -1, dtype=np.int32)
        if self.mutant:
            take = self.F < Fnew.astype(self.pr)
        else:
            take = self.F.astype(np.float64) < Fnew
        self.F[take] = Fnew[take].astype(self.pr)
        self.R[take] = ismooth
        delta = d[:, 0] + d[:, 1] + d[:, 2]
        return float(np.sum(delta * delta) / m)

    def products(self):
        return self.F.copy(), self.R.copy()


_refs = {}
_distinct = cm.Distinct()


def _reference(n, variant, fb, double_products, radii, factor=1.0):
    key = (n, variant, fb, double_products, factor)
    if key not in _refs:
        var = cm.field_variance(n, radii) * factor if variant.startswith("tab") else None
        _refs[key] = cm.Reference(n, variant, double_products, len(radii), variance=var, noise=variant != "sng")
    return _refs[key]


def test_oracle_collapses_on_the_hessian_it_is_given():
    """Oracle.set_second_derivatives: its own Hessian handed back reproduces its own pass bit for bit; half of it does not"""
    n = 16
    o = oracle_lib.Oracle(n, 0)
    o.set_density(cm.density(n))
    o.set_invgrow(*cm.invgrow())
    H = o.second_derivatives(1.0)
    tv = o.collapse_times(0)
    p = o.products()
    o.second_derivatives(3.0)
    o.set_second_derivatives(H)
    assert o.collapse_times(0) == tv
    q = o.products()
    assert np.array_equal(p["Fmax"], q["Fmax"]) and np.array_equal(p["Rmax"], q["Rmax"])
    o.set_second_derivatives([0.5 * h for h in H])
    assert o.collapse_times(0) == pytest.approx(0.25 * tv, rel=1e-14)
    assert np.mean(o.products()["Fmax"] != p["Fmax"]) > 0.8


@pytest.mark.parametrize("arithmetic", cm.ARITHMETICS)
@pytest.mark.parametrize("fb,double_products", cm.FIELD_PRODUCT_TYPES)
@pytest.mark.parametrize("variant", cm.VARIANTS)
def test_route_a_host_compilation_meets_the_contract(emul, variant, fb, double_products, arithmetic):
    n = 16 if variant == "sng" else 32
    radii = cm.RADII[n]
    ref = _reference(n, variant, fb, double_products, radii)
    side = EmulSide(emul, n, fb, double_products, variant, arithmetic)
    cm.run_ladder(side, ref, radii, double_products, arithmetic == "exact", "%s fb%d %s %s" % (variant, fb, "dp" if double_products else "sp", arithmetic))
    _distinct.note(n, variant, fb, double_products, arithmetic, side.products()[0])


@pytest.mark.parametrize("n,fb", [(20, 8), (24, 4)])
def test_route_e_sizes_host_compilation(emul, n, fb):
    radii = cm.RADII[n]
    ref = _reference(n, "plain", fb, False, radii)
    cm.run_ladder(EmulSide(emul, n, fb, False, "plain", "fast"), ref, radii, False, False, "plain %d^3 fb%d" % (n, fb))


@pytest.mark.parametrize("arithmetic", cm.ARITHMETICS)
@pytest.mark.parametrize("fb,double_products", cm.FIELD_PRODUCT_TYPES)
def test_route_c_running_maximum(emul, fb, double_products, arithmetic):
    side = EmulSide(emul, 32, fb, double_products, "plain", arithmetic)
    cm.run_running_maximum(side, lambda nr: cm.Reference(32, "plain", double_products, nr, noise=False), double_products, "fb%d %s" % (fb, arithmetic))


@pytest.mark.parametrize("fb", [8, 4])
def test_route_c_fails_a_running_maximum_compared_in_product_precision(emul, fb):
    """the mutant: fold < (float)Fnew.  A cell whose Fnew was rounded down on storing is then never taken again -- Rmax stays 0 where
    the reference moves on.  Route C must notice"""
    side = EmulSide(emul, 32, fb, False, "plain", "fast", product_precision=True)
    with pytest.raises(AssertionError):
        cm.run_running_maximum(side, lambda nr: cm.Reference(32, "plain", False, nr, noise=False), False, "mutant fb%d" % fb)


@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("flavour", [0, 1, 2])
def test_route_d_outside_the_table(emul, flavour, fb):
    """the table made for 0.1 x the variance: > 1 % of the cells beyond each of its three ranges, the same contract per cell"""
    n, radii, variant = 32, cm.RADII[32], "tab%d" % flavour
    ref = _reference(n, variant, fb, False, radii, factor=0.1)
    for i, r in enumerate(radii):
        shares = cm.shares_outside_table(_hessian(n, r, 8), ref.variance[i])
        assert min(shares) > 0.01, (r, shares)
    cm.run_ladder(EmulSide(emul, n, fb, False, variant, "fast"), ref, radii, False, False, "outside %s fb%d" % (variant, fb))


@pytest.mark.parametrize("double_products", [False, True])
def test_contract_fails_a_solve_that_is_off_in_the_seventh_digit(emul, double_products):
    """a side that hands back the true Hessian but solves on one scaled by 1 + 1e-6: far above the spread of two ulps of input noise,
    and above two fp32 ulps on many cells -- the per-cell contract must notice"""
    class Off(EmulSide):
        def collapse(self, ismooth):
            true = self.H
            self.H = [h * (1.0 + 1e-6) for h in true]
            try:
                return EmulSide.collapse(self, ismooth) / (1.0 + 1e-6) ** 2
            finally:
                self.H = true

    n, radii = 32, cm.RADII[32]
    ref = _reference(n, "plain", 8, double_products, radii)
    with pytest.raises(AssertionError):
        cm.run_ladder(Off(emul, n, 8, double_products, "plain", "fast"), ref, radii, double_products, False, "off by 1e-6")
