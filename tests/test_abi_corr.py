"""CPU-side checks of the correlation entry points: include/pinfmax.h declares them with the agreed signatures and constants, the
library exports them, pinocchio_amd/_lib.py binds them with matching argument types, pinocchio_amd/api.py mirrors each one, the core
header and the public header agree on the number of sums (through tests/cpu_emul/corr_emul.cpp), pf_halo_power and
pf_halo_multipoles are declared as before, and the refusals that need no device come with a message before any device is touched."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARED = {
    "pf_halo_correlation": "pf_ctx *ctx, int flags, size_t count, const double *pos, const double *vel, double scale, double vfac, int los, const int *mass, int nbins, "
                           "const int *mass_range, unsigned long long *ncells, unsigned long long *r2sum, double *xi, double *xi_cross, pf_corr_info *info",
    "pf_debug_corr_form": "int field_bytes, int n, int y0, int nyl, const double *spec_m, const double *spec_lin, int flags, int which, double *spec_out, pf_matter_info *info",
    "pf_debug_corr_shells": "int field_bytes, int n, int x0, int nxl, const double *real_host, int los, unsigned long long *ncells, unsigned long long *r2sum, double *xi, "
                            "double *parts, unsigned long long *nonfinite_cells",
    "pf_debug_corr_times": "double *ms",
    "pf_debug_corr_passes": "int *passes",
}
# what the issue forbids to touch
UNCHANGED = {
    "pf_halo_power": "pf_ctx *ctx, int flags, size_t count, const double *pos, double scale, const int *mass, int nbins, const int *mass_range, "
                     "unsigned long long *nmodes, unsigned long long *k2sum, double *power, double *cross, pf_halo_info *info",
    "pf_halo_multipoles": "pf_ctx *ctx, int flags, size_t count, const double *pos, const double *vel, double scale, double vfac, int los, const int *mass, int nbins, "
                          "const int *mass_range, unsigned long long *nmodes, unsigned long long *k2sum, double *power, double *cross, pf_halo_info *info",
    "pf_debug_halo_times": "double *ms",
}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "pinocchio_amd", "libpinfmax_hip.so")):
        g.build()
    from pinocchio_amd import _lib
    return _lib


def _ctype(lib, param):
    param = param.strip()
    if "*" not in param:
        return {"int": C.c_int, "size_t": C.c_size_t, "double": C.c_double}[param.rsplit(" ", 1)[0]]
    base = param[:param.index("*")].replace("const", "").strip()
    return {"pf_ctx": C.c_void_p, "double": C.POINTER(C.c_double), "unsigned long long": C.POINTER(C.c_ulonglong), "pf_halo_info": C.POINTER(lib.HaloInfo),
            "pf_corr_info": C.POINTER(lib.CorrInfo), "pf_matter_info": C.POINTER(lib.MatterInfo), "int": C.POINTER(C.c_int)}[base]


def test_the_header_declares_the_agreed_signatures_and_constants(lib):
    hdr = open(os.path.join(ROOT, "include", "pinfmax.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, params in list(DECLARED.items()) + list(UNCHANGED.items()):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in pinfmax.h"
        assert re.sub(r"\s+", " ", m.group(1)).strip() == params, name
    assert re.search(r"#define\s+PF_CORR_ORDERS\s+3\b", hdr) and re.search(r"#define\s+PF_CORR_SUMS\s+12\b", hdr)
    assert re.search(r"#define\s+PF_MULTIPOLE_ORDERS\s+3\b", hdr) and re.search(r"#define\s+PF_MULTIPOLE_SUMS\s+11\b", hdr)
    assert re.search(r"typedef\s+struct\s*\{\s*pf_halo_info\s+halo;\s*unsigned long long\s+cells,\s*nonfinite_cells;\s*\}\s*pf_corr_info;", hdr)
    for name, value in (("NGP", 1), ("DECONVOLVE", 2), ("MASS_WEIGHT", 4), ("MAX_BINS", 8)):
        assert re.search(r"#define\s+PF_HALO_%s\s+%d\b" % (name, value), hdr), name


def test_the_constants_against_the_compiler(lib):
    from test_corr_cpu import build_emul
    E = build_emul()
    s = (C.c_size_t * 6)()
    assert E.corr_emul_sizes(s) == 6
    assert list(s) == [lib.CORR_ORDERS, lib.CORR_SUMS, 3, 6, C.sizeof(lib.CorrInfo), C.sizeof(lib.HaloInfo)]
    assert [k for k, _ in lib.CorrInfo._fields_] == ["halo", "cells", "nonfinite_cells"] and C.sizeof(lib.CorrInfo) == C.sizeof(lib.HaloInfo) + 16


def test_the_library_exports_and_lib_py_binds_them(lib):
    L = lib.load()
    for name, params in list(DECLARED.items()) + list(UNCHANGED.items()):
        assert hasattr(L, name), f"{name} is not exported"
        res, args = lib.PROTOTYPES[name]
        assert res is C.c_int, name
        assert args == [_ctype(lib, p) for p in params.split(",")], name


def test_api_py_mirrors_them(lib):
    from pinocchio_amd import api
    sig = inspect.signature(api.Fmax.halo_correlation).parameters
    assert list(sig) == list(inspect.signature(api.Fmax.halo_multipoles).parameters)
    assert [sig[k].default for k in list(sig)[5:]] == [1.0, 0.0, 2, False, True, False, False, None]
    assert list(inspect.signature(api.debug_corr_form).parameters) == ["spec_m", "spec_lin", "y0", "field_bytes", "ngp", "deconvolve", "which"]
    assert list(inspect.signature(api.debug_corr_shells).parameters) == ["real", "x0", "field_bytes", "los"]
    for meth, call in ((api.Fmax.halo_correlation, "pf_halo_correlation"), (api.debug_corr_form, "pf_debug_corr_form"), (api.debug_corr_shells, "pf_debug_corr_shells"),
                       (api.debug_corr_times, "pf_debug_corr_times"), (api.corr_passes, "pf_debug_corr_passes")):
        assert "." + call + "(" in inspect.getsource(meth), call
    assert (api.CORR_ORDERS, api.CORR_SUMS) == (3, 12) and len(api.CORR_TIME_KEYS) == 6
    assert api.debug_corr_times() == (0.0,) * 6                              # no call of this thread yet
    assert api.corr_passes() == (0, 0)                                       # nothing launched by this thread yet
    with pytest.raises(ValueError):
        api.debug_corr_form([[[1.0, 2.0]]])
    with pytest.raises(ValueError):
        api.debug_corr_shells([[[1.0, 2.0]]])


def test_refusals_that_need_no_device(lib, capfd):
    L = lib.load()
    info = lib.CorrInfo()
    info.cells = 0xABCDEF
    minfo = lib.MatterInfo()
    minfo.modes = 0xABCDEF
    n = 16
    nb = L.pf_power_bins(n)
    nc, r2, bad = (C.c_ulonglong * nb)(), (C.c_ulonglong * nb)(), C.c_ulonglong(0xABCDEF)
    xi, parts = (C.c_double * (3 * nb))(), (C.c_double * (6 * nb))()
    pos = (C.c_double * 6)(1.0, 2.0, 3.0, 4.0, 5.0, 6.0)
    mass = (C.c_int * 2)(10, 20)
    rng = (C.c_int * 2)(1, 100)
    spec = (C.c_double * (2 * n * n * (n // 2 + 1)))()
    real = (C.c_double * n ** 3)()
    fm = lambda **k: L.pf_debug_corr_form(k.get("fb", 8), k.get("n", n), k.get("y0", 0), k.get("nyl", n), k.get("m", spec), k.get("lin", spec), k.get("flags", 0),
                                          k.get("which", 1), k.get("out", spec), k.get("info", C.byref(minfo)))
    sh = lambda **k: L.pf_debug_corr_shells(k.get("fb", 8), k.get("n", n), k.get("x0", 0), k.get("nxl", n), k.get("real", real), k.get("los", 2), k.get("nc", nc),
                                            k.get("r2", r2), k.get("xi", xi), k.get("parts", parts), k.get("bad", C.byref(bad)))
    calls = [(lambda: L.pf_halo_correlation(None, 0, 2, pos, None, 1.0, 0.0, 2, mass, 1, rng, nc, r2, xi, None, C.byref(info)), b"pf_halo_correlation: null argument"),
             (lambda: fm(m=None), b"null"), (lambda: fm(out=None), b"null"), (lambda: fm(info=None), b"null"), (lambda: fm(flags=4), b"unknown flag bits"),
             (lambda: fm(which=2), b"form 2"), (lambda: fm(which=-1), b"form -1"), (lambda: fm(lin=None), b"the cross form without a second spectrum"),
             (lambda: fm(fb=2), b"fields of 2 bytes"), (lambda: fm(n=15), b"a grid of 15"), (lambda: fm(y0=9, nyl=8), b"leave the grid"),
             (lambda: sh(real=None), b"null"), (lambda: sh(nc=None), b"null"), (lambda: sh(r2=None), b"null"), (lambda: sh(xi=None), b"null"), (lambda: sh(bad=None), b"null"),
             (lambda: sh(fb=16), b"fields of 16 bytes"), (lambda: sh(n=15), b"a grid of 15"), (lambda: sh(n=4096), b"a grid of 4096"), (lambda: sh(x0=10, nxl=7), b"leave the grid"),
             (lambda: sh(los=3), b"a line of sight along axis 3"), (lambda: sh(los=-1), b"a line of sight along axis -1")]
    for call, what in calls:
        assert call() != 0
        err = L.pf_last_error()
        assert what in err and (b"pf_debug_corr_form" in err or b"pf_debug_corr_shells" in err or b"pf_halo_correlation" in err), (what, err)
        assert "ERROR on task 0: pf_" in capfd.readouterr().out
        assert info.cells == 0xABCDEF and minfo.modes == 0xABCDEF and bad.value == 0xABCDEF and not any(xi[:8]) and not any(nc[:8])
    assert L.pf_debug_corr_times(None) != 0
    assert L.pf_debug_corr_passes(None) != 0
