"""CPU-side checks of the bispectrum entry points: include/pinfmax.h declares them with the agreed signatures and constants, the
library exports them, pinocchio_amd/_lib.py binds them with matching argument types, pinocchio_amd/api.py mirrors each one, the core
header and the public header agree on the number of k-bins (through tests/cpu_emul/bispec_emul.cpp), the three older halo calls are
declared as before, and the refusals that need no device come with a message before any device is touched."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import bispec_cases as bc
import np_bispec as npb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARED = {
    "pf_bispectrum_triangles": "int kmin, int dk, int nk, int *ijl",
    "pf_halo_bispectrum": "pf_ctx *ctx, int flags, size_t count, const double *pos, const double *vel, double scale, double vfac, int los, const int *mass, int nbins, "
                          "const int *mass_range, int kmin, int dk, int nk, unsigned long long *kmodes, double *ntri, double *bsum, double *psum, pf_bispec_info *info",
    "pf_debug_bispec_mask": "int field_bytes, int n, int y0, int nyl, const double *spec, int flags, int kind, int kmin, int dk, int nk, int bin, double *spec_out, "
                            "unsigned long long *kmodes, unsigned long long *nonfinite_modes",
    "pf_debug_bispec_triples": "int field_bytes, int n, int x0, int nxl, const double *fields, int kmin, int dk, int nk, double *sums, double *parts, double *pair, "
                               "double *maxima, unsigned long long *nonfinite_cells",
    "pf_debug_bispec_times": "double *ms",
}
# what the issue forbids to touch
UNCHANGED = {
    "pf_halo_power": "pf_ctx *ctx, int flags, size_t count, const double *pos, double scale, const int *mass, int nbins, const int *mass_range, "
                     "unsigned long long *nmodes, unsigned long long *k2sum, double *power, double *cross, pf_halo_info *info",
    "pf_halo_multipoles": "pf_ctx *ctx, int flags, size_t count, const double *pos, const double *vel, double scale, double vfac, int los, const int *mass, int nbins, "
                          "const int *mass_range, unsigned long long *nmodes, unsigned long long *k2sum, double *power, double *cross, pf_halo_info *info",
    "pf_halo_correlation": "pf_ctx *ctx, int flags, size_t count, const double *pos, const double *vel, double scale, double vfac, int los, const int *mass, int nbins, "
                           "const int *mass_range, unsigned long long *ncells, unsigned long long *r2sum, double *xi, double *xi_cross, pf_corr_info *info",
    "pf_debug_halo_times": "double *ms",
    "pf_debug_corr_times": "double *ms",
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
            "pf_corr_info": C.POINTER(lib.CorrInfo), "pf_bispec_info": C.POINTER(lib.BispecInfo), "int": C.POINTER(C.c_int)}[base]


def test_the_header_declares_the_agreed_signatures_and_constants(lib):
    hdr = open(os.path.join(ROOT, "include", "pinfmax.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, params in list(DECLARED.items()) + list(UNCHANGED.items()):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in pinfmax.h"
        assert re.sub(r"\s+", " ", m.group(1)).strip() == params, name
    assert re.search(r"#define\s+PF_BISPEC_MAX_KBINS\s+32\b", hdr)
    assert re.search(r"typedef\s+struct\s*\{\s*pf_halo_info\s+halo;\s*unsigned long long\s+cells,\s*nonfinite_cells;\s*\}\s*pf_bispec_info;", hdr)
    assert re.search(r"typedef\s+struct\s*\{\s*pf_halo_info\s+halo;\s*unsigned long long\s+cells,\s*nonfinite_cells;\s*\}\s*pf_corr_info;", hdr)
    for name, value in (("NGP", 1), ("DECONVOLVE", 2), ("MASS_WEIGHT", 4), ("MAX_BINS", 8)):
        assert re.search(r"#define\s+PF_HALO_%s\s+%d\b" % (name, value), hdr), name


def test_the_constants_against_the_compiler(lib):
    from test_bispec_cpu import build_emul
    E = build_emul()
    s = (C.c_size_t * 5)()
    assert E.bispec_emul_sizes(s) == 5
    assert list(s) == [lib.BISPEC_MAX_KBINS, 32, C.sizeof(lib.BispecInfo), C.sizeof(lib.HaloInfo), C.sizeof(lib.CorrInfo)]
    assert [k for k, _ in lib.BispecInfo._fields_] == ["halo", "cells", "nonfinite_cells"] and C.sizeof(lib.BispecInfo) == C.sizeof(lib.HaloInfo) + 16


def test_the_library_exports_and_lib_py_binds_them(lib):
    L = lib.load()
    for name, params in list(DECLARED.items()) + list(UNCHANGED.items()):
        assert hasattr(L, name), f"{name} is not exported"
        res, args = lib.PROTOTYPES[name]
        assert res is C.c_int, name
        assert args == [_ctype(lib, p) for p in params.split(",")], name


def test_api_py_mirrors_them(lib):
    from pinocchio_amd import api
    sig = inspect.signature(api.Fmax.halo_bispectrum).parameters
    assert list(sig) == ["self", "pos", "vel", "mass", "ranges", "kmin", "dk", "nk", "scale", "vfac", "los", "mass_weight", "ngp", "deconvolve", "box"]
    assert [sig[k].default for k in list(sig)[8:]] == [1.0, 0.0, 2, False, False, False, None]
    assert list(inspect.signature(api.debug_bispec_mask).parameters) == ["spec", "kmin", "dk", "nk", "bin", "y0", "field_bytes", "ngp", "deconvolve", "kind"]
    assert list(inspect.signature(api.debug_bispec_triples).parameters) == ["fields", "kmin", "dk", "nk", "x0", "field_bytes"]
    for meth, call in ((api.Fmax.halo_bispectrum, "pf_halo_bispectrum"), (api.debug_bispec_mask, "pf_debug_bispec_mask"), (api.debug_bispec_triples, "pf_debug_bispec_triples"),
                       (api.debug_bispec_times, "pf_debug_bispec_times"), (api.bispectrum_triangles, "pf_bispectrum_triangles")):
        assert "." + call + "(" in inspect.getsource(meth), call
    assert api.BISPEC_MAX_KBINS == 32 and len(api.BISPEC_TIME_KEYS) == 7
    assert api.debug_bispec_times() == (0.0,) * 7                            # no call of this thread yet
    with pytest.raises(ValueError):
        api.debug_bispec_mask([[[1.0, 2.0]]], 1, 1, 1, 0)
    with pytest.raises(ValueError):
        api.debug_bispec_triples([[[[1.0, 2.0]]]], 1, 1, 1)
    # the list of triples needs no device: the library's against the restatement's
    for _, kmin, dk, nk in bc.CASES + [(0, 1, 1, 32), (0, 7, 1, 5)]:
        tri = api.bispectrum_triangles(kmin, dk, nk)
        assert tri.dtype == np.int32 and [tuple(r) for r in tri] == npb.triangles(kmin, dk, nk)
    assert len(api.bispectrum_triangles(1, 1, 4)) < 20 and len(api.bispectrum_triangles(1, 2, 3)) == 10
    with pytest.raises(api.PinfmaxError, match="pf_bispectrum_triangles: k-bins"):
        api.bispectrum_triangles(1, 1, 33)


def test_refusals_that_need_no_device(lib, capfd):
    L = lib.load()
    info = lib.BispecInfo()
    info.cells = 0xABCDEF
    n, kmin, dk, nk = 16, 1, 2, 2
    nt = L.pf_bispectrum_triangles(kmin, dk, nk, None)
    assert nt == 4
    km, bad = (C.c_ulonglong * nk)(), C.c_ulonglong(0xABCDEF)
    ntri, bsum, psum = (C.c_double * nt)(), (C.c_double * nt)(), (C.c_double * nk)()
    parts, mx = (C.c_double * (2 * nt))(), (C.c_double * nk)()
    pos = (C.c_double * 6)(1.0, 2.0, 3.0, 4.0, 5.0, 6.0)
    mass = (C.c_int * 2)(10, 20)
    rng = (C.c_int * 2)(1, 100)
    spec = (C.c_double * (2 * n * n * (n // 2 + 1)))()
    real = (C.c_double * (nk * n ** 3))()
    mk = lambda **k: L.pf_debug_bispec_mask(k.get("fb", 8), k.get("n", n), k.get("y0", 0), k.get("nyl", n), k.get("spec", spec), k.get("flags", 0), k.get("kind", 0),
                                            k.get("kmin", kmin), k.get("dk", dk), k.get("nk", nk), k.get("bin", 0), k.get("out", spec), k.get("km", km), k.get("bad", C.byref(bad)))
    tr = lambda **k: L.pf_debug_bispec_triples(k.get("fb", 8), k.get("n", n), k.get("x0", 0), k.get("nxl", n), k.get("real", real), k.get("kmin", kmin), k.get("dk", dk),
                                               k.get("nk", nk), k.get("sums", bsum), k.get("parts", parts), k.get("pair", psum), k.get("mx", mx), k.get("bad", C.byref(bad)))
    calls = [(lambda: L.pf_halo_bispectrum(None, 0, 2, pos, None, 1.0, 0.0, 2, mass, 1, rng, kmin, dk, nk, km, ntri, bsum, psum, C.byref(info)), b"pf_halo_bispectrum: null argument"),
             (lambda: mk(spec=None), b"null"), (lambda: mk(out=None), b"null"), (lambda: mk(km=None), b"null"), (lambda: mk(bad=None), b"null"),
             (lambda: mk(flags=4), b"unknown flag bits"), (lambda: mk(kind=2), b"field kind 2"), (lambda: mk(kind=-1), b"field kind -1"), (lambda: mk(n=15), b"a grid of 15"),
             (lambda: mk(kmin=0), b"a kmin of 0"), (lambda: mk(dk=0), b"a dk of 0"), (lambda: mk(nk=0), b"0 k-bins"), (lambda: mk(nk=33, dk=1, n=128), b"33 k-bins"),
             (lambda: mk(nk=3), b"3 kmax = 3 (1 + 3 * 2) = 21 is above the grid of 16"), (lambda: mk(bin=2), b"k-bin 2 of 2"), (lambda: mk(bin=-1), b"k-bin -1 of 2"),
             (lambda: mk(fb=2), b"fields of 2 bytes"), (lambda: mk(y0=9, nyl=8), b"leave the grid"),
             (lambda: tr(real=None), b"null"), (lambda: tr(sums=None), b"null"), (lambda: tr(parts=None), b"null"), (lambda: tr(pair=None), b"null"), (lambda: tr(mx=None), b"null"),
             (lambda: tr(bad=None), b"null"), (lambda: tr(fb=16), b"fields of 16 bytes"), (lambda: tr(n=15), b"a grid of 15"), (lambda: tr(n=2048), b"a grid of 2048 is above 1024"),
             (lambda: tr(x0=10, nxl=7), b"leave the grid"), (lambda: tr(kmin=0), b"a kmin of 0"), (lambda: tr(nk=33), b"33 k-bins")]
    for call, what in calls:
        assert call() != 0
        err = L.pf_last_error()
        assert what in err and (b"pf_debug_bispec_mask" in err or b"pf_debug_bispec_triples" in err or b"pf_halo_bispectrum" in err), (what, err)
        assert "ERROR on task 0: pf_" in capfd.readouterr().out
        assert info.cells == 0xABCDEF and bad.value == 0xABCDEF and not any(bsum) and not any(km) and not any(mx)
    assert L.pf_bispectrum_triangles(0, 1, 1, None) == -1 and b"pf_bispectrum_triangles" in L.pf_last_error()
    assert L.pf_debug_bispec_times(None) != 0
