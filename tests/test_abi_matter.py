"""CPU-side checks of the matter-density entry points: include/pinfmax.h declares them with the agreed signatures and struct, the
library exports them, pinocchio_amd/_lib.py binds them with matching argument types and struct layout (held against the C
compiler's sizeof / offsetof through tests/cpu_emul/matter_emul.cpp), pinocchio_amd/api.py mirrors each one, and the refusals that
need no device come with a message before any device is touched."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["deposited", "nonfinite", "outside", "empty_cells", "max_cell", "sum_hi32", "sum_lo32", "modes", "nonfinite_modes"]

DECLARED = {
    "pf_matter_power": "pf_ctx *ctx, int flags, const double *weight, unsigned long long *nmodes, unsigned long long *k2sum, double *power, double *cross, "
                       "double *density_host, pf_matter_info *info",
    "pf_debug_matter_deposit": "int pb, int n, const void *vel12_host, int flags, const double *weight, unsigned long long *grid_host, pf_matter_info *info",
    "pf_debug_matter_shells": "int field_bytes, int n, int y0, int nyl, const double *spec_m, const double *spec_lin, int flags, unsigned long long *nmodes, "
                              "unsigned long long *k2sum, double *power, double *cross, pf_matter_info *info",
    "pf_debug_matter_times": "double *ms",
    "pf_debug_matter_form": "int *form",
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
        return {"int": C.c_int}[param.rsplit(" ", 1)[0]]
    base = param[:param.index("*")].replace("const", "").strip()
    return {"pf_ctx": C.c_void_p, "void": C.c_void_p, "double": C.POINTER(C.c_double), "unsigned long long": C.POINTER(C.c_ulonglong),
            "pf_matter_info": C.POINTER(lib.MatterInfo), "int": C.POINTER(C.c_int)}[base]


def test_the_header_declares_the_agreed_signatures_and_struct(lib):
    hdr = open(os.path.join(ROOT, "include", "pinfmax.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, params in DECLARED.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in pinfmax.h"
        assert re.sub(r"\s+", " ", m.group(1)).strip() == params, name
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*pf_matter_info\s*;", hdr)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "unsigned long long " + ", ".join(FIELDS) + ";"
    assert re.search(r"#define\s+PF_MATTER_NGP\s+1\b", hdr) and re.search(r"#define\s+PF_MATTER_DECONVOLVE\s+2\b", hdr)


def test_struct_size_and_offsets_against_the_compiler(lib):
    from test_matter_cpu import build_emul
    E = build_emul()
    s = (C.c_size_t * 12)()
    assert E.matter_emul_sizes(s) == 12
    info = lib.MatterInfo
    assert list(s) == [C.sizeof(info)] + [getattr(info, k).offset for k in FIELDS] + [lib.MATTER_NGP, lib.MATTER_DECONVOLVE]
    assert C.sizeof(info) == 72 and [f[0] for f in info._fields_] == FIELDS


def test_the_library_exports_and_lib_py_binds_them(lib):
    L = lib.load()
    for name, params in DECLARED.items():
        assert hasattr(L, name), f"{name} is not exported"
        res, args = lib.PROTOTYPES[name]
        assert res is C.c_int, name
        assert args == [_ctype(lib, p) for p in params.split(",")], name


def test_api_py_mirrors_them(lib):
    from pinocchio_amd import api
    assert list(inspect.signature(api.Fmax.matter_power).parameters) == ["self", "weight", "cross", "density", "ngp", "deconvolve", "box"]
    assert list(inspect.signature(api.debug_matter_deposit).parameters) == ["vel12", "ngp", "weight"]
    assert list(inspect.signature(api.debug_matter_shells).parameters) == ["spec_m", "spec_lin", "y0", "field_bytes", "ngp", "deconvolve"]
    assert list(inspect.signature(api.matter_times).parameters) == []
    assert list(inspect.signature(api.matter_form).parameters) == [] and len(api.matter_form()) == 2
    for meth, call in ((api.Fmax.matter_power, "pf_matter_power"), (api.debug_matter_deposit, "pf_debug_matter_deposit"),
                       (api.debug_matter_shells, "pf_debug_matter_shells"), (api.matter_times, "pf_debug_matter_times"), (api.matter_form, "pf_debug_matter_form")):
        assert "." + call + "(" in inspect.getsource(meth), call
    assert (api.MATTER_NGP, api.MATTER_DECONVOLVE) == (1, 2) and api.matter_times() == (0.0, 0.0, 0.0, 0.0)


def test_refusals_that_need_no_device(lib, capfd):
    L = lib.load()
    info = lib.MatterInfo()
    nb = L.pf_power_bins(16)
    nm, ks = (C.c_ulonglong * nb)(), (C.c_ulonglong * nb)()
    pw, cr = (C.c_double * nb)(), (C.c_double * nb)()
    spec = (C.c_double * (2 * 16 * 16 * 9))()
    cols = (C.c_float * (12 * 8 ** 3))()
    grid = (C.c_ulonglong * 8 ** 3)()
    w = (C.c_double * 4)(1.0, 1.0, 1.0, 1.0)
    nan_w, inf_w = (C.c_double * 4)(1.0, float("nan"), 0.0, 0.0), (C.c_double * 4)(1.0, 0.0, 0.0, float("inf"))
    dep = lambda **k: L.pf_debug_matter_deposit(k.get("pb", 4), k.get("n", 8), k.get("cols", cols), k.get("flags", 0), k.get("w", w), k.get("grid", grid),
                                                k.get("info", C.byref(info)))
    sh = lambda **k: L.pf_debug_matter_shells(k.get("fb", 8), k.get("n", 16), k.get("y0", 0), k.get("nyl", 16), k.get("m", spec), k.get("lin", spec), k.get("flags", 0),
                                              k.get("nm", nm), k.get("ks", ks), k.get("pw", pw), k.get("cr", cr), k.get("info", C.byref(info)))
    calls = [(lambda: L.pf_matter_power(None, 0, None, nm, ks, pw, None, None, C.byref(info)), b"pf_matter_power: null argument"),
             (lambda: dep(cols=None), b"null"), (lambda: dep(grid=None), b"null"), (lambda: dep(info=None), b"null"), (lambda: dep(flags=4), b"unknown flag bits"),
             (lambda: dep(w=nan_w), b"weight 1 is not finite"), (lambda: dep(w=inf_w), b"weight 3 is not finite"), (lambda: dep(pb=2), b"products of 2 bytes"),
             (lambda: dep(n=1), b"a grid of 1"), (lambda: dep(n=1024), b"a grid of 1024"),
             (lambda: sh(m=None), b"null"), (lambda: sh(nm=None), b"null"), (lambda: sh(ks=None), b"null"), (lambda: sh(pw=None), b"null"), (lambda: sh(info=None), b"null"),
             (lambda: sh(flags=8), b"unknown flag bits"), (lambda: sh(lin=None), b"cross sums without a second spectrum"), (lambda: sh(fb=2), b"fields of 2 bytes"),
             (lambda: sh(n=15), b"a grid of 15"), (lambda: sh(n=4096), b"a grid of 4096"), (lambda: sh(y0=9, nyl=8), b"leave the grid"), (lambda: sh(nyl=0), b"leave the grid")]
    for call, what in calls:
        assert call() != 0
        assert what in L.pf_last_error(), (what, L.pf_last_error())
        assert "ERROR on task 0: pf_" in capfd.readouterr().out
    assert L.pf_debug_matter_times(None) != 0 and L.pf_debug_matter_form(None) != 0
