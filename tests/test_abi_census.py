"""CPU-side checks of the arithmetic setting and the census entry points: include/pinfmax.h declares them with the agreed signatures
and structs, the library exports them, pinocchio_amd/_lib.py binds them with matching argument types and struct layouts (held
against the C compiler's sizeof / offsetof through tests/cpu_emul/census_emul.cpp), pinocchio_amd/api.py mirrors each one, and
null arguments are refused with a message before any device is touched."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

DECLARED = {
    "pf_set_arithmetic": "pf_ctx *ctx, int flavour",
    "pf_get_arithmetic": "pf_ctx *ctx",
    "pf_flavour_census": "pf_ctx *ctx, int ns, const double *radius_cells, double *true_variance, pf_census *out, size_t capacity, pf_census_cell *cells",
    "pf_debug_census": "int product_bytes, unsigned long long first_cell, size_t count, const void *fmax_fast, const int *rmax_fast, const void *fmax_exact, "
                       "const int *rmax_exact, pf_census *out, size_t capacity, pf_census_cell *cells",
}
CENSUS_FIELDS = ["cells", "differing_bits", "hist", "beyond_2ulp", "rmax_differing", "nonfinite", "outliers", "max_abs", "max_ulps", "max_abs_cell"]


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
        return {"int": C.c_int, "size_t": C.c_size_t, "unsigned long long": C.c_ulonglong}[param.rsplit(" ", 1)[0]]
    base = param[:param.index("*")].replace("const", "").strip()
    return {"pf_ctx": C.c_void_p, "void": C.c_void_p, "int": C.POINTER(C.c_int), "double": C.POINTER(C.c_double), "pf_census": C.POINTER(lib.Census),
            "pf_census_cell": C.POINTER(lib.CensusCell)}[base]


def test_the_header_declares_the_agreed_signatures_and_structs(lib):
    hdr = open(os.path.join(ROOT, "include", "pinfmax.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, params in DECLARED.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in pinfmax.h"
        assert re.sub(r"\s+", " ", m.group(1)).strip() == params, name
    assert re.search(r"enum\s*\{\s*PF_ARITH_FAST\s*=\s*0\s*,\s*PF_ARITH_EXACT\s*=\s*1\s*\}\s*;", hdr)
    assert re.search(r"#define\s+PF_CENSUS_BINS\s+64\b", hdr)
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*pf_census\s*;", hdr)
    assert m and re.findall(r"(\w+)(?:\[PF_CENSUS_BINS\])?\s*[;,]", m.group(1)) == CENSUS_FIELDS
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*pf_census_cell\s*;", hdr)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "unsigned long long cell; double fast, exact; int rmax_fast, rmax_exact;"
    assert (lib.ARITH_FAST, lib.ARITH_EXACT, lib.CENSUS_BINS) == (0, 1, 64)


def test_struct_sizes_and_offsets_against_the_compiler(lib):
    src, so = os.path.join(HERE, "cpu_emul", "census_emul.cpp"), os.path.join(HERE, "cpu_emul", "libcensus_emul.so")
    deps = [src, os.path.join(ROOT, "include", "pinfmax.h"), os.path.join(ROOT, "pinocchio_amd", "csrc", "pf_census_core.h")]
    if not os.path.exists(so) or any(os.path.getmtime(so) < os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DCENSUS_EMUL_LIB", "-o", so, src])
    E = C.CDLL(so)
    s = (C.c_size_t * 9)()
    assert E.census_emul_sizes(s) == 9
    cen, cell = lib.Census, lib.CensusCell
    assert list(s) == [C.sizeof(cen), C.sizeof(cell), cen.hist.offset, cen.beyond_2ulp.offset, cen.max_abs.offset, cen.max_abs_cell.offset, cell.fast.offset,
                       cell.rmax_fast.offset, cell.rmax_exact.offset]
    assert C.sizeof(cen) == 8 * (2 + 64 + 4 + 3) and C.sizeof(cell) == 32 and [f[0] for f in cen._fields_] == CENSUS_FIELDS
    assert [f[0] for f in cell._fields_] == ["cell", "fast", "exact", "rmax_fast", "rmax_exact"]
    from pinocchio_amd import api
    assert api.CENSUS_CELL_DTYPE.itemsize == 32 and [api.CENSUS_CELL_DTYPE.fields[f[0]][1] for f in cell._fields_] == [getattr(cell, f[0]).offset for f in cell._fields_]


def test_the_library_exports_and_lib_py_binds_them(lib):
    L = lib.load()
    for name, params in DECLARED.items():
        assert hasattr(L, name), f"{name} is not exported"
        res, args = lib.PROTOTYPES[name]
        assert res is C.c_int, name
        assert args == [_ctype(lib, p) for p in params.split(",")], name


def test_api_py_mirrors_them(lib):
    from pinocchio_amd import api
    assert list(inspect.signature(api.Fmax.set_arithmetic).parameters) == ["self", "flavour"]
    assert isinstance(api.Fmax.arithmetic, property)
    assert list(inspect.signature(api.Fmax.flavour_census).parameters) == ["self", "radii_cells", "capacity"]
    assert list(inspect.signature(api.debug_census).parameters) == ["fmax_fast", "rmax_fast", "fmax_exact", "rmax_exact", "first_cell", "capacity"]
    for meth, call in ((api.Fmax.set_arithmetic, "pf_set_arithmetic"), (api.Fmax.arithmetic.fget, "pf_get_arithmetic"), (api.Fmax.flavour_census, "pf_flavour_census"),
                       (api.debug_census, "pf_debug_census")):
        assert "." + call + "(" in inspect.getsource(meth), call


def test_null_arguments_are_refused_with_a_message(lib, capfd):
    L = lib.load()
    out = lib.Census()
    r = (C.c_double * 1)(0.0)
    one = (C.c_int * 1)(0)
    f = (C.c_float * 1)(0.0)
    assert L.pf_get_arithmetic(None) == -1
    for call, what in ((lambda: L.pf_set_arithmetic(None, 0), b"pf_set_arithmetic"),
                       (lambda: L.pf_flavour_census(None, 1, r, None, C.byref(out), 0, None), b"pf_flavour_census"),
                       (lambda: L.pf_debug_census(4, 0, 1, f, one, f, one, None, 0, None), b"pf_debug_census"),
                       (lambda: L.pf_debug_census(4, 0, 1, None, one, f, one, C.byref(out), 0, None), b"pf_debug_census"),
                       (lambda: L.pf_debug_census(4, 0, 1, f, one, f, one, C.byref(out), 3, None), b"pf_debug_census"),
                       (lambda: L.pf_debug_census(2, 0, 1, f, one, f, one, C.byref(out), 0, None), b"pf_debug_census")):
        assert call() != 0
        assert what in L.pf_last_error()
        assert "ERROR on task 0: " + what.decode() in capfd.readouterr().out


def test_census_sum_adds_counts_and_takes_maxima(lib):
    from pinocchio_amd import api
    import np_census as npc
    import census_cases as cc
    f, e, rf, re = cc.random_columns(np.float32, count=3000, frac=0.05)
    whole, _ = npc.census(f, e, rf, re)
    for cuts in ((1000, 2000), (1, 2999), (1500,)):
        parts = [npc.census(*(a[lo:hi] for a in (f, e, rf, re)))[0] for lo, hi in zip((0,) + cuts, cuts + (3000,))]
        assert npc.same(api.census_sum(parts), whole) is None, (cuts, npc.same(api.census_sum(parts), whole))
    # a rank without a finite cell takes no part in the maxima
    nanpart = npc.census(np.full(4, np.nan, np.float32), np.full(4, np.inf, np.float32), np.zeros(4, np.int32), np.zeros(4, np.int32))[0]
    got = api.census_sum([nanpart, whole])
    assert got["max_abs_cell"] == 4 + whole["max_abs_cell"] and got["max_abs"] == whole["max_abs"] and got["nonfinite"] == whole["nonfinite"] + 4
    assert api.census_sum([nanpart])["max_abs_cell"] == npc.NOCELL
