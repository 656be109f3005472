"""CPU-side checks of the power-spectrum entry points: include/pinfmax.h declares them with the agreed signatures and struct, the
library exports them, pinocchio_amd/_lib.py binds them with matching argument types and struct layout (held against the C
compiler's sizeof / offsetof through tests/cpu_emul/power_emul.cpp), pinocchio_amd/api.py mirrors each one, and the null and range
refusals that need no device come with a message before any device is touched."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import np_power as npp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

DECLARED = {
    "pf_power_bins": "int n",
    "pf_power_spectrum": "pf_ctx *ctx, int which, int ns, const double *radius_cells, unsigned long long *nmodes, unsigned long long *k2sum, double *power, "
                         "double *variance, pf_power_info *info",
    "pf_debug_power_spectrum": "int field_bytes, int n, int y0, int nyl, const double *spec_host, int ns, const double *radius_cells, unsigned long long *nmodes, "
                               "unsigned long long *k2sum, double *power, double *variance, pf_power_info *info",
    "pf_debug_power_times": "double *ms",
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
    return {"pf_ctx": C.c_void_p, "double": C.POINTER(C.c_double), "unsigned long long": C.POINTER(C.c_ulonglong), "pf_power_info": C.POINTER(lib.PowerInfo)}[base]


def test_the_header_declares_the_agreed_signatures_and_struct(lib):
    hdr = open(os.path.join(ROOT, "include", "pinfmax.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, params in DECLARED.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in pinfmax.h"
        assert re.sub(r"\s+", " ", m.group(1)).strip() == params, name
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*pf_power_info\s*;", hdr)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "unsigned long long modes; unsigned long long nonfinite;"


def test_struct_size_and_offsets_against_the_compiler(lib):
    src, so = os.path.join(HERE, "cpu_emul", "power_emul.cpp"), os.path.join(HERE, "cpu_emul", "libpower_emul.so")
    deps = [src, os.path.join(ROOT, "include", "pinfmax.h"), os.path.join(ROOT, "pinocchio_amd", "csrc", "pf_power_core.h")]
    if not os.path.exists(so) or any(os.path.getmtime(so) < os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DPOWER_EMUL_LIB", "-o", so, src])
    E = C.CDLL(so)
    s = (C.c_size_t * 4)()
    assert E.power_emul_sizes(s) == 4
    info = lib.PowerInfo
    assert list(s) == [C.sizeof(info), info.modes.offset, info.nonfinite.offset, lib.MAX_SMOOTH]
    assert C.sizeof(info) == 16 and [f[0] for f in info._fields_] == ["modes", "nonfinite"]


def test_the_library_exports_and_lib_py_binds_them(lib):
    L = lib.load()
    for name, params in DECLARED.items():
        assert hasattr(L, name), f"{name} is not exported"
        res, args = lib.PROTOTYPES[name]
        assert res is C.c_int, name
        assert args == [_ctype(lib, p) for p in params.split(",")], name


def test_api_py_mirrors_them(lib):
    from pinocchio_amd import api
    assert list(inspect.signature(api.power_bins).parameters) == ["n"]
    assert list(inspect.signature(api.Fmax.power_spectrum).parameters) == ["self", "which", "radii_cells", "box"]
    assert inspect.signature(api.Fmax.power_spectrum).parameters["which"].default == "density"
    assert list(inspect.signature(api.debug_power_spectrum).parameters) == ["spec", "y0", "field_bytes", "radii_cells"]
    assert list(inspect.signature(api.power_times).parameters) == []
    for meth, call in ((api.power_bins, "pf_power_bins"), (api.Fmax.power_spectrum, "pf_power_spectrum"), (api.debug_power_spectrum, "pf_debug_power_spectrum"),
                       (api.power_times, "pf_debug_power_times")):
        assert "." + call + "(" in inspect.getsource(meth), call


def test_power_bins_needs_no_device(lib):
    from pinocchio_amd import api
    assert api.power_bins(16) == 15
    for n in (4, 20, 36, 48, 64, 1000, 1024, 2048):
        assert api.power_bins(n) == npp.bins(n)
    assert api.power_times() == 0.0


def test_refusals_that_need_no_device(lib, capfd):
    L = lib.load()
    info = lib.PowerInfo()
    nb = L.pf_power_bins(16)
    nm, ks = (C.c_ulonglong * nb)(), (C.c_ulonglong * nb)()
    pw, var = (C.c_double * nb)(), (C.c_double * 4)()
    spec = (C.c_double * (2 * 16 * 16 * 9))()
    r = (C.c_double * 2)(1.0, 2.0)
    many = (C.c_double * (lib.MAX_SMOOTH + 1))()
    big = (C.c_double * (lib.MAX_SMOOTH + 1))()
    dbg = lambda **k: L.pf_debug_power_spectrum(k.get("fb", 8), k.get("n", 16), k.get("y0", 0), k.get("nyl", 16), k.get("spec", spec), k.get("ns", 2), k.get("r", r),
                                                k.get("nm", nm), k.get("ks", ks), k.get("pw", pw), k.get("var", var), k.get("info", C.byref(info)))
    calls = [(lambda: L.pf_power_spectrum(None, 0, 0, None, nm, ks, pw, None, C.byref(info)), b"pf_power_spectrum"),
             (lambda: dbg(spec=None), b"null"), (lambda: dbg(nm=None), b"null"), (lambda: dbg(ks=None), b"null"), (lambda: dbg(pw=None), b"null"),
             (lambda: dbg(info=None), b"null"), (lambda: dbg(r=None), b"null radius_cells or variance"), (lambda: dbg(var=None), b"null radius_cells or variance"),
             (lambda: dbg(ns=-1), b"radii not in"), (lambda: dbg(ns=lib.MAX_SMOOTH + 1, r=many, var=big), b"radii not in"),
             (lambda: dbg(r=(C.c_double * 2)(1.0, -0.5)), b"negative or not finite"), (lambda: dbg(r=(C.c_double * 2)(float("nan"), 1.0)), b"negative or not finite"),
             (lambda: dbg(r=(C.c_double * 2)(1.0, float("inf"))), b"negative or not finite"),
             (lambda: dbg(fb=2), b"fields of 2 bytes"), (lambda: dbg(n=15), b"a grid of 15"), (lambda: dbg(n=4096), b"a grid of 4096"),
             (lambda: dbg(y0=9, nyl=8), b"leave the grid"), (lambda: dbg(nyl=0), b"leave the grid")]
    for call, what in calls:
        assert call() != 0
        assert what in L.pf_last_error(), (what, L.pf_last_error())
        assert "ERROR on task 0: pf_" in capfd.readouterr().out
    assert L.pf_debug_power_times(None) != 0
