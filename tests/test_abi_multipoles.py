"""CPU-side checks of the multipole entry points: include/pinfmax.h declares them with the agreed signatures and constants, the
library exports them, pinocchio_amd/_lib.py binds them with matching argument types, pinocchio_amd/api.py mirrors each one, the core
header and the public header agree on the number of sums (through tests/cpu_emul/multipole_emul.cpp), and the refusals that need no
device come with a message before any device is touched."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARED = {
    "pf_halo_multipoles": "pf_ctx *ctx, int flags, size_t count, const double *pos, const double *vel, double scale, double vfac, int los, const int *mass, int nbins, "
                          "const int *mass_range, unsigned long long *nmodes, unsigned long long *k2sum, double *power, double *cross, pf_halo_info *info",
    "pf_debug_halo_deposit_rsd": "int n, int x0, int nxl, int flags, size_t count, const double *pos, const double *vel, double scale, double vfac, int los, const int *mass, "
                                 "int lo, int hi, unsigned long long *grid_host, pf_halo_info *info",
    "pf_debug_multipole_shells": "int field_bytes, int n, int y0, int nyl, const double *spec_m, const double *spec_lin, int flags, int los, unsigned long long *nmodes, "
                                 "unsigned long long *k2sum, double *power, double *cross, double *parts, pf_matter_info *info",
    "pf_debug_multipole_form": "int *form",
}
# what the issue forbids to touch
UNCHANGED = {
    "pf_halo_power": "pf_ctx *ctx, int flags, size_t count, const double *pos, double scale, const int *mass, int nbins, const int *mass_range, "
                     "unsigned long long *nmodes, unsigned long long *k2sum, double *power, double *cross, pf_halo_info *info",
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
            "pf_matter_info": C.POINTER(lib.MatterInfo), "int": C.POINTER(C.c_int)}[base]


def test_the_header_declares_the_agreed_signatures_and_constants(lib):
    hdr = open(os.path.join(ROOT, "include", "pinfmax.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, params in list(DECLARED.items()) + list(UNCHANGED.items()):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in pinfmax.h"
        assert re.sub(r"\s+", " ", m.group(1)).strip() == params, name
    assert re.search(r"#define\s+PF_MULTIPOLE_ORDERS\s+3\b", hdr) and re.search(r"#define\s+PF_MULTIPOLE_SUMS\s+11\b", hdr)
    for name, value in (("NGP", 1), ("DECONVOLVE", 2), ("MASS_WEIGHT", 4), ("MAX_BINS", 8)):
        assert re.search(r"#define\s+PF_HALO_%s\s+%d\b" % (name, value), hdr), name


def test_the_constants_against_the_compiler(lib):
    from test_multipoles_cpu import build_emul
    E = build_emul()
    s = (C.c_size_t * 6)()
    assert E.multipole_emul_sizes(s) == 6
    assert list(s) == [lib.MULTIPOLE_ORDERS, lib.MULTIPOLE_SUMS, 11, 5, C.sizeof(lib.HaloInfo), C.sizeof(lib.MatterInfo)]


def test_the_library_exports_and_lib_py_binds_them(lib):
    L = lib.load()
    for name, params in DECLARED.items():
        assert hasattr(L, name), f"{name} is not exported"
        res, args = lib.PROTOTYPES[name]
        assert res is C.c_int, name
        assert args == [_ctype(lib, p) for p in params.split(",")], name


def test_api_py_mirrors_them(lib):
    from pinocchio_amd import api
    sig = inspect.signature(api.Fmax.halo_multipoles).parameters
    assert list(sig) == ["self", "pos", "vel", "mass", "ranges", "scale", "vfac", "los", "mass_weight", "cross", "ngp", "deconvolve", "box"]
    assert [sig[k].default for k in list(sig)[5:]] == [1.0, 0.0, 2, False, True, False, False, None]
    assert list(inspect.signature(api.debug_halo_deposit_rsd).parameters) == ["n", "pos", "vel", "mass", "lo", "hi", "scale", "vfac", "los", "mass_weight", "ngp", "x0", "nxl"]
    assert list(inspect.signature(api.debug_multipole_shells).parameters) == ["spec_m", "spec_lin", "y0", "field_bytes", "ngp", "deconvolve", "los"]
    for meth, call in ((api.Fmax.halo_multipoles, "pf_halo_multipoles"), (api.debug_halo_deposit_rsd, "pf_debug_halo_deposit_rsd"),
                       (api.debug_multipole_shells, "pf_debug_multipole_shells"), (api.multipole_form, "pf_debug_multipole_form")):
        assert "." + call + "(" in inspect.getsource(meth), call
    assert (api.MULTIPOLE_ORDERS, api.MULTIPOLE_SUMS) == (3, 11)
    assert api.multipole_form() == (0, 0)                                    # nothing launched by this thread yet
    with pytest.raises(ValueError):
        api.debug_halo_deposit_rsd(16, [[1.0, 2.0, 3.0]], [[1.0, 2.0]], [1], 1, 2)
    with pytest.raises(ValueError):
        api.debug_multipole_shells([[[1.0, 2.0]]])


def test_refusals_that_need_no_device(lib, capfd):
    L = lib.load()
    info = lib.HaloInfo()
    info.selected = 0xABCDEF
    minfo = lib.MatterInfo()
    minfo.modes = 0xABCDEF
    n = 16
    nb = L.pf_power_bins(n)
    nm, ks = (C.c_ulonglong * nb)(), (C.c_ulonglong * nb)()
    pw, cr, parts = (C.c_double * (3 * nb))(), (C.c_double * (3 * nb))(), (C.c_double * (11 * nb))()
    pos = (C.c_double * 6)(1.0, 2.0, 3.0, 4.0, 5.0, 6.0)
    vel = (C.c_double * 6)(1.0, 2.0, 3.0, 4.0, 5.0, 6.0)
    mass = (C.c_int * 2)(10, 20)
    rng = (C.c_int * 2)(1, 100)
    grid = (C.c_ulonglong * n ** 3)()
    spec = (C.c_double * (2 * n * n * (n // 2 + 1)))()
    dep = lambda **k: L.pf_debug_halo_deposit_rsd(k.get("n", n), k.get("x0", 0), k.get("nxl", n), k.get("flags", 0), k.get("count", 2), k.get("pos", pos), k.get("vel", vel),
                                                  k.get("scale", 1.0), k.get("vfac", 0.5), k.get("los", 2), k.get("mass", mass), k.get("lo", 1), k.get("hi", 100),
                                                  k.get("grid", grid), k.get("info", C.byref(info)))
    sh = lambda **k: L.pf_debug_multipole_shells(k.get("fb", 8), k.get("n", n), k.get("y0", 0), k.get("nyl", n), k.get("m", spec), k.get("lin", spec), k.get("flags", 0),
                                                 k.get("los", 2), k.get("nm", nm), k.get("ks", ks), k.get("pw", pw), k.get("cr", cr), k.get("parts", parts),
                                                 k.get("info", C.byref(minfo)))
    calls = [(lambda: L.pf_halo_multipoles(None, 0, 2, pos, vel, 1.0, 0.5, 2, mass, 1, rng, nm, ks, pw, None, C.byref(info)), b"pf_halo_multipoles: null argument"),
             (lambda: dep(pos=None), b"null"), (lambda: dep(mass=None), b"null"), (lambda: dep(grid=None), b"null"), (lambda: dep(info=None), b"null"),
             (lambda: dep(flags=8), b"unknown flag bits"), (lambda: dep(lo=0), b"bin 0 takes the masses 0 to 100"), (lambda: dep(scale=0.0), b"a scale of 0"),
             (lambda: dep(count=2 ** 31 + 1), b"more than 2^31"), (lambda: dep(n=1), b"a grid of 1"), (lambda: dep(x0=10, nxl=7), b"leave the grid"),
             (lambda: dep(los=3), b"a line of sight along axis 3"), (lambda: dep(los=-1), b"a line of sight along axis -1"),
             (lambda: dep(vfac=float("nan")), b"a vfac of"), (lambda: dep(vfac=float("inf")), b"a vfac of inf"), (lambda: dep(vfac=float("-inf")), b"a vfac of -inf"),
             (lambda: dep(vel=None), b"a vfac of 0.5 without velocities"),
             (lambda: sh(m=None), b"null"), (lambda: sh(nm=None), b"null"), (lambda: sh(ks=None), b"null"), (lambda: sh(pw=None), b"null"), (lambda: sh(info=None), b"null"),
             (lambda: sh(flags=4), b"unknown flag bits"), (lambda: sh(los=3), b"a line of sight along axis 3"), (lambda: sh(los=-2), b"a line of sight along axis -2"),
             (lambda: sh(lin=None), b"cross sums without a second spectrum"), (lambda: sh(fb=2), b"fields of 2 bytes"), (lambda: sh(n=15), b"a grid of 15"),
             (lambda: sh(y0=9, nyl=8), b"leave the grid")]
    for call, what in calls:
        assert call() != 0
        err = L.pf_last_error()
        assert what in err and (b"pf_debug_halo_deposit_rsd" in err or b"pf_debug_multipole_shells" in err or b"pf_halo_multipoles" in err), (what, err)
        assert "ERROR on task 0: pf_" in capfd.readouterr().out
        assert info.selected == 0xABCDEF and minfo.modes == 0xABCDEF and not any(grid[:64]) and not any(pw[:8])
    assert L.pf_debug_multipole_form(None) != 0
