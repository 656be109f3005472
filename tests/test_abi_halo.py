"""CPU-side checks of the halo-power entry points: include/pinfmax.h declares them with the agreed signatures, struct and flags, the
library exports them, pinocchio_amd/_lib.py binds them with matching argument types and struct layout (held against the C
compiler's sizeof / offsetof through tests/cpu_emul/halo_emul.cpp), pinocchio_amd/api.py mirrors each one, and the refusals that
need no device come with a message before any device is touched."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["selected", "weight_sum", "weight2_hi", "weight2_lo", "nonfinite", "outside", "empty_cells", "max_cell", "modes", "nonfinite_modes"]

DECLARED = {
    "pf_halo_power": "pf_ctx *ctx, int flags, size_t count, const double *pos, double scale, const int *mass, int nbins, const int *mass_range, "
                     "unsigned long long *nmodes, unsigned long long *k2sum, double *power, double *cross, pf_halo_info *info",
    "pf_debug_halo_deposit": "int n, int x0, int nxl, int flags, size_t count, const double *pos, double scale, const int *mass, int lo, int hi, "
                             "unsigned long long *grid_host, pf_halo_info *info",
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
            "int": C.POINTER(C.c_int)}[base]


def test_the_header_declares_the_agreed_signatures_struct_and_flags(lib):
    hdr = open(os.path.join(ROOT, "include", "pinfmax.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, params in DECLARED.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in pinfmax.h"
        assert re.sub(r"\s+", " ", m.group(1)).strip() == params, name
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*pf_halo_info\s*;", hdr)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "unsigned long long " + ", ".join(FIELDS) + ";"
    for name, value in (("NGP", 1), ("DECONVOLVE", 2), ("MASS_WEIGHT", 4), ("MAX_BINS", 8)):
        assert re.search(r"#define\s+PF_HALO_%s\s+%d\b" % (name, value), hdr), name


def test_struct_size_offsets_and_flags_against_the_compiler(lib):
    from test_halo_cpu import build_emul
    E = build_emul()
    s = (C.c_size_t * 15)()
    assert E.halo_emul_sizes(s) == 15
    info = lib.HaloInfo
    assert list(s) == [C.sizeof(info)] + [getattr(info, k).offset for k in FIELDS] + [lib.HALO_NGP, lib.HALO_DECONVOLVE, lib.HALO_MASS_WEIGHT, lib.HALO_MAX_BINS]
    assert C.sizeof(info) == 80 and [f[0] for f in info._fields_] == FIELDS
    # the first two flags are the matter call's: the shell passes read them as such
    assert (lib.HALO_NGP, lib.HALO_DECONVOLVE) == (lib.MATTER_NGP, lib.MATTER_DECONVOLVE)


def test_the_library_exports_and_lib_py_binds_them(lib):
    L = lib.load()
    for name, params in DECLARED.items():
        assert hasattr(L, name), f"{name} is not exported"
        res, args = lib.PROTOTYPES[name]
        assert res is C.c_int, name
        assert args == [_ctype(lib, p) for p in params.split(",")], name


def test_api_py_mirrors_them(lib):
    from pinocchio_amd import api
    assert list(inspect.signature(api.Fmax.halo_power).parameters) == ["self", "pos", "mass", "ranges", "scale", "mass_weight", "cross", "ngp", "deconvolve", "box"]
    sig = inspect.signature(api.Fmax.halo_power).parameters
    assert (sig["scale"].default, sig["mass_weight"].default, sig["cross"].default, sig["ngp"].default, sig["deconvolve"].default, sig["box"].default) == \
        (1.0, False, True, False, False, None)
    assert list(inspect.signature(api.debug_halo_deposit).parameters) == ["n", "pos", "mass", "lo", "hi", "scale", "mass_weight", "ngp", "x0", "nxl"]
    for meth, call in ((api.Fmax.halo_power, "pf_halo_power"), (api.debug_halo_deposit, "pf_debug_halo_deposit"), (api.halo_times, "pf_debug_halo_times")):
        assert "." + call + "(" in inspect.getsource(meth), call
    assert (api.HALO_NGP, api.HALO_DECONVOLVE, api.HALO_MASS_WEIGHT, api.HALO_MAX_BINS) == (1, 2, 4, 8)
    assert api.halo_times() == (0.0, 0.0, 0.0, 0.0, 0.0) and len(api.HALO_TIME_KEYS) == 5
    with pytest.raises(ValueError):
        api.debug_halo_deposit(16, [[1.0, 2.0]], [1], 1, 2)


def test_refusals_that_need_no_device(lib, capfd):
    L = lib.load()
    info = lib.HaloInfo()
    info.selected = 0xABCDEF
    nb = L.pf_power_bins(16)
    nm, ks = (C.c_ulonglong * nb)(), (C.c_ulonglong * nb)()
    pw = (C.c_double * nb)()
    pos = (C.c_double * 6)(1.0, 2.0, 3.0, 4.0, 5.0, 6.0)
    mass = (C.c_int * 2)(10, 20)
    rng = (C.c_int * 2)(1, 100)
    grid = (C.c_ulonglong * 16 ** 3)()
    dep = lambda **k: L.pf_debug_halo_deposit(k.get("n", 16), k.get("x0", 0), k.get("nxl", 16), k.get("flags", 0), k.get("count", 2), k.get("pos", pos), k.get("scale", 1.0),
                                              k.get("mass", mass), k.get("lo", 1), k.get("hi", 100), k.get("grid", grid), k.get("info", C.byref(info)))
    calls = [(lambda: L.pf_halo_power(None, 0, 2, pos, 1.0, mass, 1, rng, nm, ks, pw, None, C.byref(info)), b"pf_halo_power: null argument"),
             (lambda: dep(pos=None), b"null"), (lambda: dep(mass=None), b"null"), (lambda: dep(grid=None), b"null"), (lambda: dep(info=None), b"null"),
             (lambda: dep(flags=8), b"unknown flag bits"), (lambda: dep(flags=-1), b"unknown flag bits"),
             (lambda: dep(lo=0), b"bin 0 takes the masses 0 to 100"), (lambda: dep(lo=5, hi=4), b"bin 0 takes the masses 5 to 4"),
             (lambda: dep(scale=0.0), b"a scale of 0"), (lambda: dep(scale=-1.0), b"a scale of -1"), (lambda: dep(scale=float("nan")), b"a scale of"),
             (lambda: dep(scale=float("inf")), b"a scale of inf"), (lambda: dep(count=2 ** 31 + 1), b"more than 2^31"),
             (lambda: dep(n=1), b"a grid of 1"), (lambda: dep(n=4096), b"a grid of 4096"), (lambda: dep(x0=-1), b"leave the grid"),
             (lambda: dep(x0=10, nxl=7), b"leave the grid"), (lambda: dep(nxl=0), b"leave the grid")]
    for call, what in calls:
        assert call() != 0
        assert what in L.pf_last_error(), (what, L.pf_last_error())
        assert "ERROR on task 0: pf_" in capfd.readouterr().out
        assert info.selected == 0xABCDEF and not any(grid[:64])
    assert L.pf_debug_halo_times(None) != 0
