"""CPU-side checks of the velocity-refresh entry points: include/pinfmax.h declares them with the agreed signatures, the library
exports them, pinocchio_amd/_lib.py binds them with matching argument types and pinocchio_amd/api.py mirrors each one."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> the parameter list of the declaration, whitespace normalised
DECLARED = {
    "pf_shift_displacements": "pf_ctx *ctx",
    "pf_drop_prev": "pf_ctx *ctx",
    "pf_prev_shifts": "pf_ctx *ctx",
    "pf_gather_velocities": "pf_ctx *ctx, const pf_peak_region *box, size_t count, const unsigned int *frag_pos, const int *order, size_t capacity, "
                            "unsigned int *index, void *vel24, size_t *found",
    "pf_refresh_velocities": "pf_ctx *ctx, const pf_peak_region *box, size_t count, const unsigned int *frag_pos, const int *order, void *frag, "
                             "const pf_product_layout *layout, const pf_prev_layout *prev, size_t *found",
    "pf_debug_gather_velocities": "int n, int x0, int nxl, int pb, const void *cols24, const pf_peak_region *box, size_t count, const unsigned int *frag_pos, "
                                  "const int *order, unsigned int *index, void *vel24, size_t *found",
}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "pinocchio_amd", "libpinfmax_hip.so")):
        g.build()
    from pinocchio_amd import _lib
    return _lib


def _ctype(lib, param):
    """the ctypes type _lib.py must bind a C parameter with"""
    param = param.strip()
    if "*" not in param:
        return {"int": C.c_int, "size_t": C.c_size_t}[param.rsplit(" ", 1)[0]]
    base = param[:param.index("*")].replace("const", "").strip()
    return {"pf_ctx": (C.c_void_p,), "void": (C.c_void_p,), "unsigned int": (C.POINTER(C.c_uint), C.c_void_p), "int": (C.POINTER(C.c_int), C.c_void_p),
            "size_t": (C.POINTER(C.c_size_t),), "pf_peak_region": (C.POINTER(lib.PeakRegion),), "pf_product_layout": (C.POINTER(lib.ProductLayout),),
            "pf_prev_layout": (C.POINTER(lib.PrevLayout),)}[base]


def test_the_header_declares_the_agreed_signatures(lib):
    hdr = open(os.path.join(ROOT, "include", "pinfmax.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, params in DECLARED.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in pinfmax.h"
        assert re.sub(r"\s+", " ", m.group(1)).strip() == params, name
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*pf_prev_layout\s*;", hdr)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "int off_Vel_prev, off_Vel_2LPT_prev, off_Vel_3LPT_1_prev, off_Vel_3LPT_2_prev;"
    # pf_product_layout keeps its size: the prev offsets travel in a struct of their own
    assert C.sizeof(lib.ProductLayout) == 32 and C.sizeof(lib.PrevLayout) == 16
    assert [f[0] for f in lib.PrevLayout._fields_] == ["off_Vel_prev", "off_Vel_2LPT_prev", "off_Vel_3LPT_1_prev", "off_Vel_3LPT_2_prev"]


def test_the_library_exports_and_lib_py_binds_them(lib):
    L = lib.load()
    for name, params in DECLARED.items():
        assert hasattr(L, name), f"{name} is not exported"
        res, args = lib.PROTOTYPES[name]
        assert res is C.c_int, name
        want = [_ctype(lib, p) for p in params.split(",")]
        assert len(args) == len(want), name
        for k, (a, w) in enumerate(zip(args, want)):
            assert a in w if isinstance(w, tuple) else a is w, (name, k)


def test_api_py_mirrors_them(lib):
    from pinocchio_amd import api
    F = api.Fmax
    assert list(inspect.signature(F.shift_displacements).parameters) == ["self"]
    assert list(inspect.signature(F.drop_prev).parameters) == ["self"]
    assert isinstance(F.prev_shifts, property)
    sig = inspect.signature(F.gather_velocities)
    assert list(sig.parameters)[:4] == ["self", "box", "frag_pos", "order"] and sig.parameters["order"].default is None
    sig = inspect.signature(F.refresh_velocities)
    assert list(sig.parameters) == ["self", "box", "frag_pos", "frag", "layout", "prev", "order"]
    assert sig.parameters["prev"].default is None and sig.parameters["order"].default is None
    assert callable(api.debug_gather_velocities) and "order" in inspect.signature(api.debug_gather_velocities).parameters
    p = api.prev_layout(56, 68)
    assert (p.off_Vel_prev, p.off_Vel_2LPT_prev, p.off_Vel_3LPT_1_prev, p.off_Vel_3LPT_2_prev) == (56, 68, -1, -1)
    # the source of each method names the call it wraps
    for meth, call in ((F.shift_displacements, "pf_shift_displacements"), (F.drop_prev, "pf_drop_prev"), (F.gather_velocities, "pf_gather_velocities"),
                       (F.refresh_velocities, "pf_refresh_velocities"), (api.debug_gather_velocities, "pf_debug_gather_velocities")):
        assert "L." + call + "(" in inspect.getsource(meth), call
    assert "pf_prev_shifts" in inspect.getsource(F.prev_shifts.fget)
