"""CPU-side checks of the particle-state entry points: include/pinfmax.h declares them with the agreed signatures and struct, the
library exports them, pinocchio_amd/_lib.py binds them with matching argument types and struct layout, and pinocchio_amd/api.py
mirrors each one."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARED = {
    "pf_point_states": "pf_ctx *ctx, const pf_plc_segment *seg, const pf_peak_region *box, const pf_point_params *par, size_t count, const unsigned int *frag_pos, "
                       "const int *order, size_t capacity, unsigned int *index, void *states, size_t *found",
    "pf_debug_point_states": "int n, int x0, int nxl, int pb, const void *fmax_col, const void *cols24, pf_ctx *tables_ctx, const pf_plc_segment *seg, "
                             "const pf_peak_region *box, const pf_point_params *par, size_t count, const unsigned int *frag_pos, const int *order, unsigned int *index, "
                             "void *states, size_t *found",
    "pf_debug_point_times": "double *ms2",
}
STRUCTS = {"pf_point_params": "double sigma0, k_sigma, k_point; int order;"}


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
        return {"int": C.c_int, "size_t": C.c_size_t}[param.rsplit(" ", 1)[0]]
    base = param[:param.index("*")].replace("const", "").strip()
    return {"pf_ctx": (C.c_void_p,), "void": (C.c_void_p,), "unsigned int": (C.POINTER(C.c_uint),), "int": (C.POINTER(C.c_int),), "double": (C.POINTER(C.c_double),),
            "size_t": (C.POINTER(C.c_size_t),), "pf_peak_region": (C.POINTER(lib.PeakRegion),), "pf_plc_segment": (C.POINTER(lib.PlcSegment),),
            "pf_point_params": (C.POINTER(lib.PointParams),)}[base]


def test_the_header_declares_the_agreed_signatures_and_struct(lib):
    hdr = open(os.path.join(ROOT, "include", "pinfmax.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, params in DECLARED.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in pinfmax.h"
        assert re.sub(r"\s+", " ", m.group(1)).strip() == params, name
    for name, body in STRUCTS.items():
        m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % name, hdr)
        assert m and re.sub(r"\s+", " ", m.group(1)).strip() == body, name


def test_struct_size_and_fields(lib):
    assert (C.sizeof(C.c_double), C.sizeof(C.c_int)) == (8, 4)
    assert C.sizeof(lib.PointParams) == 32 and [f[0] for f in lib.PointParams._fields_] == ["sigma0", "k_sigma", "k_point", "order"]
    assert lib.PointParams.k_sigma.offset == 8 and lib.PointParams.k_point.offset == 16 and lib.PointParams.order.offset == 24


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
    sig = inspect.signature(api.Fmax.point_states)
    assert list(sig.parameters) == ["self", "myseg", "z_seg", "box", "frag_pos", "sigma0", "k_sigma", "k_point", "groups_order", "z_prev", "use_v31", "order", "capacity"]
    assert sig.parameters["groups_order"].default == 2                       # ORDER_FOR_GROUPS (src/pinocchio.h:75)
    sig = inspect.signature(api.debug_point_states)
    assert list(sig.parameters) == ["n", "x0", "fmax_col", "cols24", "tables", "myseg", "z_seg", "box", "frag_pos", "sigma0", "k_sigma", "k_point", "groups_order", "z_prev",
                                    "use_v31", "order"]
    for meth, call in ((api.Fmax.point_states, "pf_point_states"), (api.debug_point_states, "pf_debug_point_states"), (api.point_times, "pf_debug_point_times")):
        assert "." + call + "(" in inspect.getsource(meth), call
    assert api.point_times() == (0.0, 0.0) or all(t >= 0.0 for t in api.point_times())


def test_the_unit_is_built_without_contraction():
    mk = open(os.path.join(ROOT, "pinocchio_amd", "csrc", "Makefile")).read()
    assert re.search(r"pf_points\.o: pf_points\.hip.*\n\t\$\(HIPCC\) \$\(BASEFLAGS\) -ffp-contract=off ", mk)
    assert " pf_points " in mk and " pf_points_core.h " in mk
