"""CPU-side checks of the group-velocity entry points: include/pinfmax.h declares them with the agreed signatures, the library
exports them, pinocchio_amd/_lib.py binds them with matching argument types and pinocchio_amd/api.py mirrors each one."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> the parameter list of the declaration, whitespace normalised
DECLARED = {
    "pf_group_velocity_sums": "pf_ctx *ctx, const pf_peak_region *box, size_t count, const unsigned int *frag_pos, const int *group_id, size_t group_stride, "
                              "int first_group, size_t capacity, int *group, unsigned int *npart, double *sum24, size_t *groups_found, size_t *particles_found",
    "pf_refresh_segment": "pf_ctx *ctx, const pf_peak_region *box, size_t count, const unsigned int *frag_pos, const int *order, const int *group_id, "
                          "size_t group_stride, int first_group, void *frag, const pf_product_layout *layout, const pf_prev_layout *prev, void *groups, "
                          "size_t ngroups, const pf_group_layout *gl, size_t *loose, size_t *grouped, size_t *mass_mismatch",
    "pf_debug_group_velocity_sums": "int n, int x0, int nxl, int pb, const void *cols24, const pf_peak_region *box, size_t count, const unsigned int *frag_pos, "
                                    "const int *group_id, int first_group, int *group, unsigned int *npart, double *sum24, size_t *groups_found, "
                                    "size_t *particles_found",
}
GROUP_FIELDS = ["stride", "off_Mass", "off_Vel", "off_Vel_2LPT", "off_Vel_3LPT_1", "off_Vel_3LPT_2", "off_Vel_prev", "off_Vel_2LPT_prev", "off_Vel_3LPT_1_prev",
                "off_Vel_3LPT_2_prev"]


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
            "double": (C.POINTER(C.c_double),), "size_t": (C.POINTER(C.c_size_t),), "pf_peak_region": (C.POINTER(lib.PeakRegion),),
            "pf_product_layout": (C.POINTER(lib.ProductLayout),), "pf_prev_layout": (C.POINTER(lib.PrevLayout),),
            "pf_group_layout": (C.POINTER(lib.GroupLayout),)}[base]


def test_the_header_declares_the_agreed_signatures(lib):
    hdr = open(os.path.join(ROOT, "include", "pinfmax.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, params in DECLARED.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in pinfmax.h"
        assert re.sub(r"\s+", " ", m.group(1)).strip() == params, name
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*pf_group_layout\s*;", hdr)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "size_t stride; long " + ", ".join(GROUP_FIELDS[1:]) + ";"
    # a size_t and nine longs; the layouts of the refresh keep their sizes
    assert C.sizeof(lib.GroupLayout) == C.sizeof(C.c_size_t) + 9 * C.sizeof(C.c_long) and C.sizeof(lib.ProductLayout) == 32 and C.sizeof(lib.PrevLayout) == 16
    assert [f[0] for f in lib.GroupLayout._fields_] == GROUP_FIELDS
    assert lib.GroupLayout._fields_[0][1] is C.c_size_t and all(f[1] is C.c_long for f in lib.GroupLayout._fields_[1:])


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
    sig = inspect.signature(F.group_velocity_sums)
    assert list(sig.parameters) == ["self", "box", "frag_pos", "group_id", "first_group", "capacity"]
    assert sig.parameters["first_group"].default == 2 and sig.parameters["capacity"].default is None       # FILAMENT + 1
    sig = inspect.signature(F.refresh_segment)
    assert list(sig.parameters) == ["self", "box", "frag_pos", "group_id", "frag", "layout", "prev", "groups", "ngroups", "group_layout", "order", "first_group"]
    assert all(sig.parameters[p].default is None for p in ("frag", "layout", "prev", "groups", "group_layout", "order")) and sig.parameters["first_group"].default == 2
    sig = inspect.signature(api.debug_group_velocity_sums)
    assert list(sig.parameters) == ["n", "x0", "cols24", "box", "frag_pos", "group_id", "first_group"] and sig.parameters["first_group"].default == 2
    g = api.group_layout(112, 4, 8, 20)
    assert (g.stride, g.off_Mass, g.off_Vel, g.off_Vel_2LPT, g.off_Vel_3LPT_1, g.off_Vel_3LPT_2_prev) == (112, 4, 8, 20, -1, -1)
    g = api.group_layout(64, off_Vel_prev=40)
    assert (g.off_Mass, g.off_Vel, g.off_Vel_prev) == (-1, -1, 40)
    # the source of each method names the call it wraps
    for meth, call in ((F.group_velocity_sums, "pf_group_velocity_sums"), (F.refresh_segment, "pf_refresh_segment"),
                       (api.debug_group_velocity_sums, "pf_debug_group_velocity_sums")):
        assert "L." + call + "(" in inspect.getsource(meth), call


def test_pf_compat_wraps_nothing_of_it():
    """recompute_group_velocities() lives in fragment.o: the reference-named host layer has no business with it"""
    src = open(os.path.join(ROOT, "pinocchio_amd", "host", "pf_compat.c")).read()
    assert "recompute_group_velocities" not in src and "pf_refresh_segment" not in src
