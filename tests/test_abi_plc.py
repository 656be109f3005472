"""CPU-side checks of the light-cone entry points: include/pinfmax.h declares them with the agreed signatures and structs, the
library exports them, pinocchio_amd/_lib.py binds them with matching argument types and struct layouts, and pinocchio_amd/api.py
mirrors each one."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARED = {
    "pf_plc_set_cosmology": "pf_ctx *ctx, const pf_plc_cosmology *cosmo",
    "pf_plc_set_geometry": "pf_ctx *ctx, const pf_plc_geometry *geom",
    "pf_plc_cross": "pf_ctx *ctx, int mode, const pf_plc_segment *seg, const pf_peak_region *box, size_t ncand, const void *groups, const pf_plc_group_layout *gl, "
                    "const void *f_lo, size_t f_lo_stride, int min_mass, size_t capacity, void *plcgroups, const pf_plc_out_layout *ol, unsigned int *cand_of, "
                    "int *rep_of, double *nz, size_t *count, size_t *unconverged",
    "pf_debug_plc_times": "double *ms2",
}
# struct -> its declaration in the header, whitespace normalised
STRUCTS = {
    "pf_plc_cosmology": "int n; const double *x, *comvdist, *hubble; int nk; const double *grow[4], *fomega[4]; double logkmin, deltalogk, k_for_GM, rad_gm0; "
                        "int nsmooth; const double *k_gm_displ;",
    "pf_plc_replication": "int i, j, k; double F1, F2;",
    "pf_plc_geometry": "double center[3], xvers[3], yvers[3], zvers[3], aperture, Fstop, InterPartDist; long long GSglobal[3]; size_t nrep; "
                       "const pf_plc_replication *repls; double LastzForPLC, delta_z; int nzbins;",
    "pf_plc_segment": "int myseg, use_v31; double z_seg, z_prev;",
    "pf_plc_group_layout": "size_t stride; long off_Mass, off_Pos, off_name, off_Flast, off_good, off_point, off_Vel, off_Vel_2LPT, off_Vel_3LPT_1, off_Vel_3LPT_2, "
                           "off_Vel_prev, off_Vel_2LPT_prev, off_Vel_3LPT_1_prev, off_Vel_3LPT_2_prev;",
    "pf_plc_out_layout": "size_t stride; long off_Mass, off_name, off_z, off_x, off_v;",
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
        return {"int": C.c_int, "size_t": C.c_size_t}[param.rsplit(" ", 1)[0]]
    base = param[:param.index("*")].replace("const", "").strip()
    return {"pf_ctx": (C.c_void_p,), "void": (C.c_void_p,), "unsigned int": (C.POINTER(C.c_uint),), "int": (C.POINTER(C.c_int),), "double": (C.POINTER(C.c_double),),
            "size_t": (C.POINTER(C.c_size_t),), "pf_peak_region": (C.POINTER(lib.PeakRegion),), "pf_plc_cosmology": (C.POINTER(lib.PlcCosmology),),
            "pf_plc_geometry": (C.POINTER(lib.PlcGeometry),), "pf_plc_segment": (C.POINTER(lib.PlcSegment),), "pf_plc_group_layout": (C.POINTER(lib.PlcGroupLayout),),
            "pf_plc_out_layout": (C.POINTER(lib.PlcOutLayout),)}[base]


def test_the_header_declares_the_agreed_signatures_and_structs(lib):
    hdr = open(os.path.join(ROOT, "include", "pinfmax.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, params in DECLARED.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in pinfmax.h"
        assert re.sub(r"\s+", " ", m.group(1)).strip() == params, name
    for name, body in STRUCTS.items():
        m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % name, hdr)
        assert m and re.sub(r"\s+", " ", m.group(1)).strip() == body, name
    assert re.search(r"#define\s+PF_PLC_LAST_CHECK\s+0\b", hdr) and re.search(r"#define\s+PF_PLC_EVENTS\s+1\b", hdr)
    assert (lib.PLC_LAST_CHECK, lib.PLC_EVENTS) == (0, 1)


def test_struct_sizes_and_fields(lib):
    p, d, i, l, z, ll = (C.sizeof(t) for t in (C.c_void_p, C.c_double, C.c_int, C.c_long, C.c_size_t, C.c_longlong))
    assert (p, d, i, l, z, ll) == (8, 8, 4, 8, 8, 8)
    # the sizes a C compiler of this ABI gives the declarations above
    assert C.sizeof(lib.PlcCosmology) == 8 + 3 * 8 + 8 + 8 * 8 + 4 * 8 + 8 + 8 == 152
    assert C.sizeof(lib.PlcReplication) == 32 and C.sizeof(lib.PlcSegment) == 24
    assert C.sizeof(lib.PlcGeometry) == 15 * 8 + 3 * 8 + 8 + 8 + 2 * 8 + 8 == 184
    assert C.sizeof(lib.PlcGroupLayout) == 8 + 14 * 8 and C.sizeof(lib.PlcOutLayout) == 8 + 5 * 8
    assert [f[0] for f in lib.PlcGroupLayout._fields_] == ["stride"] + lib.PLC_GROUP_FIELDS
    assert [f[0] for f in lib.PlcOutLayout._fields_] == ["stride", "off_Mass", "off_name", "off_z", "off_x", "off_v"]
    assert [f[0] for f in lib.PlcCosmology._fields_] == ["n", "x", "comvdist", "hubble", "nk", "grow", "fomega", "logkmin", "deltalogk", "k_for_GM", "rad_gm0", "nsmooth",
                                                         "k_gm_displ"]
    assert lib.PlcGeometry.repls.offset == 152 and lib.PlcGeometry.nzbins.offset == 176 and lib.PlcCosmology.grow.offset == 40


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
    import numpy as np
    from pinocchio_amd import api
    F = api.Fmax
    assert list(inspect.signature(F.plc_set_cosmology).parameters)[:6] == ["self", "x", "comvdist", "hubble", "grow", "fomega"]
    assert list(inspect.signature(F.plc_set_geometry).parameters)[:10] == ["self", "center", "xvers", "yvers", "zvers", "aperture", "Fstop", "InterPartDist", "GSglobal", "repls"]
    sig = inspect.signature(F.plc_cross)
    assert list(sig.parameters) == ["self", "mode", "myseg", "z_seg", "stabl", "groups", "group_layout", "z_prev", "use_v31", "f_lo", "min_mass", "capacity", "out_dtype", "nz"]
    for meth, call in ((F.plc_set_cosmology, "pf_plc_set_cosmology"), (F.plc_set_geometry, "pf_plc_set_geometry"), (F.plc_cross, "pf_plc_cross"),
                       (api.plc_times, "pf_debug_plc_times")):
        assert "." + call + "(" in inspect.getsource(meth), call
    g = api.plc_group_layout(120, 0, 4, 116, off_good=-1, off_Vel=16)
    assert (g.stride, g.off_Mass, g.off_Pos, g.off_Flast, g.off_name, g.off_good, g.off_point, g.off_Vel, g.off_Vel_3LPT_2_prev) == (120, 0, 4, 116, -1, -1, -1, 16, -1)
    # plcgroup_data as the reference's compiler lays it out (src/pinocchio.h:430-435)
    for dp, size in ((False, 48), (True, 72)):
        dt = api.plc_out_dtype(dp)
        o = api.plc_out_layout(dt)
        pb = 8 if dp else 4
        assert dt.itemsize == size and (o.stride, o.off_Mass, o.off_name, o.off_z, o.off_x, o.off_v) == (size, 0, 8, 16, 16 + pb, 16 + 4 * pb)
    dt = np.dtype([("Mass", "<i4"), ("Pos", "<f4", 3), ("Flast", "<f4"), ("Vel", "<f4", 3)])
    g = api.plc_group_layout_of(dt)
    assert (g.stride, g.off_Mass, g.off_Pos, g.off_Flast, g.off_Vel, g.off_good, g.off_Vel_2LPT) == (32, 0, 4, 16, 20, -1, -1)
