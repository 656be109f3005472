"""CPU-side checks of the catalogue entry points: include/pinfmax.h declares them with the agreed signatures and structs, the
library exports them, pinocchio_amd/_lib.py binds them with matching argument types and struct layouts, and pinocchio_amd/api.py
mirrors each one."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARED = {
    "pf_catalog": "pf_ctx *ctx, const pf_plc_segment *seg, const pf_peak_region *box, const pf_catalog_params *par, size_t ngroups, const void *groups, "
                  "const pf_plc_group_layout *gl, size_t capacity, void *catalog, const pf_catalog_out_layout *ol, unsigned int *group_of, const pf_mf_bins *bins, "
                  "int *ninbin, double *massinbin, size_t *count",
    "pf_debug_catalog_times": "double *ms2",
    "pf_debug_catalog_parts": "double *ms4",
}
# struct -> its declaration in the header, whitespace normalised
STRUCTS = {
    "pf_catalog_params": "double F, InterPartDist, ParticleMass, hfactor; long long GSglobal[3]; int pbc[3]; int min_mass;",
    "pf_catalog_out_layout": "size_t stride; long off_name, off_M, off_x, off_v, off_q, off_n;",
    "pf_mf_bins": "int nbin; double mmin, deltam;",
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
            "size_t": (C.POINTER(C.c_size_t),), "pf_peak_region": (C.POINTER(lib.PeakRegion),), "pf_plc_segment": (C.POINTER(lib.PlcSegment),),
            "pf_plc_group_layout": (C.POINTER(lib.PlcGroupLayout),), "pf_catalog_params": (C.POINTER(lib.CatalogParams),),
            "pf_catalog_out_layout": (C.POINTER(lib.CatalogOutLayout),), "pf_mf_bins": (C.POINTER(lib.MfBins),)}[base]


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


def test_struct_sizes_and_fields(lib):
    p, d, i, l, z, ll = (C.sizeof(t) for t in (C.c_void_p, C.c_double, C.c_int, C.c_long, C.c_size_t, C.c_longlong))
    assert (p, d, i, l, z, ll) == (8, 8, 4, 8, 8, 8)
    # the sizes a C compiler of this ABI gives the declarations above
    assert C.sizeof(lib.CatalogParams) == 4 * 8 + 3 * 8 + 3 * 4 + 4 == 72
    assert C.sizeof(lib.CatalogOutLayout) == 8 + 6 * 8 and C.sizeof(lib.MfBins) == 24
    assert [f[0] for f in lib.CatalogParams._fields_] == ["F", "InterPartDist", "ParticleMass", "hfactor", "GSglobal", "pbc", "min_mass"]
    assert [f[0] for f in lib.CatalogOutLayout._fields_] == ["stride", "off_name", "off_M", "off_x", "off_v", "off_q", "off_n"]
    assert [f[0] for f in lib.MfBins._fields_] == ["nbin", "mmin", "deltam"]
    assert lib.CatalogParams.GSglobal.offset == 32 and lib.CatalogParams.pbc.offset == 56 and lib.CatalogParams.min_mass.offset == 68 and lib.MfBins.mmin.offset == 8


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
    sig = inspect.signature(api.Fmax.catalog)
    assert list(sig.parameters) == ["self", "F", "myseg", "z_seg", "stabl", "Lgwbl", "groups", "InterPartDist", "ParticleMass", "GSglobal", "hfactor", "pbc", "min_mass",
                                    "group_layout", "z_prev", "use_v31", "capacity", "out_dtype", "out", "bins"]
    for meth, call in ((api.Fmax.catalog, "pf_catalog"), (api.catalog_times, "pf_debug_catalog_times"),
                       (api.catalog_parts, "pf_debug_catalog_parts")):
        assert "." + call + "(" in inspect.getsource(meth), call
    # catalog_data as the reference's compiler lays it out (src/pinocchio.h:515-524)
    for dp, light, size in ((False, False, 56), (True, False, 96), (False, True, 48), (True, True, 88)):
        dt = api.catalog_dtype(dp, light)
        o = api.catalog_out_layout(dt)
        pb = 8 if dp else 4
        assert dt.itemsize == size
        assert (o.stride, o.off_name, o.off_M, o.off_x, o.off_v, o.off_q, o.off_n) == (size, 0, 8, 8 + pb, 8 + 4 * pb, 8 + 7 * pb, -1 if light else 8 + 10 * pb)
    o = api.catalog_out_layout(np.dtype([("name", "<u8"), ("x", "<f4", 3)]))
    assert (o.stride, o.off_name, o.off_M, o.off_x, o.off_v, o.off_q, o.off_n) == (20, 0, -1, 8, -1, -1, -1)
    assert api.catalog_times() == (0.0, 0.0) or all(t >= 0.0 for t in api.catalog_times())
