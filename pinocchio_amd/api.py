"""Host-side mirror of the reference's Fmax interface on top of the C ABI.

Method names and argument meaning follow the reference (src/pinocchio.h:545-562,
637-647): compute_fmax, compute_second_derivatives, compute_collapse_times,
compute_displacements, Fmax_PDF.  All compute runs in libpinfmax_hip.so on the
GPU; numpy is only the host container of inputs and outputs.
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from . import _lib

PRODUCT_DTYPE = np.dtype(
    [("Rmax", "<i4"), ("Fmax", "<f4"), ("Vel", "<f4", 3), ("Vel_2LPT", "<f4", 3),
     ("Vel_3LPT_1", "<f4", 3), ("Vel_3LPT_2", "<f4", 3)], align=False)  # src/pinocchio.h:233-259, 56 B
# the same record of a -DDOUBLE_PRECISION_PRODUCTS build (PRODFLOAT double, src/pinocchio.h:219-225): 112 B
PRODUCT_DTYPE_DP = np.dtype(
    {"names": ["Rmax", "Fmax", "Vel", "Vel_2LPT", "Vel_3LPT_1", "Vel_3LPT_2"],
     "formats": ["<i4", "<f8", ("<f8", 3), ("<f8", 3), ("<f8", 3), ("<f8", 3)],
     "offsets": [0, 8, 16, 40, 64, 88], "itemsize": 112})


class PinfmaxError(RuntimeError):
    pass


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def plan_bytes(n: int, nranks: int = 1, field_bytes: int = 8, double_products: bool = False):
    """(bytes pf_create allocates, bytes held at most) per rank of this configuration -- pf_plan_bytes; no device needed"""
    L = _lib.load()
    cfg = _lib.Config(n=n, rank=0, nranks=nranks, device=0, field_bytes=field_bytes, flags=_lib.FLAG_DOUBLE_PRODUCTS if double_products else 0)
    a, b = C.c_size_t(), C.c_size_t()
    if L.pf_plan_bytes(C.byref(cfg), C.byref(a), C.byref(b)):
        raise PinfmaxError("pf_plan_bytes: bad configuration")
    return a.value, b.value


def _region(region):
    """None (the whole periodic box) or (start[3], len[3], safe[3]) in global grid coordinates (x, y, z) -> pf_peak_region"""
    if region is None:
        return None
    start, length, safe = region
    return _lib.PeakRegion((C.c_int * 3)(*map(int, start)), (C.c_int * 3)(*map(int, length)), (C.c_int * 3)(*map(int, safe)))


PLC_LAST_CHECK, PLC_EVENTS = _lib.PLC_LAST_CHECK, _lib.PLC_EVENTS


def plc_times():
    """device ms of the last plc_cross: (candidate passes, root + store passes); zeros without PF_PLC_TIMES=1 (pf_debug_plc_times)"""
    ms = (C.c_double * 2)()
    _lib.load().pf_debug_plc_times(ms)
    return float(ms[0]), float(ms[1])


def catalog_times():
    """device ms of the last catalog: (flag + scan passes, record + histogram passes); zeros without PF_CATALOG_TIMES=1
    (pf_debug_catalog_times)"""
    ms = (C.c_double * 2)()
    _lib.load().pf_debug_catalog_times(ms)
    return float(ms[0]), float(ms[1])


def catalog_parts():
    """the host's wall ms of the last catalog: (pack, upload, device, download + records) (pf_debug_catalog_parts)"""
    ms = (C.c_double * 4)()
    _lib.load().pf_debug_catalog_parts(ms)
    return tuple(float(x) for x in ms)


def point_times():
    """device ms of the last point_states: (select + scan passes, state pass); zeros without PF_POINT_TIMES=1 (pf_debug_point_times)"""
    ms = (C.c_double * 2)()
    _lib.load().pf_debug_point_times(ms)
    return float(ms[0]), float(ms[1])


def power_times():
    """device ms of the last power_spectrum / debug_power_spectrum; zero without PF_POWER_TIMES=1 (pf_debug_power_times)"""
    ms = (C.c_double * 1)()
    _lib.load().pf_debug_power_times(ms)
    return float(ms[0])


def power_bins(n: int) -> int:
    """shells of the power spectrum of a grid of n points per side (pf_power_bins)"""
    return int(_lib.load().pf_power_bins(int(n)))


_POWER_WHICH = {"density": 0, "kvector_2LPT": 1, "kvector_3LPT_1": 2, "kvector_3LPT_2": 3}


def _power_call(L, n, radii_cells, call):
    """the output arrays of a power call, `call(ns, radii, nmodes, k2sum, power, variance, info)` -> the dict of its results"""
    r = np.ascontiguousarray(radii_cells, dtype=np.float64).reshape(-1)
    nb = int(L.pf_power_bins(int(n)))
    nm, k2 = np.zeros(nb, dtype=np.uint64), np.zeros(nb, dtype=np.uint64)
    pw, var = np.zeros(nb), np.zeros(max(len(r), 1))
    info = _lib.PowerInfo()
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_ulonglong))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = call(len(r), dp(r) if len(r) else None, up(nm), up(k2), dp(pw), dp(var) if len(r) else None, C.byref(info))
    return rc, {"nmodes": nm, "k2sum": k2, "power": pw, "variance": var[:len(r)].copy(), "modes": int(info.modes), "nonfinite": int(info.nonfinite)}


def debug_power_spectrum(spec, y0: int = 0, field_bytes: int = 8, radii_cells=()):
    """the power kernels on the rows y0 .. y0 + nyl - 1 of a caller's spectrum, a ky-slab [nyl][n (kx)][n/2+1] complex128
    (pf_debug_power_spectrum) -> the dict of Fmax.power_spectrum with that slab's partial sums"""
    L = _lib.load()
    spec = np.ascontiguousarray(spec, dtype=np.complex128)
    if spec.ndim != 3 or spec.shape[2] != spec.shape[1] // 2 + 1:
        raise ValueError(f"a ky-slab [nyl][n][n/2+1], not {spec.shape}")
    nyl, n = spec.shape[0], spec.shape[1]
    sp = spec.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))
    rc, out = _power_call(L, n, radii_cells,
                          lambda ns, r, nm, k2, pw, var, info: L.pf_debug_power_spectrum(int(field_bytes), n, int(y0), nyl, sp, ns, r, nm, k2, pw, var, info))
    if rc:
        raise PinfmaxError(L.pf_last_error().decode() or "pf_debug_power_spectrum failed")
    return out


MATTER_NGP, MATTER_DECONVOLVE = _lib.MATTER_NGP, _lib.MATTER_DECONVOLVE


def matter_times():
    """device ms of the last matter_power / debug_matter_*: (deposit, contrast, transform, shell sums); zeros without PF_MATTER_TIMES=1
    (pf_debug_matter_times)"""
    ms = (C.c_double * 4)()
    _lib.load().pf_debug_matter_times(ms)
    return tuple(float(x) for x in ms)


def matter_form():
    """what the calling thread's last matter call launched: (deposit: 0 one particle per lane, 1 LDS-staged, -1 none yet; scans of its
    shell passes: 1, 3, or 0 for none yet) (pf_debug_matter_form)"""
    form = (C.c_int * 2)()
    _lib.load().pf_debug_matter_form(form)
    return int(form[0]), int(form[1])


EXCHANGE_KEYS = ("form", "reach_below", "reach_above", "window_planes", "block_planes", "bytes_per_peer")


def matter_exchange():
    """what the calling thread's last matter_power_slabs / debug_matter_slabs did (pf_debug_matter_exchange): form (0 no exchange,
    1 ghost planes, 2 every rank deposits the whole box), the common reach below / above in planes, the planes of the deposit window
    and of a peer block, and the bytes per peer handed to the all-to-all"""
    out = (C.c_ulonglong * 6)()
    _lib.load().pf_debug_matter_exchange(out)
    return dict(zip(EXCHANGE_KEYS, (int(x) for x in out)))


def _matter_flags(ngp, deconvolve):
    return (MATTER_NGP if ngp else 0) | (MATTER_DECONVOLVE if deconvolve else 0)


def _matter_info(info):
    return {k: int(getattr(info, k)) for k, _ in info._fields_}


def debug_matter_deposit(vel12, ngp: bool = False, weight=None):
    """the production deposit on a caller's columns [12][n][n][n], float32 or float64 (pf_debug_matter_deposit) -> (the grid
    [n][n][n] of uint64 in units of 2^-48 particle, the dict of pf_matter_info)"""
    L = _lib.load()
    vel12 = np.ascontiguousarray(vel12)
    if vel12.dtype not in (np.float32, np.float64) or vel12.ndim != 4 or vel12.shape[0] != 12 or len(set(vel12.shape[1:])) != 1:
        raise ValueError(f"columns [12][n][n][n] of float32 or float64, not {vel12.dtype} {vel12.shape}")
    n = vel12.shape[1]
    w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64).reshape(4)
    grid = np.zeros((n, n, n), dtype=np.uint64)
    info = _lib.MatterInfo()
    if L.pf_debug_matter_deposit(vel12.dtype.itemsize, n, vel12.ctypes.data_as(C.c_void_p), _matter_flags(ngp, False), None if w is None else _dp(w),
                                 grid.ctypes.data_as(C.POINTER(C.c_ulonglong)), C.byref(info)):
        raise PinfmaxError(L.pf_last_error().decode() or "pf_debug_matter_deposit failed")
    return grid, _matter_info(info)


def debug_matter_shells(spec_m, spec_lin=None, y0: int = 0, field_bytes: int = 8, ngp: bool = False, deconvolve: bool = False):
    """the production shell passes on the rows y0 .. y0 + nyl - 1 of two spectra, ky-slabs [nyl][n (kx)][n/2+1] complex128
    (pf_debug_matter_shells) -> nmodes[], k2sum[], power[], cross[] (None without spec_lin) and the counters of pf_matter_info"""
    L = _lib.load()
    spec_m = np.ascontiguousarray(spec_m, dtype=np.complex128)
    if spec_m.ndim != 3 or spec_m.shape[2] != spec_m.shape[1] // 2 + 1:
        raise ValueError(f"a ky-slab [nyl][n][n/2+1], not {spec_m.shape}")
    if spec_lin is not None:
        spec_lin = np.ascontiguousarray(spec_lin, dtype=np.complex128)
        if spec_lin.shape != spec_m.shape:
            raise ValueError(f"two slabs of one shape, not {spec_m.shape} and {spec_lin.shape}")
    nyl, n = spec_m.shape[:2]
    nb = int(L.pf_power_bins(n))
    nm, k2 = np.zeros(nb, dtype=np.uint64), np.zeros(nb, dtype=np.uint64)
    pw, cr = np.zeros(nb), np.zeros(nb)
    info = _lib.MatterInfo()
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_ulonglong))
    two = spec_lin is not None
    if L.pf_debug_matter_shells(int(field_bytes), n, int(y0), nyl, _dp(spec_m.view(np.float64)), _dp(spec_lin.view(np.float64)) if two else None,
                                _matter_flags(ngp, deconvolve), up(nm), up(k2), _dp(pw), _dp(cr) if two else None, C.byref(info)):
        raise PinfmaxError(L.pf_last_error().decode() or "pf_debug_matter_shells failed")
    out = {"nmodes": nm, "k2sum": k2, "power": pw, "cross": cr if two else None}
    out.update(_matter_info(info))
    return out


HALO_NGP, HALO_DECONVOLVE, HALO_MASS_WEIGHT, HALO_MAX_BINS = _lib.HALO_NGP, _lib.HALO_DECONVOLVE, _lib.HALO_MASS_WEIGHT, _lib.HALO_MAX_BINS
HALO_TIME_KEYS = ("select", "deposit", "contrast", "transform", "shells")


def halo_times():
    """device ms of the phases of the last halo_power, summed over its bins: (select, deposit, contrast, transform, shell sums); zeros
    without PF_HALO_TIMES=1 (pf_debug_halo_times)"""
    ms = (C.c_double * 5)()
    _lib.load().pf_debug_halo_times(ms)
    return tuple(float(x) for x in ms)


def _halo_flags(ngp, deconvolve, mass_weight):
    return (HALO_NGP if ngp else 0) | (HALO_DECONVOLVE if deconvolve else 0) | (HALO_MASS_WEIGHT if mass_weight else 0)


def _halo_list(pos, mass):
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    mass = np.ascontiguousarray(mass, dtype=np.int32)
    if pos.ndim != 2 or pos.shape[1] != 3 or mass.shape != (pos.shape[0],):
        raise ValueError(f"positions [count][3] and masses [count], not {pos.shape} and {mass.shape}")
    return pos, mass


def _halo_info(info):
    d = {k: int(getattr(info, k)) for k, _ in info._fields_}
    d["weight2"] = (d["weight2_hi"] << 64) | d["weight2_lo"]
    return d


def debug_halo_deposit(n: int, pos, mass, lo: int, hi: int, scale: float = 1.0, mass_weight: bool = False, ngp: bool = False, x0: int = 0, nxl=None):
    """the production selection and deposit of the haloes with lo <= mass <= hi on the planes [x0, x0 + nxl) of a grid of n, without a
    context (pf_debug_halo_deposit) -> (the grid [nxl][n][n] of uint64 in units of 2^-30, the dict of pf_halo_info)"""
    L = _lib.load()
    pos, mass = _halo_list(pos, mass)
    nxl = int(n) - int(x0) if nxl is None else int(nxl)
    grid = np.zeros((max(nxl, 1), int(n), int(n)), dtype=np.uint64)
    info = _lib.HaloInfo()
    if L.pf_debug_halo_deposit(int(n), int(x0), nxl, _halo_flags(ngp, False, mass_weight), len(mass), _dp(pos), float(scale), mass.ctypes.data_as(C.POINTER(C.c_int)),
                               int(lo), int(hi), grid.ctypes.data_as(C.POINTER(C.c_ulonglong)), C.byref(info)):
        raise PinfmaxError(L.pf_last_error().decode() or "pf_debug_halo_deposit failed")
    return grid, _halo_info(info)


MULTIPOLE_ORDERS, MULTIPOLE_SUMS = _lib.MULTIPOLE_ORDERS, _lib.MULTIPOLE_SUMS


def _halo_vel(vel, pos):
    """velocities [count][3] beside positions of the same shape, or None: real space"""
    if vel is None:
        return None
    vel = np.ascontiguousarray(vel, dtype=np.float64)
    if vel.shape != pos.shape:
        raise ValueError(f"velocities {vel.shape} beside positions {pos.shape}")
    return vel


def multipole_form():
    """what the calling thread's last multipole shell pass launched: (scans, accumulation passes); zeros for none yet
    (pf_debug_multipole_form)"""
    form = (C.c_int * 2)()
    _lib.load().pf_debug_multipole_form(form)
    return int(form[0]), int(form[1])


def debug_halo_deposit_rsd(n: int, pos, vel, mass, lo: int, hi: int, scale: float = 1.0, vfac: float = 0.0, los: int = 2, mass_weight: bool = False, ngp: bool = False,
                           x0: int = 0, nxl=None):
    """debug_halo_deposit with the list moved along axis `los` by vel * vfac (pf_debug_halo_deposit_rsd); vel None: real space"""
    L = _lib.load()
    pos, mass = _halo_list(pos, mass)
    vel = _halo_vel(vel, pos)
    nxl = int(n) - int(x0) if nxl is None else int(nxl)
    grid = np.zeros((max(nxl, 1), int(n), int(n)), dtype=np.uint64)
    info = _lib.HaloInfo()
    if L.pf_debug_halo_deposit_rsd(int(n), int(x0), nxl, _halo_flags(ngp, False, mass_weight), len(mass), _dp(pos), None if vel is None else _dp(vel), float(scale), float(vfac),
                                   int(los), mass.ctypes.data_as(C.POINTER(C.c_int)), int(lo), int(hi), grid.ctypes.data_as(C.POINTER(C.c_ulonglong)), C.byref(info)):
        raise PinfmaxError(L.pf_last_error().decode() or "pf_debug_halo_deposit_rsd failed")
    return grid, _halo_info(info)


def debug_multipole_shells(spec_m, spec_lin=None, y0: int = 0, field_bytes: int = 8, ngp: bool = False, deconvolve: bool = False, los: int = 2):
    """the production multipole shell passes on the rows y0 .. y0 + nyl - 1 of two spectra, ky-slabs [nyl][n (kx)][n/2+1] complex128
    (pf_debug_multipole_shells) -> nmodes[], k2sum[], power[3][], cross[3][] (None without spec_lin), parts[11][] (the positive
    sums / N^6), modes and nonfinite_modes"""
    L = _lib.load()
    spec_m = np.ascontiguousarray(spec_m, dtype=np.complex128)
    if spec_m.ndim != 3 or spec_m.shape[2] != spec_m.shape[1] // 2 + 1:
        raise ValueError(f"a ky-slab [nyl][n][n/2+1], not {spec_m.shape}")
    if spec_lin is not None:
        spec_lin = np.ascontiguousarray(spec_lin, dtype=np.complex128)
        if spec_lin.shape != spec_m.shape:
            raise ValueError(f"two slabs of one shape, not {spec_m.shape} and {spec_lin.shape}")
    nyl, n = spec_m.shape[:2]
    nb = int(L.pf_power_bins(n))
    nm, k2 = np.zeros(nb, dtype=np.uint64), np.zeros(nb, dtype=np.uint64)
    pw, cr, parts = np.zeros((MULTIPOLE_ORDERS, nb)), np.zeros((MULTIPOLE_ORDERS, nb)), np.zeros((MULTIPOLE_SUMS, nb))
    info = _lib.MatterInfo()
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_ulonglong))
    two = spec_lin is not None
    if L.pf_debug_multipole_shells(int(field_bytes), n, int(y0), nyl, _dp(spec_m.view(np.float64)), _dp(spec_lin.view(np.float64)) if two else None,
                                   _matter_flags(ngp, deconvolve), int(los), up(nm), up(k2), _dp(pw), _dp(cr) if two else None, _dp(parts), C.byref(info)):
        raise PinfmaxError(L.pf_last_error().decode() or "pf_debug_multipole_shells failed")
    return {"nmodes": nm, "k2sum": k2, "power": pw, "cross": cr if two else None, "parts": parts, "modes": int(info.modes), "nonfinite_modes": int(info.nonfinite_modes)}


CORR_ORDERS, CORR_SUMS = _lib.CORR_ORDERS, _lib.CORR_SUMS
CORR_TIME_KEYS = ("select", "deposit", "contrast", "transform", "form", "shells")


def debug_corr_times():
    """device ms of the phases of the last halo_correlation, summed over its bins: (select, deposit, contrast, transforms forward and
    reverse, form passes, shell sums); zeros without PF_CORR_TIMES=1 (pf_debug_corr_times)"""
    ms = (C.c_double * 6)()
    _lib.load().pf_debug_corr_times(ms)
    return tuple(float(x) for x in ms)


def corr_passes():
    """what the calling thread's last separation-space shell pass launched: (scans, accumulation passes); zeros for none yet
    (pf_debug_corr_passes)"""
    passes = (C.c_int * 2)()
    _lib.load().pf_debug_corr_passes(passes)
    return int(passes[0]), int(passes[1])


def debug_corr_form(spec_m, spec_lin=None, y0: int = 0, field_bytes: int = 8, ngp: bool = False, deconvolve: bool = False, which: int = 0):
    """the production form pass of halo_correlation on the rows y0 .. y0 + nyl - 1 of a ky-slab [nyl][n (kx)][n/2+1] complex128
    (pf_debug_corr_form): which 0 -> |m|^2 / N^3, which 1 -> Re(m conj lin) / N^3 (needs spec_lin), deconvolved or not, rounded once to
    the field type -> (the formed slab, complex128 with zero imaginary parts, {modes, nonfinite_modes})"""
    L = _lib.load()
    spec_m = np.ascontiguousarray(spec_m, dtype=np.complex128)
    if spec_m.ndim != 3 or spec_m.shape[2] != spec_m.shape[1] // 2 + 1:
        raise ValueError(f"a ky-slab [nyl][n][n/2+1], not {spec_m.shape}")
    if spec_lin is not None:
        spec_lin = np.ascontiguousarray(spec_lin, dtype=np.complex128)
        if spec_lin.shape != spec_m.shape:
            raise ValueError(f"two slabs of one shape, not {spec_m.shape} and {spec_lin.shape}")
    nyl, n = spec_m.shape[:2]
    out = np.zeros(spec_m.shape, dtype=np.complex128)
    info = _lib.MatterInfo()
    if L.pf_debug_corr_form(int(field_bytes), n, int(y0), nyl, _dp(spec_m.view(np.float64)), None if spec_lin is None else _dp(spec_lin.view(np.float64)),
                            _matter_flags(ngp, deconvolve), int(which), _dp(out.view(np.float64)), C.byref(info)):
        raise PinfmaxError(L.pf_last_error().decode() or "pf_debug_corr_form failed")
    return out, {"modes": int(info.modes), "nonfinite_modes": int(info.nonfinite_modes)}


def debug_corr_shells(real, x0: int = 0, field_bytes: int = 8, los: int = 2):
    """the production separation-space shell passes of halo_correlation on the planes x0 .. x0 + nxl - 1 of a real field [nxl][n][n]
    float64 (pf_debug_corr_shells) -> ncells[], r2sum[], xi[3][] (positive - negative of l = 0, 2, 4), parts[6][] (the positive
    sums) and nonfinite_cells"""
    L = _lib.load()
    real = np.ascontiguousarray(real, dtype=np.float64)
    if real.ndim != 3 or real.shape[1] != real.shape[2]:
        raise ValueError(f"planes [nxl][n][n], not {real.shape}")
    nxl, n = real.shape[:2]
    nb = int(L.pf_power_bins(n))
    nc, r2 = np.zeros(nb, dtype=np.uint64), np.zeros(nb, dtype=np.uint64)
    xi, parts = np.zeros((CORR_ORDERS, nb)), np.zeros((CORR_SUMS // 2, nb))
    bad = C.c_ulonglong(0)
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_ulonglong))
    if L.pf_debug_corr_shells(int(field_bytes), n, int(x0), nxl, _dp(real), int(los), up(nc), up(r2), _dp(xi), _dp(parts), C.byref(bad)):
        raise PinfmaxError(L.pf_last_error().decode() or "pf_debug_corr_shells failed")
    return {"ncells": nc, "r2sum": r2, "xi": xi, "parts": parts, "nonfinite_cells": int(bad.value)}


BISPEC_MAX_KBINS = _lib.BISPEC_MAX_KBINS
BISPEC_TIME_KEYS = ("select", "deposit", "contrast", "transform", "mask", "keep", "triples")


def bispectrum_triangles(kmin: int, dk: int, nk: int):
    """the ordered triples i <= j <= l of the nk linear k-bins [kmin + i dk, kmin + (i + 1) dk) that can close a triangle, in
    lexicographic order, as an int32 array [nt][3]: what the outputs of halo_bispectrum are indexed by (pf_bispectrum_triangles)"""
    L = _lib.load()
    nt = L.pf_bispectrum_triangles(int(kmin), int(dk), int(nk), None)
    if nt < 0:
        raise PinfmaxError(L.pf_last_error().decode() or "pf_bispectrum_triangles failed")
    ijl = np.zeros((nt, 3), dtype=np.int32)
    L.pf_bispectrum_triangles(int(kmin), int(dk), int(nk), ijl.ctypes.data_as(C.POINTER(C.c_int)))
    return ijl


def debug_bispec_times():
    """device ms of the phases of the last halo_bispectrum, summed over its mass bins and the count fields: (select, deposit,
    contrast, transforms, mask, keep, triples); zeros without PF_BISPEC_TIMES=1 (pf_debug_bispec_times)"""
    ms = (C.c_double * 7)()
    _lib.load().pf_debug_bispec_times(ms)
    return tuple(float(x) for x in ms)


def debug_bispec_mask(spec, kmin: int, dk: int, nk: int, bin: int, y0: int = 0, field_bytes: int = 8, ngp: bool = False, deconvolve: bool = False, kind: int = 0):
    """the production mask pass of halo_bispectrum for k-bin `bin` on the rows y0 .. y0 + nyl - 1 of a ky-slab [nyl][n (kx)][n/2+1]
    complex128 (pf_debug_bispec_mask): kind 0 the data field, 1 the count field -> (the field as complex128, {kmodes,
    nonfinite_modes})"""
    L = _lib.load()
    spec = np.ascontiguousarray(spec, dtype=np.complex128)
    if spec.ndim != 3 or spec.shape[2] != spec.shape[1] // 2 + 1:
        raise ValueError(f"a ky-slab [nyl][n][n/2+1], not {spec.shape}")
    nyl, n = spec.shape[:2]
    out = np.zeros(spec.shape, dtype=np.complex128)
    km, bad = C.c_ulonglong(0), C.c_ulonglong(0)
    if L.pf_debug_bispec_mask(int(field_bytes), n, int(y0), nyl, _dp(spec.view(np.float64)), _matter_flags(ngp, deconvolve), int(kind), int(kmin), int(dk), int(nk), int(bin),
                              _dp(out.view(np.float64)), C.byref(km), C.byref(bad)):
        raise PinfmaxError(L.pf_last_error().decode() or "pf_debug_bispec_mask failed")
    return out, {"kmodes": int(km.value), "nonfinite_modes": int(bad.value)}


def debug_bispec_triples(fields, kmin: int, dk: int, nk: int, x0: int = 0, field_bytes: int = 8):
    """the production keep, triple and pair passes of halo_bispectrum on the planes x0 .. x0 + nxl - 1 of nk real fields
    [nk][nxl][n][n] float64 (pf_debug_bispec_triples) -> sums[nt] (positive - negative), parts[2][nt] (the positive sums), pair[nk],
    maxima[nk] and nonfinite_cells"""
    L = _lib.load()
    fields = np.ascontiguousarray(fields, dtype=np.float64)
    if fields.ndim != 4 or fields.shape[0] != nk or fields.shape[2] != fields.shape[3]:
        raise ValueError(f"fields [nk][nxl][n][n] with nk = {nk}, not {fields.shape}")
    nxl, n = fields.shape[1:3]
    nt = len(bispectrum_triangles(kmin, dk, nk))
    sums, parts, pair, maxima = np.zeros(nt), np.zeros((2, nt)), np.zeros(nk), np.zeros(nk)
    bad = C.c_ulonglong(0)
    if L.pf_debug_bispec_triples(int(field_bytes), n, int(x0), nxl, _dp(fields), int(kmin), int(dk), int(nk), _dp(sums), _dp(parts), _dp(pair), _dp(maxima), C.byref(bad)):
        raise PinfmaxError(L.pf_last_error().decode() or "pf_debug_bispec_triples failed")
    return {"sums": sums, "parts": parts, "pair": pair, "maxima": maxima, "nonfinite_cells": int(bad.value)}


_ARITH ={"fast": _lib.ARITH_FAST, "exact": _lib.ARITH_EXACT}
# pf_census_cell: an outlier of the flavour census
CENSUS_CELL_DTYPE = np.dtype([("cell", "<u8"), ("fast", "<f8"), ("exact", "<f8"), ("rmax_fast", "<i4"), ("rmax_exact", "<i4")], align=False)
_CENSUS_COUNTS = ("cells", "differing_bits", "beyond_2ulp", "rmax_differing", "nonfinite", "outliers")


def _census_dict(c):
    d = {k: int(getattr(c, k)) for k in _CENSUS_COUNTS}
    d["hist"] = np.array(c.hist[:], dtype=np.uint64)
    d["max_abs"], d["max_ulps"], d["max_abs_cell"] = float(c.max_abs), float(c.max_ulps), int(c.max_abs_cell)
    return d


def debug_census(fmax_fast, rmax_fast, fmax_exact, rmax_exact, first_cell: int = 0, capacity: int = 1024):
    """the census kernels on a caller's columns (pf_debug_census): Fmax columns of one dtype, float32 or float64, Rmax int32; the
    cell indices start at first_cell -> (census dict, outlier records as CENSUS_CELL_DTYPE)"""
    L = _lib.load()
    ff, fe = np.ascontiguousarray(fmax_fast), np.ascontiguousarray(fmax_exact)
    if ff.dtype != fe.dtype or ff.dtype not in (np.float32, np.float64):
        raise ValueError(f"Fmax columns of {ff.dtype} and {fe.dtype}")
    rf, re = np.ascontiguousarray(rmax_fast, dtype=np.int32), np.ascontiguousarray(rmax_exact, dtype=np.int32)
    if not (ff.shape == fe.shape == rf.shape == re.shape and ff.ndim == 1):
        raise ValueError("four columns of one length")
    out = _lib.Census()
    capacity = int(capacity)
    rec = np.zeros(max(capacity, 1), dtype=CENSUS_CELL_DTYPE)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    if L.pf_debug_census(ff.dtype.itemsize, int(first_cell), len(ff), ff.ctypes.data_as(C.c_void_p), ip(rf), fe.ctypes.data_as(C.c_void_p), ip(re),
                         C.byref(out), capacity, rec.ctypes.data_as(C.POINTER(_lib.CensusCell)) if capacity else None):
        raise PinfmaxError(L.pf_last_error().decode() or "pf_debug_census failed")
    cen = _census_dict(out)
    return cen, rec[:min(cen["outliers"], capacity)].copy()


def census_sum(parts):
    """the census of a box from those of its ranks, in rank order: counts and histogram summed, maxima taken.  max_abs_cell becomes
    an index of the whole box -- a rank's cells follow those of the ranks before it --, of the first rank that attains max_abs"""
    parts = list(parts)
    tot = {k: sum(p[k] for p in parts) for k in _CENSUS_COUNTS}
    tot["hist"] = np.sum([np.asarray(p["hist"], dtype=np.uint64) for p in parts], axis=0, dtype=np.uint64)
    tot["max_abs"], tot["max_ulps"], tot["max_abs_cell"] = 0.0, 0.0, 2 ** 64 - 1
    before = 0
    for p in parts:
        none = p["max_abs_cell"] == 2 ** 64 - 1   # every cell of that rank is nonfinite
        if not none and (tot["max_abs_cell"] == 2 ** 64 - 1 or p["max_abs"] > tot["max_abs"]):
            tot["max_abs"], tot["max_abs_cell"] = p["max_abs"], before + p["max_abs_cell"]
        if not none:
            tot["max_ulps"] = max(tot["max_ulps"], p["max_ulps"])
        before += p["cells"]
    return tot


def debug_peaks(fmax: np.ndarray, flast: float, region=None):
    """count_peaks (src/fragment.c:605-706) by the device kernel on a caller's [n][n][n] fp32 field -> (npeaks, ngood)"""
    L = _lib.load()
    f = np.ascontiguousarray(fmax, dtype=np.float32)
    n = f.shape[0]
    if f.shape != (n, n, n):
        raise ValueError(f"field shape {f.shape}")
    rg = _region(region)
    out = (C.c_ulonglong * 2)()
    if L.pf_debug_peaks(n, f.ctypes.data_as(C.POINTER(C.c_float)), float(flast), C.byref(rg) if rg is not None else None, out):
        raise PinfmaxError(L.pf_last_error().decode() or "pf_debug_peaks failed")
    return int(out[0]), int(out[1])


def _subbox(start, length):
    return _lib.SubBox((C.c_int * 3)(*map(int, start)), (C.c_int * 3)(*map(int, length)))


def _distmap(bits, length):
    """frag_map / frag_map_update of the target sub-box: uint32 words, bit p % 32 of word p // 32 for sub-box-space index p"""
    if bits is None:
        return None, None
    m = np.ascontiguousarray(bits, dtype=np.uint32).ravel()
    cells = int(length[0]) * int(length[1]) * int(length[2])
    if m.size * 32 < cells:
        raise ValueError(f"map of {m.size} words for a sub-box of {cells} cells")
    return m, m.ctypes.data_as(C.POINTER(C.c_uint))


def debug_distribute(fmax_slab: np.ndarray, x0: int, flast: float, start, length, map=None, capacity=None):
    """distribute()'s selection and order (src/distribute.c:547-698) by the device kernels on a caller's slab [nxl][n][n] of an fp32
    field, planes x0 .. x0 + nxl - 1 of the n^3 box -> (frag_pos, local cell index, count); capacity None: room for all"""
    L = _lib.load()
    f = np.ascontiguousarray(fmax_slab, dtype=np.float32)
    nxl, n = f.shape[0], f.shape[1]
    if f.shape != (nxl, n, n):
        raise ValueError(f"slab shape {f.shape}")
    sub = _subbox(start, length)
    keep, mp = _distmap(map, length)
    cnt = C.c_size_t()
    fp = f.ctypes.data_as(C.POINTER(C.c_float))

    def call(cap, pos, idx):
        if L.pf_debug_distribute(n, int(x0), nxl, fp, float(flast), C.byref(sub), mp, cap,
                                 pos.ctypes.data_as(C.POINTER(C.c_uint)) if pos is not None else None,
                                 idx.ctypes.data_as(C.POINTER(C.c_uint)) if idx is not None else None, C.byref(cnt)):
            raise PinfmaxError(L.pf_last_error().decode() or "pf_debug_distribute failed")

    if capacity is None:
        call(0, None, None)          # a count-only call sizes the arrays
        capacity = cnt.value
    pos = np.empty(int(capacity), dtype=np.uint32)
    idx = np.empty(int(capacity), dtype=np.uint32)
    call(int(capacity), pos, idx)
    m = min(cnt.value, int(capacity))
    return pos[:m], idx[:m], int(cnt.value)


def debug_organize(fmax: np.ndarray, frag_pos: np.ndarray):
    """the ordering of sort_and_organize (src/fragment.c:484-520) by the device kernels on a caller's fp32 Fmax and frag_pos
    -> (order, sorted_pos, indices): order[i] = input index of record i of the sorted order (descending Fmax, ties in input order,
    NaN last), sorted_pos ascending = frag_pos[order][indices]"""
    L = _lib.load()
    f = np.ascontiguousarray(fmax, dtype=np.float32).ravel()
    p = np.ascontiguousarray(frag_pos, dtype=np.uint32).ravel()
    if f.size != p.size:
        raise ValueError(f"{f.size} Fmax for {p.size} positions")
    order = np.empty(f.size, dtype=np.uint32)
    spos = np.empty(f.size, dtype=np.uint32)
    ind = np.empty(f.size, dtype=np.int32)
    if L.pf_debug_organize(f.size, f.ctypes.data_as(C.POINTER(C.c_float)), p.ctypes.data_as(C.POINTER(C.c_uint)),
                           order.ctypes.data_as(C.POINTER(C.c_uint)), spos.ctypes.data_as(C.POINTER(C.c_uint)),
                           ind.ctypes.data_as(C.POINTER(C.c_int))):
        raise PinfmaxError(L.pf_last_error().decode() or "pf_debug_organize failed")
    return order, spos, ind


def _neighbours(L, ctx, frag_pos, fmax, start, length, safe, ftype):
    pos = np.ascontiguousarray(frag_pos, dtype=np.uint32).ravel()
    f = np.asarray(fmax)
    if f.dtype != ftype:
        f = f.astype(ftype)
    if f.ndim != 1 or f.size != pos.size:
        raise ValueError(f"Fmax of shape {f.shape} for {pos.size} positions")
    if pos.size > 1 and f.strides[0] <= 0:
        f = np.ascontiguousarray(f)
    stride = f.strides[0] if pos.size > 1 else f.dtype.itemsize     # a field of a structured array: the stride of its records
    rg = _region((start, length, safe))
    neigh = np.empty((pos.size, 6), dtype=np.int32)
    flags = np.empty(pos.size, dtype=np.uint8)
    peaks = (C.c_ulonglong * 2)()
    if L.pf_neighbours(ctx, C.byref(rg), pos.size, pos.ctypes.data_as(C.POINTER(C.c_uint)), C.c_void_p(f.ctypes.data), stride,
                       neigh.ctypes.data_as(C.POINTER(C.c_int)), flags.ctypes.data_as(C.POINTER(C.c_ubyte)), peaks):
        raise PinfmaxError(L.pf_last_error().decode() or "pf_neighbours failed")
    return neigh, flags, (int(peaks[0]), int(peaks[1]))


def neighbours(frag_pos, fmax, start, length, safe):
    """The neighbour table of stored particles in the order after sort_and_organize (pf_neighbours without a context: fp32 Fmax, a
    direction periodic when safe == 0) -> (neigh[count, 6], flags[count], (npeaks, ngood)).  neigh[iz, nn], nn = x-, x+, y-, y+, z-,
    z+: the index of the particle stored at that neighbour of frag_pos[iz] in the box (start, length, safe), -1 when none is (what
    the reference computes as indices[find_location(i1, j1, k1)], src/build_groups.c:274-323); flags: _lib.NEIGH_SKIP / NEIGH_GOOD /
    NEIGH_PEAK.  fmax may be a strided view (the Fmax field of a record array): only the values are uploaded."""
    return _neighbours(_lib.load(), None, frag_pos, fmax, start, length, safe, np.float32)


def _strided(a, dtype, count, what):
    """a packed array or a field of a structured record array -> (array kept alive, pointer to its first element, byte stride)"""
    a = np.asarray(a)
    if a.dtype != dtype:
        a = a.astype(dtype)
    if a.ndim != 1 or a.size != count:
        raise ValueError(f"{what} of shape {a.shape} for {count} entries")
    if count > 1 and a.strides[0] <= 0:
        a = np.ascontiguousarray(a)
    return a, C.c_void_p(a.ctypes.data), (a.strides[0] if count > 1 else a.dtype.itemsize)


def _frag_pos(frag_pos, zacc):
    """frag_pos None: the CLASSIC_FRAGMENTATION form, particle iz at position iz"""
    if frag_pos is None:
        return None, None, int(np.asarray(zacc).size)
    pos = np.ascontiguousarray(frag_pos, dtype=np.uint32).ravel()
    return pos, pos.ctypes.data_as(C.POINTER(C.c_uint)), pos.size


def distribute_back(n: int, x0: int, nxl: int, start, length, safe, frag_pos, zacc, group_id):
    """keep_data_back (src/distribute.c:799-837) by the device kernel without a context (pf_debug_distribute_back): zacc (fp32) and
    group_id of the particles at the sub-box positions frag_pos (None: particle iz at position iz) of the sub-box (start, length,
    safe) scattered into the slab planes x0 .. x0 + nxl - 1 of an n^3 box whose columns start at -1 / 0
    -> (zacc[nxl n n], group_ID[nxl n n], stored)"""
    L = _lib.load()
    pos, pp, count = _frag_pos(frag_pos, zacc)
    z = np.ascontiguousarray(zacc, dtype=np.float32).ravel()
    g = np.ascontiguousarray(group_id, dtype=np.int32).ravel()
    if z.size != count or g.size != count:
        raise ValueError(f"{z.size} zacc and {g.size} group_ID for {count} particles")
    nc = max(int(nxl), 0) * int(n) * int(n)
    zout = np.empty(nc, dtype=np.float32)
    gout = np.empty(nc, dtype=np.int32)
    rg = _region((start, length, safe))
    stored = C.c_size_t()
    if L.pf_debug_distribute_back(int(n), int(x0), int(nxl), C.byref(rg), count, pp, z.ctypes.data_as(C.POINTER(C.c_float)),
                                  g.ctypes.data_as(C.POINTER(C.c_int)), zout.ctypes.data_as(C.POINTER(C.c_float)),
                                  gout.ctypes.data_as(C.POINTER(C.c_int)), C.byref(stored)):
        raise PinfmaxError(L.pf_last_error().decode() or "pf_debug_distribute_back failed")
    return zout, gout, int(stored.value)


def _order(order, count):
    """None, or indices[] of sort_and_organize: one int32 per particle"""
    if order is None:
        return None, None
    o = np.ascontiguousarray(order, dtype=np.int32).ravel()
    if o.size != count:
        raise ValueError(f"an order of {o.size} entries for {count} particles")
    return o, o.ctypes.data_as(C.POINTER(C.c_int))


def prev_layout(off_Vel_prev=-1, off_Vel_2LPT_prev=-1, off_Vel_3LPT_1_prev=-1, off_Vel_3LPT_2_prev=-1):
    """byte offsets of the Vel*_prev fields of a record (pf_prev_layout); negative = absent"""
    return _lib.PrevLayout(int(off_Vel_prev), int(off_Vel_2LPT_prev), int(off_Vel_3LPT_1_prev), int(off_Vel_3LPT_2_prev))


def debug_gather_velocities(n: int, x0: int, cols24: np.ndarray, box, frag_pos, order=None):
    """the velocity gather of pf_gather_velocities by the device kernels without a context (pf_debug_gather_velocities): cols24 =
    [24][nxl n n] float32 or float64, the current columns 0..11 and the prev columns 0..11 of the slab planes x0 .. x0 + nxl - 1 of
    an n^3 box; box = (start, length, safe); the particles at the sub-box positions frag_pos; order None or indices[] of
    sort_and_organize -> (index[found], vel24[found][24]) in ascending particle index"""
    L = _lib.load()
    cols = np.ascontiguousarray(cols24)
    if cols.dtype not in (np.float32, np.float64):
        cols = cols.astype(np.float32)
    if cols.ndim != 2 or cols.shape[0] != 24 or cols.shape[1] % (int(n) * int(n)):
        raise ValueError(f"columns of shape {cols.shape} for slab planes of {n} x {n} cells")
    nxl = cols.shape[1] // (int(n) * int(n))
    pos = np.ascontiguousarray(frag_pos, dtype=np.uint32).ravel()
    o, op = _order(order, pos.size)
    index = np.empty(pos.size, dtype=np.uint32)
    vel = np.empty((pos.size, 24), dtype=cols.dtype)
    found = C.c_size_t()
    rg = _region(box)
    if L.pf_debug_gather_velocities(int(n), int(x0), nxl, cols.dtype.itemsize, cols.ctypes.data_as(C.c_void_p), C.byref(rg), pos.size,
                                    pos.ctypes.data_as(C.POINTER(C.c_uint)), op, index.ctypes.data_as(C.POINTER(C.c_uint)),
                                    vel.ctypes.data_as(C.c_void_p), C.byref(found)):
        raise PinfmaxError(L.pf_last_error().decode() or "pf_debug_gather_velocities failed")
    return index[:found.value], vel[:found.value]


def debug_point_states(n: int, x0: int, fmax_col: np.ndarray, cols24: np.ndarray, tables, myseg, z_seg, box, frag_pos, sigma0, k_sigma, k_point, groups_order=2,
                       z_prev=0.0, use_v31=False, order=None):
    """the particle states of pf_point_states by the device kernel on a caller's columns (pf_debug_point_states): fmax_col [nxl n n]
    and cols24 [24][nxl n n] (as debug_gather_velocities takes them) of one dtype, float32 or float64, for the slab planes x0 ..
    x0 + nxl - 1 of an n^3 box; tables: an Fmax whose plc_set_cosmology supplies the growth tables and nothing else; groups_order =
    par->order (ORDER_FOR_GROUPS); order: None or indices[] of sort_and_organize -> (index[found], states[found][8])"""
    L = _lib.load()
    cols = np.ascontiguousarray(cols24)
    if cols.dtype not in (np.float32, np.float64):
        cols = cols.astype(np.float32)
    fm = np.ascontiguousarray(fmax_col, dtype=cols.dtype).ravel()
    if cols.ndim != 2 or cols.shape[0] != 24 or cols.shape[1] % (int(n) * int(n)) or fm.size != cols.shape[1]:
        raise ValueError(f"columns of shapes {fm.shape} and {cols.shape} for slab planes of {n} x {n} cells")
    nxl = cols.shape[1] // (int(n) * int(n))
    pos = np.ascontiguousarray(frag_pos, dtype=np.uint32).ravel()
    o, op = _order(order, pos.size)
    index = np.empty(pos.size, dtype=np.uint32)
    st = np.empty((pos.size, 8), dtype=cols.dtype)
    found = C.c_size_t()
    rg = _region(box)
    seg = _lib.PlcSegment(int(myseg), int(bool(use_v31)), float(z_seg), float(z_prev))
    par = _lib.PointParams(float(sigma0), float(k_sigma), float(k_point), int(groups_order))
    if L.pf_debug_point_states(int(n), int(x0), nxl, cols.dtype.itemsize, fm.ctypes.data_as(C.c_void_p), cols.ctypes.data_as(C.c_void_p), tables.h, C.byref(seg),
                               C.byref(rg), C.byref(par), pos.size, pos.ctypes.data_as(C.POINTER(C.c_uint)), op, index.ctypes.data_as(C.POINTER(C.c_uint)),
                               st.ctypes.data_as(C.c_void_p), C.byref(found)):
        raise PinfmaxError(L.pf_last_error().decode() or "pf_debug_point_states failed")
    return index[:found.value], st[:found.value]


def group_layout(stride, off_Mass=-1, off_Vel=-1, off_Vel_2LPT=-1, off_Vel_3LPT_1=-1, off_Vel_3LPT_2=-1, off_Vel_prev=-1, off_Vel_2LPT_prev=-1,
                 off_Vel_3LPT_1_prev=-1, off_Vel_3LPT_2_prev=-1):
    """byte offsets of Mass and the Vel* / Vel*_prev fields of a group record (pf_group_layout); negative = absent"""
    return _lib.GroupLayout(int(stride), int(off_Mass), int(off_Vel), int(off_Vel_2LPT), int(off_Vel_3LPT_1), int(off_Vel_3LPT_2), int(off_Vel_prev),
                            int(off_Vel_2LPT_prev), int(off_Vel_3LPT_1_prev), int(off_Vel_3LPT_2_prev))


def plc_group_layout(stride, off_Mass, off_Pos, off_Flast, off_name=-1, off_good=-1, off_point=-1, off_Vel=-1, off_Vel_2LPT=-1, off_Vel_3LPT_1=-1,
                     off_Vel_3LPT_2=-1, off_Vel_prev=-1, off_Vel_2LPT_prev=-1, off_Vel_3LPT_1_prev=-1, off_Vel_3LPT_2_prev=-1):
    """byte offsets of the fields of a group record the light-cone test reads (pf_plc_group_layout); negative = absent"""
    return _lib.PlcGroupLayout(int(stride), int(off_Mass), int(off_Pos), int(off_name), int(off_Flast), int(off_good), int(off_point), int(off_Vel),
                               int(off_Vel_2LPT), int(off_Vel_3LPT_1), int(off_Vel_3LPT_2), int(off_Vel_prev), int(off_Vel_2LPT_prev),
                               int(off_Vel_3LPT_1_prev), int(off_Vel_3LPT_2_prev))


def plc_out_dtype(double_products=False):
    """plcgroup_data (src/pinocchio.h:430-435) as the compiler lays it out: 48 bytes, 72 with PRODFLOAT double"""
    f, pb = ("<f8", 8) if double_products else ("<f4", 4)
    return np.dtype({"names": ["Mass", "name", "z", "x", "v"], "formats": ["<i4", "<u8", f, (f, 3), (f, 3)],
                     "offsets": [0, 8, 16, 16 + pb, 16 + 4 * pb], "itemsize": 72 if double_products else 48})


def plc_out_layout(dtype):
    """pf_plc_out_layout of a structured dtype with (some of) the fields Mass, name, z, x, v"""
    off = {k: (dtype.fields[k][1] if k in dtype.fields else -1) for k in ("Mass", "name", "z", "x", "v")}
    return _lib.PlcOutLayout(dtype.itemsize, off["Mass"], off["name"], off["z"], off["x"], off["v"])


def catalog_dtype(double_products=False, light=False):
    """catalog_data (src/pinocchio.h:515-524) as the compiler lays it out: 56 bytes, 96 with PRODFLOAT double; 48 / 88 with
    LIGHT_OUTPUT (no n, no pad)"""
    f, pb = ("<f8", 8) if double_products else ("<f4", 4)
    names, formats, offsets = ["name", "M", "x", "v", "q"], ["<u8", f, (f, 3), (f, 3), (f, 3)], [0, 8, 8 + pb, 8 + 4 * pb, 8 + 7 * pb]
    size = 8 + 10 * pb
    if not light:
        names, formats, offsets = names + ["n", "pad"], formats + ["<i4", "<i4"], offsets + [size, size + 4]
        size += 8
    return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": size})


def catalog_out_layout(dtype):
    """pf_catalog_out_layout of a structured dtype with (some of) the fields name, M, x, v, q, n"""
    off = {k: (dtype.fields[k][1] if k in dtype.fields else -1) for k in ("name", "M", "x", "v", "q", "n")}
    return _lib.CatalogOutLayout(dtype.itemsize, off["name"], off["M"], off["x"], off["v"], off["q"], off["n"])


def plc_group_layout_of(dtype):
    """pf_plc_group_layout of a structured dtype whose fields carry the reference's names (Mass, Pos, Flast, name, good, point, Vel, ...)"""
    kw = {"off_" + k: dtype.fields[k][1] for k in ("Mass", "Pos", "Flast", "name", "good", "point", "Vel", "Vel_2LPT", "Vel_3LPT_1", "Vel_3LPT_2",
                                                   "Vel_prev", "Vel_2LPT_prev", "Vel_3LPT_1_prev", "Vel_3LPT_2_prev") if k in dtype.fields}
    return plc_group_layout(dtype.itemsize, **kw)


def _group_ids(group_id, count):
    """group_ID of every particle as the calls take it: (array kept alive, pointer to the first int, byte stride).  A packed int32
    array, or a strided int32 view of a field of the caller's records (read in place)"""
    g = np.asarray(group_id)
    if g.dtype != np.int32 or g.ndim != 1:
        g = np.ascontiguousarray(g, dtype=np.int32).ravel()
    if g.size != count:
        raise ValueError(f"{g.size} group IDs for {count} particles")
    stride = g.strides[0] if g.size > 1 else 4
    if stride <= 0:
        g = np.ascontiguousarray(g)
        stride = 4
    return g, C.cast(C.c_void_p(g.ctypes.data), C.POINTER(C.c_int)), stride


def debug_group_velocity_sums(n: int, x0: int, cols24: np.ndarray, box, frag_pos, group_id, first_group=2):
    """the group sums of pf_group_velocity_sums by the device kernels without a context (pf_debug_group_velocity_sums): cols24 =
    [24][nxl n n] float32 or float64 as for debug_gather_velocities; the particles at the sub-box positions frag_pos with the group
    IDs group_id -> (group[G], npart[G], sum24[G][24] float64, particles counted), the groups in ascending ID"""
    L = _lib.load()
    cols = np.ascontiguousarray(cols24)
    if cols.dtype not in (np.float32, np.float64):
        cols = cols.astype(np.float32)
    if cols.ndim != 2 or cols.shape[0] != 24 or cols.shape[1] % (int(n) * int(n)):
        raise ValueError(f"columns of shape {cols.shape} for slab planes of {n} x {n} cells")
    nxl = cols.shape[1] // (int(n) * int(n))
    pos = np.ascontiguousarray(frag_pos, dtype=np.uint32).ravel()
    g = np.ascontiguousarray(group_id, dtype=np.int32).ravel()
    if g.size != pos.size:
        raise ValueError(f"{g.size} group IDs for {pos.size} particles")
    group = np.empty(pos.size, dtype=np.int32)
    npart = np.empty(pos.size, dtype=np.uint32)
    sums = np.empty((pos.size, 24), dtype=np.float64)
    ng, npc = C.c_size_t(), C.c_size_t()
    rg = _region(box)
    if L.pf_debug_group_velocity_sums(int(n), int(x0), nxl, cols.dtype.itemsize, cols.ctypes.data_as(C.c_void_p), C.byref(rg), pos.size,
                                      pos.ctypes.data_as(C.POINTER(C.c_uint)), g.ctypes.data_as(C.POINTER(C.c_int)), int(first_group),
                                      group.ctypes.data_as(C.POINTER(C.c_int)), npart.ctypes.data_as(C.POINTER(C.c_uint)),
                                      sums.ctypes.data_as(C.POINTER(C.c_double)), C.byref(ng), C.byref(npc)):
        raise PinfmaxError(L.pf_last_error().decode() or "pf_debug_group_velocity_sums failed")
    return group[:ng.value], npart[:ng.value], sums[:ng.value], int(npc.value)


def debug_groupvel_times():
    """device ms of the last group-velocity call's stages (keys + sort, head flags + scan, reduce + fold) when PF_GROUPVEL_TIMES=1 is
    set in the environment, zeros otherwise (pf_debug_groupvel_times)"""
    L = _lib.load()
    ms = (C.c_double * 3)()
    L.pf_debug_groupvel_times(ms)
    return {"sort_ms": ms[0], "heads_ms": ms[1], "reduce_ms": ms[2]}


_WHICH = {"current": _lib.MAP_CURRENT, "update": _lib.MAP_UPDATE}


def _which(which):
    """"current" (frag_map) / "update" (frag_map_update), or the integer itself (the library refuses one that names no array)"""
    return _WHICH[which] if isinstance(which, str) else int(which)


class FragMap:
    """The two maps of fragment() (src/fragment.c:193-346) resident on the device (pf_map): CURRENT = frag_map and UPDATE =
    frag_map_update over the sub-box (start, length, safe) = (subbox.stabl, subbox.Lgwbl, subbox.safe).  ctx: the Fmax context
    whose distribute / count_peaks calls read the map (a direction is periodic when length == n); None: context-free, a direction
    is periodic when safe == 0.  A context manager: the map is destroyed on exit (before its context)."""

    def __init__(self, start, length, safe, ctx=None):
        self.L = _lib.load()
        self.ctx = ctx
        self.start, self.length, self.safe = tuple(map(int, start)), tuple(map(int, length)), tuple(map(int, safe))
        self.h = None
        h = C.c_void_p()
        rg = _region((self.start, self.length, self.safe))
        self._chk(self.L.pf_map_create(ctx.h if ctx is not None else None, C.byref(rg), C.byref(h)))
        self.h = h
        self.nwords = int(self.L.pf_map_length(self.h))
        if ctx is not None:
            ctx._maps.add(self)        # the context destroys the maps that are still open before itself (Fmax.close)

    def _chk(self, rc):
        if rc:
            raise PinfmaxError(self.L.pf_last_error().decode() or f"error {rc}")

    def close(self):
        if getattr(self, "h", None):
            self.L.pf_map_destroy(self.h)
            self.h = None
        if self.ctx is not None:
            self.ctx._maps.discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def fill_box(self):
        """create_map() (src/fragment.c:708-751): UPDATE := the well resolved box plus one layer"""
        self._chk(self.L.pf_map_fill_box(self.h))

    def update(self, pos, mass, boundary_layer_factor: float):
        """update_map() (src/build_groups.c:2246-2318): UPDATE := the spheres of the groups (pos [ngroups][3] in sub-box
        coordinates, mass [ngroups] int) that CURRENT does not hold -> (nadd0, nadd1): cells requested (with multiplicity) and
        cube cells beyond the boundary layer"""
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        mass = np.ascontiguousarray(mass, dtype=np.int32).ravel()
        if len(pos) != len(mass):
            raise ValueError(f"{len(pos)} positions for {len(mass)} masses")
        out = (C.c_ulonglong * 2)()
        self._chk(self.L.pf_map_update(self.h, len(mass), _dp(pos), mass.ctypes.data_as(C.POINTER(C.c_int)), float(boundary_layer_factor), out))
        return int(out[0]), int(out[1])

    def commit(self, merge):
        """CURRENT = UPDATE (merge false: turn 0) or CURRENT |= UPDATE (merge true: turn 1), src/fragment.c:304-309"""
        self._chk(self.L.pf_map_commit(self.h, 1 if merge else 0))

    def words(self, which="current") -> np.ndarray:
        w = np.empty(self.nwords, dtype=np.uint32)
        self._chk(self.L.pf_map_get(self.h, _which(which), w.ctypes.data_as(C.POINTER(C.c_uint))))
        return w

    def set_words(self, which, w):
        w = np.ascontiguousarray(w, dtype=np.uint32).ravel()
        if w.size != self.nwords:
            raise ValueError(f"{w.size} words for a map of {self.nwords}")
        self._chk(self.L.pf_map_set(self.h, _which(which), w.ctypes.data_as(C.POINTER(C.c_uint))))

    def atomics(self) -> int:
        """atomicOr issued by the last update() of a map created under PF_MAP_STATS=1 (measurement aid)"""
        out = C.c_ulonglong()
        self._chk(self.L.pf_debug_map_atomics(self.h, C.byref(out)))
        return int(out.value)

    def count(self, which="current") -> int:
        out = C.c_ulonglong()
        self._chk(self.L.pf_map_count(self.h, _which(which), C.byref(out)))
        return int(out.value)


class Fmax:
    """One rank's context: an x-slab of an n^3 grid on one MI355X."""

    def __init__(self, n: int, rank: int = 0, nranks: int = 1, device: int = 0, field_bytes: int = 8,
                 timing: bool = False, double_products: bool = False):
        self.L = _lib.load()
        self.double_products = bool(double_products)
        self.n, self.rank, self.nranks = int(n), int(rank), int(nranks)
        self.nxl = self.n // self.nranks
        cfg = _lib.Config(n=n, rank=rank, nranks=nranks, device=device, field_bytes=field_bytes,
                          flags=(_lib.FLAG_TIMING if timing else 0) | (_lib.FLAG_DOUBLE_PRODUCTS if double_products else 0))
        h = C.c_void_p()
        self._chk(self.L.pf_create(C.byref(h), C.byref(cfg)))
        self.h = h
        self._keep = []
        self._maps = weakref.WeakSet()  # open FragMaps bound to this context: pf_map_destroy must come before pf_destroy

    # -- plumbing ---------------------------------------------------------
    def _chk(self, rc):
        if rc:
            raise PinfmaxError(self.L.pf_last_error().decode() or f"error {rc}")

    def close(self):
        if getattr(self, "h", None):
            for m in list(getattr(self, "_maps", ())):
                m.close()
            self.L.pf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def synchronize(self):
        self._chk(self.L.pf_synchronize(self.h))

    @property
    def device_bytes(self) -> int:
        return int(self.L.pf_device_bytes(self.h))

    # -- inputs -----------------------------------------------------------
    def set_density(self, dk: np.ndarray):
        """kdensity[0]: this rank's x-slab [nxl][n][n/2+1] complex128."""
        dk = np.ascontiguousarray(dk, dtype=np.complex128)
        if dk.shape != (self.nxl, self.n, self.n // 2 + 1):
            raise ValueError(f"density slab shape {dk.shape}")
        self._chk(self.L.pf_set_density(self.h, _dp(dk.view(np.float64))))

    def synth_density(self, seed: int, sigma0: float = 2.5, slope: float = -2.0):
        self._chk(self.L.pf_synth_density(self.h, C.c_uint64(seed), sigma0, slope))

    def genic_density(self, seed: int, box_true_mpc: float, omega0: float, omega_baryon: float, hubble100: float,
                      primordial_index: float, sigma8: float = 0.0, pknorm: float = 0.0, fixed: bool = False, paired: bool = False,
                      pk_table=None, spectrum: str = "EH", wdm_mass_kev: float = 0.0) -> float:
        """GenIC_large (src/GenIC.c:73) on the device.  Give PkNorm, or sigma8 to have it computed
        (normalize_PowerSpectrum, src/cosmo.c:1058).  pk_table = (log10 k [1/Mpc], log10(k^3 P)): a tabulated spectrum
        (SPLINE[SP_PK]) instead of Eisenstein & Hu; PkNorm is then what the caller says (1 for a trusted table).
        spectrum "Efstathiou" / "PowerLaw": the other two analytic forms of PowerSpectrum(); wdm_mass_kev > 0: its warm-dark-matter
        cut-off (src/cosmo.c:953-1007).  Returns the PkNorm used."""
        p = _lib.GenicParams(omega0, omega_baryon, hubble100, primordial_index, box_true_mpc, pknorm, seed, int(fixed), int(paired))
        p.spectrum = {"EH": 0, "Efstathiou": 3, "PowerLaw": 4}[spectrum]   # FileWithInputSpectrum (src/cosmo.c:1009-1046)
        p.WDM_PartMass_in_kev = wdm_mass_kev
        if pk_table is not None:
            lk = np.ascontiguousarray(pk_table[0], dtype=np.float64)
            lp = np.ascontiguousarray(pk_table[1], dtype=np.float64)
            assert lk.shape == lp.shape and lk.ndim == 1
            p.pk_n, p.pk_logk, p.pk_logk3p = len(lk), _dp(lk), _dp(lp)
            if pknorm <= 0.0:
                p.PkNorm = 1.0
        elif pknorm <= 0.0:
            v = C.c_double()
            self._chk(self.L.pf_pk_norm(C.byref(p), sigma8, C.byref(v)))
            p.PkNorm = v.value
        self._chk(self.L.pf_genic_density(self.h, C.byref(p)))
        return p.PkNorm

    def set_invgrow(self, x, y, ismooth: int = -1):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        self._chk(self.L.pf_set_invgrow(self.h, ismooth, _dp(x), _dp(y), len(x)))

    def set_growth(self, g):
        g = np.ascontiguousarray(g, dtype=np.float64)
        assert g.shape == (4,)
        self._chk(self.L.pf_set_growth(self.h, _dp(g)))

    def set_growth_table(self, order: int, log10_growth, logkmin: float = -3.0, dlogk: float = 0.5, sign: float = 1.0):
        """k-binned growth of ScaleDep.order = order (SCALE_DEPENDENT build, src/cosmo.c:1728-1755); empty: scalar"""
        t = np.ascontiguousarray(log10_growth, dtype=np.float64)
        self._chk(self.L.pf_set_growth_table(self.h, int(order), _dp(t) if len(t) else None, len(t), logkmin, dlogk, sign))

    def set_collapse_model(self, model: int, cosmo=None, d_in=None):
        """0: ELL_CLASSIC; 1: ELL_SNG (table only) with cosmo = (Omega0, OmegaLambda, OmegaRad, OmegaK), D_in per radius"""
        cs = np.ascontiguousarray(cosmo, dtype=np.float64) if cosmo is not None else None
        di = np.ascontiguousarray(d_in, dtype=np.float64) if d_in is not None else None
        self._chk(self.L.pf_set_collapse_model(self.h, model, _dp(cs) if cs is not None else None, len(di) if di is not None else 0,
                                               _dp(di) if di is not None else None))

    def set_modified_gravity(self, fr0: float, h_over_c: float = 100.0 / 299792.458, size=None):
        """MOD_GRAV_FR force modification inside the ELL_SNG system (src/collapse_times.c:295-312); fr0 = 0: off"""
        sz = np.ascontiguousarray(size, dtype=np.float64) if size is not None else None
        self._chk(self.L.pf_set_modified_gravity(self.h, fr0, h_over_c, len(sz) if sz is not None else 0, _dp(sz) if sz is not None else None))

    def set_tabulated_ct(self, variance):
        """TABULATED_CT build: Smoothing.Variance[] per radius ([] = direct solve), src/collapse_times.c:780-1231"""
        v = np.ascontiguousarray(variance, dtype=np.float64)
        self._chk(self.L.pf_set_tabulated_ct(self.h, len(v), _dp(v) if len(v) else None))

    def ct_build(self, ismooth: int, variance: float) -> np.ndarray:
        """initialize_collapse_times(ismooth): -> CT_table[iy][ix][id]"""
        t = np.empty((50, 50, 100))
        self._chk(self.L.pf_ct_build(self.h, ismooth, variance, _dp(t)))
        return t

    def ct_load(self, ismooth: int, variance: float, table: np.ndarray):
        t = np.ascontiguousarray(table, dtype=np.float64)
        assert t.shape == (50, 50, 100)
        self._chk(self.L.pf_ct_load(self.h, ismooth, variance, _dp(t)))

    # -- the path (reference names) ----------------------------------------
    def sweep(self, radii_cells) -> np.ndarray:
        """radius loop of compute_fmax (src/fmax.c:66-150) -> TrueVariance[]"""
        r = np.ascontiguousarray(radii_cells, dtype=np.float64)
        tv = np.zeros(len(r))
        self._chk(self.L.pf_sweep(self.h, len(r), _dp(r), _dp(tv)))
        return tv

    def compute_fmax(self, radii_cells, do_lpt: bool = True) -> np.ndarray:
        """compute_fmax (src/fmax.c:36-190): sweep, then compute_displacements(1,0,z)"""
        self._chk(self.L.pf_set_sources_in_sweep(self.h, 1 if do_lpt else 0))
        try:
            tv = self.sweep(radii_cells)
        finally:
            self.L.pf_set_sources_in_sweep(self.h, 0)
        if do_lpt:
            self.compute_displacements(1, 0)
        return tv

    def compute_second_derivatives(self, radius_cells: float):
        self._chk(self.L.pf_second_derivatives(self.h, float(radius_cells)))

    def compute_collapse_times(self, ismooth: int) -> float:
        tv = C.c_double()
        self._chk(self.L.pf_collapse_times(self.h, ismooth, C.byref(tv)))
        return tv.value

    def set_transposed_spectra(self, on: bool):
        """spectra cross the interface as [ky_local][kx][kz] (params.use_transposed_fft on slabs)"""
        self._chk(self.L.pf_set_transposed_spectra(self.h, 1 if on else 0))

    def set_ct_interpolation(self, flavour: int):
        """0 BILINEAR_SPLINE (default), 1 -DTRILINEAR, 2 -DALL_SPLINE"""
        self._chk(self.L.pf_set_ct_interpolation(self.h, int(flavour)))

    def set_lpt_order(self, order: int):
        """3: -DTWO_LPT -DTHREE_LPT (default); 2: -DTWO_LPT only; 1: Zel'dovich displacements only"""
        self._chk(self.L.pf_set_lpt_order(self.h, int(order)))

    def compute_displacements(self, compute_sources: int = 1, recompute_sd: int = 0):
        self._chk(self.L.pf_displacements(self.h, int(compute_sources), int(recompute_sd)))

    def Fmax_PDF(self) -> np.ndarray:
        h = (C.c_ulonglong * _lib.NBINS)()
        self._chk(self.L.pf_fmax_pdf(self.h, h))
        return np.array(h[:], dtype=np.uint64)

    # -- outputs ----------------------------------------------------------
    def products(self) -> np.ndarray:
        lay = _lib.ProductLayout()
        self.L.pf_layout_3lpt(C.byref(lay))
        dtype = PRODUCT_DTYPE
        if self.double_products:      # PRODFLOAT double: the natural alignment of the reference's struct (Fmax at byte 8)
            dtype = PRODUCT_DTYPE_DP
            lay.stride, lay.off_Rmax, lay.off_Fmax = 112, 0, 8
            lay.off_Vel, lay.off_Vel_2LPT, lay.off_Vel_3LPT_1, lay.off_Vel_3LPT_2 = 16, 40, 64, 88
        out = np.zeros((self.nxl, self.n, self.n), dtype=dtype)
        self._chk(self.L.pf_get_products(self.h, out.ctypes.data_as(C.c_void_p), C.byref(lay)))
        return out

    def update_products(self, records: np.ndarray, layout) -> np.ndarray:
        """merge the device columns named by `layout` (a _lib.ProductLayout) into caller-held AoS records"""
        assert records.flags.c_contiguous and records.nbytes == self.nxl * self.n * self.n * layout.stride
        self._chk(self.L.pf_update_products(self.h, records.ctypes.data_as(C.c_void_p), C.byref(layout)))
        return records

    def select_sorted(self, flast: float):
        """cells with Fmax >= flast by descending Fmax (src/distribute.c:695, src/fragment.c:484-503) -> (index, Fmax)"""
        cnt = C.c_size_t()
        self._chk(self.L.pf_select_sorted(self.h, flast, 0, None, None, C.byref(cnt)))
        idx = np.empty(cnt.value, dtype=np.uint32)
        f = np.empty(cnt.value, dtype=np.float32)
        if cnt.value:
            self._chk(self.L.pf_select_sorted(self.h, flast, cnt.value, idx.ctypes.data_as(C.POINTER(C.c_uint)),
                                              f.ctypes.data_as(C.POINTER(C.c_float)), C.byref(cnt)))
        return idx, f

    def frag_map(self, start, length, safe) -> FragMap:
        """a resident map of the sub-box (subbox.stabl, subbox.Lgwbl, subbox.safe) bound to this context"""
        return FragMap(start, length, safe, ctx=self)

    def _own_map(self, m, start=None, length=None):
        if m.ctx is not self:
            raise ValueError("the FragMap belongs to another context")
        if (start is not None and tuple(map(int, start)) != m.start) or (length is not None and tuple(map(int, length)) != m.length):
            raise ValueError(f"start {tuple(start)} / length {tuple(length)} disagree with the map's box {m.start} / {m.length}")

    def count_peaks(self, flast: float, region=None, map=None, which="current"):
        """count_peaks (src/fragment.c:605-706): (peaks of the region, those in its well resolved part), summed over ranks.
        region = (start[3], len[3], safe[3]) in global grid coordinates, None = the whole periodic box.  map = a FragMap of this
        context: the count over the STORED set of the map's box (bit of `which` set and Fmax >= flast), the reference's Npeaks of
        either turn.  Collective."""
        out = (C.c_ulonglong * 2)()
        if map is not None:
            if region is not None:
                raise ValueError("a FragMap carries its own region")
            self._own_map(map)
            self._chk(self.L.pf_count_peaks_map(self.h, float(flast), map.h, _which(which), out))
            return int(out[0]), int(out[1])
        rg = _region(region)
        self._chk(self.L.pf_count_peaks(self.h, float(flast), C.byref(rg) if rg is not None else None, out))
        return int(out[0]), int(out[1])

    def select_peaks(self, flast: float):
        """this rank's peaks of the whole box by descending Fmax, ties by ascending index -> (local index, Fmax).  Collective."""
        cnt = C.c_size_t()
        # one call with room for every cell of the slab would do; two calls keep the host arrays at the size of the list
        self._chk(self.L.pf_select_peaks(self.h, float(flast), 0, None, None, C.byref(cnt)))
        idx = np.empty(cnt.value, dtype=np.uint32)
        f = np.empty(cnt.value, dtype=np.float32)
        self._chk(self.L.pf_select_peaks(self.h, float(flast), cnt.value, idx.ctypes.data_as(C.POINTER(C.c_uint)),
                                         f.ctypes.data_as(C.POINTER(C.c_float)), C.byref(cnt)))
        return idx, f

    def product_layout(self):
        """(pf_product_layout, numpy dtype) of the record products() returns"""
        lay = _lib.ProductLayout()
        self.L.pf_layout_3lpt(C.byref(lay))
        if not self.double_products:
            return lay, PRODUCT_DTYPE
        lay.stride, lay.off_Rmax, lay.off_Fmax = 112, 0, 8
        lay.off_Vel, lay.off_Vel_2LPT, lay.off_Vel_3LPT_1, lay.off_Vel_3LPT_2 = 16, 40, 64, 88
        return lay, PRODUCT_DTYPE_DP

    def distribute(self, flast: float, start, length, map=None, layout=None, capacity=None, which="current"):
        """This rank's contribution to the sub-box (start[3], length[3]) = (subbox.stabl, subbox.Lgwbl) in distribute()
        (src/distribute.c:58-175): the cells of intersection(this slab, sub-box) whose bit of `map` (uint32 words, None: every
        bit) is set and whose Fmax >= flast, in the reference's order -> (records, frag_pos, count).  layout None: the record of
        products() as a structured array; a _lib.ProductLayout: rows of `stride` bytes.  capacity None: room for all (a
        count-only call first); otherwise at most `capacity` entries are returned and count still says how many were taken.
        map = a FragMap of this context: its array `which` ("current" / "update") is read on the device, nothing is uploaded;
        start / length must be the map's.  Not collective."""
        dtype = None
        if layout is None:
            layout, dtype = self.product_layout()
        if isinstance(map, FragMap):
            self._own_map(map, start, length)

            def call(cap, rec, pos, cnt):
                return self.L.pf_distribute_map(self.h, float(flast), map.h, _which(which), C.byref(layout), cap, rec, pos, C.byref(cnt))
        else:
            sub = _subbox(start, length)
            keep, mp = _distmap(map, length)

            def call(cap, rec, pos, cnt):
                return self.L.pf_distribute(self.h, float(flast), C.byref(sub), mp, C.byref(layout), cap, rec, pos, C.byref(cnt))
        cnt = C.c_size_t()
        if capacity is None:
            self._chk(call(0, None, None, cnt))
            capacity = cnt.value
        capacity = int(capacity)
        rec = np.zeros((capacity, layout.stride), dtype=np.uint8)
        pos = np.empty(capacity, dtype=np.uint32)
        self._chk(call(capacity, rec.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.POINTER(C.c_uint)), cnt))
        m = min(cnt.value, capacity)
        rec = rec[:m]
        if dtype is not None:
            rec = rec.view(dtype).reshape(m)
        return rec, pos[:m], int(cnt.value)

    def distribute_sorted(self, flast: float, start, length, map=None, layout=None, capacity=None, which="current"):
        """distribute() followed by sort_and_organize() (src/fragment.c:484-520) for this rank's contribution to the sub-box:
        the records of distribute() by descending Fmax (ties in distribute()'s order) -> (records, frag_pos, sorted_pos, indices,
        count), with sorted_pos ascending = frag_pos[indices] (what find_location, :592-603, searches).  Arguments as
        distribute(); with a capacity below the count the first `capacity` records of the sorted order come back and
        sorted_pos / indices describe those.  map = a FragMap: as in distribute().  Not collective."""
        dtype = None
        if layout is None:
            layout, dtype = self.product_layout()
        if isinstance(map, FragMap):
            self._own_map(map, start, length)

            def call(cap, rec, pos, spos, ind, cnt):
                return self.L.pf_distribute_sorted_map(self.h, float(flast), map.h, _which(which), C.byref(layout), cap, rec, pos, spos, ind, C.byref(cnt))
        else:
            sub = _subbox(start, length)
            keep, mp = _distmap(map, length)

            def call(cap, rec, pos, spos, ind, cnt):
                return self.L.pf_distribute_sorted(self.h, float(flast), C.byref(sub), mp, C.byref(layout), cap, rec, pos, spos, ind, C.byref(cnt))
        cnt = C.c_size_t()
        if capacity is None:
            self._chk(call(0, None, None, None, None, cnt))
            capacity = cnt.value
        capacity = int(capacity)
        rec = np.zeros((capacity, layout.stride), dtype=np.uint8)
        pos = np.empty(capacity, dtype=np.uint32)
        spos = np.empty(capacity, dtype=np.uint32)
        ind = np.empty(capacity, dtype=np.int32)
        self._chk(call(capacity, rec.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.POINTER(C.c_uint)), spos.ctypes.data_as(C.POINTER(C.c_uint)),
                       ind.ctypes.data_as(C.POINTER(C.c_int)), cnt))
        m = min(cnt.value, capacity)
        rec = rec[:m]
        if dtype is not None:
            rec = rec.view(dtype).reshape(m)
        return rec, pos[:m], spos[:m], ind[:m], int(cnt.value)

    def distribute_sorted_neighbours(self, flast: float, map: FragMap, which="current", layout=None, capacity=None):
        """distribute_sorted() over the box of a FragMap of this context plus the neighbour table of the records it returns, in one
        call (pf_distribute_sorted_neighbours_map) -> (records, frag_pos, sorted_pos, indices, neigh[count, 6], flags, (npeaks,
        ngood), count).  The first four and count are those of distribute_sorted(); neigh / flags / peaks as neighbours(), for the
        box and safety layers of the map; with a capacity below the count they describe the returned records only.  Not collective."""
        dtype = None
        if layout is None:
            layout, dtype = self.product_layout()
        self._own_map(map)
        cnt = C.c_size_t()
        peaks = (C.c_ulonglong * 2)()

        def call(cap, rec, pos, spos, ind, nb, fl, pk):
            return self.L.pf_distribute_sorted_neighbours_map(self.h, float(flast), map.h, _which(which), C.byref(layout), cap, rec, pos, spos, ind,
                                                              nb, fl, pk, C.byref(cnt))
        if capacity is None:
            self._chk(call(0, None, None, None, None, None, None, None))
            capacity = cnt.value
        capacity = int(capacity)
        rec = np.zeros((capacity, layout.stride), dtype=np.uint8)
        pos = np.empty(capacity, dtype=np.uint32)
        spos = np.empty(capacity, dtype=np.uint32)
        ind = np.empty(capacity, dtype=np.int32)
        neigh = np.empty((capacity, 6), dtype=np.int32)
        flags = np.empty(capacity, dtype=np.uint8)
        self._chk(call(capacity, rec.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.POINTER(C.c_uint)), spos.ctypes.data_as(C.POINTER(C.c_uint)),
                       ind.ctypes.data_as(C.POINTER(C.c_int)), neigh.ctypes.data_as(C.POINTER(C.c_int)), flags.ctypes.data_as(C.POINTER(C.c_ubyte)), peaks))
        m = min(cnt.value, capacity)
        rec = rec[:m]
        if dtype is not None:
            rec = rec.view(dtype).reshape(m)
        return rec, pos[:m], spos[:m], ind[:m], neigh[:m], flags[:m], (int(peaks[0]), int(peaks[1])), int(cnt.value)

    def neighbours(self, frag_pos, fmax, start, length, safe):
        """neighbours() with this context: Fmax of the context's product precision, a direction periodic when length == n, the
        transfers through the hand-off pieces (pf_neighbours)"""
        return _neighbours(self.L, self.h, frag_pos, fmax, start, length, safe, np.float64 if self.double_products else np.float32)

    # -- distribute_back (src/distribute.c:703-946): zacc and group_ID back to the slab -----------------------------------
    @property
    def _zacc_dtype(self):
        return np.float64 if self.double_products else np.float32

    def back_reset(self):
        """zacc := -1, group_ID := 0 in the two columns of this slab (src/allocations.c:519-524); allocates them at first use"""
        self._chk(self.L.pf_back_reset(self.h))

    def distribute_back(self, start, length, safe, frag_pos, zacc, group_id) -> int:
        """keep_data_back / the loop of send_data_back (src/distribute.c:799-896) with this rank's slab as the receiving fft box
        (pf_distribute_back): of the particles at the sub-box positions frag_pos (None: particle iz at position iz) of the sub-box
        (start, length, safe) = (subbox.stabl, subbox.Lgwbl, subbox.safe) the good ones whose global cell lies in this slab have
        their zacc (the context's product precision) and group_id stored in the columns -> how many were.  zacc and group_id are
        packed arrays or fields of a structured record array (frag["zacc"]): only the values are uploaded.  Not collective."""
        pos, pp, count = _frag_pos(frag_pos, zacc)
        z, zp, zs = _strided(zacc, self._zacc_dtype, count, "zacc")
        g, gp, gs = _strided(group_id, np.int32, count, "group_ID")
        rg = _region((start, length, safe))
        stored = C.c_size_t()
        self._chk(self.L.pf_distribute_back(self.h, C.byref(rg), count, pp, zp, zs, gp, gs, C.byref(stored)))
        return int(stored.value)

    def back_apply(self, pos, zacc, group_id):
        """recv_data_back (src/distribute.c:911-946): entries whose position in THIS slab the sender computed (the back_data of the
        reference's send_data_back); each argument a packed array or a field of a record array (pf_back_apply)"""
        count = int(np.asarray(pos).size)
        p, ppos, ps = _strided(pos, np.uint32, count, "pos")
        z, zp, zs = _strided(zacc, self._zacc_dtype, count, "zacc")
        g, gp, gs = _strided(group_id, np.int32, count, "group_ID")
        self._chk(self.L.pf_back_apply(self.h, count, ppos, ps, zp, zs, gp, gs))

    def update_back(self, records: np.ndarray, off_zacc: int, off_group_ID: int) -> np.ndarray:
        """merge the zacc / group_ID columns into caller-held records of this slab's cells (products[i].zacc / .group_ID) at the
        given byte offsets; a negative offset skips that field, every other byte keeps its value (pf_update_back)"""
        nc = self.nxl * self.n * self.n
        if not (records.flags.c_contiguous and records.flags.writeable and records.nbytes % nc == 0):
            raise ValueError(f"records of {records.nbytes} bytes for {nc} cells")
        self._chk(self.L.pf_update_back(self.h, records.ctypes.data_as(C.c_void_p), records.nbytes // nc, int(off_zacc), int(off_group_ID)))
        return records

    # -- the redshift segments of a RECOMPUTE_DISPLACEMENTS build (src/fragment.c:398-430): Vel*_prev and the refresh of frag[] ---------
    def shift_displacements(self):
        """shift_all_displacements() (src/fragment.c:832-850): the Vel*_prev columns := the Vel* columns; they come into being at the
        first call (pf_shift_displacements)"""
        self._chk(self.L.pf_shift_displacements(self.h))

    def drop_prev(self):
        """frees the Vel*_prev columns (pf_drop_prev)"""
        self._chk(self.L.pf_drop_prev(self.h))

    @property
    def prev_shifts(self) -> int:
        """shifts since creation or since the last drop_prev(); 0: there are no Vel*_prev columns"""
        return int(self.L.pf_prev_shifts(self.h))

    def gather_velocities(self, box, frag_pos, order=None, capacity=None):
        """the velocities of the particles at the sub-box positions frag_pos of the sub-box box = (start, length, safe) whose cells
        lie in this rank's slab (pf_gather_velocities) -> (index, vel24): index[j] = the particle, ascending; vel24[j] = its
        current columns 0..11 then the prev columns 0..11, in the context's product precision.  order: None or indices[] of
        sort_and_organize (same result; another access pattern on the device).  capacity: at most so many entries come back.
        Not collective."""
        pos = np.ascontiguousarray(frag_pos, dtype=np.uint32).ravel()
        o, op = _order(order, pos.size)
        cap = pos.size if capacity is None else int(capacity)
        index = np.empty(cap, dtype=np.uint32)
        vel = np.empty((cap, 24), dtype=self._zacc_dtype)
        found = C.c_size_t()
        rg = _region(box)
        self._chk(self.L.pf_gather_velocities(self.h, C.byref(rg), pos.size, pos.ctypes.data_as(C.POINTER(C.c_uint)), op, cap,
                                              index.ctypes.data_as(C.POINTER(C.c_uint)), vel.ctypes.data_as(C.c_void_p), C.byref(found)))
        m = min(int(found.value), cap)
        return index[:m], vel[:m]

    def refresh_velocities(self, box, frag_pos, frag: np.ndarray, layout, prev=None, order=None) -> int:
        """frag[i] of every particle of frag_pos whose cell lies in this rank's slab gets the Vel* fields named by `layout` (a
        _lib.ProductLayout; off_Rmax / off_Fmax are ignored) and the Vel*_prev fields named by `prev` (prev_layout(); None: none)
        from the columns; every other byte of frag keeps its value (pf_refresh_velocities) -> how many were found.  frag: the
        caller's records, C-contiguous, layout.stride bytes each.  Not collective."""
        pos = np.ascontiguousarray(frag_pos, dtype=np.uint32).ravel()
        o, op = _order(order, pos.size)
        if not (frag.flags.c_contiguous and frag.flags.writeable and frag.nbytes == pos.size * layout.stride):
            raise ValueError(f"records of {frag.nbytes} bytes for {pos.size} particles of {layout.stride} bytes")
        found = C.c_size_t()
        rg = _region(box)
        self._chk(self.L.pf_refresh_velocities(self.h, C.byref(rg), pos.size, pos.ctypes.data_as(C.POINTER(C.c_uint)), op,
                                               frag.ctypes.data_as(C.c_void_p), C.byref(layout), C.byref(prev) if prev is not None else None,
                                               C.byref(found)))
        return int(found.value)

    def group_velocity_sums(self, box, frag_pos, group_id, first_group=2, capacity=None):
        """the fp64 sums of the 24 velocity columns over the particles of every group (pf_group_velocity_sums): of the particles at
        the sub-box positions frag_pos whose cells lie in this rank's slab, those with group_id >= first_group (FILAMENT + 1) ->
        (group, npart, sum24[G][24], groups_found, particles_found), the groups in ascending ID; capacity: at most so many groups
        come back (groups_found counts on).  group_id: int32, packed or a strided view of a field of the records.  Not collective:
        several contributors' npart and sum24 of equal IDs add up."""
        pos = np.ascontiguousarray(frag_pos, dtype=np.uint32).ravel()
        g, gp, gs = _group_ids(group_id, pos.size)
        cap = pos.size if capacity is None else int(capacity)
        group = np.empty(cap, dtype=np.int32)
        npart = np.empty(cap, dtype=np.uint32)
        sums = np.empty((cap, 24), dtype=np.float64)
        ng, npc = C.c_size_t(), C.c_size_t()
        rg = _region(box)
        self._chk(self.L.pf_group_velocity_sums(self.h, C.byref(rg), pos.size, pos.ctypes.data_as(C.POINTER(C.c_uint)), gp, gs, int(first_group), cap,
                                                group.ctypes.data_as(C.POINTER(C.c_int)), npart.ctypes.data_as(C.POINTER(C.c_uint)),
                                                sums.ctypes.data_as(C.POINTER(C.c_double)), C.byref(ng), C.byref(npc)))
        m = min(int(ng.value), cap)
        return group[:m], npart[:m], sums[:m], int(ng.value), int(npc.value)

    def refresh_segment(self, box, frag_pos, group_id, frag=None, layout=None, prev=None, groups=None, ngroups=0, group_layout=None, order=None,
                        first_group=2):
        """the step of fragment.c:416-427 in one call (pf_refresh_segment): the records frag[i] of the LOOSE particles (found,
        group_id < first_group) get their Vel* / Vel*_prev fields as refresh_velocities writes them; record g of `groups`
        (ngroups + 1 records of group_layout.stride bytes) of every group with counted particles gets the means in the fields
        group_layout names.  frag None skips the first half, groups None the second -> (loose, grouped, mass_mismatch)."""
        pos = np.ascontiguousarray(frag_pos, dtype=np.uint32).ravel()
        o, op = _order(order, pos.size)
        g, gp, gs = _group_ids(group_id, pos.size)
        if frag is not None and not (frag.flags.c_contiguous and frag.flags.writeable and frag.nbytes == pos.size * layout.stride):
            raise ValueError(f"records of {frag.nbytes} bytes for {pos.size} particles of {layout.stride} bytes")
        if groups is not None and not (groups.flags.c_contiguous and groups.flags.writeable and groups.nbytes == (int(ngroups) + 1) * group_layout.stride):
            raise ValueError(f"group records of {groups.nbytes} bytes for groups 0 .. {ngroups} of {group_layout.stride} bytes")
        loose, grouped, mism = C.c_size_t(), C.c_size_t(), C.c_size_t()
        rg = _region(box)
        self._chk(self.L.pf_refresh_segment(self.h, C.byref(rg), pos.size, pos.ctypes.data_as(C.POINTER(C.c_uint)), op, gp, gs, int(first_group),
                                            frag.ctypes.data_as(C.c_void_p) if frag is not None else None, C.byref(layout) if layout is not None else None,
                                            C.byref(prev) if prev is not None else None, groups.ctypes.data_as(C.c_void_p) if groups is not None else None,
                                            int(ngroups), C.byref(group_layout) if group_layout is not None else None, C.byref(loose), C.byref(grouped),
                                            C.byref(mism)))
        return int(loose.value), int(grouped.value), int(mism.value)

    def point_states(self, myseg, z_seg, box, frag_pos, sigma0, k_sigma, k_point, groups_order=2, z_prev=0.0, use_v31=False, order=None, capacity=None):
        """what condition_for_accretion() evaluates for a stored particle at its own collapse time, for the particles at the sub-box
        positions frag_pos of the sub-box box = (start, length, safe) whose cells lie in this rank's slab (pf_point_states) ->
        (index, states, found): index[j] = the particle, ascending; states[j] = w, w2, w31, w32 of set_weight(), sigmaD of virial()
        and q2x() of the three axes, in the context's product precision, at F = the Fmax of the particle's cell.  sigma0 =
        sqrt(TrueVariance[Nsmooth - 1]); k_sigma, k_point: the k of virial() and of set_point(); groups_order = par->order
        (ORDER_FOR_GROUPS).  order: None or indices[] of sort_and_organize (same result; another access pattern on the device).
        capacity: at most so many entries come back (found counts on).  Needs plc_set_cosmology.  Not collective."""
        pos = np.ascontiguousarray(frag_pos, dtype=np.uint32).ravel()
        o, op = _order(order, pos.size)
        cap = pos.size if capacity is None else int(capacity)
        index = np.empty(cap, dtype=np.uint32)
        st = np.empty((cap, 8), dtype=self._zacc_dtype)
        found = C.c_size_t()
        rg = _region(box)
        seg = _lib.PlcSegment(int(myseg), int(bool(use_v31)), float(z_seg), float(z_prev))
        par = _lib.PointParams(float(sigma0), float(k_sigma), float(k_point), int(groups_order))
        self._chk(self.L.pf_point_states(self.h, C.byref(seg), C.byref(rg), C.byref(par), pos.size, pos.ctypes.data_as(C.POINTER(C.c_uint)), op, cap,
                                         index.ctypes.data_as(C.POINTER(C.c_uint)), st.ctypes.data_as(C.c_void_p), C.byref(found)))
        m = min(int(found.value), cap)
        return index[:m], st[:m], int(found.value)

    def plc_set_cosmology(self, x, comvdist, hubble, grow, fomega, k_for_GM=0.0, logkmin=-3.0, deltalogk=0.5, rad_gm0=0.0, k_gm_displ=None):
        """the splines the light-cone test reads (pf_plc_set_cosmology), all at the knots x = -log10(1 + z): comvdist, hubble [n];
        grow, fomega [4][nk][n] (orders 1, 2, 31, 32; grow as log10).  nk = 1 reads k_for_GM; nk > 1 reads the k-bins logkmin +
        j deltalogk, Rad_GM[0] and k_GM_displ."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        cd = np.ascontiguousarray(comvdist, dtype=np.float64)
        hb = np.ascontiguousarray(hubble, dtype=np.float64)
        gr = np.ascontiguousarray(grow, dtype=np.float64)
        fo = np.ascontiguousarray(fomega, dtype=np.float64)
        n = x.size
        if gr.ndim == 2:
            gr, fo = gr[:, None, :], fo[:, None, :]
        if cd.shape != (n,) or hb.shape != (n,) or gr.ndim != 3 or gr.shape[0] != 4 or gr.shape[2] != n or fo.shape != gr.shape:
            raise ValueError(f"tables of shapes {cd.shape}, {hb.shape}, {gr.shape}, {fo.shape} for {n} knots")
        gr, fo = np.ascontiguousarray(gr), np.ascontiguousarray(fo)
        kg = np.ascontiguousarray(k_gm_displ, dtype=np.float64) if k_gm_displ is not None else None
        cs = _lib.PlcCosmology(n=n, x=_dp(x), comvdist=_dp(cd), hubble=_dp(hb), nk=gr.shape[1], grow=(_lib._dptr * 4)(*[_dp(gr[f]) for f in range(4)]),
                               fomega=(_lib._dptr * 4)(*[_dp(fo[f]) for f in range(4)]), logkmin=logkmin, deltalogk=deltalogk, k_for_GM=k_for_GM,
                               rad_gm0=rad_gm0, nsmooth=kg.size if kg is not None else 0, k_gm_displ=_dp(kg) if kg is not None else None)
        self._chk(self.L.pf_plc_set_cosmology(self.h, C.byref(cs)))

    def plc_set_geometry(self, center, xvers, yvers, zvers, aperture, Fstop, InterPartDist, GSglobal, repls, LastzForPLC=0.0, delta_z=1.0, nzbins=0):
        """the cone and its replications (pf_plc_set_geometry); repls: rows (i, j, k, F1, F2) (src/pinocchio.h:412-416)"""
        rp = [tuple(r) for r in repls]
        arr = (_lib.PlcReplication * max(len(rp), 1))(*[_lib.PlcReplication(int(r[0]), int(r[1]), int(r[2]), float(r[3]), float(r[4])) for r in rp])
        v3 = lambda a: (C.c_double * 3)(*map(float, a))
        gm = _lib.PlcGeometry(center=v3(center), xvers=v3(xvers), yvers=v3(yvers), zvers=v3(zvers), aperture=aperture, Fstop=Fstop, InterPartDist=InterPartDist,
                              GSglobal=(C.c_longlong * 3)(*map(int, GSglobal)), nrep=len(rp), repls=arr, LastzForPLC=LastzForPLC, delta_z=delta_z, nzbins=nzbins)
        self._plc_nzbins = int(nzbins)
        self._chk(self.L.pf_plc_set_geometry(self.h, C.byref(gm)))

    def plc_cross(self, mode, myseg, z_seg, stabl, groups, group_layout=None, z_prev=0.0, use_v31=False, f_lo=None, min_mass=0, capacity=None, out_dtype=None,
                  nz=None):
        """the light-cone test of build_groups() on `groups` (pf_plc_cross): a structured array of group states (group_layout None:
        the layout of its dtype, plc_group_layout_of) -> (records, cand_of, rep_of, count, unconverged); records: a structured array
        of out_dtype (None: plc_out_dtype) with the first min(count, capacity) crossings in (candidate, replication) order.  mode
        PLC_EVENTS reads the lower end of every candidate's interval from f_lo.  nz: the n(z) histogram, added to in place."""
        pt = np.float64 if self.double_products else np.float32
        if not groups.flags.c_contiguous:
            raise ValueError("groups must be contiguous")
        gl = group_layout if group_layout is not None else plc_group_layout_of(groups.dtype)
        ncand = groups.nbytes // gl.stride if gl.stride else 0
        od = np.dtype(out_dtype) if out_dtype is not None else plc_out_dtype(self.double_products)
        ol = plc_out_layout(od)
        fl = np.ascontiguousarray(f_lo, dtype=pt) if f_lo is not None else None
        if fl is not None and fl.size != ncand:
            raise ValueError(f"{fl.size} lower ends for {ncand} candidates")
        if nz is not None and not (nz.dtype == np.float64 and nz.flags.c_contiguous and nz.size == getattr(self, "_plc_nzbins", -1)):
            raise ValueError("nz must be a contiguous float64 array of nzbins values")
        seg = _lib.PlcSegment(int(myseg), int(bool(use_v31)), float(z_seg), float(z_prev))
        rg = _region((stabl, (1, 1, 1), (0, 0, 0)))
        # a first call counts; a second one fetches when the capacity was left to the count
        cap = ncand if capacity is None else int(capacity)
        rec = np.zeros(cap, dtype=od)
        cand = np.empty(cap, dtype=np.uint32)
        rep = np.empty(cap, dtype=np.int32)
        cnt, unc = C.c_size_t(), C.c_size_t()

        def call(cap_):
            self._chk(self.L.pf_plc_cross(self.h, int(mode), C.byref(seg), C.byref(rg), ncand, groups.ctypes.data_as(C.c_void_p) if ncand else None, C.byref(gl),
                                          fl.ctypes.data_as(C.c_void_p) if fl is not None else None, fl.itemsize if fl is not None else 0, int(min_mass), cap_,
                                          rec.ctypes.data_as(C.c_void_p), C.byref(ol), cand.ctypes.data_as(C.POINTER(C.c_uint)),
                                          rep.ctypes.data_as(C.POINTER(C.c_int)), _dp(nz) if nz is not None else None, C.byref(cnt), C.byref(unc)))
        if capacity is None:
            keep = nz.copy() if nz is not None else None
            call(cap)
            if cnt.value > cap:   # more crossings than candidates: once more with room for all of them
                cap = int(cnt.value)
                rec, cand, rep = np.zeros(cap, dtype=od), np.empty(cap, dtype=np.uint32), np.empty(cap, dtype=np.int32)
                if nz is not None:
                    nz[:] = keep
                call(cap)
        else:
            call(cap)
        m = min(int(cnt.value), cap)
        return rec[:m], cand[:m], rep[:m], int(cnt.value), int(unc.value)

    def catalog(self, F, myseg, z_seg, stabl, Lgwbl, groups, InterPartDist, ParticleMass, GSglobal, hfactor=1.0, pbc=(0, 0, 0), min_mass=0, group_layout=None,
                z_prev=0.0, use_v31=False, capacity=None, out_dtype=None, out=None, bins=None):
        """write_catalog() and compute_mf() of one output on `groups` (pf_catalog): a structured array of group states (group_layout
        None: the layout of its dtype, plc_group_layout_of; Flast need not be there) -> (records, group_of, count, ninbin, massinbin).
        records: a structured array of out_dtype (None: catalog_dtype) with the first min(count, capacity) passing groups in batch
        order -- written into `out` where one is given (its other bytes stay) --, group_of their batch indices.  bins = (nbin, mmin,
        deltam): the local mass function of all passing groups; None: ninbin and massinbin are None."""
        if not groups.flags.c_contiguous:
            raise ValueError("groups must be contiguous")
        if group_layout is not None:
            gl = group_layout
        else:
            names = groups.dtype.fields
            gl = plc_group_layout_of(groups.dtype) if "Flast" in names else plc_group_layout(groups.dtype.itemsize, off_Flast=-1, **{
                "off_" + k: names[k][1] for k in ("Mass", "Pos", "name", "good", "point", "Vel", "Vel_2LPT", "Vel_3LPT_1", "Vel_3LPT_2", "Vel_prev", "Vel_2LPT_prev",
                                                  "Vel_3LPT_1_prev", "Vel_3LPT_2_prev") if k in names})
        ngroups = groups.nbytes // gl.stride if gl.stride else 0
        od = np.dtype(out_dtype) if out_dtype is not None else (out.dtype if out is not None else catalog_dtype(self.double_products))
        ol = catalog_out_layout(od)
        cap = (ngroups if out is None else len(out)) if capacity is None else int(capacity)
        rec = out if out is not None else np.zeros(cap, dtype=od)
        if not (rec.flags.c_contiguous and rec.dtype.itemsize == od.itemsize and len(rec) >= cap):
            raise ValueError("out must be a contiguous array of at least `capacity` records of out_dtype")
        gof = np.empty(cap, dtype=np.uint32)
        seg = _lib.PlcSegment(int(myseg), int(bool(use_v31)), float(z_seg), float(z_prev))
        rg = _region((stabl, Lgwbl, (0, 0, 0)))
        par = _lib.CatalogParams(F=float(F), InterPartDist=float(InterPartDist), ParticleMass=float(ParticleMass), hfactor=float(hfactor),
                                 GSglobal=(C.c_longlong * 3)(*map(int, GSglobal)), pbc=(C.c_int * 3)(*map(int, pbc)), min_mass=int(min_mass))
        mb = nin = mas = None
        if bins is not None:
            mb = _lib.MfBins(int(bins[0]), float(bins[1]), float(bins[2]))
            nin, mas = np.zeros(max(mb.nbin, 0), dtype=np.int32), np.zeros(max(mb.nbin, 0), dtype=np.float64)
        cnt = C.c_size_t()
        self._chk(self.L.pf_catalog(self.h, C.byref(seg), C.byref(rg), C.byref(par), ngroups, groups.ctypes.data_as(C.c_void_p) if ngroups else None, C.byref(gl), cap,
                                    rec.ctypes.data_as(C.c_void_p), C.byref(ol), gof.ctypes.data_as(C.POINTER(C.c_uint)), C.byref(mb) if mb is not None else None,
                                    nin.ctypes.data_as(C.POINTER(C.c_int)) if nin is not None else None, _dp(mas) if mas is not None else None, C.byref(cnt)))
        m = min(int(cnt.value), cap)
        return rec[:m], gof[:m], int(cnt.value), nin, mas

    def organize(self, records: np.ndarray, frag_pos: np.ndarray, layout=None):
        """sort_and_organize() (src/fragment.c:484-520) on records the caller holds (contributions of several ranks to one
        sub-box, concatenated): `records` (a structured array of product_layout(), or rows of layout.stride bytes) and `frag_pos`
        (uint32) are reordered IN PLACE by descending Fmax, ties in input order -> (sorted_pos, indices)"""
        if layout is None:
            layout, _ = self.product_layout()
        count = len(frag_pos)
        if not (records.flags.c_contiguous and records.flags.writeable and records.nbytes == count * layout.stride):
            raise ValueError(f"records of {records.nbytes} bytes for {count} positions and a stride of {layout.stride}")
        if not (frag_pos.dtype == np.uint32 and frag_pos.flags.c_contiguous and frag_pos.flags.writeable):
            raise ValueError("frag_pos must be a contiguous writeable uint32 array")
        spos = np.empty(count, dtype=np.uint32)
        ind = np.empty(count, dtype=np.int32)
        self._chk(self.L.pf_organize(self.h, C.byref(layout), count, records.ctypes.data_as(C.c_void_p), frag_pos.ctypes.data_as(C.POINTER(C.c_uint)),
                                     spos.ctypes.data_as(C.POINTER(C.c_uint)), ind.ctypes.data_as(C.POINTER(C.c_int))))
        return spos, ind

    def block(self, name: str, id_bytes: int = 4) -> np.ndarray:
        """one block of the timeless snapshot (src/write_snapshot.c:207-342) for this rank's slab"""
        nc = self.nxl * self.n * self.n
        if name == "ID  ":
            out = np.empty(nc, dtype=np.uint64 if id_bytes == 8 else np.uint32)
        elif name in ("RMAX", "GRUP"):
            out = np.empty(nc, dtype=np.int32)
        elif name in ("FMAX", "ZACC"):
            out = np.empty(nc, dtype=np.float32)
        else:
            out = np.empty((nc, 3), dtype=np.float32)
        self._chk(self.L.pf_get_block(self.h, name.encode(), id_bytes, out.ctypes.data_as(C.c_void_p)))
        return out

    def second_derivative(self, i: int) -> np.ndarray:
        out = np.empty((self.nxl, self.n, self.n))
        self._chk(self.L.pf_get_second_derivative(self.h, i, _dp(out)))
        return out

    def kvector(self, which: int) -> np.ndarray:
        out = np.empty((self.nxl, self.n, self.n // 2 + 1), dtype=np.complex128)
        self._chk(self.L.pf_get_kvector(self.h, which, _dp(out.view(np.float64))))
        return out

    def density(self) -> np.ndarray:
        out = np.empty((self.nxl, self.n, self.n // 2 + 1), dtype=np.complex128)
        self._chk(self.L.pf_get_density(self.h, _dp(out.view(np.float64))))
        return out

    def replicated_rows(self, kx0: int, nkx: int) -> np.ndarray:
        """rows kx0 .. kx0 + nkx - 1 of the whole delta(k) a PF_REPLICATE_DK context transforms -> [nkx][n][n/2+1] complex128"""
        out = np.empty((nkx, self.n, self.n // 2 + 1), dtype=np.complex128)
        self._chk(self.L.pf_debug_replicated_rows(self.h, int(kx0), int(nkx), _dp(out.view(np.float64))))
        return out

    def forward_transform(self, real: np.ndarray) -> np.ndarray:
        real = np.ascontiguousarray(real, dtype=np.float64)
        assert real.shape == (self.nxl, self.n, self.n)
        out = np.empty((self.nxl, self.n, self.n // 2 + 1), dtype=np.complex128)
        self._chk(self.L.pf_forward_transform(self.h, _dp(real), _dp(out.view(np.float64))))
        return out

    def reverse_transform(self, spec: np.ndarray) -> np.ndarray:
        spec = np.ascontiguousarray(spec, dtype=np.complex128)
        assert spec.shape == (self.nxl, self.n, self.n // 2 + 1)
        out = np.empty((self.nxl, self.n, self.n))
        self._chk(self.L.pf_reverse_transform(self.h, _dp(spec.view(np.float64)), _dp(out)))
        return out

    def compute_derivative(self, spec: np.ndarray, first_derivative: int, second_derivative: int, rs_cells: float = 0.0,
                           order: int = 0) -> np.ndarray:
        """compute_derivative (src/fmax-pfft.c:255-441) of a caller-held spectrum slab -> real slab"""
        spec = np.ascontiguousarray(spec, dtype=np.complex128)
        assert spec.shape == (self.nxl, self.n, self.n // 2 + 1)
        out = np.empty((self.nxl, self.n, self.n))
        self._chk(self.L.pf_derivative(self.h, _dp(spec.view(np.float64)), first_derivative, second_derivative,
                                       float(rs_cells), int(order), _dp(out)))
        return out

    def collapse_cells(self, d: np.ndarray, ismooth: int = -1) -> np.ndarray:
        d = np.ascontiguousarray(d, dtype=np.float64).reshape(-1, 6)
        out = np.empty(len(d))
        self._chk(self.L.pf_collapse_cells(self.h, ismooth, _dp(d), len(d), _dp(out)))
        return out

    def set_arithmetic(self, flavour: str):
        """"fast" (the default forms of the solve's elementary functions) or "exact" (the reference's calls) for every solve that
        follows; a context computes after it what one created under the matching PF_EXACT_LIBM computes (pf_set_arithmetic)"""
        if flavour not in _ARITH:
            raise ValueError(f'flavour {flavour!r}: "fast" or "exact"')
        self._chk(self.L.pf_set_arithmetic(self.h, _ARITH[flavour]))

    @property
    def arithmetic(self) -> str:
        return "exact" if self.L.pf_get_arithmetic(self.h) == _lib.ARITH_EXACT else "fast"

    def flavour_census(self, radii_cells, capacity: int = 1024):
        """the sweep in both flavours on the resident density, compared on the device (pf_flavour_census; a diagnostic: two sweeps
        and a pass) -> (TrueVariance[], census dict, the first min(outliers, capacity) outlier records as CENSUS_CELL_DTYPE in
        ascending cell index).  The context is left as a plain sweep in its own flavour leaves it."""
        r = np.ascontiguousarray(radii_cells, dtype=np.float64)
        tv = np.zeros(len(r))
        out = _lib.Census()
        capacity = int(capacity)
        rec = np.zeros(max(capacity, 1), dtype=CENSUS_CELL_DTYPE)
        self._chk(self.L.pf_flavour_census(self.h, len(r), _dp(r), _dp(tv), C.byref(out), capacity,
                                           rec.ctypes.data_as(C.POINTER(_lib.CensusCell)) if capacity else None))
        cen = _census_dict(out)
        return tv, cen, rec[:min(cen["outliers"], capacity)].copy()

    def power_spectrum(self, which="density", radii_cells=(), box=None) -> dict:
        """shell sums and Gaussian-smoothed variances of a spectrum that lies on the device (pf_power_spectrum; collective over the
        ranks): which = "density" (0), "kvector_2LPT" (1), "kvector_3LPT_1" (2), "kvector_3LPT_2" (3) -> nmodes[], k2sum[], power[]
        per shell, variance[] per radius (the TrueVariance a sweep reports for it), modes, nonfinite and, with the box length
        `box`, k = (2 pi / box) sqrt(k2sum / nmodes) and pk = power / nmodes * box^3 per shell (NaN for an empty shell)"""
        w = _POWER_WHICH.get(which, which)
        rc, out = _power_call(self.L, self.n, radii_cells,
                              lambda ns, r, nm, k2, pw, var, info: self.L.pf_power_spectrum(self.h, int(w), ns, r, nm, k2, pw, var, info))
        self._chk(rc)
        if box is not None:
            nm = out["nmodes"].astype(np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                out["k"] = (2.0 * np.pi / float(box)) * np.sqrt(out["k2sum"].astype(np.float64) / nm)
                out["pk"] = out["power"] / nm * float(box) ** 3
        return out

    def matter_power(self, weight=None, cross: bool = True, density: bool = False, ngp: bool = False, deconvolve: bool = False, box=None) -> dict:
        """the density of the particles at their LPT positions and its shell sums (pf_matter_power; one rank): cloud-in-cell (or
        nearest-grid-point) assignment of the displacement columns in HBM, optionally weighted per LPT order (`weight`, four
        factors: (1, 0, 0, 0) is Zel'dovich alone), the forward transform, and per shell nmodes[], k2sum[], power[] = sum of w
        |delta_m|^2 / N^6 and, with `cross`, cross[] = sum of w Re(delta_m conj delta) / N^6 with the resident delta(k) -> those,
        the counters of pf_matter_info, with `density` the contrast [nxl][n][n] the transform read, and with the box length `box`
        k, pk and pk_cross per shell as power_spectrum forms them"""
        nb = int(self.L.pf_power_bins(self.n))
        nm, k2 = np.zeros(nb, dtype=np.uint64), np.zeros(nb, dtype=np.uint64)
        pw, cr = np.zeros(nb), np.zeros(nb)
        w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64).reshape(4)
        dens = np.zeros((self.nxl, self.n, self.n)) if density else None
        info = _lib.MatterInfo()
        up = lambda a: a.ctypes.data_as(C.POINTER(C.c_ulonglong))
        self._chk(self.L.pf_matter_power(self.h, _matter_flags(ngp, deconvolve), None if w is None else _dp(w), up(nm), up(k2), _dp(pw), _dp(cr) if cross else None,
                                         _dp(dens) if density else None, C.byref(info)))
        out = {"nmodes": nm, "k2sum": k2, "power": pw, "cross": cr if cross else None, "density": dens}
        out.update(_matter_info(info))
        if box is not None:
            f = nm.astype(np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                out["k"] = (2.0 * np.pi / float(box)) * np.sqrt(k2.astype(np.float64) / f)
                out["pk"] = pw / f * float(box) ** 3
                out["pk_cross"] = cr / f * float(box) ** 3 if cross else None
        return out

    def matter_power_slabs(self, weight=None, cross: bool = True, density: bool = False, ngp: bool = False, deconvolve: bool = False, box=None) -> dict:
        """matter_power on any number of ranks (pf_matter_power_slabs; collective: every rank calls it with the same arguments): the
        particles that leave a slab reach their planes through one all-to-all of the context, and every rank receives the bits one
        rank returns for the same box -> the dict of matter_power, the columns and counters the box's, `density` this rank's slab,
        and `exchange`, what crossed (matter_exchange())"""
        nb = int(self.L.pf_power_bins(self.n))
        nm, k2 = np.zeros(nb, dtype=np.uint64), np.zeros(nb, dtype=np.uint64)
        pw, cr = np.zeros(nb), np.zeros(nb)
        w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64).reshape(4)
        dens = np.zeros((self.nxl, self.n, self.n)) if density else None
        info = _lib.MatterInfo()
        up = lambda a: a.ctypes.data_as(C.POINTER(C.c_ulonglong))
        self._chk(self.L.pf_matter_power_slabs(self.h, _matter_flags(ngp, deconvolve), None if w is None else _dp(w), up(nm), up(k2), _dp(pw),
                                               _dp(cr) if cross else None, _dp(dens) if density else None, C.byref(info)))
        out = {"nmodes": nm, "k2sum": k2, "power": pw, "cross": cr if cross else None, "density": dens, "exchange": matter_exchange()}
        out.update(_matter_info(info))
        if box is not None:
            f = nm.astype(np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                out["k"] = (2.0 * np.pi / float(box)) * np.sqrt(k2.astype(np.float64) / f)
                out["pk"] = pw / f * float(box) ** 3
                out["pk_cross"] = cr / f * float(box) ** 3 if cross else None
        return out

    def debug_matter_slabs(self, vel12_slab, ngp: bool = False, weight=None):
        """collective test tap (pf_debug_matter_slabs): the production reach pass, deposit, exchange and fold on the caller's columns
        [12][nxl][n][n] of this rank's slab, in the context's product type -> (this rank's planes of the grid [nxl][n][n] of uint64,
        the dict of pf_matter_info for the box)"""
        T = np.float64 if self.double_products else np.float32
        v = np.ascontiguousarray(vel12_slab)
        if v.dtype != T or v.shape != (12, self.nxl, self.n, self.n):
            raise ValueError(f"columns [12][{self.nxl}][{self.n}][{self.n}] of {np.dtype(T).name}, not {v.dtype} {v.shape}")
        w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64).reshape(4)
        grid = np.zeros((self.nxl, self.n, self.n), dtype=np.uint64)
        info = _lib.MatterInfo()
        self._chk(self.L.pf_debug_matter_slabs(self.h, v.ctypes.data_as(C.c_void_p), _matter_flags(ngp, False), None if w is None else _dp(w),
                                               grid.ctypes.data_as(C.POINTER(C.c_ulonglong)), C.byref(info)))
        return grid, _matter_info(info)

    def halo_power(self, pos, mass, ranges, scale: float = 1.0, mass_weight: bool = False, cross: bool = True, ngp: bool = False, deconvolve: bool = False,
                   box=None) -> dict:
        """the power of a halo catalogue per mass bin and its cross power with the resident delta(k) (pf_halo_power; collective: every
        rank passes the whole list): pos [count][3] in units that `scale` brings to grid cells, mass [count] integers, ranges
        [nbins][2] of inclusive mass bounds -> nmodes[], k2sum[] per shell, power[b][] and cross[b][] (None without `cross`) per bin,
        the counters of pf_halo_info as arrays over the bins (weight2 as Python integers), shot[b] = sum W^2 / (sum W)^2 -- the level
        of power / nmodes that the discreteness alone gives, NaN for an empty bin -- and, with the box length `box`, k, pk[b],
        pk_cross[b] and pk_shot[b] as matter_power forms them"""
        pos, mass = _halo_list(pos, mass)
        rg = np.ascontiguousarray(ranges, dtype=np.int32)
        if rg.ndim != 2 or rg.shape[1] != 2:
            raise ValueError(f"ranges [nbins][2], not {rg.shape}")
        nbins = rg.shape[0]
        nb = int(self.L.pf_power_bins(self.n))
        nm, k2 = np.zeros(nb, dtype=np.uint64), np.zeros(nb, dtype=np.uint64)
        pw, cr = np.zeros((max(nbins, 1), nb)), np.zeros((max(nbins, 1), nb))
        info = (_lib.HaloInfo * max(nbins, 1))()
        up = lambda a: a.ctypes.data_as(C.POINTER(C.c_ulonglong))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        self._chk(self.L.pf_halo_power(self.h, _halo_flags(ngp, deconvolve, mass_weight), len(mass), _dp(pos), float(scale), ip(mass), nbins, ip(rg), up(nm), up(k2),
                                       _dp(pw), _dp(cr) if cross else None, info))
        return self._halo_result(nm, k2, pw, cr if cross else None, info, nbins, box)

    @staticmethod
    def _halo_result(nm, k2, pw, cr, info, nbins, box):
        """the dict of halo_power / halo_multipoles from the filled arrays (cr None: no cross power)"""
        cross = cr is not None
        per = [_halo_info(info[b]) for b in range(nbins)]
        out = {"nmodes": nm, "k2sum": k2, "power": pw, "cross": cr}
        for k in per[0]:
            out[k] = [p[k] for p in per] if k == "weight2" else np.array([p[k] for p in per], dtype=np.uint64)
        out["shot"] = np.array([p["weight2"] / (p["weight_sum"] * p["weight_sum"]) if p["weight_sum"] else np.nan for p in per])
        if box is not None:
            f = nm.astype(np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                out["k"] = (2.0 * np.pi / float(box)) * np.sqrt(k2.astype(np.float64) / f)
                out["pk"] = pw / f * float(box) ** 3
                out["pk_cross"] = cr / f * float(box) ** 3 if cross else None
                out["pk_shot"] = out["shot"] * float(box) ** 3
        return out

    def halo_multipoles(self, pos, vel, mass, ranges, scale: float = 1.0, vfac: float = 0.0, los: int = 2, mass_weight: bool = False, cross: bool = True, ngp: bool = False,
                        deconvolve: bool = False, box=None) -> dict:
        """the redshift-space multipoles l = 0, 2, 4 of the halo power per mass bin (pf_halo_multipoles; collective like halo_power):
        the list is moved along axis `los` by vel * vfac (vel [count][3], or None for real space; vfac: position units per velocity
        unit, (1 + z) / (100 E(z)) for km/s and Mpc/h) and every mode is weighted by L_l(mu).  Returns halo_power's dict with power and
        cross shaped [nbins][3][nb] and no factor (2 l + 1): P_l = (2 l + 1) pk[b][l / 2]; with `box`, pk and pk_cross have that shape
        too"""
        pos, mass = _halo_list(pos, mass)
        vel = _halo_vel(vel, pos)
        rg = np.ascontiguousarray(ranges, dtype=np.int32)
        if rg.ndim != 2 or rg.shape[1] != 2:
            raise ValueError(f"ranges [nbins][2], not {rg.shape}")
        nbins = rg.shape[0]
        nb = int(self.L.pf_power_bins(self.n))
        nm, k2 = np.zeros(nb, dtype=np.uint64), np.zeros(nb, dtype=np.uint64)
        pw, cr = np.zeros((max(nbins, 1), MULTIPOLE_ORDERS, nb)), np.zeros((max(nbins, 1), MULTIPOLE_ORDERS, nb))
        info = (_lib.HaloInfo * max(nbins, 1))()
        up = lambda a: a.ctypes.data_as(C.POINTER(C.c_ulonglong))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        self._chk(self.L.pf_halo_multipoles(self.h, _halo_flags(ngp, deconvolve, mass_weight), len(mass), _dp(pos), None if vel is None else _dp(vel), float(scale), float(vfac),
                                            int(los), ip(mass), nbins, ip(rg), up(nm), up(k2), _dp(pw), _dp(cr) if cross else None, info))
        return self._halo_result(nm, k2, pw, cr if cross else None, info, nbins, box)

    def halo_correlation(self, pos, vel, mass, ranges, scale: float = 1.0, vfac: float = 0.0, los: int = 2, mass_weight: bool = False, cross: bool = True, ngp: bool = False,
                         deconvolve: bool = False, box=None) -> dict:
        """the two-point correlation function of the haloes per mass bin in shells of the separation, with the Legendre weights l = 0,
        2, 4 of the angle to axis `los` (pf_halo_correlation; collective like halo_multipoles, whose list, bins and flags these are):
        ncells[], r2sum[] per shell, xi[b][3][] and xi_cross[b][3][] (None without `cross`: the correlation with the resident density)
        as plain sums -- no factor (2 l + 1), no division -- and the counters of pf_corr_info as arrays over the bins (those of
        halo_multipoles, cells, nonfinite_cells).  Formed here for convenience: xi_l[b][l/2][] = (2 l + 1) xi / ncells, xi_cross_l
        likewise, variance[b] = xi[b][0][0] (the zero-lag cell: the variance of the contrast, shot noise included) and, with the box
        length `box`, r[] = (box / n) sqrt(r2sum / ncells)"""
        pos, mass = _halo_list(pos, mass)
        vel = _halo_vel(vel, pos)
        rg = np.ascontiguousarray(ranges, dtype=np.int32)
        if rg.ndim != 2 or rg.shape[1] != 2:
            raise ValueError(f"ranges [nbins][2], not {rg.shape}")
        nbins = rg.shape[0]
        nb = int(self.L.pf_power_bins(self.n))
        nc, r2 = np.zeros(nb, dtype=np.uint64), np.zeros(nb, dtype=np.uint64)
        xi, xc = np.zeros((max(nbins, 1), CORR_ORDERS, nb)), np.zeros((max(nbins, 1), CORR_ORDERS, nb))
        info = (_lib.CorrInfo * max(nbins, 1))()
        up = lambda a: a.ctypes.data_as(C.POINTER(C.c_ulonglong))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        self._chk(self.L.pf_halo_correlation(self.h, _halo_flags(ngp, deconvolve, mass_weight), len(mass), _dp(pos), None if vel is None else _dp(vel), float(scale), float(vfac),
                                             int(los), ip(mass), nbins, ip(rg), up(nc), up(r2), _dp(xi), _dp(xc) if cross else None, info))
        per = [_halo_info(info[b].halo) for b in range(nbins)]
        out = {"ncells": nc, "r2sum": r2, "xi": xi, "xi_cross": xc if cross else None}
        for k in per[0]:
            out[k] = [p[k] for p in per] if k == "weight2" else np.array([p[k] for p in per], dtype=np.uint64)
        out["cells"] = np.array([int(info[b].cells) for b in range(nbins)], dtype=np.uint64)
        out["nonfinite_cells"] = np.array([int(info[b].nonfinite_cells) for b in range(nbins)], dtype=np.uint64)
        f = nc.astype(np.float64)
        ell = (4.0 * np.arange(CORR_ORDERS) + 1.0)[None, :, None]      # 2 l + 1 for l = 0, 2, 4
        with np.errstate(invalid="ignore", divide="ignore"):
            out["xi_l"] = ell * xi / f
            out["xi_cross_l"] = ell * xc / f if cross else None
        out["variance"] = xi[:, 0, 0].copy()
        if box is not None:
            out["r"] = (float(box) / self.n) * np.sqrt(r2.astype(np.float64) / f)
        return out

    def halo_bispectrum(self, pos, vel, mass, ranges, kmin: int, dk: int, nk: int, scale: float = 1.0, vfac: float = 0.0, los: int = 2, mass_weight: bool = False,
                        ngp: bool = False, deconvolve: bool = False, box=None) -> dict:
        """the bispectrum of the haloes per mass bin by the FFT estimator, in nk linear k-bins [kmin + i dk, kmin + (i + 1) dk) in units
        of the fundamental (pf_halo_bispectrum; collective like halo_correlation, whose list, mass bins and flags these are; 3 (kmin + nk
        dk) <= n): triangles[nt][3] (bispectrum_triangles), kmodes[nk], ntri[nt], bsum[b][nt], psum[b][nk] and the counters of
        pf_bispec_info as arrays over the mass bins.  Formed here for convenience with the box length `box`: k[nk] the bin centres, pk[b][nk]
        = box^3 psum / (N3 kmodes), B[b][nt] = box^6 bsum / (N3 ntri) and the reduced Q[b][nt] = B / (P_i P_j + P_j P_l + P_l P_i); no
        shot noise is taken off"""
        pos, mass = _halo_list(pos, mass)
        vel = _halo_vel(vel, pos)
        rg = np.ascontiguousarray(ranges, dtype=np.int32)
        if rg.ndim != 2 or rg.shape[1] != 2:
            raise ValueError(f"ranges [nbins][2], not {rg.shape}")
        nbins = rg.shape[0]
        tri = bispectrum_triangles(kmin, dk, nk)
        nt = len(tri)
        km, ntri = np.zeros(nk, dtype=np.uint64), np.zeros(nt)
        bsum, psum = np.zeros((max(nbins, 1), nt)), np.zeros((max(nbins, 1), nk))
        info = (_lib.BispecInfo * max(nbins, 1))()
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        self._chk(self.L.pf_halo_bispectrum(self.h, _halo_flags(ngp, deconvolve, mass_weight), len(mass), _dp(pos), None if vel is None else _dp(vel), float(scale), float(vfac),
                                            int(los), ip(mass), nbins, ip(rg), int(kmin), int(dk), int(nk), km.ctypes.data_as(C.POINTER(C.c_ulonglong)), _dp(ntri), _dp(bsum),
                                            _dp(psum), info))
        per = [_halo_info(info[b].halo) for b in range(nbins)]
        out = {"triangles": tri, "kmodes": km, "ntri": ntri, "bsum": bsum, "psum": psum}
        for k in per[0]:
            out[k] = [p[k] for p in per] if k == "weight2" else np.array([p[k] for p in per], dtype=np.uint64)
        out["cells"] = np.array([int(info[b].cells) for b in range(nbins)], dtype=np.uint64)
        out["nonfinite_cells"] = np.array([int(info[b].nonfinite_cells) for b in range(nbins)], dtype=np.uint64)
        if box is not None:
            N3, L = float(self.n) ** 3, float(box)
            with np.errstate(invalid="ignore", divide="ignore"):
                out["k"] = (2.0 * np.pi / L) * (kmin + dk * (np.arange(nk) + 0.5))
                pk = L ** 3 * psum / (N3 * km.astype(np.float64))
                out["pk"], out["B"] = pk, L ** 6 * bsum / (N3 * ntri)
                pi, pj, pl = pk[:, tri[:, 0]], pk[:, tri[:, 1]], pk[:, tri[:, 2]]
                out["Q"] = out["B"] / (pi * pj + pj * pl + pl * pi)
        return out

    # -- measurement ------------------------------------------------------
    def cputime(self) -> dict:
        t = _lib.CpuTime()
        self._chk(self.L.pf_get_cputime(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_}

    def reset_cputime(self):
        self._chk(self.L.pf_reset_cputime(self.h))

    def kernel_stats(self) -> list:
        arr = (_lib.KernelStat * 32)()
        n = C.c_int()
        self._chk(self.L.pf_kernel_stats(self.h, arr, 32, C.byref(n)))
        return [dict(name=arr[i].name.decode(), launches=int(arr[i].launches), total_ms=arr[i].total_ms,
                     alg_bytes=arr[i].alg_bytes) for i in range(n.value)]

    def reset_kernel_stats(self):
        self._chk(self.L.pf_reset_kernel_stats(self.h))
