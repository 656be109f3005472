"""ctypes loader of libpinfmax_hip.so (the C ABI declared in include/pinfmax.h).

There is no Python or CPU implementation behind this module: if the shared
object is missing it raises, and pf_create itself fails without a HIP device.
"""
from __future__ import annotations

import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
# PINFMAX_LIB: another build of the same library (A/B measurements of a kernel variant, csrc/Makefile VARIANT=...)
SO = os.environ.get("PINFMAX_LIB") or os.path.join(PKG, "libpinfmax_hip.so")
NBINS = 210
MAX_SMOOTH = 64

FLAG_TIMING = 1
FLAG_DOUBLE_PRODUCTS = 2
MAP_CURRENT = 0   # frag_map
MAP_UPDATE = 1    # frag_map_update
NEIGH_SKIP, NEIGH_GOOD, NEIGH_PEAK = 1, 2, 4   # PF_NEIGH_*: the flags of the neighbour table


class Config(C.Structure):
    _fields_ = [("n", C.c_int64), ("rank", C.c_int), ("nranks", C.c_int), ("device", C.c_int),
                ("field_bytes", C.c_int), ("flags", C.c_int)]


class ProductLayout(C.Structure):
    _fields_ = [("stride", C.c_size_t), ("off_Rmax", C.c_int), ("off_Fmax", C.c_int), ("off_Vel", C.c_int),
                ("off_Vel_2LPT", C.c_int), ("off_Vel_3LPT_1", C.c_int), ("off_Vel_3LPT_2", C.c_int)]


class GenicParams(C.Structure):
    _fields_ = [("Omega0", C.c_double), ("OmegaBaryon", C.c_double), ("Hubble100", C.c_double),
                ("PrimordialIndex", C.c_double), ("BoxSize_true_Mpc", C.c_double), ("PkNorm", C.c_double),
                ("RandomSeed", C.c_uint), ("FixedIC", C.c_int), ("PairedIC", C.c_int),
                ("pk_n", C.c_int), ("pk_logk", C.POINTER(C.c_double)), ("pk_logk3p", C.POINTER(C.c_double)),
                ("spectrum", C.c_int), ("WDM_PartMass_in_kev", C.c_double), ("UnitLength_in_cm", C.c_double)]


class CpuTime(C.Structure):
    _fields_ = [("fmax", C.c_double), ("deriv", C.c_double), ("fft", C.c_double), ("coll", C.c_double),
                ("lpt", C.c_double), ("mem_transf", C.c_double)]


class PeakRegion(C.Structure):
    _fields_ = [("start", C.c_int * 3), ("len", C.c_int * 3), ("safe", C.c_int * 3)]


class SubBox(C.Structure):
    _fields_ = [("start", C.c_int * 3), ("len", C.c_int * 3)]


class PrevLayout(C.Structure):
    _fields_ = [("off_Vel_prev", C.c_int), ("off_Vel_2LPT_prev", C.c_int), ("off_Vel_3LPT_1_prev", C.c_int), ("off_Vel_3LPT_2_prev", C.c_int)]


class GroupLayout(C.Structure):
    _fields_ = [("stride", C.c_size_t), ("off_Mass", C.c_long), ("off_Vel", C.c_long), ("off_Vel_2LPT", C.c_long), ("off_Vel_3LPT_1", C.c_long),
                ("off_Vel_3LPT_2", C.c_long), ("off_Vel_prev", C.c_long), ("off_Vel_2LPT_prev", C.c_long), ("off_Vel_3LPT_1_prev", C.c_long),
                ("off_Vel_3LPT_2_prev", C.c_long)]


PLC_LAST_CHECK = 0
PLC_EVENTS = 1
_dptr = C.POINTER(C.c_double)


class PlcCosmology(C.Structure):
    _fields_ = [("n", C.c_int), ("x", _dptr), ("comvdist", _dptr), ("hubble", _dptr), ("nk", C.c_int), ("grow", _dptr * 4), ("fomega", _dptr * 4),
                ("logkmin", C.c_double), ("deltalogk", C.c_double), ("k_for_GM", C.c_double), ("rad_gm0", C.c_double), ("nsmooth", C.c_int),
                ("k_gm_displ", _dptr)]


class PlcReplication(C.Structure):
    _fields_ = [("i", C.c_int), ("j", C.c_int), ("k", C.c_int), ("F1", C.c_double), ("F2", C.c_double)]


class PlcGeometry(C.Structure):
    _fields_ = [("center", C.c_double * 3), ("xvers", C.c_double * 3), ("yvers", C.c_double * 3), ("zvers", C.c_double * 3), ("aperture", C.c_double),
                ("Fstop", C.c_double), ("InterPartDist", C.c_double), ("GSglobal", C.c_longlong * 3), ("nrep", C.c_size_t),
                ("repls", C.POINTER(PlcReplication)), ("LastzForPLC", C.c_double), ("delta_z", C.c_double), ("nzbins", C.c_int)]


class PlcSegment(C.Structure):
    _fields_ = [("myseg", C.c_int), ("use_v31", C.c_int), ("z_seg", C.c_double), ("z_prev", C.c_double)]


PLC_GROUP_FIELDS = ["off_Mass", "off_Pos", "off_name", "off_Flast", "off_good", "off_point", "off_Vel", "off_Vel_2LPT", "off_Vel_3LPT_1", "off_Vel_3LPT_2",
                    "off_Vel_prev", "off_Vel_2LPT_prev", "off_Vel_3LPT_1_prev", "off_Vel_3LPT_2_prev"]


class PlcGroupLayout(C.Structure):
    _fields_ = [("stride", C.c_size_t)] + [(f, C.c_long) for f in PLC_GROUP_FIELDS]


class PlcOutLayout(C.Structure):
    _fields_ = [("stride", C.c_size_t), ("off_Mass", C.c_long), ("off_name", C.c_long), ("off_z", C.c_long), ("off_x", C.c_long), ("off_v", C.c_long)]


class CatalogParams(C.Structure):
    _fields_ = [("F", C.c_double), ("InterPartDist", C.c_double), ("ParticleMass", C.c_double), ("hfactor", C.c_double), ("GSglobal", C.c_longlong * 3),
                ("pbc", C.c_int * 3), ("min_mass", C.c_int)]


class CatalogOutLayout(C.Structure):
    _fields_ = [("stride", C.c_size_t), ("off_name", C.c_long), ("off_M", C.c_long), ("off_x", C.c_long), ("off_v", C.c_long), ("off_q", C.c_long),
                ("off_n", C.c_long)]


class MfBins(C.Structure):
    _fields_ = [("nbin", C.c_int), ("mmin", C.c_double), ("deltam", C.c_double)]


class PointParams(C.Structure):
    _fields_ = [("sigma0", C.c_double), ("k_sigma", C.c_double), ("k_point", C.c_double), ("order", C.c_int)]


ARITH_FAST, ARITH_EXACT = 0, 1   # PF_ARITH_*
CENSUS_BINS = 64


class Census(C.Structure):
    _fields_ = [("cells", C.c_ulonglong), ("differing_bits", C.c_ulonglong), ("hist", C.c_ulonglong * CENSUS_BINS), ("beyond_2ulp", C.c_ulonglong),
                ("rmax_differing", C.c_ulonglong), ("nonfinite", C.c_ulonglong), ("outliers", C.c_ulonglong), ("max_abs", C.c_double),
                ("max_ulps", C.c_double), ("max_abs_cell", C.c_ulonglong)]


class CensusCell(C.Structure):
    _fields_ = [("cell", C.c_ulonglong), ("fast", C.c_double), ("exact", C.c_double), ("rmax_fast", C.c_int), ("rmax_exact", C.c_int)]


class PowerInfo(C.Structure):
    _fields_ = [("modes", C.c_ulonglong), ("nonfinite", C.c_ulonglong)]


MATTER_NGP, MATTER_DECONVOLVE = 1, 2   # PF_MATTER_*


class MatterInfo(C.Structure):
    _fields_ = [(k, C.c_ulonglong) for k in ("deposited", "nonfinite", "outside", "empty_cells", "max_cell", "sum_hi32", "sum_lo32", "modes", "nonfinite_modes")]


HALO_NGP, HALO_DECONVOLVE, HALO_MASS_WEIGHT, HALO_MAX_BINS = 1, 2, 4, 8   # PF_HALO_*
MULTIPOLE_ORDERS, MULTIPOLE_SUMS = 3, 11   # PF_MULTIPOLE_*


class HaloInfo(C.Structure):
    _fields_ = [(k, C.c_ulonglong) for k in ("selected", "weight_sum", "weight2_hi", "weight2_lo", "nonfinite", "outside", "empty_cells", "max_cell", "modes",
                                              "nonfinite_modes")]


CORR_ORDERS, CORR_SUMS = 3, 12   # PF_CORR_*


class CorrInfo(C.Structure):
    _fields_ = [("halo", HaloInfo), ("cells", C.c_ulonglong), ("nonfinite_cells", C.c_ulonglong)]


BISPEC_MAX_KBINS = 32   # PF_BISPEC_MAX_KBINS


class BispecInfo(C.Structure):
    _fields_ = [("halo", HaloInfo), ("cells", C.c_ulonglong), ("nonfinite_cells", C.c_ulonglong)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_uint64), ("total_ms", C.c_double), ("alg_bytes", C.c_double)]


ALLTOALL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
ALLTOALLV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t),
                           C.POINTER(C.c_size_t), C.c_void_p)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)

# every symbol include/pinfmax.h declares: name -> (restype, argtypes)
_dp = C.POINTER(C.c_double)
_vp = C.c_void_p
PROTOTYPES = {
    "pf_layout_3lpt": (None, [C.POINTER(ProductLayout)]),
    "pf_create": (C.c_int, [C.POINTER(_vp), C.POINTER(Config)]),
    "pf_destroy": (C.c_int, [_vp]),
    "pf_last_error": (C.c_char_p, []),
    "pf_set_exchange": (C.c_int, [_vp, ALLTOALL_FN, _vp]),
    "pf_set_exchange_rows": (C.c_int, [_vp, ALLTOALLV_FN, _vp]),
    "pf_rccl_available": (C.c_int, []),
    "pf_release_rccl": (C.c_int, [_vp]),
    "pf_rccl_comm_count": (C.c_int, [_vp]),
    "pf_rccl_unique_id": (C.c_int, [_vp]),
    "pf_rccl_version": (C.c_int, [C.POINTER(C.c_int)]),
    "pf_init_rccl": (C.c_int, [_vp, _vp]),
    "pf_set_allreduce": (C.c_int, [_vp, ALLREDUCE_FN, _vp]),
    "pf_fabric_create": (_vp, [C.c_int]),
    "pf_fabric_destroy": (None, [_vp]),
    "pf_fabric_attach": (C.c_int, [_vp, _vp]),
    "pf_fabric_set_delay": (C.c_int, [_vp, C.c_int]),
    "pf_debug_exchange": (C.c_int, [_vp, C.c_size_t]),
    "pf_exchange_buffers": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "pf_set_stream": (C.c_int, [_vp, _vp]),
    "pf_get_stream": (_vp, [_vp]),
    "pf_set_density": (C.c_int, [_vp, _dp]),
    "pf_synth_density": (C.c_int, [_vp, C.c_uint64, C.c_double, C.c_double]),
    "pf_pk_norm": (C.c_int, [C.POINTER(GenicParams), C.c_double, _dp]),
    "pf_genic_density": (C.c_int, [_vp, C.POINTER(GenicParams)]),
    "pf_set_invgrow": (C.c_int, [_vp, C.c_int, _dp, _dp, C.c_int]),
    "pf_set_growth": (C.c_int, [_vp, _dp]),
    "pf_sweep": (C.c_int, [_vp, C.c_int, _dp, _dp]),
    "pf_second_derivatives": (C.c_int, [_vp, C.c_double]),
    "pf_collapse_times": (C.c_int, [_vp, C.c_int, _dp]),
    "pf_displacements": (C.c_int, [_vp, C.c_int, C.c_int]),
    "pf_fmax_pdf": (C.c_int, [_vp, C.POINTER(C.c_ulonglong)]),
    "pf_get_products": (C.c_int, [_vp, _vp, C.POINTER(ProductLayout)]),
    "pf_derivative": (C.c_int, [_vp, C.POINTER(C.c_double), C.c_int, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_double)]),
    "pf_select_sorted": (C.c_int, [_vp, C.c_float, C.c_size_t, C.POINTER(C.c_uint), C.POINTER(C.c_float), C.POINTER(C.c_size_t)]),
    "pf_get_block": (C.c_int, [_vp, C.c_char_p, C.c_int, _vp]),
    "pf_count_peaks": (C.c_int, [_vp, C.c_double, C.POINTER(PeakRegion), C.POINTER(C.c_ulonglong)]),
    "pf_select_peaks": (C.c_int, [_vp, C.c_double, C.c_size_t, C.POINTER(C.c_uint), C.POINTER(C.c_float), C.POINTER(C.c_size_t)]),
    "pf_debug_peaks": (C.c_int, [C.c_int, C.POINTER(C.c_float), C.c_double, C.POINTER(PeakRegion), C.POINTER(C.c_ulonglong)]),
    "pf_distribute": (C.c_int, [_vp, C.c_double, C.POINTER(SubBox), C.POINTER(C.c_uint), C.POINTER(ProductLayout), C.c_size_t, _vp,
                                C.POINTER(C.c_uint), C.POINTER(C.c_size_t)]),
    "pf_debug_distribute": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_double, C.POINTER(SubBox), C.POINTER(C.c_uint),
                                      C.c_size_t, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_size_t)]),
    "pf_distribute_sorted": (C.c_int, [_vp, C.c_double, C.POINTER(SubBox), C.POINTER(C.c_uint), C.POINTER(ProductLayout), C.c_size_t, _vp,
                                       C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "pf_organize": (C.c_int, [_vp, C.POINTER(ProductLayout), C.c_size_t, _vp, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_int)]),
    "pf_debug_organize": (C.c_int, [C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_int)]),
    "pf_map_create": (C.c_int, [_vp, C.POINTER(PeakRegion), C.POINTER(_vp)]),
    "pf_map_destroy": (None, [_vp]),
    "pf_map_length": (C.c_size_t, [_vp]),
    "pf_map_fill_box": (C.c_int, [_vp]),
    "pf_map_update": (C.c_int, [_vp, C.c_size_t, _dp, C.POINTER(C.c_int), C.c_double, C.POINTER(C.c_ulonglong)]),
    "pf_map_commit": (C.c_int, [_vp, C.c_int]),
    "pf_map_get": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_uint)]),
    "pf_map_set": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_uint)]),
    "pf_map_count": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_ulonglong)]),
    "pf_debug_map_atomics": (C.c_int, [_vp, C.POINTER(C.c_ulonglong)]),
    "pf_distribute_map": (C.c_int, [_vp, C.c_double, _vp, C.c_int, C.POINTER(ProductLayout), C.c_size_t, _vp, C.POINTER(C.c_uint),
                                    C.POINTER(C.c_size_t)]),
    "pf_distribute_sorted_map": (C.c_int, [_vp, C.c_double, _vp, C.c_int, C.POINTER(ProductLayout), C.c_size_t, _vp, C.POINTER(C.c_uint),
                                           C.POINTER(C.c_uint), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "pf_count_peaks_map": (C.c_int, [_vp, C.c_double, _vp, C.c_int, C.POINTER(C.c_ulonglong)]),
    "pf_neighbours": (C.c_int, [_vp, C.POINTER(PeakRegion), C.c_size_t, C.POINTER(C.c_uint), _vp, C.c_size_t, C.POINTER(C.c_int),
                                C.POINTER(C.c_ubyte), C.POINTER(C.c_ulonglong)]),
    "pf_debug_neigh_ms": (C.c_int, [_dp, _dp]),
    "pf_distribute_sorted_neighbours_map": (C.c_int, [_vp, C.c_double, _vp, C.c_int, C.POINTER(ProductLayout), C.c_size_t, _vp, C.POINTER(C.c_uint),
                                                      C.POINTER(C.c_uint), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_ubyte),
                                                      C.POINTER(C.c_ulonglong), C.POINTER(C.c_size_t)]),
    "pf_back_reset": (C.c_int, [_vp]),
    "pf_distribute_back": (C.c_int, [_vp, C.POINTER(PeakRegion), C.c_size_t, C.POINTER(C.c_uint), _vp, C.c_size_t, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "pf_back_apply": (C.c_int, [_vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_size_t]),
    "pf_update_back": (C.c_int, [_vp, _vp, C.c_size_t, C.c_long, C.c_long]),
    "pf_debug_distribute_back": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(PeakRegion), C.c_size_t, C.POINTER(C.c_uint), C.POINTER(C.c_float),
                                           C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "pf_shift_displacements": (C.c_int, [_vp]),
    "pf_drop_prev": (C.c_int, [_vp]),
    "pf_prev_shifts": (C.c_int, [_vp]),
    "pf_gather_velocities": (C.c_int, [_vp, C.POINTER(PeakRegion), C.c_size_t, C.POINTER(C.c_uint), C.POINTER(C.c_int), C.c_size_t, C.POINTER(C.c_uint), _vp,
                                       C.POINTER(C.c_size_t)]),
    "pf_refresh_velocities": (C.c_int, [_vp, C.POINTER(PeakRegion), C.c_size_t, C.POINTER(C.c_uint), C.POINTER(C.c_int), _vp, C.POINTER(ProductLayout),
                                        C.POINTER(PrevLayout), C.POINTER(C.c_size_t)]),
    "pf_debug_gather_velocities": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.POINTER(PeakRegion), C.c_size_t, C.POINTER(C.c_uint), C.POINTER(C.c_int),
                                             C.POINTER(C.c_uint), _vp, C.POINTER(C.c_size_t)]),
    "pf_group_velocity_sums": (C.c_int, [_vp, C.POINTER(PeakRegion), C.c_size_t, C.POINTER(C.c_uint), C.POINTER(C.c_int), C.c_size_t, C.c_int, C.c_size_t,
                                         C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(C.c_double), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "pf_refresh_segment": (C.c_int, [_vp, C.POINTER(PeakRegion), C.c_size_t, C.POINTER(C.c_uint), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_size_t, C.c_int,
                                     _vp, C.POINTER(ProductLayout), C.POINTER(PrevLayout), _vp, C.c_size_t, C.POINTER(GroupLayout), C.POINTER(C.c_size_t),
                                     C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "pf_debug_group_velocity_sums": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.POINTER(PeakRegion), C.c_size_t, C.POINTER(C.c_uint),
                                               C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(C.c_double),
                                               C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "pf_debug_groupvel_times": (C.c_int, [C.POINTER(C.c_double)]),
    "pf_plc_set_cosmology": (C.c_int, [_vp, C.POINTER(PlcCosmology)]),
    "pf_plc_set_geometry": (C.c_int, [_vp, C.POINTER(PlcGeometry)]),
    "pf_plc_cross": (C.c_int, [_vp, C.c_int, C.POINTER(PlcSegment), C.POINTER(PeakRegion), C.c_size_t, _vp, C.POINTER(PlcGroupLayout), _vp, C.c_size_t, C.c_int,
                               C.c_size_t, _vp, C.POINTER(PlcOutLayout), C.POINTER(C.c_uint), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_size_t),
                               C.POINTER(C.c_size_t)]),
    "pf_debug_plc_times": (C.c_int, [C.POINTER(C.c_double)]),
    "pf_catalog": (C.c_int, [_vp, C.POINTER(PlcSegment), C.POINTER(PeakRegion), C.POINTER(CatalogParams), C.c_size_t, _vp, C.POINTER(PlcGroupLayout), C.c_size_t, _vp,
                             C.POINTER(CatalogOutLayout), C.POINTER(C.c_uint), C.POINTER(MfBins), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_size_t)]),
    "pf_debug_catalog_times": (C.c_int, [C.POINTER(C.c_double)]),
    "pf_debug_catalog_parts": (C.c_int, [C.POINTER(C.c_double)]),
    "pf_point_states": (C.c_int, [_vp, C.POINTER(PlcSegment), C.POINTER(PeakRegion), C.POINTER(PointParams), C.c_size_t, C.POINTER(C.c_uint), C.POINTER(C.c_int),
                                  C.c_size_t, C.POINTER(C.c_uint), _vp, C.POINTER(C.c_size_t)]),
    "pf_debug_point_states": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.POINTER(PlcSegment), C.POINTER(PeakRegion), C.POINTER(PointParams),
                                        C.c_size_t, C.POINTER(C.c_uint), C.POINTER(C.c_int), C.POINTER(C.c_uint), _vp, C.POINTER(C.c_size_t)]),
    "pf_debug_point_times": (C.c_int, [C.POINTER(C.c_double)]),
    "pf_set_collapse_model": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double)]),
    "pf_set_modified_gravity": (C.c_int, [_vp, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_double)]),
    "pf_set_tabulated_ct": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_double)]),
    "pf_ct_build": (C.c_int, [_vp, C.c_int, C.c_double, C.POINTER(C.c_double)]),
    "pf_ct_load": (C.c_int, [_vp, C.c_int, C.c_double, C.POINTER(C.c_double)]),
    "pf_debug_math": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_size_t, C.POINTER(C.c_double)]),
    "pf_debug_stream_rate": (C.c_int, [_vp, C.c_int, C.c_int, _dp]),
    "pf_debug_lines": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, _dp, _dp]),
    "pf_debug_pk": (C.c_int, [C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int]),
    "pf_debug_gfft": (C.c_int, [C.c_int, C.c_int, _dp, _dp]),
    "pf_debug_gfft_lines": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp]),
    "pf_debug_strided_jobs": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, _dp, _dp]),
    "pf_debug_strided_band": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _dp, _dp, C.POINTER(C.c_int)]),
    "pf_debug_zpass_jobs": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_double,
                                      _dp, C.c_int, _dp, _dp, _dp, _dp, C.POINTER(C.c_int)]),
    "pf_debug_strided_xfuse": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                         _dp, _dp, _dp]),
    "pf_debug_invariant_reruns": (C.c_int, [_vp]),
    "pf_solve_ran_beside_zpass": (C.c_int, [_vp]),
    "pf_transform_path": (C.c_int, [_vp]),
    "pf_invgrow_table_status": (C.c_int, [_vp, C.c_int, _dp]),
    "pf_set_loopback_exchange": (C.c_int, [_vp, C.c_int]),
    "pf_loopback_active": (C.c_int, [_vp]),
    "pf_set_sources_in_sweep": (C.c_int, [_vp, C.c_int]),
    "pf_set_lpt_order": (C.c_int, [_vp, C.c_int]),
    "pf_set_ct_interpolation": (C.c_int, [_vp, C.c_int]),
    "pf_set_transposed_spectra": (C.c_int, [_vp, C.c_int]),
    "pf_replicated_spectrum": (C.c_int, [_vp]),
    "pf_update_products": (C.c_int, [_vp, _vp, C.POINTER(ProductLayout)]),
    "pf_set_growth_table": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_double, C.c_double, C.c_double]),
    "pf_get_second_derivative": (C.c_int, [_vp, C.c_int, _dp]),
    "pf_get_kvector": (C.c_int, [_vp, C.c_int, _dp]),
    "pf_get_density": (C.c_int, [_vp, _dp]),
    "pf_debug_replicated_rows": (C.c_int, [_vp, C.c_int, C.c_int, _dp]),
    "pf_plan_bytes": (C.c_int, [C.POINTER(Config), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "pf_forward_transform": (C.c_int, [_vp, _dp, _dp]),
    "pf_reverse_transform": (C.c_int, [_vp, _dp, _dp]),
    "pf_collapse_cells": (C.c_int, [_vp, C.c_int, _dp, C.c_size_t, _dp]),
    "pf_set_arithmetic": (C.c_int, [_vp, C.c_int]),
    "pf_get_arithmetic": (C.c_int, [_vp]),
    "pf_flavour_census": (C.c_int, [_vp, C.c_int, _dp, _dp, C.POINTER(Census), C.c_size_t, C.POINTER(CensusCell)]),
    "pf_debug_census": (C.c_int, [C.c_int, C.c_ulonglong, C.c_size_t, _vp, C.POINTER(C.c_int), _vp, C.POINTER(C.c_int), C.POINTER(Census), C.c_size_t,
                                  C.POINTER(CensusCell)]),
    "pf_power_bins": (C.c_int, [C.c_int]),
    "pf_power_spectrum": (C.c_int, [_vp, C.c_int, C.c_int, _dp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), _dp, _dp, C.POINTER(PowerInfo)]),
    "pf_debug_power_spectrum": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.c_int, _dp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), _dp, _dp,
                                          C.POINTER(PowerInfo)]),
    "pf_debug_power_times": (C.c_int, [_dp]),
    "pf_matter_power": (C.c_int, [_vp, C.c_int, _dp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), _dp, _dp, _dp, C.POINTER(MatterInfo)]),
    "pf_debug_matter_deposit": (C.c_int, [C.c_int, C.c_int, _vp, C.c_int, _dp, C.POINTER(C.c_ulonglong), C.POINTER(MatterInfo)]),
    "pf_debug_matter_shells": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), _dp, _dp,
                                         C.POINTER(MatterInfo)]),
    "pf_debug_matter_times": (C.c_int, [_dp]),
    "pf_debug_matter_form": (C.c_int, [C.POINTER(C.c_int)]),
    "pf_matter_power_slabs": (C.c_int, [_vp, C.c_int, _dp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), _dp, _dp, _dp, C.POINTER(MatterInfo)]),
    "pf_debug_matter_slabs": (C.c_int, [_vp, _vp, C.c_int, _dp, C.POINTER(C.c_ulonglong), C.POINTER(MatterInfo)]),
    "pf_debug_matter_exchange": (C.c_int, [C.POINTER(C.c_ulonglong)]),
    "pf_halo_power": (C.c_int, [_vp, C.c_int, C.c_size_t, _dp, C.c_double, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_ulonglong),
                                C.POINTER(C.c_ulonglong), _dp, _dp, C.POINTER(HaloInfo)]),
    "pf_debug_halo_deposit": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, _dp, C.c_double, C.POINTER(C.c_int), C.c_int, C.c_int,
                                        C.POINTER(C.c_ulonglong), C.POINTER(HaloInfo)]),
    "pf_debug_halo_times": (C.c_int, [_dp]),
    "pf_halo_multipoles": (C.c_int, [_vp, C.c_int, C.c_size_t, _dp, _dp, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int),
                                     C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), _dp, _dp, C.POINTER(HaloInfo)]),
    "pf_debug_halo_deposit_rsd": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, _dp, _dp, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int,
                                            C.POINTER(C.c_ulonglong), C.POINTER(HaloInfo)]),
    "pf_debug_multipole_shells": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), _dp, _dp, _dp,
                                            C.POINTER(MatterInfo)]),
    "pf_debug_multipole_form": (C.c_int, [C.POINTER(C.c_int)]),
    "pf_halo_correlation": (C.c_int, [_vp, C.c_int, C.c_size_t, _dp, _dp, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int),
                                      C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), _dp, _dp, C.POINTER(CorrInfo)]),
    "pf_debug_corr_form": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, C.POINTER(MatterInfo)]),
    "pf_debug_corr_shells": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), _dp, _dp,
                                       C.POINTER(C.c_ulonglong)]),
    "pf_debug_corr_passes": (C.c_int, [C.POINTER(C.c_int)]),
    "pf_debug_corr_times": (C.c_int, [_dp]),
    "pf_bispectrum_triangles": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "pf_halo_bispectrum": (C.c_int, [_vp, C.c_int, C.c_size_t, _dp, _dp, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int),
                                     C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ulonglong), _dp, _dp, _dp, C.POINTER(BispecInfo)]),
    "pf_debug_bispec_mask": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp,
                                       C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "pf_debug_bispec_triples": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.POINTER(C.c_ulonglong)]),
    "pf_debug_bispec_times": (C.c_int, [_dp]),
    "pf_get_cputime": (C.c_int, [_vp, C.POINTER(CpuTime)]),
    "pf_reset_cputime": (C.c_int, [_vp]),
    "pf_kernel_stats": (C.c_int, [_vp, C.POINTER(KernelStat), C.c_int, C.POINTER(C.c_int)]),
    "pf_reset_kernel_stats": (C.c_int, [_vp]),
    "pf_synchronize": (C.c_int, [_vp]),
    "pf_device_bytes": (C.c_size_t, [_vp]),
}

_lib = None


def source_sha() -> str:
    """16 hex digits identifying the kernel sources next to this file (csrc/*.hip, *.h, *.cpp): stamps counter profiles, so
    that numbers measured on other kernels are never attached to a run (bench.py, profiles/tools/summarise.py)"""
    import glob
    import hashlib
    h = hashlib.sha256()
    for path in sorted(glob.glob(os.path.join(PKG, "csrc", "*.hip")) + glob.glob(os.path.join(PKG, "csrc", "*.h")) +
                       glob.glob(os.path.join(PKG, "csrc", "*.cpp"))):
        h.update(os.path.basename(path).encode())
        with open(path, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def load():
    """Load the HIP library; raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO):
            raise ImportError(
                f"{SO} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). pinocchio_amd has no CPU fallback.")
        L = C.CDLL(SO)
        for name, (res, args) in PROTOTYPES.items():
            f = getattr(L, name)  # AttributeError if the ABI and the header disagree
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib
