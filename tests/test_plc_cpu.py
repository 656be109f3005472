"""The light-cone test of build_groups() without a device: the arithmetic of the device path (pinocchio_amd/csrc/pf_plc_core.h,
compiled for the host in tests/cpu_emul/plc_emul.cpp and run pair by pair as the reference runs it) against the numpy restatement
(tests/np_plc.py) on the cases of tests/plc_cases.py, with the pass criteria the GPU test applies to the kernels.  The inputs'
own conditions -- at most 1e-3 of the tried pairs within 8 ulp32(L) of zero, condition_PLC monotonic on every crossing interval, no
crossing pair on the aperture's edge -- are checked here with the oracle alone.  The same file as a program reads the same cases
under -fsanitize=address,undefined."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import np_plc as npp
import plc_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emul", "plc_emul.cpp")
SO = os.path.join(HERE, "cpu_emul", "libplc_emul.so")
EXE = os.path.join(HERE, "cpu_emul", "plc_emul_san")
HDRS = [os.path.join(HERE, "..", "pinocchio_amd", "csrc", h) for h in ("pf_plc_core.h", "pf_collapse_core.h")]


def _stale(product):
    return not os.path.exists(product) or any(os.path.getmtime(product) < os.path.getmtime(s) for s in [SRC] + HDRS)


@pytest.fixture(scope="module")
def emul():
    if _stale(SO):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DPLC_EMUL_LIB", "-o", SO, SRC])
    L = C.CDLL(SO)
    L.plc_emul_run.restype = C.c_longlong
    L.plc_emul_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong)]
    return L


def run_emul(L, c, capacity=None):
    hdr, data = c.flat()
    cap = max(1, c.ncand * len(c.reps)) if capacity is None else capacity
    rec, oc, orr = np.zeros((cap + 1, 7)), np.zeros(cap + 1, np.int32), np.zeros(cap + 1, np.int32)
    nz, unc = np.zeros(c.nzbins + 1), C.c_longlong()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    n = L.plc_emul_run(vp(hdr), vp(data), cap, vp(rec), vp(oc), vp(orr), vp(nz), C.byref(unc))
    assert n >= 0
    m = min(n, cap)
    od = np.zeros(m, dtype=pc.out_dtype(c.T))
    od["z"], od["x"], od["v"] = rec[:m, 0], rec[:m, 1:4], rec[:m, 4:7]
    od["Mass"], od["name"] = c.groups["Mass"][oc[:m]], c.groups["name"][oc[:m]]
    return od, oc[:m], orr[:m], int(n), int(unc.value), nz[:c.nzbins]


def test_spline_is_gsl_natural_cubic():
    """np_plc.cspline against the closed form on three knots and against its own knots and natural ends"""
    c = npp.cspline([0.0, 1.0, 2.0], [0.0, 1.0, 0.0])
    assert np.allclose(c[1], [0.0, -1.5, 0.0]) and np.allclose(c[2][:2], [1.5, 0.0]) and np.allclose(c[3][:2], [-0.5, 0.5])
    cos = pc.cosmology(1)
    assert np.allclose(cos.comvdist(1.0 / np.array(pc.fixture()["rows"])[:, 0] - 1.0), np.array(pc.fixture()["rows"])[:, 1], rtol=0, atol=1e-9)
    # linear extrapolation outside
    x, y = cos.x, cos.comv[0]
    z_hi = 10.0 ** (-(x[0] - 0.01)) - 1.0
    assert np.isclose(cos.comvdist(z_hi), y[0] - 0.01 * (y[1] - y[0]) / (x[1] - x[0]), rtol=1e-12)


@pytest.mark.parametrize("name", list(pc.CASES))
def test_the_inputs_keep_their_conditions(name):
    pc.case(name).input_conditions()


@pytest.mark.parametrize("name", list(pc.CASES))
def test_core_on_the_host_against_numpy(emul, name):
    c = pc.case(name)
    od, oc, orr, n, unc, nz = run_emul(emul, c)
    c.check(od, oc, orr, n, unc)
    assert np.array_equal(nz, c.nz_expected(od))


def test_the_cases_do_cross(emul):
    """the crossing sets the cases are named after"""
    count = lambda name: run_emul(emul, pc.case(name))[3]
    assert count("n0") == 0 and count("none") == 0 and count("n1_r1_all") == 1 and count("all_r65") == 64 * 65
    od, oc, orr, n, _, _ = run_emul(emul, pc.case("last_r65"))
    assert n == 1 and oc.tolist() == [64] and orr.tolist() == [64]
    # Flast == F2 is tried at an event and not in the last check; F_lo == F1 is tried
    assert run_emul(emul, pc.case("equality_events"))[1].tolist() == [0, 1] and run_emul(emul, pc.case("equality_last_check"))[1].tolist() == [0]
    # the aperture: the groups at 25 degrees are stored, those at 35 are not
    assert run_emul(emul, pc.case("aperture"))[1].tolist() == list(range(0, 64, 2))
    # a group of no extent (Mass 0: interp at its top, k > kmax) is among the stored records of the scale-dependent cases
    for name in ("nk10", "f64_nk10", "n1025_r65_events_seg1_nk10_o2"):
        assert (run_emul(emul, pc.case(name))[0]["Mass"] == 0).any(), name
    assert count("n63_r13") > 10 and count("n1025_r65_events_seg1_nk10_o2") > 100 and count("f64_nk10") > 30


def test_line_1588_and_the_v31_switch_differ(emul):
    a, b = run_emul(emul, pc.case("n65_r13_seg1")), run_emul(emul, pc.case("n65_r13_seg1_v31"))
    assert a[3] > 0 and b[3] > 0
    same = min(a[3], b[3])
    assert a[3] != b[3] or not np.array_equal(a[0]["x"][:same], b[0]["x"][:same])


def test_capacity(emul):
    c = pc.case("n63_r13")
    full = run_emul(emul, c)
    for cap in (0, 5, full[3]):
        od, oc, orr, n, unc, _ = run_emul(emul, c, capacity=cap)
        assert n == full[3] and np.array_equal(od, full[0][:cap])


def test_program_under_sanitizers(emul, tmp_path):
    """the stand-alone build of the same file on every case: clean under the sanitizers, and crossings and the sum of z exactly those of
    the library build"""
    if _stale(EXE):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-o", EXE, SRC])
    names = list(pc.CASES)
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for n in names:
            hdr, data = pc.case(n).flat()
            np.array([hdr.size, data.size], dtype=np.int64).tofile(f)
            hdr.tofile(f)
            data.tofile(f)
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and len(lines) == len(names) and "ERROR" not in out.stderr
    for k, n in enumerate(names):
        od, _, _, count, unc, _ = run_emul(emul, pc.case(n))
        zsum = 0.0
        for z in od["z"].astype(np.float64).tolist():
            zsum += z
        w = lines[k].split()
        assert w[:2] == ["case", "%d:" % k] and int(w[3]) == count and int(w[5]) == unc == 0 and float(w[7]) == zsum, (n, lines[k], count, zsum)
