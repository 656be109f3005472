"""The particle states at collapse time without a device: the arithmetic of the device path (pinocchio_amd/csrc/pf_points_core.h,
compiled for the host in tests/cpu_emul/points_emul.cpp and run particle by particle) against the numpy restatement
(tests/np_points.py) on the cases of tests/points_cases.py, with the pass criteria the GPU test applies to the kernel.  The inputs'
own conditions are checked here with the oracle alone.  The same file as a program reads the same cases under
-fsanitize=address,undefined."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import np_points as npo
import plc_cases as pc
import points_cases as qc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emul", "points_emul.cpp")
SO = os.path.join(HERE, "cpu_emul", "libpoints_emul.so")
EXE = os.path.join(HERE, "cpu_emul", "points_emul_san")
HDRS = [os.path.join(HERE, "..", "pinocchio_amd", "csrc", h) for h in ("pf_points_core.h", "pf_plc_core.h", "pf_refresh_core.h", "pf_back_core.h", "pf_neigh_core.h",
                                                                      "pf_collapse_core.h")]


def _stale(product):
    return not os.path.exists(product) or any(os.path.getmtime(product) < os.path.getmtime(s) for s in [SRC] + HDRS)


@pytest.fixture(scope="module")
def emul():
    if _stale(SO):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DPOINTS_EMUL_LIB", "-o", SO, SRC])
    L = C.CDLL(SO)
    L.points_emul_run.restype = C.c_longlong
    L.points_emul_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    return L


def run_emul(L, c, capacity=None):
    hdr, data = c.flat()
    cap = c.count if capacity is None else capacity
    rec, idx = np.zeros((cap + 1, 8)), np.zeros(cap + 1, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    found = L.points_emul_run(vp(hdr), vp(data), cap, vp(rec), vp(idx))
    assert found >= 0
    m = min(found, cap)
    return idx[:m].copy(), rec[:m].astype(c.T), int(found)


@pytest.mark.parametrize("name", list(qc.CASES))
def test_the_inputs_keep_their_conditions(name):
    qc.case(name).input_conditions()


@pytest.mark.parametrize("name", list(qc.CASES))
def test_core_on_the_host_against_numpy(emul, name):
    c = qc.case(name)
    index, states, found = run_emul(emul, c)
    c.check(index, states, found, printer=print)


def test_the_bound_for_double_products_is_twice_the_measurement_rounded_up():
    m = qc.MEASURED_ULP64
    assert m is not None and m > 0 and qc.ULP64_BOUND == 2.0 ** np.ceil(np.log2(2.0 * m))


def test_the_k_branches_are_those_of_interpolate_growth():
    cos = pc.cosmology(10)
    assert abs(cos.kmin - 1e-3) < 1e-18 and abs(cos.kmax - 10 ** 1.5) < 1e-12
    for k, want in ((5e-4, (0, 0.0, False)), (50.0, (9, 0.0, False)), (1.5e-3, (0, np.log10(1.5) / 0.5, True)), (0.02, (2, (np.log10(0.02) + 3.0) / 0.5 - 2, True))):
        _, kk, dk, both = npo.k_branch(cos, k, (1,))
        assert (int(kk[0]), bool(both[0])) == (want[0], want[2]) and abs(float(dk[0]) - want[1]) < 1e-15, k
    one = npo.k_branch(pc.cosmology(1), 123.0, (2,))
    assert not one[3].any() and not one[1].any()


def test_the_orders_the_context_lacks_are_zero(emul):
    for name, zero in (("o3_lpt2", (2, 3)), ("o2_lpt1_seg1", (1, 2, 3)), ("o3", ())):
        c = qc.case(name)
        _, st, _ = run_emul(emul, c)
        for f in range(4):
            assert (not st[:, f].any()) == (f in zero), (name, f)
    # ... and q2x then runs at the lower order: the states of order 3 on columns of order 2 are those of order 2
    a, b = qc.case("o3_lpt2"), qc.Case("o2_lpt2", order=2, lpt_order=2, seed=14)
    assert run_emul(emul, a)[1].tobytes() == run_emul(emul, b)[1].tobytes()


def test_line_1588_and_the_v31_switch_differ(emul):
    a, b = run_emul(emul, qc.case("seg1_o3")), run_emul(emul, qc.case("seg1_o3_v31"))
    assert a[2] == b[2] > 0 and not np.array_equal(a[1][:, 5:], b[1][:, 5:]) and np.array_equal(a[1][:, :5], b[1][:, :5])


def test_wrap_cases_in_closed_form(emul):
    for name in ("wrap_zero", "wrap_zero_f64_seg1"):
        c = qc.case(name)
        _, st, _ = run_emul(emul, c)
        assert st[:, 5:].tobytes() == c.oracle()["q"].tobytes(), name
    for name in ("wrap_both", "wrap_both_seg1_f64"):
        c = qc.case(name)
        _, st, _ = run_emul(emul, c)
        y = st[:, 6].astype(np.float64)
        assert (y >= 0).all() and (y <= 16).all() and c.oracle()["hi"][:, 1].any() and c.oracle()["lo"][:, 1].any(), name


def test_capacity(emul):
    c = qc.case("slab24")
    full = run_emul(emul, c)
    for cap in (0, 5, full[2]):
        index, st, found = run_emul(emul, c, capacity=cap)
        assert found == full[2] and st.tobytes() == full[1][:cap].tobytes() and np.array_equal(index, full[0][:cap])
        c.check(index, st, found, capacity=cap)


def test_program_under_sanitizers(emul, tmp_path):
    """the stand-alone build of the same file on every case: clean under the sanitizers, and the counts and the sum of x[0] exactly
    those of the library build"""
    if _stale(EXE):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-o", EXE, SRC])
    names = list(qc.CASES)
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for n in names:
            hdr, data = qc.case(n).flat()
            np.array([hdr.size, data.size], dtype=np.int64).tofile(f)
            hdr.tofile(f)
            data.tofile(f)
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and len(lines) == len(names) and "ERROR" not in out.stderr
    for k, n in enumerate(names):
        _, st, found = run_emul(emul, qc.case(n))
        xsum = 0.0
        for x in st[:, 5].astype(np.float64).tolist():
            xsum += x
        w = lines[k].split()
        assert w[:2] == ["case", "%d:" % k] and int(w[3]) == found and float(w[5]) == xsum, (n, lines[k], found, xsum)
