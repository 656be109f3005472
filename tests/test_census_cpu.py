"""The flavour census without a device: the per-cell classification of the device path (pinocchio_amd/csrc/pf_census_core.h, compiled
for the host in tests/cpu_emul/census_emul.cpp and run cell by cell) against the numpy restatement of the definitions
(tests/np_census.py) on the planted columns of tests/census_cases.py, for float and double products.  The same file as a program
reads the same cases under -fsanitize=address,undefined."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import census_cases as cc
import np_census as npc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "cpu_emul", "census_emul.cpp")
SO = os.path.join(HERE, "cpu_emul", "libcensus_emul.so")
EXE = os.path.join(HERE, "cpu_emul", "census_emul_san")
HDRS = [os.path.join(ROOT, "pinocchio_amd", "csrc", "pf_census_core.h"), os.path.join(ROOT, "include", "pinfmax.h")]
COUNT_FIELDS = ("cells", "differing_bits", "beyond_2ulp", "rmax_differing", "nonfinite", "outliers")


class Census(C.Structure):   # (this test's own statement of pf_census; the package's is held against the header in test_abi_census.py)
    _fields_ = [("cells", C.c_ulonglong), ("differing_bits", C.c_ulonglong), ("hist", C.c_ulonglong * 64), ("beyond_2ulp", C.c_ulonglong),
                ("rmax_differing", C.c_ulonglong), ("nonfinite", C.c_ulonglong), ("outliers", C.c_ulonglong), ("max_abs", C.c_double), ("max_ulps", C.c_double),
                ("max_abs_cell", C.c_ulonglong)]


def _stale(product):
    return not os.path.exists(product) or any(os.path.getmtime(product) < os.path.getmtime(s) for s in [SRC] + HDRS)


@pytest.fixture(scope="module")
def emul():
    if _stale(SO):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DCENSUS_EMUL_LIB", "-o", SO, SRC])
    L = C.CDLL(SO)
    L.census_emul_run.restype = C.c_int
    L.census_emul_run.argtypes = [C.c_int, C.c_ulonglong, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Census), C.c_size_t, C.c_void_p]
    return L


def run_emul(L, fast, exact, rf, re, first_cell=0, capacity=None):
    cap = len(fast) if capacity is None else capacity
    out = Census()
    rec = np.zeros(cap + 1, dtype=npc.CELL_DTYPE)
    rec["cell"][cap] = 0xABCDEF    # the element behind the capacity stays as it is
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.census_emul_run(fast.dtype.itemsize, first_cell, len(fast), vp(fast), vp(rf), vp(exact), vp(re), C.byref(out), cap, vp(rec)) == 0
    assert rec["cell"][cap] == 0xABCDEF
    cen = {k: int(getattr(out, k)) for k in COUNT_FIELDS}
    cen["hist"] = np.array(out.hist[:], dtype=np.uint64)
    cen["max_abs"], cen["max_ulps"], cen["max_abs_cell"] = float(out.max_abs), float(out.max_ulps), int(out.max_abs_cell)
    return cen, rec[:min(cen["outliers"], cap)].copy()


CASES = [(np.dtype(T).name, c[0]) for T in cc.DTYPES for c in cc.cases(T)]


def _case(tname, name):
    return next(c for c in cc.cases(np.dtype(tname).type) if c[0] == name)


@pytest.mark.parametrize("tname,name", CASES)
def test_core_on_the_host_against_numpy(emul, tname, name):
    _, f, e, rf, re, first = _case(tname, name)
    got, rec = run_emul(emul, f, e, rf, re, first)
    want, wrec = npc.census(f, e, rf, re, first)
    print(name, tname, {k: got[k] for k in COUNT_FIELDS}, got["max_abs"], got["max_ulps"], got["max_abs_cell"], np.flatnonzero(got["hist"]))
    assert npc.same(got, want) is None, npc.same(got, want)
    assert npc.same_records(rec, wrec)
    npc.invariants(got)
    npc.invariants(want)


def test_the_planted_cells_fall_where_the_definitions_say(emul):
    """the restatement itself, cell by cell on the planted column: what each planted cell was planted for"""
    for T in cc.DTYPES:
        f, e, rf, re = cc.planted(T)
        bins, nonfin = [], []
        for i in range(len(f)):
            c, _ = run_emul(emul, f[i:i + 1], e[i:i + 1], rf[i:i + 1], re[i:i + 1])
            assert npc.same(c, npc.census(f[i:i + 1], e[i:i + 1], rf[i:i + 1], re[i:i + 1])[0]) is None, i
            nonfin.append(c["nonfinite"])
            bins.append(-1 if c["nonfinite"] else int(np.flatnonzero(c["hist"])[0]))
        last = 63
        pw = 51 if T is np.float64 else 21    # 2^50 (2^20) ulp: bin k with 2^(k-2) < u <= 2^(k-1)
        assert bins[:16] == [0, 0, 0, 1, 2, 3, 3, 4, 2, 3, 1, 1, 1, 4, 2, 2 + (52 if T is np.float64 else 23)], (T, bins)
        assert bins[16:19] == [pw, pw + 1, 1 + (52 if T is np.float64 else 23)], (T, bins)    # (the last: 2^12 in ulps of 2^12)
        # max against 1: 2^(128 + 23) ulp and more; max against -max: d = +inf with double products, 2^25 ulp of the top binade with float ones
        assert bins[19:21] == [last, last if T is np.float64 else 26], (T, bins)
        assert bins[21:] == [-1, -1, 0, -1, -1, -1, 0, -1, -1, 0, 3], (T, bins)
        whole, rec = run_emul(emul, f, e, rf, re)
        assert whole["rmax_differing"] == 3 and whole["differing_bits"] == len(f) - 4 and whole["nonfinite"] == 7
        assert whole["beyond_2ulp"] == sum(b >= 3 for b in bins) and len(rec) == whole["outliers"] == whole["beyond_2ulp"] + 7
        assert whole["max_abs"] == (np.inf if T is np.float64 else 2.0 * float(np.finfo(np.float32).max)) and whole["max_abs_cell"] == 20


def test_exactly_two_ulp_is_not_beyond_two_ulp(emul):
    for T in cc.DTYPES:
        for x in (1.0, 1.5, 0.3, -2.75, 1000.0, 2.0 ** -40):
            e = np.array([x], dtype=T)
            sp = np.spacing(np.maximum(np.abs(e), T(1)))
            for k, beyond in ((1, 0), (2, 0), (3, 1), (-2, 0), (-3, 1)):
                c, rec = run_emul(emul, e + T(k) * sp, e, np.zeros(1, np.int32), np.zeros(1, np.int32))
                assert c["beyond_2ulp"] == beyond == len(rec) and c["max_ulps"] == abs(k), (T, x, k, c)


def test_first_cell_across_2_32(emul):
    _, f, e, rf, re, first = _case("float32", "across_2_32")
    c, rec = run_emul(emul, f, e, rf, re, first)
    assert first == 2 ** 32 - 5 and len(f) == 11
    assert rec["cell"].tolist() == [2 ** 32 - 3, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5] and c["max_abs_cell"] == 2 ** 32 + 5 and c["nonfinite"] == 1


def test_capacity(emul):
    for T in cc.DTYPES:
        f, e, rf, re = cc.random_columns(T)
        full, frec = run_emul(emul, f, e, rf, re)
        assert full["outliers"] > 500
        for cap in (0, 1, full["outliers"] - 1, full["outliers"], full["outliers"] + 7):
            c, rec = run_emul(emul, f, e, rf, re, capacity=cap)
            assert npc.same(c, full) is None and npc.same_records(rec, frec[:cap])
            assert npc.same_records(rec, npc.census(f, e, rf, re, 0, capacity=cap)[1])
        assert (np.diff(frec["cell"].astype(np.int64)) > 0).all()


def test_program_under_sanitizers(emul, tmp_path):
    """the stand-alone build of the same file on every case, with a record array of exactly the capacity: clean under the
    sanitizers, and the counts those of the library build"""
    if _stale(EXE):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-o", EXE, SRC])
    todo = []
    for T in cc.DTYPES:
        for c in cc.cases(T):
            nout = npc.census(*c[1:5])[0]["outliers"]
            for cap in sorted({0, nout // 2, nout + 3}):
                todo.append((c, cap))
    path = tmp_path / "cases.bin"
    with open(path, "wb") as fh:
        for (name, f, e, rf, re, first), cap in todo:
            np.array([f.dtype.itemsize, first, len(f), cap], dtype=np.int64).tofile(fh)
            for a in (f, e, rf, re):
                b = a.tobytes()
                fh.write(b + b"\0" * (-len(b) % 8))
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True)
    print(out.stdout[-3000:], out.stderr[-3000:])
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and len(lines) == len(todo) and "ERROR" not in out.stderr
    for k, ((name, f, e, rf, re, first), cap) in enumerate(todo):
        c, rec = run_emul(emul, f, e, rf, re, first, capacity=cap)
        w = lines[k].split()
        assert w[:2] == ["case", "%d:" % k], lines[k]
        got = dict(zip(w[2::2], (int(x) for x in w[3::2])))
        assert got == {"outliers": c["outliers"], "beyond": c["beyond_2ulp"], "differing": c["differing_bits"], "nonfinite": c["nonfinite"],
                       "histsum": int(c["hist"].sum()), "maxcell": c["max_abs_cell"], "cellsum": int(rec["cell"].astype(object).sum()) % 2 ** 64 if len(rec) else 0}, (name, cap)
