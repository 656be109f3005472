"""The halo-power call without a device: the per-halo arithmetic of the device path (pinocchio_amd/csrc/pf_halo_core.h, compiled
for the host in tests/cpu_emul/halo_emul.cpp) against the numpy restatement (tests/np_halo.py) on the planted lists of
tests/halo_cases.py -- grids and counters integer for integer, contrasts bit for bit --, the restatement against a brute-force loop
over the haloes in Python integers, and what each planted case was planted for, said of the restatement alone.  The same file as a
program reads the cases under -fsanitize=address,undefined."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import halo_cases as hc
import np_halo as nph

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "cpu_emul", "halo_emul.cpp")
SO = os.path.join(HERE, "cpu_emul", "libhalo_emul.so")
EXE = os.path.join(HERE, "cpu_emul", "halo_emul_san")
HDRS = [os.path.join(ROOT, "pinocchio_amd", "csrc", "pf_halo_core.h"), os.path.join(ROOT, "pinocchio_amd", "csrc", "pf_power_core.h"),
        os.path.join(ROOT, "include", "pinfmax.h")]
FIELDS = ("selected", "weight_sum", "weight2_hi", "weight2_lo", "nonfinite", "outside", "empty_cells", "max_cell", "modes", "nonfinite_modes")
WINDOWS = lambda n: ((0, n), (5, 3), (n - 1, 1))


class Info(C.Structure):   # (this test's own statement of pf_halo_info; the package's is held against the header in test_abi_halo.py)
    _fields_ = [(k, C.c_ulonglong) for k in FIELDS]


def _stale(product):
    return not os.path.exists(product) or any(os.path.getmtime(product) < os.path.getmtime(s) for s in [SRC] + HDRS)


def build_emul():
    if _stale(SO):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DHALO_EMUL_LIB", "-o", SO, SRC])
    L = C.CDLL(SO)
    vp = C.c_void_p
    L.halo_emul_deposit.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, vp, C.c_double, vp, C.c_int, C.c_int, vp, C.POINTER(Info)]
    L.halo_emul_contrast.argtypes = [C.c_int, C.c_size_t, vp, C.c_ulonglong, C.c_int, vp]
    return L


@pytest.fixture(scope="module")
def emul():
    return build_emul()


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def emul_deposit(L, n, case, lo, hi, ngp, x0=0, nxl=None):
    nxl = n - x0 if nxl is None else nxl
    grid = np.full(nxl * n * n + 1, 0x5A5A5A, np.uint64)     # a refused call leaves it as it is; the element behind the output always
    info = Info()
    flags = (1 if ngp else 0) | (4 if case["mass_weight"] else 0)
    rc = L.halo_emul_deposit(n, x0, nxl, flags, len(case["mass"]), _vp(case["pos"]), case["scale"], _vp(case["mass"]), lo, hi, _vp(grid), C.byref(info))
    assert rc in (0, 3) and grid[-1] == 0x5A5A5A
    got = {k: int(getattr(info, k)) for k in nph.INT_KEYS}
    if rc == 3:
        assert np.all(grid == 0x5A5A5A)
        return None, got
    return grid[:-1].reshape(nxl, n, n), got


def check(got, want, name, what, n, x0, nxl, ngp):
    g, gi = got
    w, wi = want
    if w is None:
        assert g is None and what == ("refused",) and {k: gi[k] for k in wi} == wi, name
        return
    assert what != ("refused",) and g is not None and g.dtype == np.uint64 and np.array_equal(g, w), name
    assert gi == wi, (name, gi, wi)
    if what is None:
        return
    if what[0] == "counts":
        assert (gi["selected"], gi["nonfinite"], gi["outside"]) == what[1:], name
    elif what[0] == "empty":
        assert gi["selected"] == gi["weight_sum"] == 0 and not np.any(g) and gi["empty_cells"] == nxl * n * n, name
    elif what[0] == "cell":
        (cx, cy, cz), value = what[1:]
        if x0 <= cx < x0 + nxl:
            assert int(g[cx - x0, cy, cz]) == value == gi["max_cell"] and gi["empty_cells"] == nxl * n * n - 1, name
        else:
            assert not np.any(g), name


@pytest.fixture(scope="module")
def wanted():
    """the restatement of every planted deposit on the whole box, computed once: (n, case, range index, ngp) -> (grid, info)"""
    out = {}
    for n in (16, 24):
        for case in hc.cases(n):
            for r, (lo, hi) in enumerate(case["ranges"]):
                for ngp in (False, True):
                    out[n, case["name"], r, ngp] = nph.deposit(n, case["pos"], case["mass"], lo, hi, case["scale"], case["mass_weight"], ngp)
    return out


def window_of(want, n, x0, nxl):
    """the planes [x0, x0 + nxl) of a whole-box restatement, with the two counters of those planes"""
    g, info = want
    if g is None:
        return want
    w = g[x0:x0 + nxl]
    return w, dict(info, empty_cells=int((w == 0).sum()), max_cell=int(w.max()))


@pytest.mark.parametrize("n", [16, 24])
def test_planted_lists(emul, wanted, n):
    for case in hc.cases(n):
        for r, (lo, hi) in enumerate(case["ranges"]):
            for ngp in (False, True):
                for x0, nxl in WINDOWS(n):
                    want = window_of(wanted[n, case["name"], r, ngp], n, x0, nxl)
                    check(emul_deposit(emul, n, case, lo, hi, ngp, x0, nxl), want, (case["name"], n, r, ngp, x0, nxl), case["what"][r], n, x0, nxl, ngp)


def test_the_window_of_the_restatement_is_its_own(wanted):
    """np_halo.deposit with a window against the window cut from its whole box"""
    n = 16
    case = next(c for c in hc.cases(n) if c["name"] == "random_777_weighted")
    for ngp in (False, True):
        g, info = nph.deposit(n, case["pos"], case["mass"], 100, 2 ** 31 - 1, 1.0, True, ngp, 5, 3)
        w, wi = window_of(wanted[n, case["name"], 1, ngp], n, 5, 3)
        assert np.array_equal(g, w) and info == wi


@pytest.mark.parametrize("n", [16, 24])
def test_contrast(emul, wanted, n):
    """cell / mean - 1 with the bin's own mean, bit for bit in both field types; the mean of the contrast is zero to rounding"""
    for case in hc.cases(n):
        for r in range(len(case["ranges"])):
            g, info = wanted[n, case["name"], r, False]
            if g is None or not info["weight_sum"]:
                continue
            for fb in (8, 4):
                out = np.zeros(n ** 3 + 1)
                out[-1] = 123.5
                assert emul.halo_emul_contrast(n, n ** 3, _vp(np.ascontiguousarray(g)), info["weight_sum"], fb, _vp(out)) == 0 and out[-1] == 123.5
                want = nph.contrast(g, info["weight_sum"], n, fb)
                assert np.array_equal(out[:-1].view(np.uint64), want.ravel().view(np.uint64)), (case["name"], r, fb)
            assert abs(float(np.mean(nph.contrast(g, info["weight_sum"], n)))) < 1e-9
    # one unit weight per cell: the mean is 2^30 and the contrast exactly zero
    g = np.full((n, n, n), 1 << 30, np.uint64)
    assert nph.mean(n ** 3, n) == float(1 << 30) and not np.any(nph.contrast(g, n ** 3, n))


@pytest.mark.parametrize("n", [16, 24])
def test_the_restatement_against_a_brute_force_loop(wanted, n):
    for case in hc.cases(n):
        for r, (lo, hi) in enumerate(case["ranges"]):
            for ngp in (False, True):
                g, info = wanted[n, case["name"], r, ngp]
                cells, bi = nph.brute_force(n, case["pos"], case["mass"], lo, hi, case["scale"], case["mass_weight"], ngp)
                assert {k: info[k] for k in bi} == bi, (case["name"], r, ngp)
                if g is None:
                    assert bi["weight_sum"] >= 1 << 34
                    continue
                dense = np.zeros((n, n, n), np.uint64)
                for (x, y, z), v in cells.items():
                    dense[x, y, z] = v
                assert np.array_equal(g, dense), (case["name"], r, ngp)
                assert sum(cells.values()) == info["weight_sum"] << 30


def random_positions(n):
    return hc.random_list(3, 40, n)[0]


def test_what_the_planted_cases_were_planted_for(wanted):
    """said of the restatement alone, so that a case cannot lose its point unnoticed"""
    for n in (16, 24):
        by = {c["name"]: c for c in hc.cases(n)}
        p = nph.positions(by["upper_edge"]["pos"], 1.0, n)
        assert p[0, 0] < n and p[0, 0] > n - 1e-12 and np.all(p[1] == n) and p[2, 1] == n and np.all(nph.classes(p, n) == 0)
        p = nph.positions(by["product_is_n"]["pos"], by["product_is_n"]["scale"], n)
        assert p[0, 0] == 0.0 and np.all(p[1] == 0.0) and np.all(by["product_is_n"]["pos"][1] * by["product_is_n"]["scale"] == n)
        sc = by["scaled"]
        assert np.any(nph.positions(sc["pos"], sc["scale"], n) != random_positions(n))   # the product rounds: not the positions the list was made from
        g, info = wanted[n, "headroom_15", 0, False]
        assert int(g[n - 1, 0, n - 1]) == 15 << 60 and info["weight_sum"] == 15 << 30 < 1 << 34
        g, info = wanted[n, "headroom_16", 0, False]
        assert g is None and info["weight_sum"] == 1 << 34
        _, info = wanted[n, "largest_int", 0, False]
        assert info["weight2_hi"] == 0 and info["weight2_lo"] == 3 * (2 ** 31 - 1) ** 2 and info["weight2_lo"] >> 32 > 0
        g, info = wanted[n, "one_cell", 0, True]
        assert int(g[3, 4, 5]) == 300 << 30 and info["empty_cells"] == n ** 3 - 1
        g, info = wanted[n, "one_cell", 0, False]
        assert 1 < np.count_nonzero(g) <= 27 and info["selected"] == 300
        g0, i0 = wanted[n, "range_ends", 0, False]
        g5, i5 = wanted[n, "range_ends", 5, False]
        assert i0["selected"] == 5 and i5["selected"] == 2 and np.all(g5 <= g0)           # overlapping ranges: the narrower is part of the wider
        assert len(by["random_777"]["mass"]) % 64 != 0 and len(by["random_777"]["mass"]) > 256
        assert nph.shot({"weight_sum": 4, "weight2_hi": 0, "weight2_lo": 4}) == 0.25 and np.isnan(nph.shot({"weight_sum": 0, "weight2_hi": 0, "weight2_lo": 0}))


def test_program_under_sanitizers(emul, tmp_path):
    """the stand-alone build of the same file on the planted lists, with arrays of exactly the sizes: clean under the sanitizers, and
    the numbers those of the library build"""
    if _stale(EXE):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-o", EXE, SRC])
    n = 16
    runs = [(case, lo, hi, ngp, x0, nxl) for case in hc.cases(n) for lo, hi in case["ranges"] for ngp in (False, True) for x0, nxl in ((0, n), (n - 1, 1))]
    path = tmp_path / "cases.bin"
    with open(path, "wb") as fh:
        for case, lo, hi, ngp, x0, nxl in runs:
            np.array([n, x0, nxl, (1 if ngp else 0) | (4 if case["mass_weight"] else 0), len(case["mass"]), lo, hi], dtype=np.int64).tofile(fh)
            np.array([case["scale"]], dtype=np.float64).tofile(fh)
            case["pos"].tofile(fh)
            case["mass"].tofile(fh)
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True)
    print(out.stdout[-3000:], out.stderr[-3000:])
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and len(lines) == len(runs) and "ERROR" not in out.stderr
    for k, (case, lo, hi, ngp, x0, nxl) in enumerate(runs):
        g, info = emul_deposit(emul, n, case, lo, hi, ngp, x0, nxl)
        got = dict(zip(lines[k].split()[2::2], lines[k].split()[3::2]))
        assert int(got["rc"]) == (3 if g is None else 0), k
        keys = ("selected", "weight_sum", "weight2_hi", "weight2_lo", "nonfinite", "outside") + (() if g is None else ("empty", "max"))
        assert [int(got[key]) for key in keys] == [info[{"empty": "empty_cells", "max": "max_cell"}.get(key, key)] for key in keys], k
        if g is not None:
            h = 1469598103934665603
            for x in g.ravel().tolist():
                h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
            assert int(got["hash"]) == h, k
