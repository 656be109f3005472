"""The matter-density call without a device: the per-particle and per-mode arithmetic of the device path
(pinocchio_amd/csrc/pf_matter_core.h, compiled for the host in tests/cpu_emul/matter_emul.cpp) against the numpy restatement
(tests/np_matter.py) on the planted columns and spectra of tests/matter_cases.py -- grids and counters integer for integer, the shell
sums to the tolerance tests/test_gpu_power.py derives for sums of positive terms --, the restatement of the shell sums against a
direct numpy sum, and the deconvolution table against mpmath.  The same file as a program reads the cases under
-fsanitize=address,undefined.

The tolerance of the two cross parts.  A cross term re_m re + im_m im is two products and one sum, each rounded once, and the file is
compiled without contraction: the library and the restatement form the SAME bits for every term, whatever cancels inside it (held
below, term by term, through the masks).  Each part is then a sum of positive terms, as `power` is: the restatement adds them exactly
(math.fsum) and the fixed-point form drops less than 2^-95 of the part's largest term per term and rounds three times in the
conversion, once more for 1 / N^6.  So TOL_POWER = 1e-14 of tests/test_gpu_power.py holds for power, cross_pos and cross_neg alike
(with the deconvolution too: its table differs between two libms by an ulp or two per entry, six entries per auto term).  `cross`
is their difference formed once: it is held to TOL_POWER of cross_pos + cross_neg."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import matter_cases as mc
import np_matter as npm
import np_power as npp
import power_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "cpu_emul", "matter_emul.cpp")
SO = os.path.join(HERE, "cpu_emul", "libmatter_emul.so")
EXE = os.path.join(HERE, "cpu_emul", "matter_emul_san")
HDRS = [os.path.join(ROOT, "pinocchio_amd", "csrc", "pf_matter_core.h"), os.path.join(ROOT, "pinocchio_amd", "csrc", "pf_power_core.h"),
        os.path.join(ROOT, "include", "pinfmax.h")]
TOL_POWER = 1e-14
INT_KEYS = ("deposited", "nonfinite", "outside", "empty_cells", "max_cell", "sum_hi32", "sum_lo32")


class Info(C.Structure):   # (this test's own statement of pf_matter_info; the package's is held against the header in test_abi_matter.py)
    _fields_ = [(k, C.c_ulonglong) for k in ("deposited", "nonfinite", "outside", "empty_cells", "max_cell", "sum_hi32", "sum_lo32", "modes", "nonfinite_modes")]


def _stale(product):
    return not os.path.exists(product) or any(os.path.getmtime(product) < os.path.getmtime(s) for s in [SRC] + HDRS)


def build_emul():
    if _stale(SO):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DMATTER_EMUL_LIB", "-o", SO, SRC])
    L = C.CDLL(SO)
    vp = C.c_void_p
    L.matter_emul_deposit.argtypes = [C.c_int, C.c_int, vp, C.c_int, vp, vp, C.POINTER(Info)]
    L.matter_emul_shells.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp, C.POINTER(Info)]
    L.matter_emul_deconv.argtypes = [C.c_int, C.c_int, vp]
    return L


@pytest.fixture(scope="module")
def emul():
    return build_emul()


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def emul_deposit(L, vel12, weight=None, ngp=False):
    n = vel12.shape[1]
    grid = np.zeros(n ** 3 + 1, np.uint64)
    grid[-1] = 0xABCDEF     # the element behind the output stays as it is
    w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
    info = Info()
    assert L.matter_emul_deposit(vel12.dtype.itemsize, n, _vp(np.ascontiguousarray(vel12)), 1 if ngp else 0, _vp(w), _vp(grid), C.byref(info)) == 0
    assert grid[-1] == 0xABCDEF
    return grid[:-1].reshape(n, n, n), {k: int(getattr(info, k)) for k in INT_KEYS}


def emul_shells(L, m, lin=None, y0=0, fb=8, ngp=False, deconvolve=False):
    m = np.ascontiguousarray(m, dtype=np.complex128)
    lin = None if lin is None else np.ascontiguousarray(lin, dtype=np.complex128)
    nyl, n = m.shape[:2]
    nb = npp.bins(n)
    nm, ks = np.zeros(nb + 1, np.uint64), np.zeros(nb + 1, np.uint64)
    pw, cr, parts = np.zeros(nb + 1), np.zeros(nb + 1), np.zeros(2 * nb + 1)
    nm[-1] = ks[-1] = 0xABCDEF
    pw[-1] = cr[-1] = parts[-1] = 123.5
    info = Info()
    flags = (1 if ngp else 0) | (2 if deconvolve else 0)
    assert L.matter_emul_shells(fb, n, y0, nyl, _vp(m), _vp(lin), flags, _vp(nm), _vp(ks), _vp(pw), _vp(cr) if lin is not None else None, _vp(parts), C.byref(info)) == 0
    assert nm[-1] == ks[-1] == 0xABCDEF and pw[-1] == cr[-1] == parts[-1] == 123.5
    return {"nmodes": nm[:-1], "k2sum": ks[:-1], "power": pw[:-1], "cross": cr[:-1] if lin is not None else None, "cross_pos": parts[:nb], "cross_neg": parts[nb:2 * nb],
            "modes": int(info.modes), "nonfinite_modes": int(info.nonfinite_modes)}


def check_grid(got, want, name, what, n):
    g, gi = got
    w, wi = want
    assert g.dtype == np.uint64 and np.array_equal(g, w), name
    assert gi == wi, (name, gi, wi)
    assert gi["sum_hi32"] * (1 << 32) + gi["sum_lo32"] == gi["deposited"] * npm.ONE, name
    assert gi["deposited"] + gi["nonfinite"] + gi["outside"] == n ** 3, name
    if what == "uniform":
        assert np.all(g == np.uint64(npm.ONE)) and gi["max_cell"] == npm.ONE and gi["empty_cells"] == 0, name
    elif what is not None and what[0] == "one_cell":
        assert int(g[what[1]]) == n ** 3 * npm.ONE == gi["max_cell"] and gi["empty_cells"] == n ** 3 - 1, name
    elif what is not None and what[0] == "counts":
        assert (gi["nonfinite"], gi["outside"]) == what[1:], name


def check_shells(got, want, what, with_parts=True):
    assert np.array_equal(got["nmodes"], want["nmodes"]) and np.array_equal(got["k2sum"], want["k2sum"]), what
    assert (got["modes"], got["nonfinite_modes"]) == (want["modes"], want["nonfinite_modes"]), what
    keys = ["power"] + (["cross_pos", "cross_neg"] if with_parts and want["cross"] is not None else [])
    r = {k: npp.rel(got[k], want[k]) for k in keys}
    print(what, r)
    assert all(v <= TOL_POWER for v in r.values()), (what, r)
    if want["cross"] is not None:
        scale = want["cross_pos"] + want["cross_neg"]
        d = np.abs(got["cross"] - want["cross"])
        print(what, "cross", float(np.max(d / np.where(scale > 0, scale, 1.0))))
        assert np.all(d <= TOL_POWER * scale), what


@pytest.fixture(scope="module")
def wanted():
    """the restatement of every planted deposit, computed once: (n, dtype name, case name) -> (grid, info)"""
    out = {}
    for n in (16, 24):
        for dt in (np.float32, np.float64):
            for name, v, w, ngp, _ in mc.cases(n, dt):
                out[n, np.dtype(dt).name, name] = npm.deposit(v, w, ngp)
    return out


@pytest.mark.parametrize("n", [16, 24])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_planted_deposits(emul, wanted, n, dt):
    for name, v, w, ngp, what in mc.cases(n, dt):
        want = wanted[n, np.dtype(dt).name, name]
        check_grid(emul_deposit(emul, v, w, ngp), want, (name, n, dt), what, n)
        if w is not None and set(w) <= {0.0, 1.0}:   # a 0 / 1 weight is the columns cleared by hand
            by_hand = emul_deposit(emul, mc.zeroed_by_hand(v, w), None, ngp)
            assert np.array_equal(by_hand[0], want[0]) and by_hand[1] == want[1], name


def test_what_the_planted_cases_were_planted_for(wanted):
    """said of the restatement alone, so that a case cannot lose its point unnoticed"""
    for n in (16, 24):
        v = next(c[1] for c in mc.cases(n, np.float32) if c[0] == "wrap_to_exactly_n")
        pos = npm.positions(v)
        assert all(np.any(p == np.float32(n)) for p in pos) and np.all(npm.classes(pos, n) == 0)
        pos64 = npm.positions(next(c[1] for c in mc.cases(n, np.float64) if c[0] == "wrap_to_exactly_n"))
        assert not any(np.any(p == n) for p in pos64)
        for dt in (np.float32, np.float64):
            pos = npm.positions(next(c[1] for c in mc.cases(n, dt) if c[0] == "below_half_a_cell"))
            assert np.floor(pos[0] - dt(0.5)).min() == -1
            p = npm.positions(next(c[1] for c in mc.cases(n, dt) if c[0] == "d_one_ulp_below_one"))[2][0, 0, 0]
            u = p - dt(0.5)
            d = u - np.floor(u)
            assert d == np.nextafter(dt(1), dt(0)) and int(d * dt(65536)) == 65535
            g, info = wanted[n, np.dtype(dt).name, "smooth_random_rms3"]
            assert info["deposited"] == n ** 3 and info["max_cell"] > 2 * npm.ONE
            v = next(c[1] for c in mc.cases(n, dt) if c[0] == "smooth_random_rms3")
            assert 2.9 < np.sqrt(np.mean(v[0].astype(np.float64) ** 2)) < 3.1


def test_the_deconvolution_table_against_mpmath(emul):
    import mpmath
    mpmath.mp.prec = 120
    for n in (16, 24, 48, 1024):
        for p in (1, 2):
            t = np.zeros(n // 2 + 1)
            assert emul.matter_emul_deconv(n, p, _vp(t)) == 0
            ref = [1.0] + [float((mpmath.pi * j / n / mpmath.sin(mpmath.pi * j / n)) ** p) for j in range(1, n // 2 + 1)]
            r = np.max(np.abs(t - ref) / ref)
            print("deconvolution table", n, p, r)
            assert t[0] == 1.0 and r <= 8 * np.finfo(np.float64).eps      # pi j / n, sin, two quotients, a square: each within an ulp
            assert npp.rel(npm.deconv_table(n, p == 1), ref) <= 8 * np.finfo(np.float64).eps


@pytest.mark.parametrize("fb", [8, 4])
def test_planted_modes(emul, fb):
    n = 16
    for name, m, lin, expect in mc.planted_modes(n):
        for dec in (False, True):
            got, want = emul_shells(emul, m, lin, 0, fb, False, dec), npm.shells(m, lin, 0, fb, False, dec)
            check_shells(got, want, (name, fb, dec))
            if not dec:     # exact small numbers: no rounding in any order
                for b in range(npp.bins(n)):
                    e = expect.get(b, (0.0, 0.0, 0.0))
                    assert (got["power"][b], got["cross_pos"][b], got["cross_neg"][b]) == tuple(x / float(n ** 6) for x in e), (name, b)
                    assert got["cross"][b] == (e[1] - e[2]) / float(n ** 6)
        if name == "cross_cancels":
            assert got["cross"][1] == 0.0 and got["cross_pos"][1] == got["cross_neg"][1] > 0


@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("n", [16, 20])
def test_random_boxes_and_their_slabs(emul, fb, n):
    m, lin = pc.random_box(31, n), pc.random_box(32, n)
    lin = 0.7 * m + 0.5 * lin        # correlated: most cross terms positive, some negative
    for ngp, dec in ((False, False), (False, True), (True, True)):
        whole = emul_shells(emul, m, lin, 0, fb, ngp, dec)
        want = npm.shells(m, lin, 0, fb, ngp, dec)
        check_shells(whole, want, (n, fb, ngp, dec))
        assert np.count_nonzero(want["cross_neg"]) > n // 4 and int(whole["nmodes"].sum()) == n ** 3
        # the two parts through the masks, the way the device tests reach them
        mp_, mn_ = npm.cross_masks(m, lin, 0, fb, ngp, dec)
        assert np.array_equal(emul_shells(emul, m, mp_, 0, fb, ngp, dec)["cross"], whole["cross_pos"])
        assert np.array_equal(emul_shells(emul, m, mn_, 0, fb, ngp, dec)["cross"], -whole["cross_neg"])
        halves = [emul_shells(emul, m[a:a + n // 2], lin[a:a + n // 2], a, fb, ngp, dec) for a in (0, n // 2)]
        for k in ("nmodes", "k2sum"):
            assert np.array_equal(halves[0][k] + halves[1][k], whole[k])
        for k in ("power", "cross_pos", "cross_neg"):
            assert npp.rel(halves[0][k] + halves[1][k], whole[k]) <= TOL_POWER
    only = emul_shells(emul, m, None, 0, fb)
    assert only["cross"] is None and np.array_equal(only["power"], emul_shells(emul, m, lin, 0, fb)["power"])


def test_the_restatement_of_the_shell_sums_against_a_direct_sum():
    """power against tests/np_power.py, cross against numpy's own complex product summed per shell"""
    n = 16
    m, lin = pc.random_box(41, n), pc.random_box(42, n)
    got = npm.shells(m, lin)
    ref = npp.power(m)
    assert np.array_equal(got["power"], ref["power"]) and np.array_equal(got["nmodes"], ref["nmodes"]) and np.array_equal(got["k2sum"], ref["k2sum"])
    _, sh, w = npp.geometry(n)
    x = w * (m * np.conj(lin)).real
    direct = np.array([x[sh == b].sum() for b in range(npp.bins(n))]) / float(n ** 6)
    scale = np.array([np.abs(x[sh == b]).sum() for b in range(npp.bins(n))]) / float(n ** 6)
    assert np.all(np.abs(got["cross"] - direct) <= 1e-13 * scale) and np.allclose(got["cross_pos"] + got["cross_neg"], scale, rtol=1e-13)
    # non-finite parts: counted, in no sum
    bad = m.copy()
    bad[3, 2, 1] = np.nan
    bad[0, 0, 8] = np.inf
    out = npm.shells(bad, lin)
    assert out["nonfinite_modes"] == 3 and np.all(np.isfinite(out["power"])) and np.all(np.isfinite(out["cross"]))


def test_program_under_sanitizers(emul, tmp_path):
    """the stand-alone build of the same file on the planted cases, with arrays of exactly the sizes: clean under the sanitizers, and
    the numbers those of the library build"""
    if _stale(EXE):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-o", EXE, SRC])
    dep = [(v, w, ngp) for dt in (np.float32, np.float64) for _, v, w, ngp, _ in mc.cases(16, dt)]
    dep.append((mc.smooth_random(24, np.float32, 3), None, False))
    sh = [(fb, m, lin, 0, dec) for fb in (8, 4) for _, m, lin, _ in mc.planted_modes(16) for dec in (False, True)]
    sh += [(8, pc.random_box(3, 20)[7:12], pc.random_box(4, 20)[7:12], 7, True), (4, pc.random_box(3, 20)[19:20], None, 19, False)]
    path = tmp_path / "cases.bin"
    with open(path, "wb") as fh:
        for v, w, ngp in dep:
            np.array([0, v.dtype.itemsize, v.shape[1], 1 if ngp else 0, 0 if w is None else 1], dtype=np.int64).tofile(fh)
            np.array(w if w is not None else (0, 0, 0, 0), dtype=np.float64).tofile(fh)
            np.ascontiguousarray(v).tofile(fh)
        for fb, m, lin, y0, dec in sh:
            np.array([1, fb, m.shape[1], y0, m.shape[0], 2 if dec else 0, 0 if lin is None else 1], dtype=np.int64).tofile(fh)
            np.ascontiguousarray(m, dtype=np.complex128).tofile(fh)
            if lin is not None:
                np.ascontiguousarray(lin, dtype=np.complex128).tofile(fh)
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True)
    print(out.stdout[-3000:], out.stderr[-3000:])
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and len(lines) == len(dep) + len(sh) and "ERROR" not in out.stderr
    for k, (v, w, ngp) in enumerate(dep):
        g, info = emul_deposit(emul, v, w, ngp)
        got = dict(zip(lines[k].split()[2::2], lines[k].split()[3::2]))
        h = 1469598103934665603
        for x in g.ravel().tolist():
            h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        assert [int(got[key]) for key in ("deposited", "nonfinite", "outside", "empty", "max", "hi", "lo", "hash")] == [info[key] for key in INT_KEYS] + [h], k
    for k, (fb, m, lin, y0, dec) in enumerate(sh):
        c = emul_shells(emul, m, lin, y0, fb, False, dec)
        got = dict(zip(lines[len(dep) + k].split()[2::2], lines[len(dep) + k].split()[3::2]))
        assert (int(got["nmodes"]), int(got["k2sum"]), int(got["nonfinite"])) == (int(c["nmodes"].sum()), int(c["k2sum"].sum()), c["nonfinite_modes"]), k
        sp, sc = 0.0, 0.0
        for b in range(len(c["power"])):
            sp += c["power"][b]
            sc += c["cross"][b] if lin is not None else 0.0
        assert float.fromhex(got["power"]) == sp and float.fromhex(got["cross"]) == sc, k
