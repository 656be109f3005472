"""The redshift-space multipoles without a device: the arithmetic of the device path (pf_halo_pos_rsd of
pinocchio_amd/csrc/pf_halo_core.h and pinocchio_amd/csrc/pf_multipole_core.h, compiled for the host in
tests/cpu_emul/multipole_emul.cpp) against the numpy restatement (tests/np_multipoles.py): moved positions bit for bit, grids and
counters integer for integer, the Legendre weights of every mode bit for bit, the eleven sums of a shell within the fixed point's
TOL_POWER of math.fsum -- and what each planted case was planted for, said of the restatement alone.  The same file as a program
reads the cases under -fsanitize=address,undefined."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import halo_cases as hc
import multipole_cases as mc
import np_halo as nph
import np_matter as npm
import np_multipoles as npl
import np_power as npp
from test_halo_cpu import Info, WINDOWS, window_of

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "cpu_emul", "multipole_emul.cpp")
SO = os.path.join(HERE, "cpu_emul", "libmultipole_emul.so")
EXE = os.path.join(HERE, "cpu_emul", "multipole_emul_san")
HDRS = [os.path.join(ROOT, "pinocchio_amd", "csrc", h) for h in ("pf_halo_core.h", "pf_power_core.h", "pf_matter_core.h", "pf_multipole_core.h")] + \
       [os.path.join(ROOT, "include", "pinfmax.h")]
TOL_POWER = 1e-14        # the fixed-point shell sums against math.fsum (tests/test_gpu_power.py)


def _stale(product):
    return not os.path.exists(product) or any(os.path.getmtime(product) < os.path.getmtime(s) for s in [SRC] + HDRS)


def build_emul():
    if _stale(SO):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DMULTIPOLE_EMUL_LIB", "-o", SO, SRC])
    L = C.CDLL(SO)
    vp = C.c_void_p
    L.multipole_emul_positions.argtypes = [C.c_int, C.c_size_t, vp, vp, C.c_double, C.c_double, C.c_int, vp, vp]
    L.multipole_emul_deposit.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, vp, vp, C.c_double, C.c_double, C.c_int, vp, C.c_int, C.c_int, vp, C.POINTER(Info)]
    L.multipole_emul_weights.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    L.multipole_emul_shells.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    return L


@pytest.fixture(scope="module")
def emul():
    return build_emul()


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def emul_deposit(L, n, case, lo, hi, ngp, x0=0, nxl=None, mass_weight=False):
    nxl = n - x0 if nxl is None else nxl
    grid = np.full(nxl * n * n + 1, 0x5A5A5A, np.uint64)
    info = Info()
    flags = (1 if ngp else 0) | (4 if mass_weight else 0)
    rc = L.multipole_emul_deposit(n, x0, nxl, flags, len(case["mass"]), _vp(case["pos"]), _vp(case["vel"]), case["scale"], case["vfac"], case["los"], _vp(case["mass"]), lo, hi,
                                  _vp(grid), C.byref(info))
    assert rc in (0, 3) and grid[-1] == 0x5A5A5A
    got = {k: int(getattr(info, k)) for k in nph.INT_KEYS}
    return (None, got) if rc == 3 else (grid[:-1].reshape(nxl, n, n), got)


@pytest.mark.parametrize("n", [16, 24])
def test_moved_positions_bit_for_bit_and_what_the_cases_were_planted_for(emul, n):
    for los in range(3):
        for case in mc.velocity_cases(n, los):
            name = (case["name"], n, los)
            count = len(case["mass"])
            want = nph.positions(npl.moved(case["pos"], case["vel"], case["vfac"], los), case["scale"], n)
            out, cls = np.full((count + 1, 3), 123.5), np.full(count + 1, 77, np.int32)
            assert emul.multipole_emul_positions(n, count, _vp(case["pos"]), _vp(case["vel"]), case["scale"], case["vfac"], los, _vp(out), _vp(cls)) == 0
            assert np.all(out[-1] == 123.5) and cls[-1] == 77
            assert np.array_equal(out[:-1].view(np.uint64), want.view(np.uint64)), name
            assert np.array_equal(cls[:-1], nph.classes(want, n)), name
            # said of the restatement alone
            if case["p_los"] is not None:
                assert np.array_equal(want[:, los], np.array(case["p_los"]), equal_nan=True), (name, want[:, los])
                for j, x in zip([j for j in range(3) if j != los], (3.5, 7.25)):
                    assert np.all(want[:, j] == x), name
            c = nph.classes(want, n)
            assert (int((c == 0).sum()), int((c == 1).sum()), int((c == 2).sum())) == case["counts"], name
            # without velocities the same list is the real-space one
            real = np.full((count, 3), 123.5)
            assert emul.multipole_emul_positions(n, count, _vp(case["pos"]), None, case["scale"], 5.0, los, _vp(real), _vp(cls)) == 0
            assert np.array_equal(real.view(np.uint64), nph.positions(case["pos"], case["scale"], n).view(np.uint64)), name
        rnd = next(c for c in mc.velocity_cases(n, los) if c["name"] == "random_777")
        s = npl.moved(rnd["pos"], rnd["vel"], rnd["vfac"], los)
        assert np.all(s[:, [j for j in range(3) if j != los]] == rnd["pos"][:, [j for j in range(3) if j != los]])
        shift = (s[:, los] - rnd["pos"][:, los]) * rnd["scale"]
        assert 1.0 < np.std(shift) < 2.0 and np.any(s[:, los] * rnd["scale"] >= n) and np.any(s[:, los] < 0)      # cells; both edges are crossed


@pytest.mark.parametrize("n", [16, 24])
def test_deposits_integer_for_integer(emul, n):
    for los in range(3):
        for case in mc.velocity_cases(n, los):
            for ngp in (False, True):
                for mw in (False, True):
                    whole = npl.deposit(n, case["pos"], case["vel"], case["mass"], 1, 2 ** 31 - 1, case["scale"], case["vfac"], los, mw, ngp)
                    assert (whole[1]["selected"], whole[1]["nonfinite"], whole[1]["outside"]) == case["counts"]
                    for x0, nxl in WINDOWS(n):
                        g, info = emul_deposit(emul, n, case, 1, 2 ** 31 - 1, ngp, x0, nxl, mw)
                        w, wi = window_of(whole, n, x0, nxl)
                        assert np.array_equal(g, w) and info == wi, (case["name"], n, los, ngp, mw, x0, nxl)
    # no velocities: the planted lists of the halo call give the halo call's grids
    for case in hc.cases(n):
        lo, hi = case["ranges"][0]
        want = nph.deposit(n, case["pos"], case["mass"], lo, hi, case["scale"], case["mass_weight"], False)
        got = emul_deposit(emul, n, dict(case, vel=None, vfac=0.0, los=1), lo, hi, False, mass_weight=case["mass_weight"])
        if want[0] is None:
            assert got[0] is None
            continue
        assert np.array_equal(got[0], want[0]) and got[1] == want[1], case["name"]


@pytest.mark.parametrize("n", [16, 24])
def test_the_weights_of_every_mode_bit_for_bit(emul, n):
    nzh = n // 2 + 1
    for los in range(3):
        for y0, nyl in ((0, n), (n // 2, n // 2), (3, 5)):
            L2, L4 = np.full(nyl * n * nzh + 1, 123.5), np.full(nyl * n * nzh + 1, 123.5)
            assert emul.multipole_emul_weights(n, los, y0, nyl, _vp(L2), _vp(L4)) == 0 and L2[-1] == L4[-1] == 123.5
            w2, w4, (a, k2) = npl.legendre(n, los, y0, nyl)
            assert np.array_equal(L2[:-1].view(np.uint64), w2.ravel().view(np.uint64)), (n, los, y0)
            assert np.array_equal(L4[:-1].view(np.uint64), w4.ravel().view(np.uint64)), (n, los, y0)
        # said of the restatement alone: the closed forms at mu = 1 and mu = 0, the range, the polynomial in float
        w2, w4, (a, k2) = npl.legendre(n, los)
        on, across = (a == k2) & (k2 > 0), (a == 0) & (k2 > 0)
        assert np.all(w2[on] == 1.0) and np.all(w4[on] == 1.0) and np.all(w2[across] == -0.5) and np.all(w4[across] == 0.375)
        assert w2[0, 0, 0] == 0.0 == w4[0, 0, 0] and np.all((w2 >= -0.5) & (w2 <= 1.0)) and np.all((w4 >= -3.0 / 7.0 - 1e-15) & (w4 <= 1.0))
        mu2 = np.where(k2 > 0, a / np.maximum(k2, 1), 0.0)
        nz = k2 > 0
        assert np.max(np.abs(w2 - 0.5 * (3 * mu2 - 1))[nz]) < 1e-15 and np.max(np.abs(w4 - 0.125 * (35 * mu2 * mu2 - 30 * mu2 + 3))[nz]) < 2e-15
    ax, ay, az = (npl.legendre(n, los)[2][0] for los in range(3))
    k2 = npp.geometry(n)[0]
    assert np.array_equal(ax + ay + az, k2) and ax[5, 3, 2] == 9 and ay[5, 3, 2] == 25 and az[5, 3, 2] == 4 and ax[0, n - 1, 0] == 1      # [ky][kx][kz]


@pytest.mark.parametrize("n", [16, 24])
def test_the_eleven_sums_of_a_shell(emul, n):
    """the emulation's fixed point (the library's) against math.fsum over the same terms: integers equal, every part within TOL_POWER"""
    nb = npp.bins(n)
    a, b = mc.random_spectra(n, 3 + n)
    a[3, 2, 1] = np.nan                      # a mode that is not finite: counted, and in no sum
    for los in range(3):
        for y0, nyl, lin in ((0, n, b), (n // 2, n // 2, b), (0, n, None)):
            sa = np.ascontiguousarray(a[y0:y0 + nyl])
            sb = None if lin is None else np.ascontiguousarray(lin[y0:y0 + nyl])
            nm, ks, nonfin = np.zeros(nb + 1, np.uint64), np.zeros(nb + 1, np.uint64), np.zeros(1, np.uint64)
            parts = np.full(11 * nb + 1, 123.5)
            assert emul.multipole_emul_shells(n, los, y0, nyl, _vp(sa.view(np.float64)), None if sb is None else _vp(sb.view(np.float64)), _vp(nm), _vp(ks), _vp(parts), _vp(nonfin)) == 0
            assert parts[-1] == 123.5
            want = npl.shells(sa, sb, y0, 8, False, False, los)
            assert np.array_equal(nm[:-1], want["nmodes"]) and np.array_equal(ks[:-1], want["k2sum"]) and int(nonfin[0]) == want["nonfinite_modes"] == (2 if y0 == 0 else 0)
            got = parts[:-1].reshape(11, nb)
            assert npp.rel(got, want["parts"]) <= TOL_POWER, (n, los, y0, npp.rel(got, want["parts"]))
            if lin is None:
                assert not np.any(got[5:]) and not np.any(want["parts"][5:])
            assert np.all(np.count_nonzero(want["parts"][:5 if lin is None else 11], axis=1) > nb // 2)        # every sum has terms in most shells
            # l = 0 is the sum of the matter call
            m = npm.shells(sa, sb, y0)
            assert np.array_equal(want["power"][0], m["power"])
            assert lin is None or (np.array_equal(want["parts"][5], m["cross_pos"]) and np.array_equal(want["parts"][6], m["cross_neg"]))


def test_program_under_sanitizers(emul, tmp_path):
    """the stand-alone build of the same file on the planted lists, with arrays of exactly the sizes: clean under the sanitizers, and
    the numbers those of the library build"""
    if _stale(EXE):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-o", EXE, SRC])
    n = 16
    runs = [(case, ngp, x0, nxl, vel) for los in range(3) for case in mc.velocity_cases(n, los) for ngp in (False, True) for x0, nxl in ((0, n), (n - 1, 1))
            for vel in (True, False)]
    path = tmp_path / "cases.bin"
    with open(path, "wb") as fh:
        for case, ngp, x0, nxl, vel in runs:
            np.array([n, x0, nxl, 1 if ngp else 0, len(case["mass"]), 1, 2 ** 31 - 1, case["los"], 1 if vel else 0], dtype=np.int64).tofile(fh)
            np.array([case["scale"], case["vfac"] if vel else 0.0], dtype=np.float64).tofile(fh)
            case["pos"].tofile(fh)
            if vel:
                case["vel"].tofile(fh)
            case["mass"].tofile(fh)
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True)
    print(out.stdout[-3000:], out.stderr[-3000:])
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and len(lines) == len(runs) and "ERROR" not in out.stderr
    for k, (case, ngp, x0, nxl, vel) in enumerate(runs):
        c = case if vel else dict(case, vel=None, vfac=0.0)
        g, info = emul_deposit(emul, n, c, 1, 2 ** 31 - 1, ngp, x0, nxl)
        got = dict(zip(lines[k].split()[2::2], lines[k].split()[3::2]))
        assert int(got["rc"]) == 0 and g is not None, k
        keys = ("selected", "weight_sum", "nonfinite", "outside", "empty", "max")
        assert [int(got[key]) for key in keys] == [info[{"empty": "empty_cells", "max": "max_cell"}.get(key, key)] for key in keys], k
        h = 1469598103934665603
        for x in g.ravel().tolist():
            h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        assert int(got["hash"]) == h, k
        assert float.fromhex(got["lsum"]) != 0.0 and float.fromhex(got["psum"]) > 0.0, k
