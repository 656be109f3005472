"""The separation-space pass of the halo correlation function without a device: the arithmetic of the device path
(pinocchio_amd/csrc/pf_corr_core.h, compiled for the host in tests/cpu_emul/corr_emul.cpp) against the numpy restatement
(tests/np_corr.py): shell, Legendre weights and sum index of every cell bit for bit, the counts of the lattice of separations
against those of the Hermitian-weighted half-spectrum (tests/np_power.py), the six positive sums of a shell within the fixed point's
TOL_POWER of math.fsum, the element of the form pass -- and what each planted field was planted for, said of the restatement alone.
The same file as a program runs under -fsanitize=address,undefined."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import corr_cases as cc
import np_corr as npc
import np_power as npp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "cpu_emul", "corr_emul.cpp")
SO = os.path.join(HERE, "cpu_emul", "libcorr_emul.so")
EXE = os.path.join(HERE, "cpu_emul", "corr_emul_san")
HDRS = [os.path.join(ROOT, "pinocchio_amd", "csrc", h) for h in ("pf_power_core.h", "pf_matter_core.h", "pf_multipole_core.h", "pf_corr_core.h")] + \
       [os.path.join(ROOT, "include", "pinfmax.h")]
TOL_POWER = 1e-14        # the fixed-point shell sums against math.fsum (tests/test_gpu_power.py)


def _stale(product):
    return not os.path.exists(product) or any(os.path.getmtime(product) < os.path.getmtime(s) for s in [SRC] + HDRS)


def build_emul():
    if _stale(SO):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DCORR_EMUL_LIB", "-o", SO, SRC])
    L = C.CDLL(SO)
    vp = C.c_void_p
    L.corr_emul_cells.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    L.corr_emul_index.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    L.corr_emul_shells.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.corr_emul_form.argtypes = [C.c_size_t, vp, vp, C.c_double, vp, vp]
    return L


@pytest.fixture(scope="module")
def emul():
    return build_emul()


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def emul_shells(L, real, los, x0=0):
    nxl, n = real.shape[:2]
    nb = npp.bins(n)
    nc, r2, bad = np.zeros(nb + 1, np.uint64), np.zeros(nb + 1, np.uint64), np.zeros(1, np.uint64)
    parts = np.full(6 * nb + 1, 123.5)
    real = np.ascontiguousarray(real)
    assert L.corr_emul_shells(n, los, x0, nxl, _vp(real), _vp(nc), _vp(r2), _vp(parts), _vp(bad)) == 0 and parts[-1] == 123.5
    return {"ncells": nc[:-1], "r2sum": r2[:-1], "parts": parts[:-1].reshape(6, nb), "nonfinite_cells": int(bad[0])}


@pytest.mark.parametrize("n", [16, 24])
def test_shell_and_weights_of_every_cell_bit_for_bit(emul, n):
    for los in range(3):
        for x0, nxl in ((0, n), (n // 2, n // 2), (3, 5)):
            nc = nxl * n * n
            r2, sh = np.full(nc + 1, 77, np.uint64), np.full(nc + 1, 77, np.int32)
            L2, L4 = np.full(nc + 1, 123.5), np.full(nc + 1, 123.5)
            assert emul.corr_emul_cells(n, los, x0, nxl, _vp(r2), _vp(sh), _vp(L2), _vp(L4)) == 0
            assert r2[-1] == 77 and sh[-1] == 77 and L2[-1] == L4[-1] == 123.5
            wr2, wsh, w2, w4, _ = npc.geometry(n, los, x0, nxl)
            assert np.array_equal(r2[:-1], wr2.ravel().astype(np.uint64)) and np.array_equal(sh[:-1], wsh.ravel().astype(np.int32)), (n, los, x0)
            assert np.array_equal(L2[:-1].view(np.uint64), w2.ravel().view(np.uint64)) and np.array_equal(L4[:-1].view(np.uint64), w4.ravel().view(np.uint64)), (n, los, x0)
        # said of the restatement alone: n/2 stays positive, the closed forms at mu = 1 and mu = 0, the origin
        r2, sh, w2, w4, a = npc.geometry(n, los)
        assert r2[n // 2, 0, 0] == (n // 2) ** 2 and r2[n - 1, 1, n - 1] == 3 and sh[0, 0, 0] == 0 and sh.max() == npp.bins(n) - 1
        on, across = (a == r2) & (r2 > 0), (a == 0) & (r2 > 0)
        assert np.all(w2[on] == 1.0) and np.all(w4[on] == 1.0) and np.all(w2[across] == -0.5) and np.all(w4[across] == 0.375)
        assert w2[0, 0, 0] == 0.0 == w4[0, 0, 0]
        idx = [0, 0, 0]
        idx[los] = n - 2
        assert a[tuple(idx)] == 4 and a[tuple(np.roll(idx, 1))] == 0


@pytest.mark.parametrize("n", [16, 24])
def test_the_lattice_of_separations_counts_like_the_half_spectrum(emul, n):
    want = npp.power(np.zeros((n, n, n // 2 + 1), np.complex128))
    for los in (0, 2):
        got = emul_shells(emul, np.zeros((n, n, n)), los)
        assert np.array_equal(got["ncells"], want["nmodes"]) and np.array_equal(got["r2sum"], want["k2sum"])
        assert int(got["ncells"].sum()) == n ** 3 and not np.any(got["parts"])
        rest = npc.shells(np.zeros((n, n, n)), 0, 8, los)
        assert np.array_equal(rest["ncells"], want["nmodes"]) and np.array_equal(rest["r2sum"], want["k2sum"])
    # windows of planes add up to the box, in integers
    for wins in cc.x_windows(n):
        parts = [emul_shells(emul, np.zeros((nxl, n, n)), 1, x0) for x0, nxl in wins]
        assert np.array_equal(np.sum([p["ncells"] for p in parts], axis=0, dtype=np.uint64), want["nmodes"])
        assert np.array_equal(np.sum([p["r2sum"] for p in parts], axis=0, dtype=np.uint64), want["k2sum"])


@pytest.mark.parametrize("n", [16, 24])
def test_the_sum_index_of_every_term(emul, n):
    f = cc.random_field(n, 11 + n)
    f[1, 2, 3] = np.nan
    f[0, 0, 0] = -2.0                      # the origin: l = 0 alone, in the negative sum
    for los in range(3):
        for x0, nxl in ((0, n), (3, 5)):
            part = np.ascontiguousarray(f[x0:x0 + nxl])
            idx = np.full(3 * part.size + 1, 99, np.int32)
            assert emul.corr_emul_index(n, los, x0, nxl, _vp(part), _vp(idx)) == 0 and idx[-1] == 99
            want = npc.sum_index(part, los, x0)
            assert np.array_equal(idx[:-1].reshape(want.shape), want), (n, los, x0)
        want = npc.sum_index(f, los)
        assert list(want[:, 0, 0, 0]) == [1, -1, -1] and list(want[:, 1, 2, 3]) == [-1, -1, -1]
        assert set(np.unique(want[0])) == {-1, 0, 1} and set(np.unique(want[1])) == {-1, 2, 3} and set(np.unique(want[2])) == {-1, 4, 5}


@pytest.mark.parametrize("n", [16, 24])
def test_the_six_sums_of_a_shell(emul, n):
    """the emulation's fixed point (the library's) against math.fsum over the same terms: integers equal, every part within TOL_POWER"""
    f = cc.random_field(n, 5 + n)
    f[3, 2, 1] = np.inf                    # a cell that is not finite: counted, and in no sum
    for los in range(3):
        for wins in cc.x_windows(n):
            got = [emul_shells(emul, f[x0:x0 + nxl], los, x0) for x0, nxl in wins]
            want = [npc.shells(f[x0:x0 + nxl], x0, 8, los) for x0, nxl in wins]
            for g, w in zip(got, want):
                assert np.array_equal(g["ncells"], w["ncells"]) and np.array_equal(g["r2sum"], w["r2sum"]) and g["nonfinite_cells"] == w["nonfinite_cells"]
                assert npp.rel(g["parts"], w["parts"]) <= TOL_POWER, (n, los, npp.rel(g["parts"], w["parts"]))
            assert sum(g["nonfinite_cells"] for g in got) == 1
        whole = npc.shells(f, 0, 8, los)
        assert np.all(np.count_nonzero(whole["parts"], axis=1) > npp.bins(n) // 2)        # every sum has terms in most shells
        assert np.array_equal(whole["parts"][:2], npc.shells(f, 0, 8, (los + 1) % 3)["parts"][:2])   # l = 0 knows no line of sight
    # what the planted fields were planted for
    for los in range(3):
        d = 3
        on, across = emul_shells(emul, cc.on_los(n, los, d), los), emul_shells(emul, cc.across_los(n, los, n - d), los)
        for got, want in ((on, [3.0, 0.0, 3.0, 0.0, 3.0, 0.0]), (across, [3.0, 0.0, 0.0, 1.5, 1.125, 0.0])):
            assert list(got["parts"][:, d]) == want and np.count_nonzero(got["parts"]) == 3
        neg = emul_shells(emul, cc.across_los(n, los, d, -4.0), los)
        assert list(neg["parts"][:, d]) == [0.0, 4.0, 2.0, 0.0, 0.0, 1.5]


def test_the_element_of_the_form_pass(emul):
    t = np.array([12.0, 0.0, -3.0, np.inf, np.nan, 5.0, np.inf, 1e-320])
    k2 = np.array([1, 4, 7, 2, 3, 0, 0, 9], np.uint32)
    out, bad = np.full(len(t) + 1, 123.5), np.full(len(t) + 1, 9, np.int32)
    n3 = float(24 ** 3)
    assert emul.corr_emul_form(len(t), _vp(t), _vp(k2), n3, _vp(out), _vp(bad)) == 0 and out[-1] == 123.5 and bad[-1] == 9
    with np.errstate(invalid="ignore"):
        want = np.where(np.isfinite(t) & (k2 > 0), np.where(np.isfinite(t), t, 0.0) / n3, 0.0)
    assert np.array_equal(out[:-1].view(np.uint64), want.view(np.uint64)) and list(bad[:-1]) == [0, 0, 0, 1, 1, 0, 1, 0]
    # the restatement on a slab: the same elements, zero at k = 0, the weight of what is not finite
    n = 16
    a, b = cc.planted_spectra(n)
    a[2, 3, 4] = np.inf + 0j
    for which in (0, 1):
        q, nonfin = npc.form(a, b, 0, 8, False, False, which)
        assert q[0, 0, 0] == 0.0 and q[2, 3, 4] == 0.0 and nonfin == 2
        assert q[0, 0, n // 2] == ((3.0 + 1) ** 2 + 16.0 if which == 0 else -((3.0 + 1) * 1.0 - 4.0 * 0.5)) / n ** 3
        assert np.count_nonzero(q) == 5


def test_program_under_sanitizers(emul):
    """the stand-alone build of the same file with arrays of exactly the sizes: clean under the sanitizers, and its numbers those of
    the library build on the same field"""
    if _stale(EXE):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-o", EXE, SRC])
    for n, los, x0, nxl, seed in ((16, 0, 0, 16, 1), (16, 2, 15, 1, 2), (24, 1, 3, 5, 3)):
        out = subprocess.run([EXE, str(n), str(los), str(x0), str(nxl), str(seed)], capture_output=True, text=True)
        print(out.stdout[-2000:], out.stderr[-2000:])
        assert out.returncode == 0 and "ERROR" not in out.stderr
        got = dict(zip(out.stdout.split()[0::2], out.stdout.split()[1::2]))
        assert int(got["cells"]) == nxl * n * n and int(got["nonfinite"]) == 1
        assert float.fromhex(got["psum"]) > 0.0 and float.fromhex(got["lsum"]) != 0.0
