"""The slab form of the matter-density call without a device: the plan arithmetic of pinocchio_amd/csrc/pf_matter_slabs_core.h,
compiled for the host in tests/cpu_emul/matter_slabs_emul.cpp, against the brute-force restatement (tests/np_matter_slabs.py) --
windows, block lists and B exhaustively on small grids, the reach of planted slabs --, and P emulated ranks (reach, windowed deposit,
pack, exchange, fold) against the one-rank restatement of the whole box (tests/np_matter.py), integer for integer.  The same file as
a program runs the cases under -fsanitize=address,undefined."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import matter_cases as mc
import np_matter as npm
import np_matter_slabs as nps

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "cpu_emul", "matter_slabs_emul.cpp")
SO = os.path.join(HERE, "cpu_emul", "libmatter_slabs_emul.so")
EXE = os.path.join(HERE, "cpu_emul", "matter_slabs_emul_san")
HDRS = [os.path.join(ROOT, "pinocchio_amd", "csrc", h) for h in ("pf_matter_slabs_core.h", "pf_matter_core.h", "pf_power_core.h")] + [os.path.join(ROOT, "include", "pinfmax.h")]
INT_KEYS = ("deposited", "nonfinite", "outside", "empty_cells", "max_cell", "sum_hi32", "sum_lo32")
BOXES = [(8, 2), (8, 4), (8, 8), (12, 3)]


class Info(C.Structure):
    _fields_ = [(k, C.c_ulonglong) for k in ("deposited", "nonfinite", "outside", "empty_cells", "max_cell", "sum_hi32", "sum_lo32", "modes", "nonfinite_modes")]


def _stale(product):
    return not os.path.exists(product) or any(os.path.getmtime(product) < os.path.getmtime(s) for s in [SRC] + HDRS)


@pytest.fixture(scope="module")
def emul():
    if _stale(SO):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DMATTER_SLABS_EMUL_LIB", "-o", SO, SRC])
    L = C.CDLL(SO)
    vp = C.c_void_p
    L.slabs_emul_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.slabs_emul_reach.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp]
    L.slabs_emul_box.argtypes = [C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, C.POINTER(Info), vp]
    return L


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def emul_plan(L, n, P, hlo, hhi):
    nxl = n // P
    out = np.full(2 + 2 * P + P * P * (1 + nxl) + 1, -77, np.int32)
    assert L.slabs_emul_plan(n, P, hlo, hhi, _vp(out)) == 0 and out[-1] == -77
    win = [(int(out[2 + 2 * r]), int(out[3 + 2 * r])) for r in range(P)]
    rest = out[2 + 2 * P:-1].reshape(P, P, 1 + nxl)
    lists = [[rest[r, q, 1:1 + rest[r, q, 0]].tolist() for q in range(P)] for r in range(P)]
    assert all(np.all(rest[r, q, 1 + rest[r, q, 0]:] == -1) for r in range(P) for q in range(P))
    return int(out[0]), int(out[1]), win, lists


def emul_reach(L, slab, x0, weight=None, ngp=False):
    nxl, n = slab.shape[1], slab.shape[2]
    out = np.array([-7, -7, -77], np.int32)
    w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
    assert L.slabs_emul_reach(slab.dtype.itemsize, n, nxl, x0, _vp(np.ascontiguousarray(slab)), 1 if ngp else 0, _vp(w), _vp(out)) == 0 and out[2] == -77
    return int(out[0]), int(out[1])


def emul_box(L, vel12, P, weight=None, ngp=False):
    n = vel12.shape[1]
    grid = np.zeros(n ** 3 + 1, np.uint64)
    grid[-1] = 0xABCDEF
    exch = np.zeros(7, np.uint64)
    exch[-1] = 0xABCDEF
    w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
    info = Info()
    rc = L.slabs_emul_box(vel12.dtype.itemsize, n, P, _vp(np.ascontiguousarray(vel12)), 1 if ngp else 0, _vp(w), _vp(grid), C.byref(info), _vp(exch))
    assert rc == 0 and grid[-1] == 0xABCDEF == exch[-1], rc
    return grid[:-1].reshape(n, n, n), {k: int(getattr(info, k)) for k in INT_KEYS}, dict(zip(nps.EXCHANGE_KEYS, (int(x) for x in exch[:6])))


@pytest.mark.parametrize("n", [8, 12, 16])
def test_the_plan_exhaustively(emul, n):
    """every P dividing n, every Hlo, Hhi in 0 .. n: windows, lists and B against the brute-force statement; every window plane that is
    not the rank's own has exactly one (peer, slot); the lists a sender packs by are the lists a receiver folds by (one function of
    (r, q) on every rank: held here as equality with the brute-force lists); the whole box exactly when nxl + Hlo + Hhi >= n"""
    for P in [p for p in range(1, n + 1) if n % p == 0]:
        nxl = n // P
        for hlo in range(n + 1):
            for hhi in range(n + 1):
                form, B, win, lists = emul_plan(emul, n, P, hlo, hhi)
                wantL, wantB = nps.block_lists(n, P, hlo, hhi)
                whole = nxl + hlo + hhi >= n
                assert lists == wantL and B == wantB == max([len(l) for row in lists for l in row] + [0]), (P, hlo, hhi)
                assert form == nps.exchange(n, P, hlo, hhi)["form"] and (form == 2) == (whole and P > 1 and hlo + hhi > 0), (P, hlo, hhi)
                for r in range(P):
                    w0, wn = win[r]
                    planes = [(w0 + k) % n for k in range(wn)]
                    assert planes == nps.window(n, P, r, hlo, hhi) and ((w0, wn) == (0, n)) == whole, (P, r, hlo, hhi)
                    assert len(set(planes)) == wn <= n and all((r * nxl + l) in planes for l in range(nxl))
                    ghosts = [g for g in planes if g // nxl != r]
                    sent = [q * nxl + l for q in range(P) for l in lists[r][q]]
                    assert sorted(sent) == sorted(ghosts) and len(set(sent)) == len(sent) and not lists[r][r], (P, r, hlo, hhi)
                    assert all(l == sorted(l) and len(l) <= B for l in lists[r])


def planted(n, P, dt):
    return nps.shift_cases(n, P, dt)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_reach_of_planted_slabs(emul, dt):
    for n, P in [(16, 1), (16, 4), (8, 8), (12, 3)]:
        nxl = n // P
        todo = planted(n, P, dt) + [(c[0], c[1], c[2], c[3], None) for c in mc.cases(n, dt)]
        for name, v, w, ngp, expect in todo:
            per_rank = []
            for r in range(P):
                slab = v[:, r * nxl:(r + 1) * nxl]
                got = emul_reach(emul, slab, r * nxl, w, ngp)
                assert got == nps.reach(slab, r * nxl, w, ngp), (name, n, P, r)
                per_rank.append(got)
            common = (max(a for a, _ in per_rank), max(b for _, b in per_rank))
            assert common == nps.box_reach(v, P, w, ngp)
            if expect is not None:
                assert common == expect, (name, n, P, common)


@pytest.fixture(scope="module")
def wanted():
    """the one-rank restatement of every planted box, computed once: (n, P, dtype name, case name) -> (grid, info)"""
    out = {}
    for n, P in BOXES:
        for dt in (np.float32, np.float64):
            for name, v, w, ngp, _ in planted(n, P, dt):
                out[n, P, np.dtype(dt).name, name] = npm.deposit(v, w, ngp)
    return out


@pytest.mark.parametrize("n,P", BOXES)
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_emulated_ranks_give_the_grid_of_one_rank(emul, wanted, n, P, dt):
    forms = set()
    for name, v, w, ngp, expect in planted(n, P, dt):
        grid, info, exch = emul_box(emul, v, P, w, ngp)
        g1, i1 = wanted[n, P, np.dtype(dt).name, name]
        assert grid.dtype == np.uint64 and np.array_equal(grid, g1), (name, n, P)
        assert info == i1, (name, info, i1)
        hlo, hhi = nps.box_reach(v, P, w, ngp)
        assert exch == nps.exchange(n, P, hlo, hhi), (name, exch)
        if expect is not None:
            assert (exch["reach_below"], exch["reach_above"]) == expect, name
        if name.startswith("zero"):
            assert exch["form"] == 0 and exch["bytes_per_peer"] == 0
        forms.add(exch["form"])
    assert forms == {0, 1, 2}, forms       # the planted boxes reach every form
    g, i, e = emul_box(emul, planted(n, P, dt)[4][1], 1)        # one rank: no exchange, the same grid
    assert e["form"] == 0 and e["window_planes"] == n and e["block_planes"] == 0 and np.array_equal(g, wanted[n, P, np.dtype(dt).name, "normal_1p5"][0])


def test_program_under_sanitizers(emul, tmp_path):
    """the stand-alone build of the same file on the planted boxes, with arrays of exactly the sizes: clean under the sanitizers, and
    the numbers those of the library build"""
    if _stale(EXE):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-o", EXE, SRC])
    todo = [(v, w, ngp, P) for n, P in BOXES for dt in (np.float32, np.float64) for _, v, w, ngp, _ in planted(n, P, dt)]
    path = tmp_path / "cases.bin"
    with open(path, "wb") as fh:
        for v, w, ngp, P in todo:
            np.array([v.dtype.itemsize, v.shape[1], P, 1 if ngp else 0, 0 if w is None else 1], dtype=np.int64).tofile(fh)
            np.array(w if w is not None else (0, 0, 0, 0), dtype=np.float64).tofile(fh)
            np.ascontiguousarray(v).tofile(fh)
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True)
    print(out.stdout[-3000:], out.stderr[-3000:])
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and len(lines) == len(todo) and "ERROR" not in out.stderr
    for k, (v, w, ngp, P) in enumerate(todo):
        g, info, exch = emul_box(emul, v, P, w, ngp)
        got = dict(zip(lines[k].split()[2::2], lines[k].split()[3::2]))
        h = 1469598103934665603
        for x in g.ravel().tolist():
            h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        assert [int(got[key]) for key in ("deposited", "nonfinite", "outside", "empty", "max", "hi", "lo", "hash")] == [info[key] for key in INT_KEYS] + [h], k
        assert [int(got[key]) for key in ("form", "below", "above", "window", "block", "bytes")] == [exch[key] for key in nps.EXCHANGE_KEYS], k
