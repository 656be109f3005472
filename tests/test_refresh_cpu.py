"""The velocity refresh without a device: the numpy restatement (tests/np_refresh.py) gives hand-written answers, and the cell
arithmetic and compaction of the device path (pinocchio_amd/csrc/pf_refresh_core.h, compiled for the host in
tests/cpu_emul/refresh_emul.cpp) agree with it particle by particle.  The same file as a program runs under
-fsanitize=address,undefined against a C port of the reference's loop (src/distribute.c:806-830 without the good_particle test)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import np_refresh as npr

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emul", "refresh_emul.cpp")
SO = os.path.join(HERE, "cpu_emul", "librefresh_emul.so")
EXE = os.path.join(HERE, "cpu_emul", "refresh_emul_san")
LARGE = os.path.join(HERE, "cpu_emul", "large_boxes.h")      # the boxes the mains of the programs share
HDRS = [os.path.join(HERE, "..", "pinocchio_amd", "csrc", h) for h in ("pf_refresh_core.h", "pf_back_core.h", "pf_neigh_core.h", "pf_distribute_boxes.h")]

# (n, start, len, safe): the boxes of tests/test_gpu_refresh.py -- the whole periodic box; wraps in x and z with y periodic; two
# x-ranges of which a slab meets one; the mixed-radix grid -- and two small ones, one with a start beyond the box (reduced to it)
BOXES = [(16, (0, 0, 0), (16, 16, 16), (0, 0, 0)),
         (16, (-3, 0, 13), (7, 16, 5), (1, 0, 1)),
         (16, (14, 0, 2), (9, 16, 5), (2, 0, 2)),
         (24, (20, 3, 0), (9, 5, 24), (2, 1, 0)),
         (8, (6, 2, 5), (4, 3, 5), (1, 1, 2)),
         (8, (-15, 9, 0), (8, 4, 3), (0, 1, 1))]


def _slabs(n):
    """the whole box, its halves and an odd cut"""
    return [(0, n), (0, n // 2), (n // 2, n // 2), (n // 4, 3)]


def _cols(n, nxl, dtype=np.float32):
    """cols24[c][cell] = c 2^20 + cell: the value names its column and its cell (exactly in columns 0 .. 15 of floats)"""
    nc = nxl * n * n
    return (np.arange(24, dtype=np.int64)[:, None] * 2 ** 20 + np.arange(nc, dtype=np.int64)[None, :]).astype(dtype)


# ------------------------------------------------------------------------------------------------------------------------
# hand-written answers
def test_a_box_of_4_3_5_in_a_box_of_8():
    n, start, length = 8, (6, 2, 5), (4, 3, 5)
    # positions k + 5 (j + 3 i): (0,0,0) (3,2,4) (1,1,3) (2,1,2) -> global (6,2,5) (1,4,1) (7,3,0) (0,3,7): x and z wrap
    pos = np.array([0, 59, 23, 37], dtype=np.uint32)
    assert [tuple(int(v[q]) for v in npr.coords(pos, length)) for q in range(4)] == [(0, 0, 0), (3, 2, 4), (1, 1, 3), (2, 1, 2)]
    found, fftpos = npr.cells(n, 0, 8, start, length, pos)
    assert found.all() and fftpos.tolist() == [5 + 8 * (2 + 8 * 6), 1 + 8 * (4 + 8 * 1), 0 + 8 * (3 + 8 * 7), 7 + 8 * (3 + 8 * 0)] == [405, 97, 472, 31]
    cols = _cols(n, 8)
    index, vel = npr.gather(n, 0, 8, start, length, pos, cols)
    assert index.tolist() == [0, 1, 2, 3] and vel.shape == (4, 24) and vel.dtype == np.float32
    # the corner particle (0,0,0) lies in every safety layer: it is found all the same
    # (a float holds c 2^20 + cell exactly up to column 15; beyond, an odd cell rounds to its even neighbour -- the column still shows)
    assert vel[0, :16].tolist() == [c * 2 ** 20 + 405 for c in range(16)] and vel[0, 16:].tolist() == [c * 2 ** 20 + 404 for c in range(16, 24)]
    assert vel[3, 13] == 13 * 2 ** 20 + 31
    # planes 4 .. 7 hold particles 0 and 2, at local planes 2 and 3; planes 0 .. 3 the two others
    index, vel = npr.gather(n, 4, 4, start, length, pos, _cols(n, 4))
    assert index.tolist() == [0, 2] and vel[:, 0].tolist() == [5 + 8 * (2 + 8 * 2), 0 + 8 * (3 + 8 * 3)] == [149, 216]
    index, vel = npr.gather(n, 0, 4, start, length, pos, _cols(n, 4))
    assert index.tolist() == [1, 3] and vel[:, 15].tolist() == [15 * 2 ** 20 + 97, 15 * 2 ** 20 + 31] and vel[:, 23].tolist() == [23 * 2 ** 20 + 96, 23 * 2 ** 20 + 32]
    # planes 2 .. 5 hold none of them; a duplicate position is found twice
    assert len(npr.gather(n, 2, 4, start, length, pos, _cols(n, 4))[0]) == 0
    index, vel = npr.gather(n, 4, 4, start, length, np.array([23, 59, 23], dtype=np.uint32), _cols(n, 4))
    assert index.tolist() == [0, 2] and np.array_equal(vel[0], vel[1]) and vel[0, 1] == 2 ** 20 + 216


def test_the_scatter_into_records():
    # records of 40 bytes filled with 0xAB; Vel at byte 4, Vel_3LPT_1_prev at byte 24, nothing else named
    frag = np.full((3, 40), 0xAB, dtype=np.uint8)
    vel = (np.arange(48, dtype=np.float32) + 0.5).reshape(2, 24)
    out = npr.scatter(frag, np.array([2, 0]), vel, (4, -1, -1, -1), (-1, -1, 24, -1))
    assert np.all(frag == 0xAB) and np.all(out[1] == 0xAB)
    assert out[2, 4:16].copy().view(np.float32).tolist() == [0.5, 1.5, 2.5] and out[0, 4:16].copy().view(np.float32).tolist() == [24.5, 25.5, 26.5]
    # values 12 + 3 * 2 .. of a particle: the third prev field
    assert out[2, 24:36].copy().view(np.float32).tolist() == [18.5, 19.5, 20.5] and out[0, 24:36].copy().view(np.float32).tolist() == [42.5, 43.5, 44.5]
    rest = np.ones(40, dtype=bool)
    rest[4:16] = rest[24:36] = False
    assert np.all(out[:, rest] == 0xAB)
    # doubles: fields of 24 bytes
    vel8 = vel.astype(np.float64)
    out = npr.scatter(np.full((3, 64), 0xAB, dtype=np.uint8), np.array([1]), vel8[:1], (-1, 8, -1, -1), (-1, -1, -1, 32))
    assert out[1, 8:32].copy().view(np.float64).tolist() == [3.5, 4.5, 5.5] and out[1, 32:56].copy().view(np.float64).tolist() == [21.5, 22.5, 23.5]
    assert np.all(out[[0, 2]] == 0xAB) and np.all(out[1, :8] == 0xAB) and np.all(out[1, 56:] == 0xAB)


# ------------------------------------------------------------------------------------------------------------------------
# the host compilation of the device path's arithmetic
def _stale(out):
    return (not os.path.exists(out)) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in [SRC, LARGE] + HDRS)


@pytest.fixture(scope="module")
def emul():
    if _stale(SO):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DREFRESH_EMUL_LIB", "-o", SO, SRC])
    L = C.CDLL(SO)
    ip, up, bp, fp = C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(C.c_ubyte), C.POINTER(C.c_float)
    L.emul_cells.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip, ip, C.c_size_t, up, ip, ip, bp, C.POINTER(C.c_ulonglong)]
    L.emul_gather.restype = C.c_ulonglong
    L.emul_gather.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip, ip, C.c_size_t, up, ip, fp, C.c_size_t, up, fp]
    L.port_gather.restype = C.c_ulonglong
    L.port_gather.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip, C.c_size_t, up, fp, up, fp]
    return L


def _i3(v):
    return (C.c_int * 3)(*map(int, v))


@pytest.mark.parametrize("box", BOXES, ids=lambda b: "n%d-%s" % (b[0], "x".join(map(str, b[2]))))
def test_the_device_arithmetic_equals_the_restatement(emul, box):
    n, start, length, safe = box
    rng = np.random.default_rng(7 * sum(length) + n)
    ncells = length[0] * length[1] * length[2]
    every = np.arange(ncells, dtype=np.uint32)
    # 60 % of the positions in random order and a tenth of them once more; 700 particles are three blocks of 256 and a rest
    pos = rng.permutation(ncells)[:max(1, int(round(0.6 * ncells)))].astype(np.uint32)
    pos = np.concatenate([pos, rng.choice(pos, len(pos) // 10)])
    count = len(pos)
    orders = [None, rng.permutation(count).astype(np.int32), np.argsort(pos, kind="stable").astype(np.int32)]
    ip, up, bp, fp = C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(C.c_ubyte), C.POINTER(C.c_float)
    total = 0
    for x0, nxl in _slabs(n):
        # per cell of the sub-box
        coord = np.zeros((ncells, 3), dtype=np.int32)
        glob = np.zeros((ncells, 3), dtype=np.int32)
        found = np.zeros(ncells, dtype=np.uint8)
        addr = np.zeros(ncells, dtype=np.uint64)
        emul.emul_cells(n, x0, nxl, _i3(start), _i3(length), _i3(safe), ncells, every.ctypes.data_as(up), coord.ctypes.data_as(ip), glob.ctypes.data_as(ip),
                        found.ctypes.data_as(bp), addr.ctypes.data_as(C.POINTER(C.c_ulonglong)))
        i, j, k = npr.coords(every, length)
        assert np.array_equal(coord, np.stack([i, j, k], axis=1))
        for d, c in enumerate((i, j, k)):
            assert np.array_equal(glob[:, d], (c + start[d]) % n)
        wfound, wpos = npr.cells(n, x0, nxl, start, length, every)
        assert np.array_equal(found.astype(bool), wfound)
        assert np.array_equal(addr[wfound].astype(np.int64), wpos[wfound]) and not addr[~wfound].any()
        assert wpos[wfound].size == 0 or (wpos[wfound].min() >= 0 and wpos[wfound].max() < nxl * n * n)
        # the safety layers play no part: with safe = 0 .. 2 everywhere the same cells
        if (x0, nxl) == (0, n):
            assert wfound.all()
        # the gather, thread by thread
        cols = _cols(n, nxl)
        windex, wvel = npr.gather(n, x0, nxl, start, length, pos, cols)
        total += len(windex)
        for order in orders:
            for cap in (count, len(windex) // 2):
                index = np.full(cap + 1, 0xDEADBEEF, dtype=np.uint32)
                vel = np.full(24 * cap + 1, -7.0, dtype=np.float32)
                nfound = emul.emul_gather(n, x0, nxl, _i3(start), _i3(length), _i3(safe), count, pos.ctypes.data_as(up),
                                          order.ctypes.data_as(ip) if order is not None else None, cols.ctypes.data_as(fp), cap, index.ctypes.data_as(up),
                                          vel.ctypes.data_as(fp))
                m = min(len(windex), cap)
                assert nfound == len(windex)
                assert np.array_equal(index[:m], windex[:m]) and np.array_equal(vel[:24 * m].reshape(m, 24), wvel[:m])
                assert np.all(index[m:] == 0xDEADBEEF) and np.all(vel[24 * m:] == -7.0)
        if all(-n < s < n for s in start):   # the reference's stabl lies in (-n, n): its loop adds n once
            index = np.zeros(count, dtype=np.uint32)
            vel = np.zeros(24 * count, dtype=np.float32)
            nfound = emul.port_gather(n, x0, nxl, _i3(start), _i3(length), count, pos.ctypes.data_as(up), cols.ctypes.data_as(fp), index.ctypes.data_as(up),
                                      vel.ctypes.data_as(fp))
            assert nfound == len(windex) and np.array_equal(index[:nfound], windex) and np.array_equal(vel[:24 * nfound].reshape(-1, 24), wvel)
    # the two halves are disjoint and together they are every particle; with the whole box that is each particle twice
    assert total >= 2 * count


def test_the_emulation_under_the_sanitizers():
    if _stale(EXE):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", EXE, SRC])
    out = subprocess.run([EXE], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.count("found") == 16 and "MISMATCH" not in out.stdout
