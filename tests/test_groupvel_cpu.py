"""The group velocities of a segment without a device: the numpy restatement (tests/np_groupvel.py) gives hand-written answers, and the
arithmetic of the device path (pinocchio_amd/csrc/pf_groupvel_core.h, compiled for the host in tests/cpu_emul/groupvel_emul.cpp: key
packing, the reduction of a tile with its carries, the fold) agrees with it for tiles of 2, 3, 64 and 1024 keys.  The same file as a
program runs under -fsanitize=address,undefined against a C restatement of the reference's loop (src/fragment.c:852-909)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import np_groupvel as npg
import np_refresh as npr

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emul", "groupvel_emul.cpp")
SO = os.path.join(HERE, "cpu_emul", "libgroupvel_emul.so")
EXE = os.path.join(HERE, "cpu_emul", "groupvel_emul_san")
LARGE = os.path.join(HERE, "cpu_emul", "large_boxes.h")      # the boxes the mains of the programs share
HDRS = [os.path.join(HERE, "..", "pinocchio_amd", "csrc", h)
        for h in ("pf_groupvel_core.h", "pf_refresh_core.h", "pf_back_core.h", "pf_neigh_core.h", "pf_distribute_boxes.h")]

# (n, start, len, safe): boxes of tests/test_refresh_cpu.py
BOXES = [(16, (0, 0, 0), (16, 16, 16), (0, 0, 0)),
         (16, (-3, 0, 13), (7, 16, 5), (1, 0, 1)),
         (16, (14, 0, 2), (9, 16, 5), (2, 0, 2)),
         (8, (6, 2, 5), (4, 3, 5), (1, 1, 2))]
SHAPES = [(1, 2), (3, 1), (16, 4), (64, 16)]     # (keys of a unit, units of a tile): tiles of 2, 3, 64 and the device's 1024


def _cols(n, nxl):
    """cols24[c][cell] = 1000 c + cell: integer-valued, so that every sum is exact"""
    nc = nxl * n * n
    return (np.arange(24, dtype=np.int64)[:, None] * 1000 + np.arange(nc, dtype=np.int64)[None, :]).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------------
# hand-written answers
def test_a_box_of_4_3_5_in_a_box_of_8():
    n, start, length = 8, (6, 2, 5), (4, 3, 5)
    # the particles of tests/test_refresh_cpu.py: cells 405, 97, 472, 31; the first once more
    pos = np.array([0, 59, 23, 37, 0], dtype=np.uint32)
    gid = np.array([5, 1, 5, 2, 5], dtype=np.int32)
    cols = _cols(n, 8)
    found, loose, counted, cell = npg.classes(n, 0, 8, start, length, pos, gid, 2)
    assert found.all() and loose.tolist() == [False, True, False, False, False] and counted.tolist() == [True, False, True, True, True]
    assert cell.tolist() == [405, 97, 472, 31, 405]
    group, npart, s = npg.sums(n, 0, 8, start, length, pos, gid, 2, cols)
    assert group.tolist() == [2, 5] and npart.tolist() == [1, 3]                      # the duplicate counts twice
    assert s[0].tolist() == [1000 * c + 31 for c in range(24)]
    assert s[1].tolist() == [3 * 1000 * c + 405 + 472 + 405 for c in range(24)]
    ig, inp, isum = npg.int_sums(n, 0, 8, start, length, pos, gid, 2, cols)
    assert ig.tolist() == [2, 5] and inp.tolist() == [1, 3] and np.array_equal(isum, s)
    # first_group 0: the loose particle is a group of its own
    group, npart, s = npg.sums(n, 0, 8, start, length, pos, gid, 0, cols)
    assert group.tolist() == [1, 2, 5] and npart.tolist() == [1, 1, 3] and s[0, 3] == 3097
    # planes 4 .. 7 hold particles 0, 2 and 4, at local planes 2 and 3: cells 149 and 216
    group, npart, s = npg.sums(n, 4, 4, start, length, pos, gid, 2, _cols(n, 4))
    assert group.tolist() == [5] and npart.tolist() == [3] and s[0, 0] == 149 + 216 + 149 and s[0, 23] == 3 * 23000 + 514
    # planes 0 .. 3 hold the two others: one loose, one counted; planes 2 .. 5 none
    found, loose, counted, _ = npg.classes(n, 0, 4, start, length, pos, gid, 2)
    assert found.tolist() == [False, True, False, True, False] and loose.sum() == 1 and counted.sum() == 1
    assert len(npg.sums(n, 2, 4, start, length, pos, gid, 2, _cols(n, 4))[0]) == 0


def test_a_row_of_sixteen():
    # the first z-row of the 16^3 box: cells 0 .. 15; groups 3 (cells 0..4), 2 (5..9), loose (10, 11), 9 (12..15)
    n = 16
    box = ((0, 0, 0), (16, 16, 16))
    pos = np.arange(16, dtype=np.uint32)
    gid = np.array([3] * 5 + [2] * 5 + [0, 1] + [9] * 4, dtype=np.int32)
    group, npart, s = npg.sums(n, 0, 16, box[0], box[1], pos, gid, 2, _cols(n, 16))
    assert group.tolist() == [2, 3, 9] and npart.tolist() == [5, 5, 4]
    assert s[:, 0].tolist() == [35, 10, 54] and s[:, 2].tolist() == [10035, 10010, 8054]


def test_the_scatter_of_the_means():
    groups = np.full((6, 40), 0xAB, dtype=np.uint8)
    s = np.arange(48, dtype=np.float64).reshape(2, 24) + 1.0
    out = npg.scatter_means(groups, [5, 2], [4, 3], s, (4, -1, -1, -1, -1, -1, 24, -1), np.float32)
    assert np.all(groups == 0xAB) and np.all(out[[0, 1, 3, 4]] == 0xAB)
    assert out[5, 4:16].copy().view(np.float32).tolist() == [0.25, 0.5, 0.75]
    assert out[5, 24:36].copy().view(np.float32).tolist() == [19 / 4, 20 / 4, 21 / 4]      # values 12 + 3 * 2 ..: the third prev field
    assert out[2, 4:16].copy().view(np.float32).tolist() == [np.float32(25 / 3), np.float32(26 / 3), 9.0]
    rest = np.ones(40, dtype=bool)
    rest[4:16] = rest[24:36] = False
    assert np.all(out[:, rest] == 0xAB)
    out = npg.scatter_means(np.full((3, 64), 0xAB, dtype=np.uint8), [1], [3], s[:1], (-1, 8, -1, -1, -1, -1, -1, 32), np.float64)
    assert out[1, 8:32].copy().view(np.float64).tolist() == [4 / 3, 5 / 3, 2.0] and out[1, 32:56].copy().view(np.float64).tolist() == [22 / 3, 23 / 3, 8.0]


def test_the_reference_loop_restated():
    vel = np.zeros((5, 24), dtype=np.float32)
    vel[:, 0] = [1, 2, 4, 8, 16]
    vel[:, 23] = [0.5, 0.25, 0.125, 1, 1]
    ref = npg.reference_means(vel, [2, 3, 2, 1, 3], 2, np.random.default_rng(0))
    assert sorted(ref) == [2, 3] and ref[2][0] == 2 and ref[3][0] == 2
    assert ref[2][1][0] == 2.5 and ref[3][1][0] == 9.0 and ref[2][1][23] == 0.3125 and ref[3][1][23] == 0.625


# ------------------------------------------------------------------------------------------------------------------------
# the host compilation of the device path's arithmetic
def _stale(out):
    return (not os.path.exists(out)) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in [SRC, LARGE] + HDRS)


@pytest.fixture(scope="module")
def emul():
    if _stale(SO):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DGROUPVEL_EMUL_LIB", "-o", SO, SRC])
    L = C.CDLL(SO)
    ip, up, bp, dp, ullp = C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(C.c_ubyte), C.POINTER(C.c_double), C.POINTER(C.c_ulonglong)
    L.emul_classes.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip, ip, C.c_size_t, up, ip, C.c_int, bp]
    L.emul_keys.argtypes = [C.c_size_t, up, ullp, C.c_ulonglong]
    L.emul_group_sums.restype = C.c_ulonglong
    L.emul_group_sums.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip, ip, C.c_size_t, up, ip, C.c_int, dp, C.c_int, C.c_int, ip, up, dp, ullp]
    return L


def _i3(v):
    return (C.c_int * 3)(*map(int, v))


def test_the_keys(emul):
    rng = np.random.default_rng(1)
    for ncell in (1, 2, 1000, 4096, 4097, 2 ** 32):
        cell = np.sort(rng.integers(0, ncell, 500).astype(np.uint64))
        cell[-1] = ncell - 1
        gid = np.sort(rng.integers(0, 2 ** 31, 500).astype(np.uint32))
        gid[100:140] = gid[100]                                   # runs of equal IDs: the cells decide
        gid[-1] = 2 ** 31 - 1
        assert emul.emul_keys(500, gid.ctypes.data_as(C.POINTER(C.c_uint)), cell.ctypes.data_as(C.POINTER(C.c_ulonglong)), ncell) == 0


def _emul_sums(emul, n, x0, nxl, box, pos, gid, first, cols, shape):
    start, length, safe = box
    count = len(pos)
    group = np.full(count + 1, -77, dtype=np.int32)
    npart = np.full(count + 1, 0xDEADBEEF, dtype=np.uint32)
    s = np.full(24 * count + 1, -7.0)
    counted = C.c_ulonglong()
    cols = np.ascontiguousarray(cols, dtype=np.float64)
    G = emul.emul_group_sums(n, x0, nxl, _i3(start), _i3(length), _i3(safe), count, pos.ctypes.data_as(C.POINTER(C.c_uint)),
                             gid.ctypes.data_as(C.POINTER(C.c_int)), first, cols.ctypes.data_as(C.POINTER(C.c_double)), shape[0], shape[1],
                             group.ctypes.data_as(C.POINTER(C.c_int)), npart.ctypes.data_as(C.POINTER(C.c_uint)), s.ctypes.data_as(C.POINTER(C.c_double)),
                             C.byref(counted))
    assert np.all(group[G:] == -77) and np.all(npart[G:] == 0xDEADBEEF) and np.all(s[24 * G:] == -7.0)      # the canaries
    return group[:G], npart[:G], s[:24 * G].reshape(G, 24), counted.value


def _grouping(rng, count, kind):
    if kind == "ones":                                            # groups of one particle, sparse IDs
        return (2 + 3 * rng.permutation(count)).astype(np.int32)
    if kind == "one":                                             # all in one group
        return np.full(count, 7, dtype=np.int32)
    if kind == "none":
        return rng.integers(0, 2, count).astype(np.int32)
    if kind == "big":                                             # one group of three fifths, small ones and loose particles
        g = rng.integers(0, 40, count).astype(np.int32)
        g[rng.random(count) < 0.6] = 21
        return g
    return rng.integers(0, max(3, count // 6), count).astype(np.int32)     # "mixed": about six per group, two IDs loose


@pytest.mark.parametrize("box", BOXES, ids=lambda b: "n%d-%s" % (b[0], "x".join(map(str, b[2]))))
def test_the_device_arithmetic_equals_the_restatement(emul, box):
    n, start, length, safe = box
    rng = np.random.default_rng(11 * sum(length) + n)
    ncells = length[0] * length[1] * length[2]
    pos = rng.permutation(ncells)[:max(1, int(round(0.6 * ncells)))].astype(np.uint32)
    pos = np.concatenate([pos, rng.choice(pos, len(pos) // 10)])  # duplicates
    count = len(pos)
    up, ip, bp = C.POINTER(C.c_uint), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)
    for x0, nxl in [(0, n), (0, n // 2), (n // 2, n // 2), (n // 4, 3)]:
        cols = _cols(n, nxl)
        fcols = rng.standard_normal((24, nxl * n * n)).astype(np.float32)
        for kind in ("mixed", "ones", "one", "none", "big"):
            gid = _grouping(rng, count, kind)
            for first in (2, 0):
                found, loose, counted, _ = npg.classes(n, x0, nxl, start, length, pos, gid, first)
                cls = np.zeros(count, dtype=np.uint8)
                emul.emul_classes(n, x0, nxl, _i3(start), _i3(length), _i3(safe), count, pos.ctypes.data_as(up), gid.ctypes.data_as(ip), first, cls.ctypes.data_as(bp))
                assert np.array_equal(cls, loose * 1 + counted * 2) and np.array_equal(cls > 0, found)
                want = npg.int_sums(n, x0, nxl, start, length, pos, gid, first, cols)
                fwant = npg.sums(n, x0, nxl, start, length, pos, gid, first, fcols)
                fabs = npg.abs_sums(n, x0, nxl, start, length, pos, gid, first, fcols)
                for shape in SHAPES:
                    g, m, s, c = _emul_sums(emul, n, x0, nxl, box[1:], pos, gid, first, cols, shape)
                    assert c == counted.sum() == m.sum()
                    assert np.array_equal(g, want[0]) and np.array_equal(m, want[1]) and s.tobytes() == want[2].tobytes(), (kind, first, shape)
                    # random floats: within the bound of fp64 summation in any order
                    g, m, s, c = _emul_sums(emul, n, x0, nxl, box[1:], pos, gid, first, fcols, shape)
                    assert np.array_equal(g, fwant[0]) and np.array_equal(m, fwant[1])
                    assert np.all(np.abs(s - fwant[2]) <= m[:, None] * 2.0 ** -53 * fabs), (kind, first, shape)
            if kind == "none":
                assert npg.classes(n, x0, nxl, start, length, pos, gid, 2)[2].sum() == len(npg.sums(n, x0, nxl, start, length, pos, gid, 2, cols)[0]) == 0


def test_the_emulation_under_the_sanitizers():
    if _stale(EXE):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", EXE, SRC])
    out = subprocess.run([EXE], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.count("groups") == 16 and "MISMATCH" not in out.stdout
