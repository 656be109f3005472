"""The box table of the device's distribute (pinocchio_amd/csrc/pf_distribute_boxes.h) compiled for the host
(tests/cpu_emul/distribute_emul.cpp) against the numpy restatement of the reference's loops (tests/np_distribute.py): the C++
intersection() on 10^4 random (slab, sub-box) pairs, and the decomposition of the kernels -- wavefront slots, masks, workgroup
counts, ranks -- walked lane by lane on the CPU.  No device needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import np_distribute as npd

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emul", "distribute_emul.cpp")
SO = os.path.join(HERE, "cpu_emul", "libdistribute_emul.so")
HDR = os.path.join(HERE, "..", "pinocchio_amd", "csrc", "pf_distribute_boxes.h")


@pytest.fixture(scope="module")
def emul():
    if (not os.path.exists(SO)) or os.path.getmtime(SO) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    L = C.CDLL(SO)
    ip, up = C.POINTER(C.c_int), C.POINTER(C.c_uint)
    L.emul_intersection.argtypes = [C.c_int, ip, ip, ip]
    L.emul_distribute.restype = C.c_longlong
    L.emul_distribute.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_double, ip, ip, up, C.c_ulonglong, up, up]
    return L


def _ints(v):
    return (C.c_int * len(v))(*[int(x) for x in v])


def test_cxx_intersection_equals_the_numpy_one_on_random_pairs(emul):
    rng = np.random.default_rng(2024)
    seen = {k: 0 for k in range(9)}
    double_segment = full = 0
    for trial in range(10000):
        n = int(rng.choice([4, 6, 16, 24, 50, 128, 200]))
        fbox = [0] * 3 + [n] * 3
        if trial % 3:                                   # an x-slab; otherwise any FFT box (the reference's pencils)
            p = int(rng.choice([q for q in (1, 2, 4, 8) if n % q == 0]))
            fbox[3] = n // p
            fbox[0] = int(rng.integers(0, p)) * fbox[3]
        else:
            for d in range(3):
                fbox[3 + d] = int(rng.integers(1, n + 1))
                fbox[d] = int(rng.integers(0, n - fbox[3 + d] + 1))
        length = [n if rng.random() < 0.2 else int(rng.integers(1, n + 1)) for _ in range(3)]
        start = [int(rng.integers(-n + 1, n)) for _ in range(3)]
        want = npd.intersection(n, fbox, start + length)
        out = (C.c_int * 48)()
        nb = emul.emul_intersection(n, _ints(fbox), _ints(start + length), out)
        got = [(list(out[6 * i:6 * i + 3]), list(out[6 * i + 3:6 * i + 6])) for i in range(nb)]
        assert got == want, (n, fbox, start, length)
        seen[nb] += 1
        full += any(v == n for v in length)
        double_segment += any((start[d] % n) + length[d] > n for d in range(3))
        # the boxes tile (FFT box) x (sub-box): as many cells as the two have in common, counted one dimension at a time
        common = 1
        for d in range(3):
            inside = np.zeros(n, dtype=bool)
            inside[(start[d] + np.arange(length[d])) % n] = True
            common *= int(inside[fbox[d]:fbox[d] + fbox[3 + d]].sum())
        assert sum(b[1][0] * b[1][1] * b[1][2] for b in got) == common
    print("boxes per pair:", seen, "pairs with len == n:", full, "with a double segment:", double_segment)
    assert seen[0] and seen[1] and seen[2] and seen[4] and seen[8] and full > 1000 and double_segment > 1000


@pytest.mark.parametrize("n", [4, 16, 24, 40])
def test_the_decomposition_of_the_kernels_equals_the_restatement(emul, n):
    for x0, nxl, start, length, words, flast, field in npd.random_cases(n, 60, seed=100 + n):
        wcell, wpos = npd.contribution(field, n, x0, start, length, flast, words)
        cap = len(wcell) + 3
        pos = np.zeros(cap, dtype=np.uint32)
        cell = np.zeros(cap, dtype=np.uint32)
        mp = words.ctypes.data_as(C.POINTER(C.c_uint)) if words is not None else None
        got = emul.emul_distribute(n, x0, nxl, field.ctypes.data_as(C.POINTER(C.c_float)), flast, _ints(start), _ints(length), mp, cap,
                                   pos.ctypes.data_as(C.POINTER(C.c_uint)), cell.ctypes.data_as(C.POINTER(C.c_uint)))
        assert got == len(wcell), (x0, nxl, start, length, flast)
        assert np.array_equal(pos[:got], wpos) and np.array_equal(cell[:got], wcell), (x0, nxl, start, length, flast)


def test_refusals_of_the_table(emul):
    f = np.zeros((4, 4, 4), dtype=np.float32)
    fp = f.ctypes.data_as(C.POINTER(C.c_float))
    buf = np.zeros(4, dtype=np.uint32).ctypes.data_as(C.POINTER(C.c_uint))
    assert emul.emul_distribute(4, 0, 4, fp, 1.0, _ints([0, 0, 0]), _ints([4, 5, 4]), None, 0, buf, buf) == -1
    assert emul.emul_distribute(4, 0, 4, fp, 1.0, _ints([0, 0, 0]), _ints([0, 4, 4]), None, 0, buf, buf) == -1
    assert emul.emul_distribute(4, 0, 4, fp, 1.0, _ints([0, 0, 0]), _ints([4, 4, 4]), None, 0, buf, buf) == 0
