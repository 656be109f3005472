"""The fragmentation maps without a device: the vectorised numpy restatement of create_map() / update_map() (tests/np_maps.py)
against a literal port of the reference's triple loop on tiny boxes, and the cell arithmetic of the device kernels
(pinocchio_amd/csrc/pf_map_core.h, compiled for the host in tests/cpu_emul/map_emul.cpp and walked lane by lane) against the
restatement: bits, both counts, and that the word form ORs whole runs.  The same file as a program runs under
-fsanitize=address,undefined against a C port of the loop."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import np_maps

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emul", "map_emul.cpp")
SO = os.path.join(HERE, "cpu_emul", "libmap_emul.so")
EXE = os.path.join(HERE, "cpu_emul", "map_emul_san")
LARGE = os.path.join(HERE, "cpu_emul", "large_boxes.h")      # the boxes the mains of the programs share
HDR = os.path.join(HERE, "..", "pinocchio_amd", "csrc", "pf_map_core.h")

# (len, safe, periodic directions)
BOXES = [((20, 23, 37), (4, 4, 4), (False, False, False)),
         ((20, 23, 37), (1, 1, 1), (False, False, False)),
         ((32, 22, 32), (0, 5, 0), (True, False, True)),
         ((16, 16, 16), (0, 0, 0), (True, True, True)),
         ((7, 64, 5), (2, 3, 1), (False, False, False))]


def _stale(out):
    return (not os.path.exists(out)) or os.path.getmtime(out) < max(os.path.getmtime(SRC), os.path.getmtime(HDR), os.path.getmtime(LARGE))


@pytest.fixture(scope="module")
def emul():
    if _stale(SO):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    L = C.CDLL(SO)
    ip, up = C.POINTER(C.c_int), C.POINTER(C.c_uint)
    L.emul_fill_box.restype = C.c_longlong
    L.emul_fill_box.argtypes = [ip, ip, ip, up]
    L.emul_update.restype = C.c_longlong
    L.emul_update.argtypes = [ip, ip, C.c_int, C.POINTER(C.c_double), ip, C.c_double, up, up, C.POINTER(C.c_ulonglong), C.c_int]
    return L


def _ints(v):
    return (C.c_int * len(v))(*[int(x) for x in v])


def groups_for(length, pbc, count, seed, max_mass):
    """seeded groups: centres anywhere in the box and up to three cells outside it in a direction that is not periodic, inside it in
    a periodic one (the reference wraps once); masses log-uniform in 1 .. max_mass, capped so that no sphere is larger than a
    periodic direction"""
    rng = np.random.default_rng(seed)
    pos = np.empty((count, 3))
    for d in range(3):
        pos[:, d] = rng.uniform(0.0, length[d] - 0.6, count) if pbc[d] else rng.uniform(-3.0, length[d] + 3.0, count)
    mass = np.exp(rng.uniform(0.0, np.log(max_mass), count)).astype(np.int32)
    return pos, np.maximum(mass, 1)


def test_words_of_and_bits_of():
    rng = np.random.default_rng(1)
    b = rng.random((3, 5, 7)) < 0.5
    w = np_maps.words_of(b)
    assert w.dtype == np.uint32 and len(w) == 4 and w[-1] >> (105 - 96) == 0
    for p in range(105):
        assert bool((w[p // 32] >> (p % 32)) & 1) == bool(b.ravel()[p])
    assert np.array_equal(np_maps.bits_of(w, b.shape), b)


@pytest.mark.parametrize("length,safe,pbc", BOXES)
def test_create_map_is_the_box_plus_one_layer(length, safe, pbc):
    m = np_maps.create_map(length, safe, pbc)
    want = np.zeros(length, dtype=bool)
    lo = [0 if pbc[d] else safe[d] - 1 for d in range(3)]
    hi = [length[d] if pbc[d] else length[d] - safe[d] + 1 for d in range(3)]
    for i in range(lo[0], hi[0]):              # the reference's loop
        for j in range(lo[1], hi[1]):
            want[i, j, lo[2]:hi[2]] = True
    assert np.array_equal(m, want)
    assert m.sum() == np.prod([hi[d] - lo[d] for d in range(3)])


@pytest.mark.parametrize("length,safe,pbc", BOXES[:4])
def test_the_vectorised_update_equals_the_triple_loop(length, safe, pbc):
    cur = np_maps.create_map(length, safe, pbc)
    pos, mass = groups_for(length, pbc, 40, seed=sum(length), max_mass=3000)
    pos[0] = (-0.3, length[1] - 0.4, 7.5)                                    # (int)(pos + 0.5): 0, len - 1 + 1 -> len, 8
    if pbc[0]:
        pos[0, 0] = 0.2
    if pbc[1]:
        pos[0, 1] = length[1] - 0.6
    mass[0] = 40
    for blf in (2.0, 3.0):
        m = mass.copy()
        for d in range(3):                     # no sphere larger than a periodic direction
            if pbc[d]:
                while max(np_maps.centre_and_size((0, 0, 0), int(v), blf)[1] for v in m) > length[d]:
                    m = np.maximum(m // 2, 1)
        fast, nf = np_maps.update_map(cur, pos, m, blf, pbc)
        slow, ns = np_maps.update_map_loops(cur, pos, m, blf, pbc)
        print(length, pbc, blf, int(fast.sum()), nf)
        assert np.array_equal(fast, slow) and nf == ns
        assert not np.any(fast & cur)                                        # update never repeats a current bit
        if all(pbc):
            assert fast.sum() == 0 and nf == (0, 0)                          # create_map set everything: nothing to request
        elif cur.all():
            assert fast.sum() == 0 and nf[0] == 0 and nf[1] > 0              # safe = 1: the box plus one layer is everything
        else:
            assert nf[0] >= fast.sum() > 0 and nf[1] > 0
    # on an empty current map the spheres overlap: multiplicity
    fast, nf = np_maps.update_map(np.zeros(length, dtype=bool), pos, mass // 8 + 1, 2.0, pbc)
    slow, ns = np_maps.update_map_loops(np.zeros(length, dtype=bool), pos, mass // 8 + 1, 2.0, pbc)
    assert np.array_equal(fast, slow) and nf == ns and nf[0] > fast.sum()


def test_centre_and_size_truncate_as_c_does():
    assert np_maps.centre_and_size((-0.3, 22.6, 7.5), 1, 2.0) == ([0, 23, 8], 1)       # 2 * (1 / 4.19)^(1/3) + 0.5 = 1.74
    assert np_maps.centre_and_size((-0.7, -1.2, 0.49), 1, 0.5)[0] == [0, 0, 0]           # (int)(-0.2) = (int)(-0.7) = 0
    assert np_maps.centre_and_size((0, 0, 0), 1, 0.5)[1] == 0
    assert np_maps.centre_and_size((0, 0, 0), 50000, 3.0)[1] == 69
    assert np_maps.centre_and_size((0, 0, 0), 30, 3.0)[1] == 6


@pytest.mark.parametrize("length,safe,pbc", BOXES)
def test_the_fill_kernel_walked_on_the_cpu(emul, length, safe, pbc):
    want = np_maps.words_of(np_maps.create_map(length, safe, pbc))
    got = np.full(len(want), 0xDEADBEEF, dtype=np.uint32)
    ors = emul.emul_fill_box(_ints(length), _ints(safe), _ints([int(p) for p in pbc]), got.ctypes.data_as(C.POINTER(C.c_uint)))
    assert ors >= 0, ors
    assert np.array_equal(got, want)
    rows = np.prod([(length[d] if pbc[d] else length[d] - 2 * safe[d] + 2) for d in range(2)])
    assert ors <= 2 * rows                                                   # at most the two end words of a row are ORed


@pytest.mark.parametrize("length,safe,pbc", BOXES[:4] + [((96, 80, 72), (6, 6, 6), (False, False, False))])
def test_the_sphere_kernel_walked_on_the_cpu(emul, length, safe, pbc):
    cur = np_maps.create_map(length, safe, pbc)
    big = length == (96, 80, 72)
    pos, mass = groups_for(length, pbc, 60, seed=7 + sum(length), max_mass=50000 if big else 3000)
    mass[:3] = (1, 2, 50000 if big else 3000)                                 # sizes 1 and 2; with BLF 3 a row of 136 cells
    for blf, current in ((2.0, cur), (3.0 if big else 2.5, np.zeros(length, dtype=bool))):
        m = mass.copy()
        for d in range(3):
            if pbc[d]:
                while max(np_maps.centre_and_size((0, 0, 0), int(v), blf)[1] for v in m) > length[d]:
                    m = np.maximum(m // 2, 1)
        want, nw = np_maps.update_map(current, pos, m, blf, pbc)
        cw = np_maps.words_of(current)
        res = {}
        for words in (1, 0):
            got = np.zeros(len(cw), dtype=np.uint32)
            nadd = (C.c_ulonglong * 2)()
            ors = emul.emul_update(_ints(length), _ints([int(p) for p in pbc]), len(m), np.ascontiguousarray(pos).ctypes.data_as(C.POINTER(C.c_double)),
                                   np.ascontiguousarray(m, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int)), blf,
                                   cw.ctypes.data_as(C.POINTER(C.c_uint)), got.ctypes.data_as(C.POINTER(C.c_uint)), nadd, words)
            assert ors >= 0, ors
            assert np.array_equal(got, np_maps.words_of(want)) and (int(nadd[0]), int(nadd[1])) == nw
            res[words] = ors
        print(length, blf, nw, "word ORs", res[1], "bit ORs", res[0])
        assert res[0] == nw[0]                                               # the per-bit form: one OR per requested cell
        if nw[0]:
            assert res[1] < res[0]


def test_the_emulation_under_the_sanitizers():
    if _stale(EXE):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-DMAP_EMUL_MAIN",
                               "-o", EXE, SRC])
    out = subprocess.run([EXE], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.count("word ORs") == 4
