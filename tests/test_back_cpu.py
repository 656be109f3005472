"""distribute_back without a device: the numpy restatement (tests/np_back.py) gives hand-written answers and agrees with a literal
particle-by-particle walk of the reference's loop (src/distribute.c:806-834), and the cell arithmetic of the device path
(pinocchio_amd/csrc/pf_back_core.h, compiled for the host in tests/cpu_emul/back_emul.cpp) agrees with it particle by particle.  The
same file as a program runs under -fsanitize=address,undefined against a C port of the loop."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import np_back as npb

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emul", "back_emul.cpp")
SO = os.path.join(HERE, "cpu_emul", "libback_emul.so")
EXE = os.path.join(HERE, "cpu_emul", "back_emul_san")
LARGE = os.path.join(HERE, "cpu_emul", "large_boxes.h")      # the boxes the mains of the programs share
HDRS = [os.path.join(HERE, "..", "pinocchio_amd", "csrc", h) for h in ("pf_back_core.h", "pf_neigh_core.h", "pf_distribute_boxes.h")]

# (n, start, len, safe): the boxes of tests/test_gpu_back.py -- every particle good; wraps in all three directions from a negative
# start; one periodic direction; the mixed-radix grid; the slab case -- and two small ones: all of a direction inside the safety layers
# but one plane, and a start beyond the box (reduced to it)
BOXES = [(16, (0, 0, 0), (16, 16, 16), (0, 0, 0)),
         (16, (-3, 10, 13), (11, 9, 8), (2, 1, 3)),
         (16, (5, 0, -2), (7, 16, 12), (1, 0, 2)),
         (24, (20, 3, 0), (9, 5, 24), (2, 1, 0)),
         (40, (19, 0, 33), (17, 9, 40), (2, 1, 0)),
         (8, (7, 7, 7), (3, 5, 8), (1, 2, 0)),
         (8, (-15, 9, 0), (8, 4, 3), (0, 1, 1))]


def _slabs(n):
    """the whole box, its halves and an odd cut"""
    return [(0, n), (0, n // 2), (n // 2, n // 2), (n // 4, 3)]


def _particles(rng, length, fraction=0.6):
    cells = length[0] * length[1] * length[2]
    pos = rng.permutation(cells)[:max(1, int(round(fraction * cells)))].astype(np.uint32)
    zacc = rng.random(len(pos)).astype(np.float32) * 10.0
    zacc[rng.random(len(pos)) < 0.15] = -1.0
    gid = rng.integers(0, 2 ** 31, len(pos)).astype(np.int32)
    gid[rng.random(len(pos)) < 0.15] = 0
    return pos, zacc, gid


# ------------------------------------------------------------------------------------------------------------------------
# hand-written answers
def test_a_periodic_box_of_27():
    n, start, length, safe = 3, (1, 2, 0), (3, 3, 3), (0, 0, 0)
    pos = np.array([0, 26, 13, 5], dtype=np.uint32)            # (0,0,0) (2,2,2) (1,1,1) (0,1,2)
    zacc = np.array([0.5, 1.5, -1.0, 2.5], dtype=np.float32)
    gid = np.array([7, 0, 9, 11], dtype=np.int32)
    # every particle is good; (i, j, k) -> ((i + 1) % 3, (j + 2) % 3, k): cells (1,2,0) = 15, (0,1,2) = 5, (2,0,1) = 19, (1,0,2) = 11
    z, g, stored = npb.distribute_back(n, 0, 3, start, length, safe, pos, zacc, gid)
    assert stored == 4
    wz, wg = np.full(27, -1.0, dtype=np.float32), np.zeros(27, dtype=np.int32)
    wz[[15, 5, 19, 11]] = zacc
    wg[[15, 5, 19, 11]] = gid
    assert np.array_equal(z, wz) and np.array_equal(g, wg)
    # cell 19 holds the zacc it started with (-1) but a group; cell 5 the group it started with (0) but a zacc; the 23 others -1 / 0
    assert z[19] == -1.0 and g[19] == 9 and z[5] == 1.5 and g[5] == 0 and int((z == -1.0).sum()) == 24 and int((g == 0).sum()) == 24
    # the slab of plane 1 alone takes the two particles of x = 0: local cells 15 - 9 and 11 - 9
    z, g, stored = npb.distribute_back(n, 1, 1, start, length, safe, pos, zacc, gid)
    assert stored == 2 and np.flatnonzero(g).tolist() == [2, 6] and z[6] == 0.5 and z[2] == 2.5 and g[6] == 7 and g[2] == 11
    assert int((z == -1.0).sum()) == 7
    # planes 0 and 2 take one each; the three slabs together are the whole box
    parts = [npb.distribute_back(n, x, 1, start, length, safe, pos, zacc, gid) for x in range(3)]
    assert [p[2] for p in parts] == [1, 2, 1] and np.array_equal(np.concatenate([p[0] for p in parts]), wz)


def test_a_box_of_4_5_6_with_safety_layers():
    # every cell of the sub-box stored, in the CLASSIC form (particle iz at position iz); zacc = iz + 0.5, group_ID = iz + 1
    n, start, length, safe = 8, (6, 0, 5), (4, 5, 6), (1, 1, 1)
    zacc = np.arange(120, dtype=np.float32) + 0.5
    gid = np.arange(120, dtype=np.int32) + 1
    z, g, stored = npb.distribute_back(n, 0, 8, start, length, safe, None, zacc, gid)
    # good: x in 1..2, y in 1..3, z in 1..4 -> 24 particles; x 1, 2 -> planes 7, 0 (a wrap); z 1..4 -> 6, 7, 0, 1 (a wrap)
    assert stored == 24 and int((g != 0).sum()) == 24 and int((z != -1.0).sum()) == 24
    want = {}
    for i, gx in ((1, 7), (2, 0)):
        for j in (1, 2, 3):
            for k, gz in ((1, 6), (2, 7), (3, 0), (4, 1)):
                want[gz + 8 * (j + 8 * gx)] = k + 6 * (j + 5 * i)
    assert sorted(want) == np.flatnonzero(g).tolist()
    assert all(z[c] == iz + 0.5 and g[c] == iz + 1 for c, iz in want.items())
    assert want[25] == 82 and want[462] == 37                  # (2,3,4) -> (0,3,1); (1,1,1) -> (7,1,6)
    # a border particle is not stored: (0,2,3) = position 15 would land on (6,2,0) = cell 400
    assert z[400] == -1.0 and g[400] == 0
    # planes 4 .. 7: the twelve particles of x = 1, on local plane 3
    z, g, stored = npb.distribute_back(n, 4, 4, start, length, safe, None, zacc, gid)
    assert stored == 12 and z[206] == 37.5 and g[206] == 38 and np.all(np.flatnonzero(g) // 64 == 3)
    # columns that hold something already keep it where nothing is stored
    z0 = np.full(256, 3.0, dtype=np.float32)
    g0 = np.full(256, 5, dtype=np.int32)
    z, g, stored = npb.distribute_back(n, 4, 4, start, length, safe, None, zacc, gid, z0, g0)
    assert stored == 12 and int((z != 3.0).sum()) == 12 and int((g != 5).sum()) == 12 and np.all(z0 == 3.0)


# ------------------------------------------------------------------------------------------------------------------------
# the reference's loop, particle by particle
def _walk(n, x0, nxl, stabl, Lgwbl, safe, frag_pos, zacc, gid):
    fft_box = (x0, 0, 0, nxl, n, n)
    pz, pg = npb.fresh(n, nxl)
    for iz in range(len(zacc)):
        I = int(frag_pos[iz]) if frag_pos is not None else iz
        kbox = I % Lgwbl[2]
        kk = I // Lgwbl[2]
        jbox = kk % Lgwbl[1]
        ibox = kk // Lgwbl[1]
        good_particle = (ibox >= safe[0] and ibox < Lgwbl[0] - safe[0] and jbox >= safe[1] and jbox < Lgwbl[1] - safe[1] and
                         kbox >= safe[2] and kbox < Lgwbl[2] - safe[2])
        ibox = (ibox + stabl[0] + n) % n
        jbox = (jbox + stabl[1] + n) % n
        kbox = (kbox + stabl[2] + n) % n
        if (good_particle and fft_box[0] <= ibox < fft_box[0] + fft_box[3] and fft_box[1] <= jbox < fft_box[1] + fft_box[4] and
                fft_box[2] <= kbox < fft_box[2] + fft_box[5]):
            fftpos = (kbox - fft_box[2]) + fft_box[5] * ((jbox - fft_box[1]) + fft_box[4] * (ibox - fft_box[0]))
            pz[fftpos] = zacc[iz]
            pg[fftpos] = gid[iz]
    return pz, pg


@pytest.mark.parametrize("box", BOXES[:4] + BOXES[5:], ids=lambda b: "n%d-%s" % (b[0], "x".join(map(str, b[2]))))
def test_the_restatement_equals_the_loop(box):
    n, start, length, safe = box
    stabl = start if all(-n < s < n for s in start) else tuple(s % n for s in start)   # the reference's stabl lies in (-n, n): its loop adds n once
    rng = np.random.default_rng(sum(length) + n)
    cells = length[0] * length[1] * length[2]
    pos, zacc, gid = _particles(rng, length, fraction=min(0.6, 400.0 / cells))
    total = 0
    for x0, nxl in _slabs(n):
        for fp in (pos, None):
            pz, pg = _walk(n, x0, nxl, stabl, length, safe, fp, zacc, gid)
            z, g, stored = npb.distribute_back(n, x0, nxl, start, length, safe, fp, zacc, gid)
            assert np.array_equal(z, pz) and np.array_equal(g, pg), (x0, nxl, fp is None)
            spos, sz, sg = npb.send_data_back(n, x0, nxl, start, length, safe, fp, zacc, gid)
            assert stored == len(spos) and len(np.unique(spos)) == stored
            total += stored
    assert total > 0


# ------------------------------------------------------------------------------------------------------------------------
# the host compilation of the device path's arithmetic
def _stale(out):
    return (not os.path.exists(out)) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in [SRC, LARGE] + HDRS)


@pytest.fixture(scope="module")
def emul():
    if _stale(SO):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    L = C.CDLL(SO)
    ip, up, bp, fp = C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(C.c_ubyte), C.POINTER(C.c_float)
    L.emul_cells.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip, ip, C.c_size_t, up, ip, bp, ip, bp, C.POINTER(C.c_ulonglong)]
    for f in (L.emul_back, L.port_back):
        f.restype = C.c_ulonglong
        f.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip, ip, C.c_size_t, up, fp, ip, fp, ip]
    return L


def _i3(v):
    return (C.c_int * 3)(*map(int, v))


@pytest.mark.parametrize("box", BOXES, ids=lambda b: "n%d-%s" % (b[0], "x".join(map(str, b[2]))))
def test_the_device_arithmetic_equals_the_restatement(emul, box):
    n, start, length, safe = box
    rng = np.random.default_rng(7 * sum(length) + n)
    cells = length[0] * length[1] * length[2]
    every = np.arange(cells, dtype=np.uint32)
    pos, zacc, gid = _particles(rng, length)
    ip, up, bp, fp = C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(C.c_ubyte), C.POINTER(C.c_float)
    for x0, nxl in _slabs(n):
        # per cell of the sub-box
        coord = np.zeros((cells, 3), dtype=np.int32)
        glob = np.zeros((cells, 3), dtype=np.int32)
        good, taken = np.zeros(cells, dtype=np.uint8), np.zeros(cells, dtype=np.uint8)
        addr = np.zeros(cells, dtype=np.uint64)
        emul.emul_cells(n, x0, nxl, _i3(start), _i3(length), _i3(safe), cells, every.ctypes.data_as(up), coord.ctypes.data_as(ip), good.ctypes.data_as(bp),
                        glob.ctypes.data_as(ip), taken.ctypes.data_as(bp), addr.ctypes.data_as(C.POINTER(C.c_ulonglong)))
        i, j, k = npb.coords(every, length)
        assert np.array_equal(coord, np.stack([i, j, k], axis=1))
        wgood = np.ones(cells, dtype=bool)
        for d, c in enumerate((i, j, k)):
            wgood &= (c >= safe[d]) & (c < length[d] - safe[d])
            assert np.array_equal(glob[:, d], (c + start[d]) % n)
        wtaken, wpos = npb.selection(n, x0, nxl, start, length, safe, every)
        assert np.array_equal(good.astype(bool), wgood) and np.array_equal(taken.astype(bool), wtaken)
        assert np.array_equal(addr[wtaken].astype(np.int64), wpos[wtaken]) and not addr[~wtaken].any()
        assert wpos[wtaken].size == 0 or (wpos[wtaken].min() >= 0 and wpos[wtaken].max() < nxl * n * n)
        # the scatter, particle by particle, with and without frag_pos
        for fpos in (pos, None):
            wz, wg, wstored = npb.distribute_back(n, x0, nxl, start, length, safe, fpos, zacc, gid)
            for fn in (emul.emul_back,) + ((emul.port_back,) if all(-n < s < n for s in start) else ()):
                z, g = npb.fresh(n, nxl)
                stored = fn(n, x0, nxl, _i3(start), _i3(length), _i3(safe), len(zacc), fpos.ctypes.data_as(up) if fpos is not None else None,
                            zacc.ctypes.data_as(fp), gid.ctypes.data_as(ip), z.ctypes.data_as(fp), g.ctypes.data_as(ip))
                assert stored == wstored and np.array_equal(z, wz) and np.array_equal(g, wg), (x0, nxl, fpos is None)


def test_the_emulation_under_the_sanitizers():
    if _stale(EXE):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-DBACK_EMUL_MAIN",
                               "-o", EXE, SRC])
    out = subprocess.run([EXE], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.count("stored") == 16 and "MISMATCH" not in out.stdout
