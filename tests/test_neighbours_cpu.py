"""The neighbour table without a device: the numpy restatement (tests/np_neighbours.py) gives hand-written answers and the peak counts
of the two older restatements (np_organize.count_peaks, np_peaks.count_peaks), and the cell arithmetic and lookup of the device path
(pinocchio_amd/csrc/pf_neigh_core.h, compiled for the host in tests/cpu_emul/neighbours_emul.cpp) agree with it cell by cell."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import np_neighbours as npn
import np_organize as npo
import np_peaks

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emul", "neighbours_emul.cpp")
SO = os.path.join(HERE, "cpu_emul", "libneighbours_emul.so")
HDR = os.path.join(HERE, "..", "pinocchio_amd", "csrc", "pf_neigh_core.h")

SKIP, GOOD, PEAK = npn.SKIP, npn.GOOD, npn.PEAK


# ------------------------------------------------------------------------------------------------------------------------
# hand-written answers
def test_a_full_periodic_box_of_27():
    # particle iz sits at position iz and Fmax falls with iz: the sorted order is the position order
    pos = np.arange(27, dtype=np.uint32)
    f = (27 - np.arange(27)).astype(np.float32)
    neigh, flags, peaks = npn.neighbours(pos, f, (3, 3, 3), (0, 0, 0), (True, True, True))
    assert neigh[0].tolist() == [18, 9, 6, 3, 2, 1]            # (0,0,0): every "minus" neighbour wraps
    assert neigh[13].tolist() == [4, 22, 10, 16, 12, 14]       # (1,1,1)
    assert neigh[26].tolist() == [17, 8, 23, 20, 25, 24]       # (2,2,2): every "plus" neighbour wraps
    assert neigh[5].tolist() == [23, 14, 2, 8, 4, 3]           # (0,1,2)
    # only particle 0 has no neighbour of a larger Fmax
    assert flags.tolist() == [GOOD | PEAK] + [GOOD] * 26 and peaks == (1, 1)


def test_a_box_with_borders_and_holes():
    # 4 x 5 x 6, no periodic direction, safe = 1; every cell stored but five; Fmax RISES with the position, so particle iz is the
    # one of rank 114 - iz in position order and a larger iz means a smaller Fmax
    length, safe, pbc = (4, 5, 6), (1, 1, 1), (False, False, False)
    removed = [0, 37, 46, 51, 75]                              # (0,0,0) (1,1,1) (1,2,4) (1,3,3) (2,2,3)
    pos = np.setdiff1d(np.arange(120), removed)[::-1].astype(np.uint32)
    f = np.arange(115, 0, -1).astype(np.float32)
    neigh, flags, peaks = npn.neighbours(pos, f, length, safe, pbc)

    def iz(p):
        return 114 - (p - sum(r < p for r in removed))
    assert pos[iz(45)] == 45 and pos[iz(38)] == 38 and pos[iz(15)] == 15
    # (1,2,3): x+ (2,2,3), y+ (1,3,3) and z+ (1,2,4) are not stored; the other three have a smaller Fmax: the one peak
    assert (iz(45), iz(15), iz(39), iz(44)) == (71, 100, 77, 72)
    assert neigh[71].tolist() == [100, -1, 77, -1, 72, -1] and flags[71] == GOOD | PEAK
    # (1,1,2): z- (1,1,1) is not stored
    assert iz(38) == 78 and neigh[78].tolist() == [107, 50, 83, 72, -1, 77] and flags[78] == GOOD
    # (0,2,3): on the border of x -- nothing looked up, not a good particle
    assert neigh[100].tolist() == [-1] * 6 and flags[100] == SKIP
    # the 24 - 4 stored cells of the interior are the good ones; every border cell is skipped
    assert int((flags & GOOD > 0).sum()) == 20 and int((flags & SKIP > 0).sum()) == 115 - 20
    assert not np.any((flags & SKIP > 0) & (flags & (GOOD | PEAK) > 0))
    assert peaks == (1, 1)


def test_periodic_directions_of_length_one_and_two():
    pos = np.arange(10, dtype=np.uint32)
    f = (10 - np.arange(10)).astype(np.float32)
    neigh, flags, peaks = npn.neighbours(pos, f, (1, 2, 5), (0, 0, 0), (True, True, True))
    assert neigh[0].tolist() == [0, 0, 5, 5, 4, 1]             # x: its own neighbour; y: the same particle twice
    assert neigh[7].tolist() == [7, 7, 2, 2, 6, 8]
    assert neigh[9].tolist() == [9, 9, 4, 4, 8, 5]
    # Fmax > Fmax of itself never holds
    assert flags.tolist() == [GOOD] * 10 and peaks == (0, 0)
    # without the direction of length 1 the largest Fmax is a peak
    neigh, flags, peaks = npn.neighbours(pos, f, (1, 2, 5), (1, 0, 0), (False, True, True))
    assert flags.tolist() == [SKIP] * 10 and peaks == (0, 0) and np.all(neigh == -1)
    pos2 = np.arange(6, dtype=np.uint32)
    f2 = (6 - np.arange(6)).astype(np.float32)
    neigh, flags, peaks = npn.neighbours(pos2, f2, (3, 2, 1), (1, 0, 0), (False, True, True))
    # x = 1 alone is not skipped: positions 2 (1,0,0) and 3 (1,1,0); z of length 1 makes each its own neighbour
    assert neigh[2].tolist() == [0, 4, 3, 3, 2, 2] and neigh[3].tolist() == [1, 5, 2, 2, 3, 3]
    assert flags.tolist() == [SKIP, SKIP, GOOD, GOOD, SKIP, SKIP] and peaks == (0, 0)


# ------------------------------------------------------------------------------------------------------------------------
# peak counts against the older restatements
def _field(rng, n, kind):
    f = (rng.random((n, n, n)) * 4.0 - 0.5).astype(np.float32)
    if kind == 1:
        f = np.asarray([-0.5, 0.0, 0.5, 1.0, 1.5, 2.5, 3.0], dtype=np.float32)[rng.integers(0, 7, (n, n, n))]
    if kind == 2:
        special = np.asarray([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1.0, -1e-40, 1e-40], dtype=np.float32)
        pick = rng.random((n, n, n)) < 0.6
        f[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    return f


def _stored(rng, sub, flast):
    """the stored list of a sub-box in the order after sort_and_organize: (frag_pos, Fmax)"""
    flat = sub.ravel()
    with np.errstate(invalid="ignore"):
        cell = np.flatnonzero(flat.astype(np.float64) >= flast)
    rng.shuffle(cell)
    o = npo.order(flat[cell])
    return cell[o].astype(np.uint32), flat[cell][o]


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["continuous", "seven values", "zeros infinities nan"])
def test_peak_counts_equal_the_older_restatements(kind):
    rng = np.random.default_rng(60 + kind)
    n = 12
    field = _field(rng, n, kind)
    for flast in (-np.inf, 0.0, 1.0, 2.0):
        # the whole periodic box: count_peaks through find_location
        pos, f = _stored(rng, field, flast)
        spos, ind = npo.index(pos)
        neigh, flags, peaks = npn.neighbours(pos, f, (n, n, n), (0, 0, 0), (True, True, True))
        assert peaks[0] == npo.count_peaks(f, pos, spos, ind, (n, n, n)) == peaks[1]
        assert peaks == np_peaks.count_peaks(field, flast)
        # sub-boxes with borders: the field form on the cut-out
        for start, length, safe in (((-2, 3, 0), (7, n, 5), (2, 0, 1)), ((5, 5, 5), (n, 9, n), (0, 3, 0)), ((1, -1, 7), (6, 6, 6), (1, 2, 1)),
                                    ((0, 0, 0), (3, n, 1), (1, 0, 1)), ((4, 0, 2), (n, n, 2), (0, 0, 1))):
            pbc = tuple(v == n for v in length)
            pos, f = _stored(rng, np_peaks.cut(field, start, length), flast)
            neigh, flags, peaks = npn.neighbours(pos, f, length, safe, pbc)
            assert peaks == np_peaks.count_peaks(field, flast, (start, length, safe)), (flast, start, length)
            assert peaks[0] == int((flags & PEAK > 0).sum()) and peaks[1] == int((flags & (PEAK | GOOD) == PEAK | GOOD).sum())


# ------------------------------------------------------------------------------------------------------------------------
# the host compilation of the device path's arithmetic
@pytest.fixture(scope="module")
def emul():
    if (not os.path.exists(SO)) or os.path.getmtime(SO) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    L = C.CDLL(SO)
    ip, up, bp = C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(C.c_ubyte)
    L.emul_cells.argtypes = [ip, ip, ip, C.c_size_t, up, ip, bp, bp, up, up, bp]
    L.emul_rowstart.argtypes = [ip, C.c_uint, up, up]
    L.emul_ranks.argtypes = [ip, ip, ip, C.c_uint, up, up, C.POINTER(C.c_longlong)]
    return L


def _i3(v):
    return (C.c_int * 3)(*map(int, v))


BOXES = ((1, 1, 1), (2, 2, 2), (3, 4, 5), (6, 5, 64))


@pytest.mark.parametrize("length", BOXES)
def test_cell_arithmetic_equals_the_restatement(emul, length):
    cells = length[0] * length[1] * length[2]
    pos = np.arange(cells, dtype=np.uint32)
    for pbc in itertools.product((False, True), repeat=3):
        safe = tuple(0 if pbc[d] else (2 if length[d] >= 5 else 1) for d in range(3))
        coord = np.zeros((cells, 3), dtype=np.int32)
        skip, good = np.zeros(cells, dtype=np.uint8), np.zeros(cells, dtype=np.uint8)
        row = np.zeros(cells, dtype=np.uint32)
        npos = np.zeros((cells, 6), dtype=np.uint32)
        wrapped = np.zeros((cells, 6), dtype=np.uint8)
        up, bp = C.POINTER(C.c_uint), C.POINTER(C.c_ubyte)
        emul.emul_cells(_i3(length), _i3(pbc), _i3(safe), cells, pos.ctypes.data_as(up), coord.ctypes.data_as(C.POINTER(C.c_int)),
                        skip.ctypes.data_as(bp), good.ctypes.data_as(bp), row.ctypes.data_as(up), npos.ctypes.data_as(up), wrapped.ctypes.data_as(bp))
        i, j, k = npn.coords(pos, length)
        wskip, wgood = npn.skip_good(pos, length, safe, pbc)
        wnpos, wwrapped = npn.neighbour_positions(pos, length, pbc)
        assert np.array_equal(coord, np.stack([i, j, k], axis=1)), pbc
        assert np.array_equal(skip.astype(bool), wskip) and np.array_equal(good.astype(bool), wgood), pbc
        assert np.array_equal(row, j + length[1] * i), pbc
        live = ~wskip
        assert np.array_equal(npos[live], wnpos[live]) and np.array_equal(wrapped[live].astype(bool), wwrapped[live]), pbc
        assert not npos[~live].any()


@pytest.mark.parametrize("length", BOXES + ((17, 9, 70),))
def test_both_lookups_equal_find_location(emul, length):
    """the row form (z from the neighbouring ranks, x and y from a search of one z-row) and the plain form (a search of everything),
    walked rank by rank, find what find_location finds -- for every fill, the empty rows and the single particle among them"""
    rng = np.random.default_rng(sum(length))
    cells = length[0] * length[1] * length[2]
    up = C.POINTER(C.c_uint)
    for pbc in itertools.product((False, True), repeat=3):
        safe = tuple(0 if pbc[d] else 1 for d in range(3))
        for fill in (0.0, 0.05, 0.5, 1.0):
            m = max(1, int(round(fill * cells)))
            spos = np.sort(rng.choice(cells, size=m, replace=False)).astype(np.uint32)
            rowstart = np.zeros(length[0] * length[1] + 1, dtype=np.uint32)
            emul.emul_rowstart(_i3(length), m, spos.ctypes.data_as(up), rowstart.ctypes.data_as(up))
            assert np.array_equal(rowstart, np.searchsorted(spos, np.arange(length[0] * length[1] + 1, dtype=np.int64) * length[2]))
            wskip, _ = npn.skip_good(spos, length, safe, pbc)
            wnpos, _ = npn.neighbour_positions(spos, length, pbc)
            want = np.stack([npo.find_location(spos, np.arange(m), wnpos[:, nn]) for nn in range(6)], axis=1)
            want[wskip] = -1
            for rs in (rowstart.ctypes.data_as(up), None):
                rank = np.zeros((m, 6), dtype=np.int64)
                emul.emul_ranks(_i3(length), _i3(pbc), _i3(safe), m, spos.ctypes.data_as(up), rs, rank.ctypes.data_as(C.POINTER(C.c_longlong)))
                assert np.array_equal(rank, want), (pbc, fill, rs is None)
