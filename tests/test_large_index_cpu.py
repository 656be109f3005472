"""The fragmentation stages at production-size sub-box positions, without a device.

The device stages of fragment() are written for sub-boxes of up to 2^32 cells at n = 2048: positions z + Lz (y + Ly x) pass 2^31 and
approach 2^32.  This module holds what the GPU tests of tests/test_gpu_large_index.py stand on:
  * the boxes: A just past 2^31 cells, B exactly 2^32 (the largest legal box; x and y periodic at n = 2048), C just below 2^32 with no
    periodic direction, and a ladder of boxes whose position sorts run over 21 .. 32 bits;
  * large_set(): one particle set per large box, about 2 10^5 distinct positions, made without any array over the cells -- edge
    positions, full blocks of 6 x 6 x 70 cells where neighbours and wraps must be found, and random sparse positions -- with the
    conditions that make a comparison on it meaningful asserted from the restatements alone;
  * the sparse restatements (np_distribute.contribution_sparse, np_maps.create_map_words / update_map_sparse), pinned here against the
    dense forms on the seeded cases of the older tests;
  * the device headers compiled for the host (tests/cpu_emul) on A, B and C against the restatements, and the *_emul_san programs,
    whose mains run the same boxes under -fsanitize=address,undefined."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import np_back as npb
import np_distribute as npd
import np_groupvel as npg
import np_maps
import np_neighbours as npn
import np_organize as npo
import np_refresh as npr
import test_back_cpu
import test_groupvel_cpu
import test_maps_cpu
import test_refresh_cpu
from test_back_cpu import emul as back_emul                  # noqa: F401  (the fixtures that build and load the host compilations)
from test_distribute_boxes import emul as dist_emul          # noqa: F401
from test_groupvel_cpu import emul as gv_emul                # noqa: F401
from test_maps_cpu import emul as map_emul                   # noqa: F401
from test_neighbours_cpu import emul as neigh_emul           # noqa: F401
from test_refresh_cpu import emul as refresh_emul            # noqa: F401

TWO31, TWO32 = 1 << 31, 1 << 32

# ------------------------------------------------------------------------------------------------------------------------
# the boxes.  n: the box the sub-box is cut from (a direction is periodic when len == n; without a context, when safe == 0: the two
# agree here); wrapped: a start from which the sub-box wraps in all three directions
BOX_A = (1291, 1291, 1291)      # 2 151 685 171 cells: just past 2^31
BOX_B = (2048, 2048, 1024)      # 2^32 cells exactly
BOX_C = (1625, 1626, 1625)      # 4 293 656 250 cells: 1 311 046 below 2^32
LARGE = {"A": dict(length=BOX_A, n=1296, safe=(1, 3, 3), wrapped=(700, 800, 900)),
         "B": dict(length=BOX_B, n=2048, safe=(0, 0, 3), wrapped=(5, 7, 1500)),
         "C": dict(length=BOX_C, n=2048, safe=(1, 2, 3), wrapped=(1000, 900, 1100))}
TOO_LARGE = (2048, 2048, 1025)  # more than 2^32 cells: every stage refuses it
# (len, bits of the position sort)
LADDER = (((128, 128, 128), 21), ((129, 128, 128), 22), ((256, 256, 256), 24), ((257, 256, 256), 25), ((2048, 1024, 1024), 31),
          ((2048, 1024, 1025), 32), (BOX_B, 32))
BLOCK = (6, 6, 70)              # z-rows longer than a wavefront


def cells_of(length):
    return int(length[0]) * int(length[1]) * int(length[2])


def sort_bits(cells):
    """the bits a sort of positions below `cells` must visit"""
    return max(1, (cells - 1).bit_length())


def pbc_of(safe):
    return tuple(s == 0 for s in safe)


def slab_x0(geom, start, nxl):
    """the slab of nxl planes on the last x-planes of the sub-box"""
    x0 = (start[0] + geom["length"][0] - nxl) % geom["n"]
    assert x0 + nxl <= geom["n"]
    return x0


def fmax_of_kind(rng, count, kind):
    """fp32 Fmax of the three kinds of tests/test_gpu_organize.py: 0 continuous; 1 seven distinct values (nearly every comparison is a
    tie and the stable rule decides); 2 zeros of both signs, infinities and NaN among the values"""
    f = (rng.random(count) * 4.0 - 0.5).astype(np.float32)
    if kind == 1:
        f = np.asarray([-0.5, 0.0, 0.5, 1.0, 1.5, 2.5, 3.0], dtype=np.float32)[rng.integers(0, 7, count)]
    if kind == 2:
        special = np.asarray([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1.0, -1e-40, 1e-40], dtype=np.float32)
        pick = rng.random(count) < 0.6
        f[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
        assert count < 63 or (np.isnan(f).any() and np.isinf(f).any() and (np.signbit(f) & (f == 0)).any())
    return f


def random_positions(rng, cells, count):
    """`count` distinct positions below `cells` in random order; nothing of size `cells` is made"""
    got = np.zeros(0, dtype=np.int64)
    while len(got) < count:
        got = np.unique(np.concatenate([got, rng.integers(0, cells, 2 * (count - len(got)) + 16, dtype=np.int64)]))
    return rng.permutation(got)[:count]


def block_positions(length, corner, shape=BLOCK):
    """every position of the block of `shape` cells at `corner`, which lies inside the box"""
    c = [int(corner[d]) + np.arange(shape[d], dtype=np.int64) for d in range(3)]
    assert all(c[d][0] >= 0 and c[d][-1] < length[d] for d in range(3)), (length, corner)
    return (c[2][None, None, :] + int(length[2]) * (c[1][None, :, None] + int(length[1]) * c[0][:, None, None])).ravel()


def corner_across(length, p):
    """the corner of a block that holds position p near its middle (moved inside the box where p lies near a face)"""
    L = [int(v) for v in length]
    c = (p // (L[2] * L[1]), (p // L[2]) % L[1], p % L[2])
    return tuple(min(max(c[d] - BLOCK[d] // 2, 0), L[d] - BLOCK[d]) for d in range(3))


def structured_positions(length, pbc):
    """the parts of a large set that are not random: 0, 2^31 - 1, 2^31, cells - 1; the eight corners; full blocks at the origin corner,
    at the far corner, across the z-row that holds position 2^31 and on both faces of every periodic direction (a z-face takes four)"""
    L = [int(v) for v in length]
    cells = cells_of(L)
    parts = [np.array([p for p in (0, TWO31 - 1, TWO31, cells - 1) if p < cells], dtype=np.int64)]
    parts.append(np.array([k + L[2] * (j + L[1] * i) for i in (0, L[0] - 1) for j in (0, L[1] - 1) for k in (0, L[2] - 1)], dtype=np.int64))
    corners = [(0, 0, 0), tuple(L[d] - BLOCK[d] for d in range(3))]
    if cells > TWO31:
        corners.append(corner_across(L, TWO31))
    for d in range(3):
        if pbc[d]:
            for face in (0, L[d] - BLOCK[d]):
                for side in range(4 if d == 2 else 1):      # a block shows 36 cells on a z-face: four of them side by side in y
                    corner = [L[e] // 2 - BLOCK[e] // 2 for e in range(3)]
                    corner[d] = face
                    corner[1] += BLOCK[1] * side if d == 2 else 0
                    corners.append(tuple(corner))
    parts += [block_positions(L, c) for c in corners]
    return np.unique(np.concatenate(parts))


def neighbour_census(pos, length, safe, pbc):
    """from the restatement: (found neighbours per direction [6], found neighbours reached by a wrap per direction [6])"""
    spos, ind = npo.index(pos)
    skip, _ = npn.skip_good(pos, length, safe, pbc)
    npos, wrapped = npn.neighbour_positions(pos, length, pbc)
    found = np.stack([npo.find_location(spos, ind, npos[:, nn]) >= 0 for nn in range(6)], axis=1) & ~skip[:, None]
    return found.sum(axis=0), (found & wrapped).sum(axis=0)


@functools.lru_cache(maxsize=None)
def large_set(name, kind, periodic=False):
    """The particle set of box A, B or C with Fmax of kind 0 (continuous), 1 (few values) or 2 (zeros, infinities, NaN):
    -> dict(pos uint32 in input order, f float32, order / spos / ind: np_organize.organize of them, neigh / flags / peaks:
    np_neighbours.neighbours of the sorted set), about 2 10^5 particles.  periodic: the same box with no safety layer, every
    direction periodic (blocks on all six faces).  The arrays are shared between tests: read only."""
    geom = LARGE[name]
    length = geom["length"]
    safe = (0, 0, 0) if periodic else geom["safe"]
    pbc = pbc_of(safe)
    cells = cells_of(length)
    rng = np.random.default_rng(1000 * kind + ord(name) + (7 if periodic else 0))
    fixed = structured_positions(length, pbc)
    pos = np.unique(np.concatenate([fixed, random_positions(rng, cells, 200000 - len(fixed))]))
    assert pos[0] == 0 and pos[-1] == cells - 1 and len(pos) >= 190000
    pos = rng.permutation(pos).astype(np.uint32)
    f = fmax_of_kind(rng, len(pos), kind)
    order, spos, ind = npo.organize(f, pos)
    neigh, flags, peaks = npn.neighbours(pos[order], f[order], length, safe, pbc)
    # the set is not vacuous
    if cells > TWO31 + (TWO31 >> 1):
        assert (pos >= TWO31).mean() >= 0.4, name
    assert TWO31 - 1 in spos and TWO31 in spos
    found, wrapped = neighbour_census(pos, length, safe, pbc)
    assert found.min() >= 1000, (name, found)
    for d in range(3):
        if pbc[d]:
            assert wrapped[2 * d] >= 100 and wrapped[2 * d + 1] >= 100, (name, wrapped)
        else:
            assert wrapped[2 * d] == wrapped[2 * d + 1] == 0
    assert peaks[0] >= 1 and peaks[1] >= 1, (name, peaks)
    out = dict(pos=pos, f=f, order=order, spos=spos, ind=ind, neigh=neigh, flags=flags, peaks=peaks, length=length, safe=safe, pbc=pbc)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _i3(v):
    return (C.c_int * 3)(*map(int, v))


UP, IP, BP, FP = C.POINTER(C.c_uint), C.POINTER(C.c_int), C.POINTER(C.c_ubyte), C.POINTER(C.c_float)
ULLP = C.POINTER(C.c_ulonglong)


# ------------------------------------------------------------------------------------------------------------------------
# the generator
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_the_large_sets_are_not_vacuous(name):
    for kind in (0, 1, 2):
        s = large_set(name, kind)                      # (asserts its own conditions)
        cells = cells_of(s["length"])
        assert len(np.unique(s["pos"])) == len(s["pos"]) and int(s["pos"].max()) == cells - 1
        assert np.array_equal(s["spos"], np.sort(s["pos"])) and s["spos"].dtype == np.uint32
        print(name, kind, len(s["pos"]), "particles,", int((s["pos"] >= TWO31).sum()), "at or beyond 2^31, peaks", s["peaks"])
    s = large_set("A", 0, periodic=True)
    assert s["pbc"] == (True, True, True) and not (s["flags"] & npn.SKIP).any()
    assert [sort_bits(cells_of(length)) for length, _ in LADDER] == [bits for _, bits in LADDER]
    assert cells_of(BOX_B) == TWO32 and TWO31 < cells_of(BOX_A) < TWO31 + (1 << 23) and TWO32 - cells_of(BOX_C) == 1311046
    assert cells_of(TOO_LARGE) > TWO32


def test_random_positions_are_distinct_and_span_the_range():
    rng = np.random.default_rng(5)
    p = random_positions(rng, TWO32, 100000)
    assert len(np.unique(p)) == 100000 and p.min() >= 0 and p.max() < TWO32 and (p >= TWO31).mean() > 0.45
    assert sorted(random_positions(rng, 40, 40).tolist()) == list(range(40))


# ------------------------------------------------------------------------------------------------------------------------
# the sparse restatements against the dense ones
@pytest.mark.parametrize("n", [4, 16, 24, 40])
def test_sparse_contribution_equals_contribution(n):
    taken = 0
    for seed in (n, 100 + n):                          # the cases of tests/test_gpu_distribute.py and tests/test_distribute_boxes.py
        for x0, nxl, start, length, words, flast, field in npd.random_cases(n, 60, seed=seed):
            wcell, wpos = npd.contribution(field, n, x0, start, length, flast, words)
            cell, pos = npd.contribution_sparse(field, n, x0, start, length, flast, words)
            assert cell.dtype == pos.dtype == np.int64
            assert np.array_equal(cell, wcell) and np.array_equal(pos, wpos), (x0, nxl, start, length, flast)
            taken += len(cell)
    assert taken > 0


def test_map_bits_at_equals_map_bits():
    rng = np.random.default_rng(3)
    words = rng.integers(0, 2 ** 32, 40, dtype=np.uint64).astype(np.uint32)
    pos = rng.permutation(40 * 32)
    assert np.array_equal(npd.map_bits_at(words, pos), npd.map_bits(words, 40 * 32)[pos])
    assert npd.map_bits_at(None, pos.reshape(40, 32)).all()


@pytest.mark.parametrize("length,safe,pbc", test_maps_cpu.BOXES)
def test_sparse_create_map_equals_create_map(length, safe, pbc):
    dense = np_maps.create_map(length, safe, pbc)
    words = np_maps.words_of(dense)
    index = np.random.default_rng(1).permutation(len(words))
    assert np.array_equal(np_maps.create_map_words(length, safe, pbc, index), words[index])
    assert np_maps.create_map_count(length, safe, pbc) == int(dense.sum())
    lo, hi = np_maps.box_ranges(length, safe, pbc)
    assert np.array_equal(np_maps.in_ranges(np.arange(dense.size), length, lo, hi), dense.ravel())


@pytest.mark.parametrize("length,safe,pbc", test_maps_cpu.BOXES[:4] + [((96, 80, 72), (6, 6, 6), (False, False, False))])
def test_sparse_update_equals_update_map(length, safe, pbc):
    lo, hi = np_maps.box_ranges(length, safe, pbc)
    cur = np_maps.create_map(length, safe, pbc)
    big = length == (96, 80, 72)
    for seed, count, max_mass in ((sum(length), 40, 3000), (7 + sum(length), 60, 50000 if big else 3000)):      # the groups of tests/test_maps_cpu.py
        pos, mass = test_maps_cpu.groups_for(length, pbc, count, seed=seed, max_mass=max_mass)
        for blf, current, fn in ((2.0, cur, lambda p: np_maps.in_ranges(p, length, lo, hi)), (2.5, np.zeros(length, dtype=bool), None)):
            m = mass.copy()
            for d in range(3):
                if pbc[d]:
                    while max(np_maps.centre_and_size((0, 0, 0), int(v), blf)[1] for v in m) > length[d]:
                        m = np.maximum(m // 2, 1)
            want, nadd = np_maps.update_map(current, pos, m, blf, pbc)
            got, gadd, words = np_maps.update_map_sparse(fn, length, pos, m, blf, pbc)
            assert gadd == nadd and np.array_equal(got, np.flatnonzero(want.ravel()))
            w = np_maps.words_of(want)
            assert sorted(words) == np.flatnonzero(w).tolist() and all(int(w[k]) == v for k, v in words.items())


# ------------------------------------------------------------------------------------------------------------------------
# the device headers, compiled for the host, on the large boxes
def _starts(geom):
    return ((0, 0, 0), geom["wrapped"])


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_neighbour_arithmetic_on_the_large_boxes(neigh_emul, name):
    for periodic in ((False, True) if name == "A" else (False,)):
        s = large_set(name, 0, periodic)
        length, safe, pbc = s["length"], s["safe"], s["pbc"]
        pos, m = s["spos"], len(s["spos"])
        coord = np.zeros((m, 3), dtype=np.int32)
        skip, good = np.zeros(m, dtype=np.uint8), np.zeros(m, dtype=np.uint8)
        row = np.zeros(m, dtype=np.uint32)
        npos = np.zeros((m, 6), dtype=np.uint32)
        wrapped = np.zeros((m, 6), dtype=np.uint8)
        neigh_emul.emul_cells(_i3(length), _i3(pbc), _i3(safe), m, pos.ctypes.data_as(UP), coord.ctypes.data_as(IP), skip.ctypes.data_as(BP),
                              good.ctypes.data_as(BP), row.ctypes.data_as(UP), npos.ctypes.data_as(UP), wrapped.ctypes.data_as(BP))
        i, j, k = npn.coords(pos, length)
        wskip, wgood = npn.skip_good(pos, length, safe, pbc)
        wnpos, wwrapped = npn.neighbour_positions(pos, length, pbc)
        assert np.array_equal(coord, np.stack([i, j, k], axis=1))
        assert np.array_equal(skip.astype(bool), wskip) and np.array_equal(good.astype(bool), wgood)
        assert np.array_equal(row, j + length[1] * i)
        live = ~wskip
        assert np.array_equal(npos[live], wnpos[live]) and np.array_equal(wrapped[live].astype(bool), wwrapped[live])
        assert live.sum() > 1000 and (wnpos[live] >= TWO31).any()
        # both lookups, rank by rank
        nrows = length[0] * length[1]
        rowstart = np.zeros(nrows + 1, dtype=np.uint32)
        neigh_emul.emul_rowstart(_i3(length), m, pos.ctypes.data_as(UP), rowstart.ctypes.data_as(UP))
        assert np.array_equal(rowstart, np.searchsorted(pos, np.arange(nrows + 1, dtype=np.int64) * length[2]))
        want = np.stack([npo.find_location(pos, np.arange(m), wnpos[:, nn]) for nn in range(6)], axis=1)
        want[wskip] = -1
        assert (want >= 0).sum(axis=0).min() >= 1000
        for rs in (rowstart.ctypes.data_as(UP), None):
            rank = np.zeros((m, 6), dtype=np.int64)
            neigh_emul.emul_ranks(_i3(length), _i3(pbc), _i3(safe), m, pos.ctypes.data_as(UP), rs, rank.ctypes.data_as(C.POINTER(C.c_longlong)))
            assert np.array_equal(rank, want), (name, periodic, rs is None)


def slab_planes(geom, where, nxl):
    """x0 of a slab of the sub-box at start (0, 0, 0): on its last planes, or with the plane that holds position 2^31 first"""
    length = geom["length"]
    return length[0] - nxl if where == "last" else TWO31 // (length[1] * length[2])


def back_slabs(geom):
    """(start, nxl, x0): one and two planes on the last x-planes of the sub-box from both starts -- in a direction that is not periodic
    the last plane lies in the safety layer and only the one before it (safe = 1) holds good particles -- and the planes that hold
    position 2^31, well inside"""
    out = [(start, nxl, slab_x0(geom, start, nxl)) for start in ((0, 0, 0), geom["wrapped"]) for nxl in (1, 2)]
    return out + [((0, 0, 0), nxl, slab_planes(geom, "mid", nxl)) for nxl in (1, 2)]


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_back_arithmetic_on_the_large_boxes(back_emul, name):
    geom, s = LARGE[name], large_set(name, 0)
    n, length, safe, pos = geom["n"], geom["length"], geom["safe"], s["pos"]
    count = len(pos)
    rng = np.random.default_rng(17)
    zacc = rng.integers(0, 2 ** 24, count).astype(np.float32)
    gid = rng.integers(0, 2 ** 31, count).astype(np.int32)
    gid[:3] = (2 ** 31 - 1, 0, 1)
    total = []
    for start, nxl, x0 in back_slabs(geom):
        coord, glob = np.zeros((count, 3), dtype=np.int32), np.zeros((count, 3), dtype=np.int32)
        good, taken = np.zeros(count, dtype=np.uint8), np.zeros(count, dtype=np.uint8)
        addr = np.zeros(count, dtype=np.uint64)
        back_emul.emul_cells(n, x0, nxl, _i3(start), _i3(length), _i3(safe), count, pos.ctypes.data_as(UP), coord.ctypes.data_as(IP), good.ctypes.data_as(BP),
                             glob.ctypes.data_as(IP), taken.ctypes.data_as(BP), addr.ctypes.data_as(ULLP))
        c = npb.coords(pos, length)
        assert np.array_equal(coord, np.stack(c, axis=1))
        for d in range(3):
            assert np.array_equal(glob[:, d], (c[d] + start[d]) % n)
        wtaken, wpos = npb.selection(n, x0, nxl, start, length, safe, pos)
        assert np.array_equal(taken.astype(bool), wtaken) and np.array_equal(addr[wtaken].astype(np.int64), wpos[wtaken]) and not addr[~wtaken].any()
        wz, wg, wstored = npb.distribute_back(n, x0, nxl, start, length, safe, pos, zacc, gid)
        for fn in (back_emul.emul_back, back_emul.port_back):
            z, g = npb.fresh(n, nxl)
            stored = fn(n, x0, nxl, _i3(start), _i3(length), _i3(safe), count, pos.ctypes.data_as(UP), zacc.ctypes.data_as(FP), gid.ctypes.data_as(IP),
                        z.ctypes.data_as(FP), g.ctypes.data_as(IP))
            assert stored == wstored and np.array_equal(z, wz) and np.array_equal(g, wg), (name, start, nxl)
        total.append(wstored)
    print(name, "stored per slab", total)
    assert total[1] >= 100 and total[3] >= 100 and total[5] >= 1000       # two planes on the last ones; the block across 2^31


def hashed_columns(n, nxl, dtype=np.float32, rows=24):
    """[rows][nxl n n] integer-valued columns below 2^24 (exact in fp32), different from cell to cell and from column to column"""
    ncell = nxl * n * n
    return ((np.arange(rows * ncell, dtype=np.uint32) * np.uint32(2654435761)) >> np.uint32(8)).astype(dtype).reshape(rows, ncell)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_refresh_arithmetic_on_the_large_boxes(refresh_emul, name):
    geom, s = LARGE[name], large_set(name, 0)
    n, length, safe, pos = geom["n"], geom["length"], geom["safe"], s["pos"]
    count = len(pos)
    cols = hashed_columns(n, 1)
    for start, x0 in (((0, 0, 0), slab_planes(geom, "last", 1)), ((0, 0, 0), slab_planes(geom, "mid", 1)), (geom["wrapped"], slab_x0(geom, geom["wrapped"], 1))):
        coord, glob = np.zeros((count, 3), dtype=np.int32), np.zeros((count, 3), dtype=np.int32)
        found = np.zeros(count, dtype=np.uint8)
        addr = np.zeros(count, dtype=np.uint64)
        refresh_emul.emul_cells(n, x0, 1, _i3(start), _i3(length), _i3(safe), count, pos.ctypes.data_as(UP), coord.ctypes.data_as(IP), glob.ctypes.data_as(IP),
                                found.ctypes.data_as(BP), addr.ctypes.data_as(ULLP))
        wfound, wcell = npr.cells(n, x0, 1, start, length, pos)
        assert np.array_equal(coord, np.stack(npr.coords(pos, length), axis=1))
        assert np.array_equal(found.astype(bool), wfound) and np.array_equal(addr[wfound].astype(np.int64), wcell[wfound]) and not addr[~wfound].any()
        assert wfound.sum() >= 100
        windex, wvel = npr.gather(n, x0, 1, start, length, pos, cols)
        for order in (None, s["ind"]):
            index = np.full(count, 0xDEADBEEF, dtype=np.uint32)
            vel = np.full((count, 24), -7.0, dtype=np.float32)
            got = refresh_emul.emul_gather(n, x0, 1, _i3(start), _i3(length), _i3(safe), count, pos.ctypes.data_as(UP),
                                           order.ctypes.data_as(IP) if order is not None else None, cols.ctypes.data_as(FP), count, index.ctypes.data_as(UP),
                                           vel.ctypes.data_as(FP))
            assert got == len(windex) and np.array_equal(index[:got], windex) and np.array_equal(vel[:got], wvel)
            assert np.all(index[got:] == 0xDEADBEEF)


def spread_group_ids(rng, count):
    """group IDs over [2, 2^31 - 1]: three large groups (one with the largest ID), singletons with IDs of their own, a few loose"""
    gid = np.unique(rng.integers(2, 2 ** 31 - 1, 2 * count, dtype=np.int64))
    gid = rng.permutation(gid)[:count].astype(np.int32)
    r = rng.random(count)
    gid[r < 0.25] = 2 ** 31 - 1
    gid[(r >= 0.25) & (r < 0.45)] = 2
    gid[(r >= 0.45) & (r < 0.6)] = 2 ** 30 + 12345
    gid[(r >= 0.6) & (r < 0.65)] = rng.integers(0, 2, int(((r >= 0.6) & (r < 0.65)).sum()))
    return gid


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_group_velocity_arithmetic_on_the_large_boxes(gv_emul, name):
    geom, s = LARGE[name], large_set(name, 0)
    n, length, safe, pos = geom["n"], geom["length"], geom["safe"], s["pos"]
    count = len(pos)
    rng = np.random.default_rng(23)
    gid = spread_group_ids(rng, count)
    cols = hashed_columns(n, 1, np.float64)
    box = ((0, 0, 0), length, safe)
    for where in ("last", "mid"):
        x0 = slab_planes(geom, where, 1)
        found, loose, counted, cell = npg.classes(n, x0, 1, box[0], length, pos, gid, 2)
        cls = np.zeros(count, dtype=np.uint8)
        gv_emul.emul_classes(n, x0, 1, _i3(box[0]), _i3(length), _i3(safe), count, pos.ctypes.data_as(UP), gid.ctypes.data_as(IP), 2, cls.ctypes.data_as(BP))
        assert np.array_equal(cls, loose * 1 + counted * 2) and counted.sum() >= 100 and loose.sum() >= 1
        want = npg.int_sums(n, x0, 1, box[0], length, pos, gid, 2, cols)
        assert want[1].max() > 10 and (want[1] == 1).sum() > 10 and int(want[0].max()) == 2 ** 31 - 1
        for shape in ((3, 1), (64, 16)):
            g, m, sm, c = test_groupvel_cpu._emul_sums(gv_emul, n, x0, 1, box, pos, gid, 2, cols, shape)
            assert c == counted.sum() and np.array_equal(g, want[0]) and np.array_equal(m, want[1]) and sm.tobytes() == want[2].tobytes(), (name, where, shape)
        # the keys of the counted particles order as (ID, cell), whole IDs and cells come back from them
        idx = np.flatnonzero(counted)
        o = np.lexsort((cell[idx], gid[idx]))
        kg, kc = gid[idx][o].astype(np.uint32), cell[idx][o].astype(np.uint64)
        assert gv_emul.emul_keys(len(idx), kg.ctypes.data_as(UP), kc.ctypes.data_as(ULLP), n * n) == 0


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_distribute_decomposition_on_the_large_boxes(dist_emul, name):
    """one plane with a random map of the whole sub-box (the bit of a cell is looked up at word pos >> 5, up to 2^27 - 1), two planes
    with every bit set"""
    geom = LARGE[name]
    n, length = geom["n"], geom["length"]
    cells = cells_of(length)
    rng = np.random.default_rng(31)
    words = rng.integers(0, TWO32, (cells + 31) // 32, dtype=np.uint32)
    for k, start in enumerate(_starts(geom)):
        for nxl in (1, 2):
            x0 = slab_x0(geom, start, nxl)
            field = npd.random_field(rng, (nxl, n, n), (k + nxl) % 3)
            flast = npd.FLASTS[(2 * k + nxl) % len(npd.FLASTS)]
            mp = words if nxl == 1 else None
            wcell, wpos = npd.contribution_sparse(field, n, x0, start, length, flast, mp)
            nboxes = len(npd.intersection(n, [x0, 0, 0, nxl, n, n], list(start) + list(length)))
            assert len(wpos) > 1000 and wpos.max() >= cells - 2 * length[1] * length[2] and nboxes == (4 if k else 1)
            assert mp is None or int(wpos.max()) >> 5 >= len(words) - 1 - length[1] * length[2] // 32
            cap = len(wcell) + 3
            pos, cell = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
            got = dist_emul.emul_distribute(n, x0, nxl, field.ctypes.data_as(FP), flast, _i3(start), _i3(length),
                                            mp.ctypes.data_as(UP) if mp is not None else None, cap, pos.ctypes.data_as(UP), cell.ctypes.data_as(UP))
            assert got == len(wcell) and np.array_equal(pos[:got], wpos) and np.array_equal(cell[:got], wcell), (name, start, nxl)
    f = np.zeros((1, 4, 4), dtype=np.float32)
    buf = np.zeros(4, dtype=np.uint32).ctypes.data_as(UP)
    assert dist_emul.emul_distribute(2048, 0, 1, f.ctypes.data_as(FP), np.inf, _i3((0, 0, 0)), _i3(TOO_LARGE), None, 0, buf, buf) == -2


def map_groups(length, pbc, seed):
    """groups of sizes 1 .. 40 (boundary_layer_factor 2) centred at the far corner, across position 2^31, and on both faces of every
    periodic direction; at the origin corner too.  -> (pos [G][3], mass [G])"""
    L = [int(v) for v in length]
    rng = np.random.default_rng(seed)
    at31 = [TWO31 // (L[2] * L[1]), (TWO31 // L[2]) % L[1], TWO31 % L[2]]
    centres = [[L[0] - 1, L[1] - 1, L[2] - 1], [L[0] - 9, L[1] - 3, L[2] - 20], at31, [at31[0], at31[1], max(at31[2] - 5, 0)], [0, 0, 0], [3, 1, 30]]
    for d in range(3):
        if pbc[d]:
            for face in (0, 2, L[d] - 1, L[d] - 7):
                c = [L[e] // 2 + int(rng.integers(-20, 20)) for e in range(3)]
                c[d] = face
                centres.append(c)
    sizes = [1, 2, 40, 33] + [int(v) for v in rng.integers(1, 41, len(centres))]
    sizes = sizes[:len(centres)]
    mass = np.array([mass_of_size(sz) for sz in sizes], dtype=np.int32)
    pos = np.array(centres, dtype=np.float64) + rng.uniform(-0.45, 0.45, (len(centres), 3))
    assert [np_maps.centre_and_size(pos[g], mass[g], 2.0) for g in range(len(mass))] == [(list(centres[g]), sizes[g]) for g in range(len(mass))]
    return pos, mass


def mass_of_size(size, blf=2.0):
    """a mass whose sphere has this size: the middle of the masses that give it"""
    lo = 4.188790205 * ((size - 0.5) / blf) ** 3
    hi = 4.188790205 * ((size + 0.5) / blf) ** 3
    return max(1, int((lo + hi) / 2))


@pytest.mark.parametrize("name,periodic", [("A", False), ("A", True), ("B", False), ("C", False)], ids=["A", "A periodic", "B", "C"])
def test_map_arithmetic_on_the_large_boxes(map_emul, name, periodic):
    """periodic: box A with no safety layer -- spheres on all six faces wrap, in z beyond position 2^31"""
    geom = LARGE[name]
    length, safe = geom["length"], (0, 0, 0) if periodic else geom["safe"]
    pbc = pbc_of(safe)
    cells = cells_of(length)
    nwords = (cells + 31) // 32
    map_emul.emul_fill_words.restype = C.c_longlong
    map_emul.emul_fill_words.argtypes = [IP, IP, IP, C.c_size_t, ULLP, UP]
    map_emul.emul_update_sparse.restype = C.c_longlong
    map_emul.emul_update_sparse.argtypes = [IP, IP, C.c_int, C.POINTER(C.c_double), IP, C.c_double, IP, IP, C.c_size_t, ULLP, UP, C.POINTER(C.c_size_t), ULLP,
                                            C.c_int]
    # the fill: the first and last word of 2 10^4 z-rows, the words around 2^31, the ends of the map, 10^5 random words
    rng = np.random.default_rng(41)
    rows = np.unique(np.concatenate([rng.integers(0, length[0] * length[1], 20000), [0, length[0] * length[1] - 1]]))
    index = np.unique(np.concatenate([rows * length[2] // 32, (rows * length[2] + length[2] - 1) // 32, rng.integers(0, nwords, 100000),
                                      [0, nwords - 1, (TWO31 >> 5) - 1, TWO31 >> 5]])).astype(np.uint64)
    mask = np.full(len(index), 0xDEADBEEF, dtype=np.uint32)
    pairs = map_emul.emul_fill_words(_i3(length), _i3(safe), _i3(pbc), len(index), index.ctypes.data_as(ULLP), mask.ctypes.data_as(UP))
    assert pairs > 0, pairs
    want = np_maps.create_map_words(length, safe, pbc, index)
    assert np.array_equal(mask, want) and (want == 0xFFFFFFFF).any() and ((want != 0) & (want != 0xFFFFFFFF)).any()
    assert (want == 0).any() or (pbc[0] and pbc[1])                       # (whole z-rows outside the box: none when x and y are periodic)
    # the spheres, on the filled map and on an empty one, in both forms
    pos, mass = map_groups(length, pbc, seed=43)
    lo, hi = np_maps.box_ranges(length, safe, pbc)
    for current in (lambda p: np_maps.in_ranges(p, length, lo, hi), None):
        wpos, wadd, wwords = np_maps.update_map_sparse(current, length, pos, mass, 2.0, pbc)
        assert (wadd[1] > 0) == (not all(pbc)) and (current is not None or (wadd[0] > len(wpos) > 10000 and wpos.max() == cells - 1 and TWO31 in wpos))
        res = {}
        for words in (1, 0):
            cap = len(wwords) + 5
            ow, om = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint32)
            nout, nadd = C.c_size_t(), (C.c_ulonglong * 2)()
            ors = map_emul.emul_update_sparse(_i3(length), _i3(pbc), len(mass), pos.ctypes.data_as(C.POINTER(C.c_double)), mass.ctypes.data_as(IP), 2.0,
                                              _i3(lo) if current is not None else None, _i3(hi) if current is not None else None, cap, ow.ctypes.data_as(ULLP),
                                              om.ctypes.data_as(UP), C.byref(nout), nadd, words)
            assert ors >= 0, ors
            assert (int(nadd[0]), int(nadd[1])) == wadd and nout.value == len(wwords)
            assert dict(zip(ow[:nout.value].tolist(), om[:nout.value].tolist())) == wwords, (name, words)
            res[words] = ors
        assert res[0] == wadd[0] and (wadd[0] == 0 or res[1] < res[0])


# ------------------------------------------------------------------------------------------------------------------------
# the stand-alone programs under the sanitizers: their mains run A, B and C too ("large box" lines)
SAN = {"back": (test_back_cpu, ["-DBACK_EMUL_MAIN"]), "refresh": (test_refresh_cpu, []), "groupvel": (test_groupvel_cpu, []),
       "map": (test_maps_cpu, ["-DMAP_EMUL_MAIN"])}


@pytest.mark.parametrize("which", sorted(SAN))
def test_the_sanitizer_programs_run_the_large_boxes(which):
    mod, defines = SAN[which]
    if mod._stale(mod.EXE):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"] + defines +
                              ["-o", mod.EXE, mod.SRC])
    out = subprocess.run([mod.EXE], capture_output=True, text=True)
    large = [line for line in out.stdout.splitlines() if line.startswith("large box")]
    print("\n".join(large), out.stderr)
    assert out.returncode == 0 and "MISMATCH" not in out.stdout and "mismatch" not in out.stdout
    assert sorted(line.split()[2] for line in large) == ["A", "B", "C"]
