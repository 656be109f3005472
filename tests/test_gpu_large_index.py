"""The device stages of fragment() at production-size sub-box positions (csrc/pf_organize.hip, pf_neighbours.hip, pf_distribute.hip,
pf_back.hip, pf_refresh.hip, pf_groupvel.hip, pf_map.hip) against the numpy restatements, through the context-free taps: a slab of
one or two planes and 2 10^5 particles are enough to hand a stage positions up to 2^32 - 1, sorts of 21 .. 32 bits and a box of
exactly 2^32 cells.  The boxes, the particle sets and the sparse restatements are those of tests/test_large_index_cpu.py, which pins
them without a device.  Every comparison is exact: positions, indices, flags, counts and bit words are integers, and the floating-point
columns hold integers below 2^24.

The largest device allocation is the map of box B: two arrays of 512 MB.

Not reached from here (they need a context of n^3 cells): the position sort of pf_distribute_sorted (bits_for in pf_organize.hip),
the record gather of k_org_gather beyond 2^32 words, k_peaks<MAP> and pf_select_sorted / pf_get_block at a large global index."""
import ctypes as C
import functools

import numpy as np
import pytest

import np_back as npb
import np_distribute as npd
import np_groupvel as npg
import np_maps
import np_neighbours as npn
import np_organize as npo
import np_refresh as npr
from test_large_index_cpu import (BLOCK, BOX_B, LADDER, LARGE, TOO_LARGE, TWO31, TWO32, back_slabs, block_positions, cells_of, corner_across, fmax_of_kind, hashed_columns,
                                  large_set, map_groups, pbc_of, random_positions, slab_planes, slab_x0, sort_bits, spread_group_ids)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


# ------------------------------------------------------------------------------------------------------------------------
# sort_and_organize: keys over the whole unsigned 32-bit range
@pytest.mark.parametrize("kind", [0, 1, 2], ids=["continuous", "seven values", "zeros infinities nan"])
@pytest.mark.parametrize("name", ["B", "C"])
def test_organize_sorts_positions_up_to_2_32(api, name, kind):
    s = large_set(name, kind)
    order, spos, ind = api.debug_organize(s["f"], s["pos"])
    assert np.array_equal(order, s["order"])
    assert np.array_equal(spos, s["spos"]) and np.array_equal(ind, s["ind"])
    assert int(spos[-1]) == cells_of(s["length"]) - 1 and (spos >= TWO31).mean() >= 0.4


# ------------------------------------------------------------------------------------------------------------------------
# the neighbour table: position sorts of 21 .. 32 bits, rows up to 2048 x 2048, positions on both sides of 2^31
@functools.lru_cache(maxsize=None)
def ladder_case(k):
    """a random fill of 2 10^5 particles of ladder box k in the order after sort_and_organize, and the restatement's table; safe
    changes from box to box: all periodic, none, x and z.  In the large boxes a random fill leaves a few dozen neighbours, and a sort
    that drops the top bit of the positions would go unnoticed: full blocks at both corners and across position 2^(bits - 1), where
    the top bit of the sort sets in, make sure that neighbours are looked up on both sides of it"""
    length, bits = LADDER[k]
    cells = cells_of(length)
    top = 1 << (bits - 1)
    safe = ((0, 0, 0), (1, 2, 3), (0, 2, 0))[k % 3]
    rng = np.random.default_rng(300 + k)
    corners = [(0, 0, 0), tuple(length[d] - BLOCK[d] for d in range(3)), corner_across(length, top)]
    pos = np.unique(np.concatenate([[0, top - 1, top, cells - 1], random_positions(rng, cells, 200000)] + [block_positions(length, c) for c in corners]))
    pos = rng.permutation(pos).astype(np.uint32)
    f = fmax_of_kind(rng, len(pos), k % 3)
    o = npo.order(f)
    pos, f = pos[o], f[o]
    want = npn.neighbours(pos, f, length, safe, pbc_of(safe))
    assert sort_bits(cells) == bits and int(pos.max()) == cells - 1
    beyond = pos >= top                                                       # particles the top bit of the sort places
    found = want[0] >= 0                                                      # ... and lookups that start or end at one of them
    involved = found & (beyond[:, None] | beyond[np.where(found, want[0], 0)])
    assert beyond.sum() >= 500 and involved.sum() >= 500, (length, int(beyond.sum()), int(involved.sum()))
    return pos, f, length, safe, want


def _check_neighbours(api, monkeypatch, pos, f, length, safe, want):
    wneigh, wflags, wpeaks = want
    for form in ("1", "0"):
        monkeypatch.setenv("PF_NEIGH_ROWS", form)
        neigh, flags, peaks = api.neighbours(pos, f, (0, 0, 0), length, safe)
        assert peaks == wpeaks, (length, form)
        assert np.array_equal(flags, wflags) and np.array_equal(neigh, wneigh), (length, form)
    print(length, safe, "peaks", wpeaks, "found per direction", (wneigh >= 0).sum(axis=0).tolist())


@pytest.mark.parametrize("k", range(len(LADDER)), ids=["x".join(map(str, length)) for length, _ in LADDER])
def test_neighbours_on_the_ladder_of_sort_widths(api, monkeypatch, k):
    pos, f, length, safe, want = ladder_case(k)
    assert (want[0] >= 0).any() and want[2][0] > 0
    _check_neighbours(api, monkeypatch, pos, f, length, safe, want)


@pytest.mark.parametrize("name,periodic", [("A", False), ("A", True), ("B", False), ("C", False)], ids=["A", "A periodic", "B", "C"])
def test_neighbours_on_the_large_boxes(api, monkeypatch, name, periodic):
    s = large_set(name, 2 if name == "C" else 1 if name == "B" else 0, periodic)
    o = s["order"]
    _check_neighbours(api, monkeypatch, s["pos"][o], s["f"][o], s["length"], s["safe"], (s["neigh"], s["flags"], s["peaks"]))


# ------------------------------------------------------------------------------------------------------------------------
# distribute: frag_pos up to 2^32 - 1 from a slab on the last x-planes of the sub-box
def _check_distribute(api, n, x0, field, start, length, flast, words=None, capacity=False):
    wcell, wpos = npd.contribution_sparse(field, n, x0, start, length, flast, words)
    pos, cell, count = api.debug_distribute(field, x0, flast, start, length, map=words)
    assert count == len(wpos), (start, length, flast)
    assert np.array_equal(pos, wpos) and np.array_equal(cell, wcell), (start, length, flast)
    if capacity and count > 3:
        cap = count // 3
        pos, cell, count = api.debug_distribute(field, x0, flast, start, length, map=words, capacity=cap)
        assert count == len(wpos) and len(pos) == len(cell) == cap and np.array_equal(pos, wpos[:cap]) and np.array_equal(cell, wcell[:cap])
    return count, int(wpos.max()) if count else -1


@pytest.mark.parametrize("nxl", [1, 2])
@pytest.mark.parametrize("wrapped", [False, True], ids=["straight", "wrapped"])
@pytest.mark.parametrize("name", ["B", "C"])
def test_distribute_to_the_last_planes_of_a_large_sub_box(api, name, wrapped, nxl):
    geom = LARGE[name]
    n, length = geom["n"], geom["length"]
    start = geom["wrapped"] if wrapped else (0, 0, 0)
    x0 = slab_x0(geom, start, nxl)
    nboxes = len(npd.intersection(n, [x0, 0, 0, nxl, n, n], list(start) + list(length)))
    assert nboxes == (4 if wrapped else 1)                                   # y and z wrap; x lies in its wrapped segment alone
    rng = np.random.default_rng(500 + 10 * nxl + wrapped + ord(name))
    seen = []
    for kind in (0, 1, 2):
        field = npd.random_field(rng, (nxl, n, n), kind)
        for flast in ((-np.inf, np.inf), (1.75, float(np.nextafter(1.0, 2.0))), (0.0, 1.0))[kind]:
            seen.append(_check_distribute(api, n, x0, field, start, length, flast, capacity=(kind == 1 and flast == 1.75)))
    print(name, start, nxl, "(count, largest frag_pos):", seen)
    assert max(c for c, _ in seen) == nxl * length[1] * length[2]          # Flast = -inf takes every cell of the planes
    assert max(p for _, p in seen) == cells_of(length) - 1 and min(c for c, _ in seen) == 0


def test_distribute_with_a_map_of_67_million_words(api):
    geom = LARGE["A"]
    n, length = geom["n"], geom["length"]
    rng = np.random.default_rng(77)
    words = rng.integers(0, TWO32, (cells_of(length) + 31) // 32, dtype=np.uint32)
    assert len(words) > 67000000
    for start, nxl in (((0, 0, 0), 2), (geom["wrapped"], 1)):
        x0 = slab_x0(geom, start, nxl)
        field = npd.random_field(rng, (nxl, n, n), 0)
        count, largest = _check_distribute(api, n, x0, field, start, length, 1.0, words=words)
        print("A", start, nxl, "count", count, "largest frag_pos", largest)
        assert count > 100000 and largest >= TWO31


# ------------------------------------------------------------------------------------------------------------------------
# distribute_back: the same geometries, the particle sets, zacc and group_ID up to 2^31 - 1
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_distribute_back_from_a_large_sub_box(api, name):
    geom, s = LARGE[name], large_set(name, 0)
    n, length, safe, pos = geom["n"], geom["length"], geom["safe"], s["pos"]
    rng = np.random.default_rng(17)
    zacc = rng.integers(0, 2 ** 24, len(pos)).astype(np.float32)
    zacc[:2] = (float(2 ** 31 - 128), -1.0)                                    # (the largest fp32 below 2^31)
    gid = rng.integers(0, 2 ** 31, len(pos)).astype(np.int32)
    gid[:3] = (2 ** 31 - 1, 0, 1)
    stored = []
    for start, nxl, x0 in back_slabs(geom):
        wz, wg, wstored = npb.distribute_back(n, x0, nxl, start, length, safe, pos, zacc, gid)
        z, g, got = api.distribute_back(n, x0, nxl, start, length, safe, pos, zacc, gid)
        assert got == wstored and np.array_equal(z, wz) and np.array_equal(g, wg), (name, start, nxl, x0)
        stored.append(got)
    print(name, "stored per slab", stored)
    assert stored[1] >= 100 and stored[3] >= 100 and stored[5] >= 1000


# ------------------------------------------------------------------------------------------------------------------------
# the velocity gather and the group sums: box C in a box of 1632^3
N_C = 1632


@functools.lru_cache(maxsize=1)
def _columns(nxl, pb):
    return hashed_columns(N_C, nxl, np.float32 if pb == 4 else np.float64)


def _c_box():
    geom = dict(LARGE["C"], n=N_C)
    return geom, ((0, 0, 0), geom["length"], geom["safe"])


@pytest.mark.parametrize("pb", [4, 8])
@pytest.mark.parametrize("nxl", [1, 2])
def test_gather_velocities_of_a_large_sub_box(api, nxl, pb):
    geom, box = _c_box()
    s = large_set("C", 0)
    cols = _columns(nxl, pb)
    for where in ("last", "mid"):
        x0 = slab_planes(geom, where, nxl)
        for order in (None, s["ind"]):
            pos = s["pos"] if order is None else s["pos"][s["order"]]           # indices[] belongs to the sorted order
            windex, wvel = npr.gather(N_C, x0, nxl, box[0], box[1], pos, cols)
            index, vel = api.debug_gather_velocities(N_C, x0, cols, box, pos, order=order)
            assert len(windex) >= 100 * nxl and vel.dtype == cols.dtype
            assert np.array_equal(index, windex) and np.array_equal(vel, wvel), (where, order is None)


@pytest.mark.parametrize("pb", [4, 8])
@pytest.mark.parametrize("nxl", [1, 2])
def test_group_velocity_sums_of_a_large_sub_box(api, nxl, pb):
    geom, box = _c_box()
    s = large_set("C", 0)
    cols = _columns(nxl, pb)
    gid = spread_group_ids(np.random.default_rng(23), len(s["pos"]))
    for where in ("last", "mid"):
        x0 = slab_planes(geom, where, nxl)
        wgroup, wnpart, wsum = npg.int_sums(N_C, x0, nxl, box[0], box[1], s["pos"], gid, 2, cols)
        group, npart, sums, counted = api.debug_group_velocity_sums(N_C, x0, cols, box, s["pos"], gid)
        assert wnpart.max() > 10 and (wnpart == 1).sum() > 10 and int(wgroup.max()) == 2 ** 31 - 1 and int(wgroup.min()) == 2
        assert counted == int(wnpart.sum()) and np.array_equal(group, wgroup) and np.array_equal(npart, wnpart)
        assert sums.tobytes() == wsum.tobytes(), where


# ------------------------------------------------------------------------------------------------------------------------
# the maps without a context
def _check_words(m, which, wwords, sample):
    """the whole array: the words the restatement names hold its masks, `sample` of the others are zero, and the bit count is its"""
    w = m.words(which)
    keys = np.fromiter(wwords.keys(), dtype=np.int64, count=len(wwords))
    vals = np.fromiter(wwords.values(), dtype=np.uint64, count=len(wwords)).astype(np.uint32)
    assert np.array_equal(w[keys], vals)
    rest = np.setdiff1d(sample, keys)
    assert not w[rest].any()
    return w


@pytest.mark.parametrize("periodic", [False, True], ids=["safe 1 3 3", "periodic"])
def test_map_of_box_a(api, monkeypatch, periodic):
    """periodic: the box with no safety layer.  The groups on its six faces wrap -- in z beyond position 2^31 -- and create_map sets
    every bit, so that nothing is left to request beside it; the update on the empty map is the one that places wrapped cells"""
    geom = LARGE["A"]
    length, safe = geom["length"], (0, 0, 0) if periodic else geom["safe"]
    pbc = pbc_of(safe)
    cells = cells_of(length)
    nwords = (cells + 31) // 32
    rng = np.random.default_rng(41)
    rows = np.arange(length[0] * length[1], dtype=np.int64)                    # the first and last word of every z-row
    index = np.unique(np.concatenate([rows * length[2] // 32, (rows * length[2] + length[2] - 1) // 32, rng.integers(0, nwords, 100000),
                                      [0, nwords - 1, (TWO31 >> 5) - 1, TWO31 >> 5]]))
    box_words = np_maps.create_map_words(length, safe, pbc, index)
    box_count = np_maps.create_map_count(length, safe, pbc)
    pos, mass = map_groups(length, pbc, seed=43)
    lo, hi = np_maps.box_ranges(length, safe, pbc)
    wpos, wadd, wwords = np_maps.update_map_sparse(lambda p: np_maps.in_ranges(p, length, lo, hi), length, pos, mass, 2.0, pbc)
    epos, eadd, ewords = np_maps.update_map_sparse(None, length, pos, mass, 2.0, pbc)
    assert eadd[0] > len(epos) > 10000 and int(epos.max()) == cells - 1 and TWO31 in epos
    if periodic:
        assert box_count == cells and wadd == (0, 0) and eadd[1] == 0 and len(mass) == 6 + 12
        # the cells that only a wrap reaches (without periodic directions they fall outside) lie on both sides of 2^31
        wrapped = np.setdiff1d(epos, np_maps.update_map_sparse(None, length, pos, mass, 2.0, (False, False, False))[0])
        assert (wrapped < TWO31).sum() >= 1000 and (wrapped >= TWO31).sum() >= 1000
    else:
        assert wadd[1] > 0 and len(wpos) > 1000
    keys = np.fromiter(wwords.keys(), dtype=np.int64, count=len(wwords))
    vals = np.fromiter(wwords.values(), dtype=np.uint64, count=len(wwords)).astype(np.uint32)
    results = []
    for form in ("1", "0"):                                                   # PF_MAP_WORDS is read when a map is created
        monkeypatch.setenv("PF_MAP_WORDS", form)
        with api.FragMap((0, 0, 0), length, safe) as m:
            assert m.nwords == nwords
            # an empty CURRENT: every sphere cell inside the box is requested
            assert m.update(pos, mass, 2.0) == eadd
            assert m.count("update") == len(epos) and m.count("current") == 0
            w_empty = _check_words(m, "update", ewords, index)
            # create_map, turn 0
            m.fill_box()
            assert m.count("update") == box_count
            assert np.array_equal(m.words("update")[index], box_words)
            m.commit(False)
            assert m.count("current") == box_count
            # the spheres beside the box
            assert m.update(pos, mass, 2.0) == wadd
            assert m.count("update") == len(wpos) and m.count("current") == box_count
            w_upd = _check_words(m, "update", wwords, index)
            # turn 1: frag_map |= frag_map_update (update never holds a bit of CURRENT)
            m.commit(True)
            assert m.count("current") == box_count + len(wpos)
            cur = m.words("current")
            merged = box_words.copy()
            at = np.searchsorted(index, keys)
            hit = (at < len(index)) & (index[np.minimum(at, len(index) - 1)] == keys)
            np.bitwise_or.at(merged, at[hit], vals[hit])
            assert np.array_equal(cur[index], merged) and np.array_equal(cur[keys] & w_upd[keys], w_upd[keys])
            m.commit(False)
            assert m.count("current") == len(wpos)
            results.append((w_empty, w_upd))
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])     # both forms, word for word


def test_map_of_box_b_update_and_count(api, monkeypatch):
    """x and y periodic: the groups on those faces wrap, and the far corner is the last bit of the last word.  Every touched word is
    compared, in both forms; the bit count says that no other word is set"""
    geom = LARGE["B"]
    length, safe = geom["length"], geom["safe"]
    pbc = pbc_of(safe)
    pos, mass = map_groups(length, pbc, seed=47)
    epos, eadd, ewords = np_maps.update_map_sparse(None, length, pos, mass, 2.0, pbc)
    assert int(epos.max()) == TWO32 - 1 and int(epos.min()) == 0 and TWO31 in epos
    wrapped = np.setdiff1d(epos, np_maps.update_map_sparse(None, length, pos, mass, 2.0, (False, False, False))[0])
    assert (wrapped < TWO31).sum() >= 1000 and (wrapped >= TWO31).sum() >= 1000
    sample = np.random.default_rng(48).integers(0, 1 << 27, 100000)
    for form in ("1", "0"):
        monkeypatch.setenv("PF_MAP_WORDS", form)
        with api.FragMap((0, 0, 0), length, safe) as m:
            assert m.nwords == 1 << 27
            assert m.update(pos, mass, 2.0) == eadd
            assert m.count("update") == len(epos) and m.count("current") == 0
            _check_words(m, "update", ewords, sample)
            m.fill_box()
            assert m.count("update") == np_maps.create_map_count(length, safe, pbc) == 2048 * 2048 * 1020


# ------------------------------------------------------------------------------------------------------------------------
# the edge: 2^32 cells are accepted (every test above on box B), one z-plane more is refused before anything is launched
def test_a_box_of_more_than_2_32_cells_is_refused_by_every_stage(api):
    from pinocchio_amd import _lib
    L = _lib.load()
    pos = np.array([0, 5, 77], dtype=np.uint32)
    f = np.array([3.0, 2.0, 1.0], dtype=np.float32)
    gid = np.array([2, 2, 3], dtype=np.int32)
    safe = (0, 0, 1)
    box = ((0, 0, 0), TOO_LARGE, safe)
    assert cells_of(TOO_LARGE) == TWO32 + 2048 * 2048
    with pytest.raises(api.PinfmaxError, match=r"pf_neighbours: a sub-box of more than 2\^32 cells"):
        api.neighbours(pos, f, (0, 0, 0), TOO_LARGE, safe)
    with pytest.raises(api.PinfmaxError, match=r"pf_map_create: a sub-box of more than 2\^32 cells"):
        api.FragMap((0, 0, 0), TOO_LARGE, safe)
    slab = np.zeros((1, 2048, 2048), dtype=np.float32)
    with pytest.raises(api.PinfmaxError, match=r"pf_debug_distribute: a sub-box of more than 2\^32 cells"):
        api.debug_distribute(slab, 0, 0.0, (0, 0, 0), TOO_LARGE)
    with pytest.raises(api.PinfmaxError, match=r"pf_debug_distribute_back: a sub-box of more than 2\^32 cells"):
        api.distribute_back(2048, 0, 1, (0, 0, 0), TOO_LARGE, safe, pos, f, gid)
    cols = np.zeros((24, 2048 * 2048), dtype=np.float32)
    with pytest.raises(api.PinfmaxError, match=r"pf_debug_gather_velocities: a sub-box of more than 2\^32 cells"):
        api.debug_gather_velocities(2048, 0, cols, box, pos)
    with pytest.raises(api.PinfmaxError, match=r"pf_debug_group_velocity_sums: a sub-box of more than 2\^32 cells"):
        api.debug_group_velocity_sums(2048, 0, cols, box, pos, gid)
    # box B itself through the two taps that the tests above run on box C
    bbox = ((0, 0, 0), BOX_B, LARGE["B"]["safe"])
    far = np.array([TWO32 - 1, TWO32 - 1024, 0], dtype=np.uint32)             # the last cell and the first of its z-row: plane 2047
    found, cell = npr.cells(2048, 2047, 1, bbox[0], BOX_B, far)
    assert found.tolist() == [True, True, False] and cell[:2].tolist() == [1023 + 2048 * 2047, 2048 * 2047]
    cols = hashed_columns(2048, 1)
    index, vel = api.debug_gather_velocities(2048, 2047, cols, bbox, far)
    assert index.tolist() == [0, 1] and np.array_equal(vel, cols[:, cell[:2]].T)
    group, npart, sums, counted = api.debug_group_velocity_sums(2048, 2047, cols, bbox, far, gid)
    assert group.tolist() == [2] and npart.tolist() == [2] and counted == 2
    assert np.array_equal(sums[0], cols[:, cell[0]].astype(np.float64) + cols[:, cell[1]])
    # the slab: cell_index and the keys of the group sums hold a cell index below 2^32, so 2^32 cells are the limit of both taps and
    # 1025 planes of 2048^2 are refused (before the slab, which is not there, is read)
    sub = _lib.SubBox((C.c_int * 3)(0, 0, 0), (C.c_int * 3)(8, 8, 8))
    cnt = C.c_size_t()
    assert L.pf_debug_distribute(2048, 0, 1025, slab.ctypes.data_as(C.POINTER(C.c_float)), 0.0, C.byref(sub), None, 0, None, None, C.byref(cnt)) != 0
    assert "pf_debug_distribute: a slab of 4299161600 cells" in L.pf_last_error().decode()
    rg = api._region(((0, 0, 0), (8, 8, 8), (1, 1, 1)))
    ng, npc = C.c_size_t(), C.c_size_t()
    assert L.pf_debug_group_velocity_sums(2048, 0, 1025, 4, cols.ctypes.data_as(C.c_void_p), C.byref(rg), 3, pos.ctypes.data_as(C.POINTER(C.c_uint)),
                                          gid.ctypes.data_as(C.POINTER(C.c_int)), 2, None, None, None, C.byref(ng), C.byref(npc)) != 0
    assert "pf_debug_group_velocity_sums: a slab of 4299161600 cells" in L.pf_last_error().decode()
