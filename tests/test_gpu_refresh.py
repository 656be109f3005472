"""The velocity refresh of a redshift segment on the device (pf_shift_displacements, pf_drop_prev, pf_gather_velocities,
pf_refresh_velocities, pf_debug_gather_velocities; csrc/pf_refresh.hip) against the numpy restatement of the reference's loop
(tests/np_refresh.py, pinned on the CPU by tests/test_refresh_cpu.py).  Values are copied, never computed: every comparison is exact."""
import ctypes as C
import functools

import numpy as np
import pytest

import np_refresh as npr
from pinocchio_amd import synth
from test_gpu_multirank import run_ranks

pytestmark = pytest.mark.gpu

RADII = np.array([2.0, 1.0, 0.5, 0.0])
G1 = synth.growth_multipliers()
G2 = G1 * np.array([0.75, 0.5, 0.625, 0.875])       # another redshift: every order moves, by factors a float multiplies exactly
G3 = G1 * np.array([0.5, 0.25, 0.375, 0.125])


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


# (n, x0, nxl, start, len, safe)
TAP = {"whole": (16, 0, 16, (0, 0, 0), (16, 16, 16), (0, 0, 0)),
       "wraps in x and z": (16, 0, 16, (-3, 0, 13), (7, 16, 5), (1, 0, 1)),
       "two x-ranges, one hits": (16, 4, 4, (14, 0, 2), (9, 16, 5), (2, 0, 2)),
       "misses the slab": (16, 8, 4, (14, 0, 2), (9, 16, 5), (2, 0, 2)),
       "24 whole": (24, 0, 24, (0, 0, 0), (24, 24, 24), (0, 0, 0)),
       "24 slab": (24, 21, 3, (20, 3, 0), (9, 5, 24), (2, 1, 0)),
       "boundary layer": (16, 0, 16, (3, 4, 5), (8, 7, 6), (2, 2, 2))}


@functools.lru_cache(maxsize=None)
def _cols(n, nxl, dtype="f4"):
    """cols24[c][cell] = c 2^20 + cell as floats: the value names its column and its cell (computed once, shared, left alone).  As
    doubles a 2^-30 is added, which no float holds"""
    nc = nxl * n * n
    c = (np.arange(24, dtype=np.int64)[:, None] * 2 ** 20 + np.arange(nc, dtype=np.int64)[None, :]).astype(dtype)
    if dtype == "f8":
        c += 2.0 ** -30
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _positions(name, count=None):
    """positions of the box in random order with duplicates among them (count None: 1.2 positions per cell)"""
    length = TAP[name][4]
    ncells = length[0] * length[1] * length[2]
    rng = np.random.default_rng(sum(length) + 31 * TAP[name][0])
    pos = rng.integers(0, ncells, int(1.2 * ncells) if count is None else count).astype(np.uint32)
    pos.setflags(write=False)
    return pos


def _tap(api, name, pos, order=None, dtype="f4"):
    n, x0, nxl, start, length, safe = TAP[name]
    cols = _cols(n, nxl, dtype)
    got = api.debug_gather_velocities(n, x0, cols, (start, length, safe), pos, order)
    want = npr.gather(n, x0, nxl, start, length, pos, cols)
    return got, want


def _same(got, want):
    return (got[0].dtype == np.uint32 and np.array_equal(got[0], want[0]) and got[1].dtype == want[1].dtype and got[1].shape == want[1].shape
            and got[1].tobytes() == want[1].tobytes())


# ------------------------------------------------------------------------------------------------------------------------
# the context-free tap on prescribed columns
@pytest.mark.parametrize("name", ["whole", "wraps in x and z", "two x-ranges, one hits", "misses the slab", "24 whole", "24 slab"])
def test_the_tap_equals_the_restatement(api, name):
    pos = _positions(name)
    assert len(np.unique(pos)) < len(pos)                      # duplicates
    got, want = _tap(api, name, pos)
    assert _same(got, want)
    if name == "misses the slab":
        assert len(got[0]) == 0
    elif name in ("whole", "wraps in x and z", "24 whole"):
        assert np.array_equal(got[0], np.arange(len(pos)))      # the slab is the box: every particle, in its order
    else:
        assert 0 < len(got[0]) < len(pos)
    # the order changes which thread serves which particle and nothing else: a random one, and the true position order
    rng = np.random.default_rng(3)
    for order in (rng.permutation(len(pos)), np.argsort(pos, kind="stable")):
        assert _same(_tap(api, name, pos, order.astype(np.int32))[0], want), name


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 777])
def test_the_tap_on_odd_counts(api, count):
    # 777: three workgroups of 256 and nine particles
    for name in ("wraps in x and z", "two x-ranges, one hits"):
        pos = _positions(name, count)
        got, want = _tap(api, name, pos)
        assert _same(got, want), name
        got, _ = _tap(api, name, pos, np.argsort(pos, kind="stable").astype(np.int32))
        assert _same(got, want), name


def test_the_tap_finds_the_boundary_layer(api):
    """safe = (2, 2, 2) in a box without a periodic direction: 8 x 7 x 6 cells of which 4 x 3 x 2 are good.  Every particle has
    velocities (the good_particle test of distribute_back has no place here)"""
    name = "boundary layer"
    n, x0, nxl, start, length, safe = TAP[name]
    pos = np.arange(8 * 7 * 6, dtype=np.uint32)
    got, want = _tap(api, name, pos)
    assert _same(got, want) and len(got[0]) == 336
    i, j, k = npr.coords(pos, length)
    good = (i >= 2) & (i < 6) & (j >= 2) & (j < 5) & (k >= 2) & (k < 4)
    assert good.sum() == 24 and np.array_equal(got[0][~good], pos[~good])
    # the corner (0, 0, 0) of the box is cell (3, 4, 5)
    assert got[1][0, 0] == 5 + 16 * (4 + 16 * 3) and got[1][0, 12] == 12 * 2 ** 20 + 5 + 16 * (4 + 16 * 3)


def test_the_tap_on_double_columns(api):
    for name in ("wraps in x and z", "24 slab"):
        pos = _positions(name)
        got, want = _tap(api, name, pos, dtype="f8")
        assert got[1].dtype == np.float64 and _same(got, want) and len(got[0])
        assert np.any(got[1].astype(np.float32) != got[1])
        got, _ = _tap(api, name, pos, np.argsort(pos, kind="stable").astype(np.int32), dtype="f8")
        assert _same(got, want)


# ------------------------------------------------------------------------------------------------------------------------
# with a context
BOX16 = ((-3, 0, 13), (7, 16, 5), (1, 0, 1))


def _first_segment(f, dk, order=3):
    f.set_density(dk)
    f.set_invgrow(*synth.invgrow_table("lcdm"))
    f.set_lpt_order(order)
    f.sweep(RADII)
    f.set_growth(G1)
    f.compute_displacements(1, 0)


def _next_segment(f, g):
    """fragment.c:398-410: shift_all_displacements(); compute_displacements(0, 0, z)"""
    f.shift_displacements()
    f.set_growth(g)
    f.compute_displacements(0, 0)


def _cols_of(*products):
    """the 24 columns of a slab from its records: the Vel* of the first argument, then those of the second"""
    out = []
    for p in products:
        p = p.reshape(-1)
        for name in ("Vel", "Vel_2LPT", "Vel_3LPT_1", "Vel_3LPT_2"):
            out += [np.ascontiguousarray(p[name][:, e]) for e in range(3)]
    return np.stack(out)


def _layout(stride, rmax, fmax, vel):
    from pinocchio_amd import _lib
    return _lib.ProductLayout(stride, rmax, fmax, *vel)


def _bytes_equal(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def test_two_segments_on_one_rank(api):
    n = 16
    start, length, safe = BOX16
    lay = _layout(104, 0, 4, (8, 20, 32, 44))                  # product_data of -DRECOMPUTE_DISPLACEMENTS (src/pinocchio.h:233-259)
    prev = api.prev_layout(56, 68, 80, 92)
    with api.Fmax(n) as f:
        _first_segment(f, synth.make_density(n, seed=5))
        A = f.products()
        assert f.prev_shifts == 0
        held = f.device_bytes
        f.shift_displacements()
        assert f.prev_shifts == 1 and f.device_bytes == held + 48 * n ** 3
        assert _bytes_equal(f.products(), A)                   # a copy: Vel == Vel_prev until the next displacements
        f.set_growth(G2)
        f.compute_displacements(0, 0)
        B = f.products()
        for name in ("Vel", "Vel_2LPT", "Vel_3LPT_1", "Vel_3LPT_2"):
            assert np.any(B[name] != A[name]) and np.any(A[name] != 0), name
        assert _bytes_equal(B["Fmax"], A["Fmax"]) and _bytes_equal(B["Rmax"], A["Rmax"])
        flast = float(np.median(A["Fmax"]))
        rec, pos, spos, ind, count = f.distribute_sorted(flast, start, length, layout=lay)
        assert count == len(pos) > 100 and rec.shape == (count, 104) and not rec[:, 56:].any()
        found, cell = npr.cells(n, 0, n, start, length, pos)
        assert found.all()
        # what distribute has just delivered: Vel* = B of the record's cell
        Bc, Ac = B.reshape(-1)[cell], A.reshape(-1)[cell]
        names = (("Vel", 8), ("Vel_2LPT", 20), ("Vel_3LPT_1", 32), ("Vel_3LPT_2", 44))
        for name, off in names:
            assert _bytes_equal(rec[:, off:off + 12], Bc[name]), name
        # the compact form: both sets
        index, vel = f.gather_velocities(BOX16, pos)
        assert _same((index, vel), npr.gather(n, 0, n, start, length, pos, _cols_of(B, A)))
        assert _same(f.gather_velocities(BOX16, pos, order=ind), (index, vel))
        # in place.  The Vel* fields are cleared and the spare bytes filled with a pattern first
        work = rec.copy()
        work[:, 8:56] = 0
        work[:, 56:] = 0xA5
        before = work.copy()
        assert f.refresh_velocities(BOX16, pos, work, lay) == count                        # prev = None: a plain Vel* refresh
        assert _bytes_equal(work[:, :56], rec[:, :56]) and np.all(work[:, 56:] == 0xA5)
        assert np.all(before[:, 56:] == 0xA5)
        assert f.refresh_velocities(BOX16, pos, work, lay, prev, order=ind) == count
        assert _bytes_equal(work[:, :56], rec[:, :56])                                     # Rmax, Fmax untouched, Vel* = B
        for (name, _), off in zip(names, (56, 68, 80, 92)):
            assert _bytes_equal(work[:, off:off + 12], Ac[name]), name
        assert _bytes_equal(work, npr.scatter(before, index, vel, (8, 20, 32, 44), (56, 68, 80, 92)))
        # records with spare bytes around the fields, two of the eight fields named
        lay2 = _layout(112, -1, -1, (-1, 12, -1, -1))
        work2 = np.full((count, 112), 0x5A, dtype=np.uint8)
        assert f.refresh_velocities(BOX16, pos, work2, lay2, api.prev_layout(off_Vel_3LPT_2_prev=96)) == count
        assert _bytes_equal(work2, npr.scatter(np.full((count, 112), 0x5A, dtype=np.uint8), index, vel, (-1, 12, -1, -1), (-1, -1, -1, 96)))
        assert np.all(work2[:, :12] == 0x5A) and np.all(work2[:, 24:96] == 0x5A) and np.all(work2[:, 108:] == 0x5A)
        # a third segment: prev = B
        _next_segment(f, G3)
        assert f.prev_shifts == 2 and f.device_bytes == held + 48 * n ** 3
        D = f.products()
        assert np.any(D["Vel"] != B["Vel"])
        assert _same(f.gather_velocities(BOX16, pos, order=ind), npr.gather(n, 0, n, start, length, pos, _cols_of(D, B)))


@pytest.mark.parametrize("order", [1, 2])
def test_lower_lpt_orders(api, order):
    n = 16
    start, length, safe = BOX16
    pos = _positions("wraps in x and z")
    with api.Fmax(n) as f:
        _first_segment(f, synth.make_density(n, seed=6), order)
        A = f.products()
        _next_segment(f, G2)
        B = f.products()
        index, vel = f.gather_velocities(BOX16, pos)
        assert _same((index, vel), npr.gather(n, 0, n, start, length, pos, _cols_of(B, A)))
        kmax = {1: 3, 2: 6}[order]                               # columns 3 o .. 3 o + 2 of order o: Zel'dovich, 2LPT
        assert vel[:, :kmax].any() and vel[:, 12:12 + kmax].any() and np.any(vel[:, :3] != vel[:, 12:15])
        assert not vel[:, kmax:12].any() and not vel[:, 12 + kmax:].any()           # the slots of the orders that are not computed
        # absent offsets: those fields keep their bytes
        lay = _layout(104, 0, 4, (8, 20, -1, -1) if order == 2 else (8, -1, -1, -1))
        prev = api.prev_layout(56, 68) if order == 2 else api.prev_layout(56)
        work = np.full((len(pos), 104), 0xA5, dtype=np.uint8)
        assert f.refresh_velocities(BOX16, pos, work, lay, prev) == len(pos)
        off_cur = (8, 20, -1, -1) if order == 2 else (8, -1, -1, -1)
        off_prev = (56, 68, -1, -1) if order == 2 else (56, -1, -1, -1)
        assert _bytes_equal(work, npr.scatter(np.full((len(pos), 104), 0xA5, dtype=np.uint8), index, vel, off_cur, off_prev))
        assert np.all(work[:, 32:56] == 0xA5) and np.all(work[:, 80:] == 0xA5) and np.all(work[:, :8] == 0xA5)


def test_double_products(api):
    n = 16
    start, length, safe = BOX16
    with api.Fmax(n, double_products=True) as f:
        _first_segment(f, synth.make_density(n, seed=7))
        A = f.products()
        held = f.device_bytes
        _next_segment(f, G2)
        assert f.device_bytes == held + 96 * n ** 3
        B = f.products()
        assert A["Vel"].dtype == np.float64 and np.any(B["Vel"].astype(np.float32) != B["Vel"])
        lay = _layout(200, -1, 0, (8, 32, 56, 80))               # 25 doubles: Fmax, Vel*, Vel*_prev
        rec, pos, spos, ind, count = f.distribute_sorted(float(np.median(A["Fmax"])), start, length, layout=lay)
        assert count > 100 and rec.shape == (count, 200)
        index, vel = f.gather_velocities(BOX16, pos, order=ind)
        assert vel.dtype == np.float64 and _same((index, vel), npr.gather(n, 0, n, start, length, pos, _cols_of(B, A)))
        work = rec.copy()
        work[:, 8:] = 0xA5
        assert f.refresh_velocities(BOX16, pos, work, lay, api.prev_layout(104, 128, 152, 176)) == count
        assert _bytes_equal(work[:, :104], rec[:, :104])
        assert _bytes_equal(work, npr.scatter(rec, index, vel, (8, 32, 56, 80), (104, 128, 152, 176)))


@functools.lru_cache(maxsize=None)
def _one_rank(order):
    """the two segments on one rank (computed once, shared, left alone) -> (A, B) whole boxes"""
    from pinocchio_amd import api as _api
    n = 16
    with _api.Fmax(n) as f:
        _first_segment(f, synth.make_density(n, seed=8), order)
        A = f.products()
        _next_segment(f, G2)
        return A, f.products()


@pytest.mark.parametrize("P", [1, 2, 4])
def test_every_rank_finds_its_own(api, P):
    """P ranks on one GPU through the in-process fabric; each rank's call finds the particles of its slab.  At LPT order 2 every
    column is the one-rank context's bit for bit (tests/test_gpu_multirank.py), so the values are held against that context; at
    order 3 the 3LPT(b) columns depend on the decomposition in the last bit, and the values are held against the ranks' own products"""
    n = 16
    nxl = n // P
    dk = synth.make_density(n, seed=8)
    for name in ("whole", "wraps in x and z"):
        _, _, _, start, length, safe = TAP[name]
        pos = _positions(name)
        box = (start, length, safe)
        order_of_pos = np.argsort(pos, kind="stable").astype(np.int32)
        for lpt in (2, 3):
            def body(f, r):
                _first_segment(f, dk[r * nxl:(r + 1) * nxl], lpt)
                A = f.products()
                _next_segment(f, G2)
                B = f.products()
                return A, B, f.gather_velocities(box, pos), f.gather_velocities(box, pos, order=order_of_pos)

            if P == 1:
                with api.Fmax(n) as f1:
                    res = [body(f1, 0)]
            else:
                res = run_ranks(api, n, P, body)
            whole = npr.gather(n, 0, n, start, length, pos, _cols_of(np.concatenate([r[1] for r in res]), np.concatenate([r[0] for r in res])))
            assert np.array_equal(whole[0], np.arange(len(pos)))
            seen = np.zeros(len(pos), dtype=int)
            for r, (A, B, got, got_ordered) in enumerate(res):
                assert _same(got, npr.gather(n, r * nxl, nxl, start, length, pos, _cols_of(B, A))), (name, lpt, r)
                assert _same(got_ordered, got)
                seen[got[0]] += 1
                assert _bytes_equal(got[1], whole[1][got[0]])
            assert np.all(seen == 1)                              # disjoint, and together all of count
            if lpt == 2:
                A1, B1 = _one_rank(2)
                one = npr.gather(n, 0, n, start, length, pos, _cols_of(B1, A1))
                assert _same(whole, one) and one[1][:, :6].any() and not one[1][:, 6:12].any()


def test_several_pieces(api, monkeypatch):
    """staging pieces of 1 MB: 32768 particles go up, and about 3 MB of velocities come back, in several"""
    monkeypatch.setenv("PF_HANDOFF_CHUNK_MB", "1")
    n = 32
    box = ((0, 0, 0), (n, n, n), (0, 0, 0))
    rng = np.random.default_rng(11)
    pos = rng.permutation(n ** 3).astype(np.uint32)
    with api.Fmax(n) as f:
        _first_segment(f, synth.make_density(n, seed=9))
        A = f.products()
        _next_segment(f, G2)
        B = f.products()
        want = npr.gather(n, 0, n, box[0], box[1], pos, _cols_of(B, A))
        assert len(want[0]) == n ** 3 and want[1].nbytes == 96 * n ** 3
        assert _same(f.gather_velocities(box, pos), want)
        assert _same(f.gather_velocities(box, pos, order=np.argsort(pos).astype(np.int32)), want)
        lay = _layout(104, 0, 4, (8, 20, 32, 44))
        for order in (None, np.argsort(pos).astype(np.int32)):
            work = np.full((n ** 3, 104), 0xA5, dtype=np.uint8)
            assert f.refresh_velocities(box, pos, work, lay, api.prev_layout(56, 68, 80, 92), order=order) == n ** 3
            assert _bytes_equal(work, npr.scatter(np.full((n ** 3, 104), 0xA5, dtype=np.uint8), want[0], want[1], (8, 20, 32, 44), (56, 68, 80, 92)))


def test_a_capacity_below_the_count(api):
    from pinocchio_amd import _lib
    L = _lib.load()
    n = 16
    _, _, _, start, length, safe = TAP["two x-ranges, one hits"]
    pos = _positions("two x-ranges, one hits")
    rg = api._region((start, length, safe))
    up, ip = C.POINTER(C.c_uint), C.POINTER(C.c_int)
    with api.Fmax(n) as f:                                        # nothing computed
        with pytest.raises(api.PinfmaxError, match="products not computed"):
            f.gather_velocities((start, length, safe), pos)
    with api.Fmax(n) as f:
        _first_segment(f, synth.make_density(n, seed=5))
        A = f.products()
        _next_segment(f, G2)
        B = f.products()
        want = npr.gather(n, 0, n, start, length, pos, _cols_of(B, A))
        total = len(want[0])
        assert total == len(pos)
        for order in (None, np.argsort(pos, kind="stable").astype(np.int32)):
            for cap in (0, 1, 255, 256, 300, total - 1):
                index = np.full(cap + 8, 0xDEADBEEF, dtype=np.uint32)
                vel = np.full(24 * cap + 8, -7.0, dtype=np.float32)
                found = C.c_size_t()
                assert L.pf_gather_velocities(f.h, C.byref(rg), len(pos), pos.ctypes.data_as(up), order.ctypes.data_as(ip) if order is not None else None,
                                              cap, index.ctypes.data_as(up), C.c_void_p(vel.ctypes.data), C.byref(found)) == 0
                assert found.value == total                       # the counting goes on
                assert np.array_equal(index[:cap], want[0][:cap]) and _bytes_equal(vel[:24 * cap], want[1][:cap])
                assert np.all(index[cap:] == 0xDEADBEEF) and np.all(vel[24 * cap:] == -7.0)     # the canaries
            # a count alone, and either output alone
            found = C.c_size_t()
            assert L.pf_gather_velocities(f.h, C.byref(rg), len(pos), pos.ctypes.data_as(up), None, total, None, None, C.byref(found)) == 0 and found.value == total
            index = np.zeros(total, dtype=np.uint32)
            assert L.pf_gather_velocities(f.h, C.byref(rg), len(pos), pos.ctypes.data_as(up), order.ctypes.data_as(ip) if order is not None else None, total,
                                          index.ctypes.data_as(up), None, None) == 0 and np.array_equal(index, want[0])
            vel = np.zeros((total, 24), dtype=np.float32)
            assert L.pf_gather_velocities(f.h, C.byref(rg), len(pos), pos.ctypes.data_as(up), order.ctypes.data_as(ip) if order is not None else None, total,
                                          None, C.c_void_p(vel.ctypes.data), None) == 0 and _bytes_equal(vel, want[1])


def test_drop_prev_gives_the_memory_back(api):
    n = 24                                                        # the mixed-radix path
    _, _, _, start, length, safe = TAP["24 slab"]
    pos = _positions("24 slab")
    box = (start, length, safe)
    for dp, pb in ((False, 4), (True, 8)):
        with api.Fmax(n, double_products=dp) as f:
            _first_segment(f, synth.make_density(n, seed=10))
            A = f.products()
            held = f.device_bytes
            f.drop_prev()                                         # nothing to drop
            assert f.device_bytes == held and f.prev_shifts == 0
            # before any shift the prev slots read zero
            index, vel = f.gather_velocities(box, pos)
            assert _same((index, vel), npr.gather(n, 0, n, start, length, pos, _cols_of(A, np.zeros_like(A))))
            _next_segment(f, G2)
            B = f.products()
            assert f.device_bytes == held + 12 * pb * n ** 3 and f.prev_shifts == 1
            f.drop_prev()
            assert f.device_bytes == held and f.prev_shifts == 0
            assert _same(f.gather_velocities(box, pos), npr.gather(n, 0, n, start, length, pos, _cols_of(B, np.zeros_like(B))))
            with pytest.raises(api.PinfmaxError, match="no pf_shift_displacements yet"):
                f.refresh_velocities(box, pos, np.zeros((len(pos), 208), dtype=np.uint8), _layout(208, -1, -1, (8, -1, -1, -1)), api.prev_layout(104))
            _next_segment(f, G3)                                  # a later shift works again
            assert f.device_bytes == held + 12 * pb * n ** 3 and f.prev_shifts == 1
            assert _same(f.gather_velocities(box, pos), npr.gather(n, 0, n, start, length, pos, _cols_of(f.products(), B)))


# ------------------------------------------------------------------------------------------------------------------------
def test_refusals(api, capfd):
    """decided on the host, before anything is launched: an error with a message, the context usable afterwards"""
    n = 16
    start, length, safe = BOX16
    ncells = 7 * 16 * 5
    pos = _positions("wraps in x and z")
    count = len(pos)
    lay = _layout(104, 0, 4, (8, 20, 32, 44))
    prev = api.prev_layout(56, 68, 80, 92)
    with api.Fmax(n) as f:
        f.set_density(synth.make_density(n, seed=5))
        f.set_invgrow(*synth.invgrow_table("lcdm"))
        f.sweep(RADII)
        # a shift before displacements
        held = f.device_bytes
        with pytest.raises(api.PinfmaxError, match="pf_shift_displacements: displacements not computed"):
            f.shift_displacements()
        assert f.prev_shifts == 0 and f.device_bytes == held
        f.set_growth(G1)
        f.compute_displacements(1, 0)
        A = f.products()
        good = npr.gather(n, 0, n, start, length, pos, _cols_of(A, np.zeros_like(A)))
        assert _same(f.gather_velocities(BOX16, pos), good)

        def refused(match, call):
            with pytest.raises(api.PinfmaxError, match=match):
                call()
            assert _same(f.gather_velocities(BOX16, pos), good), match

        # prev fields before a shift (prev = None is always allowed)
        work = np.full((count, 104), 0xA5, dtype=np.uint8)
        refused("pf_refresh_velocities: the layout names a \\*_prev field but there is no pf_shift_displacements yet",
                lambda: f.refresh_velocities(BOX16, pos, work, lay, prev))
        assert np.all(work == 0xA5)
        assert f.refresh_velocities(BOX16, pos, work, lay) == count
        _next_segment(f, G2)
        good = npr.gather(n, 0, n, start, length, pos, _cols_of(f.products(), A))
        work = np.full((count, 104), 0xA5, dtype=np.uint8)
        # a position that is not below Lx Ly Lz: the first offender is named
        bad = pos.copy()
        bad[300] = 2 ** 32 - 1
        bad[5] = ncells
        refused(r"pf_gather_velocities: frag_pos\[5\] = 560 lies outside the 560 cells of the box", lambda: f.gather_velocities(BOX16, bad))
        refused(r"pf_refresh_velocities: frag_pos\[5\] = 560 lies outside", lambda: f.refresh_velocities(BOX16, bad, work, lay, prev))
        # an order entry that is not below count
        order = np.argsort(pos, kind="stable").astype(np.int32)
        order[7] = count
        order[400] = -1
        refused(r"pf_gather_velocities: order\[7\] = %d is no index of the %d particles" % (count, count), lambda: f.gather_velocities(BOX16, pos, order=order))
        refused(r"pf_refresh_velocities: order\[7\]", lambda: f.refresh_velocities(BOX16, pos, work, lay, prev, order=order))
        # a stride or an offset that is no multiple of four; a field that leaves the record
        for stride, vel, pv in ((102, (8, 20, 32, 44), None), (104, (8, 22, 32, 44), None), (104, (8, 20, 32, 44), (58, -1, -1, -1)),
                                (104, (8, 20, 32, 96), None), (104, (8, 20, 32, 44), (-1, -1, -1, 96))):
            w = np.full((count, stride), 0xA5, dtype=np.uint8)
            refused("pf_refresh_velocities: bad layout", lambda: f.refresh_velocities(BOX16, pos, w, _layout(stride, 0, 4, vel), api.prev_layout(*pv) if pv else None))
            assert np.all(w == 0xA5)
        # fields that overlap: within the layout, within prev, and between the two
        for vel, pv in (((8, 16, 32, 44), (56, 68, 80, 92)), ((8, 20, 32, 44), (56, 60, 80, 92)), ((8, 20, 32, 44), (52, 68, 80, 92))):
            refused("pf_refresh_velocities: fields of the layout overlap", lambda: f.refresh_velocities(BOX16, pos, work, _layout(104, 0, 4, vel), api.prev_layout(*pv)))
        assert np.all(work == 0xA5)
        # len outside [1, n]; the box of a map made for another n
        refused("pf_gather_velocities: box does not fit: len\\[0\\] = 17", lambda: f.gather_velocities((start, (17, 16, 5), safe), pos))
        refused("pf_gather_velocities: box does not fit: len\\[2\\] = 0", lambda: f.gather_velocities((start, (7, 16, 0), safe), pos))
        refused("pf_refresh_velocities: box does not fit", lambda: f.refresh_velocities(((0, 0, 0), (24, 24, 24), (0, 0, 0)), pos, work, lay, prev))
        refused("pf_gather_velocities: safe\\[0\\] = 0 in a direction that is not periodic", lambda: f.gather_velocities(((0, 0, 0), (8, 8, 8), (0, 0, 0)), pos))
        # ... and the good call in place
        assert f.refresh_velocities(BOX16, pos, work, lay, prev) == count
        assert _bytes_equal(work, npr.scatter(np.full((count, 104), 0xA5, dtype=np.uint8), good[0], good[1], (8, 20, 32, 44), (56, 68, 80, 92)))
    # the tap refuses the same
    with pytest.raises(api.PinfmaxError, match=r"pf_debug_gather_velocities: frag_pos\[5\] = 560"):
        api.debug_gather_velocities(n, 0, _cols(n, n), BOX16, bad)
    with pytest.raises(api.PinfmaxError, match=r"pf_debug_gather_velocities: order\[7\]"):
        api.debug_gather_velocities(n, 0, _cols(n, n), BOX16, pos, order)
    with pytest.raises(api.PinfmaxError, match="planes 12 .. 16 of a box of 16"):
        api.debug_gather_velocities(n, 12, _cols(n, 5), BOX16, pos)
    out = capfd.readouterr().out
    assert "ERROR on task 0: pf_gather_velocities: frag_pos[5]" in out and "ERROR on task 0: pf_shift_displacements: displacements not computed" in out


def test_an_order_that_is_no_permutation(api):
    """entries all below count, one particle twice and one never: the omitted particle's entry reads 0xFFFFFFFF / zero, its record keeps
    every byte, and everything else is as with a permutation"""
    n = 16
    start, length, safe = BOX16
    pos = _positions("wraps in x and z")
    count = len(pos)
    lay = _layout(104, 0, 4, (8, 20, 32, 44))
    order = np.argsort(pos, kind="stable").astype(np.int32)
    omitted = int(order[300])
    order[300] = order[299]
    with api.Fmax(n) as f:
        _first_segment(f, synth.make_density(n, seed=5))
        A = f.products()
        _next_segment(f, G2)
        want = npr.gather(n, 0, n, start, length, pos, _cols_of(f.products(), A))
        index, vel = f.gather_velocities(BOX16, pos, order=order)
        assert len(index) == count and index[omitted] == 0xFFFFFFFF and not vel[omitted].any()
        rest = np.arange(count) != omitted
        assert np.array_equal(index[rest], want[0][rest]) and _bytes_equal(vel[rest], want[1][rest])
        work = np.full((count, 104), 0xA5, dtype=np.uint8)
        assert f.refresh_velocities(BOX16, pos, work, lay, api.prev_layout(56, 68, 80, 92), order=order) == count
        full = npr.scatter(np.full((count, 104), 0xA5, dtype=np.uint8), want[0], want[1], (8, 20, 32, 44), (56, 68, 80, 92))
        assert np.all(work[omitted] == 0xA5) and _bytes_equal(work[rest], full[rest])
        # a layout that names no field writes nothing and still counts
        assert f.refresh_velocities(BOX16, pos, work, _layout(104, 0, 4, (-1, -1, -1, -1))) == count and np.all(work[omitted] == 0xA5)
