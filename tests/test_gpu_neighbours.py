"""The neighbour table on the device (pf_neighbours, pf_distribute_sorted_neighbours_map; csrc/pf_neighbours.hip) against the numpy
restatement of the reference's loop (tests/np_neighbours.py, pinned on the CPU by tests/test_neighbours_cpu.py) and against the
device's own count_peaks kernels.  Indices, flags and counts are integers: every comparison is exact."""
import ctypes as C
import functools

import numpy as np
import pytest

import np_neighbours as npn
import np_organize as npo
from test_gpu_distribute import _same_records, _swept
from test_gpu_organize import _inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


# ------------------------------------------------------------------------------------------------------------------------
# the context-free call on caller's arrays.  (len; safe): a direction is periodic when safe == 0.  (17, 9, 70): z-rows of 70
# straddle a wavefront, directions mixed
BOXES = (((1, 1, 1), (0, 0, 0)), ((2, 2, 2), (0, 0, 0)), ((3, 4, 5), (1, 1, 1)), ((6, 5, 64), (0, 2, 0)), ((17, 9, 70), (2, 0, 3)),
         ((96, 96, 96), (0, 0, 0)))
BOX_IDS = ["1x1x1", "2x2x2", "3x4x5 borders", "6x5x64", "17x9x70 mixed", "96^3"]


def _counts(length):
    """nothing; one particle; around a wavefront, a workgroup, a 4096 group; fills 0.05 (most rows empty), 0.5 and 1.0"""
    cells = length[0] * length[1] * length[2]
    out = [0, 1] + [c for c in (63, 64, 65, 257, 4097) if c <= cells] + [int(round(fill * cells)) for fill in (0.05, 0.5, 1.0)]
    return sorted(set(out))


@functools.lru_cache(maxsize=None)
def _case(ibox, count, kind):
    """a stored set in the order after sort_and_organize and the restatement's table of it (computed once, shared, left alone)"""
    length, safe = BOXES[ibox]
    cells = length[0] * length[1] * length[2]
    rng = np.random.default_rng(1000 * ibox + 10 * kind + count % 7)
    f = _inputs(rng, count, kind)[0]
    pos = rng.choice(cells, size=count, replace=False).astype(np.uint32)
    o = npo.order(f)
    pos, f = pos[o], f[o]
    want = npn.neighbours(pos, f, length, safe, tuple(s == 0 for s in safe))
    for a in (pos, f, want[0], want[1]):
        a.setflags(write=False)
    return pos, f, want


def _same_table(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and tuple(got[2]) == tuple(want[2])


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["continuous", "seven values", "zeros infinities nan"])
@pytest.mark.parametrize("ibox", range(len(BOXES)), ids=BOX_IDS)
def test_neighbours_equal_the_restatement(api, ibox, kind):
    length, safe = BOXES[ibox]
    cells = length[0] * length[1] * length[2]
    for count in _counts(length):
        pos, f, want = _case(ibox, count, kind)
        got = api.neighbours(pos, f, (0, 0, 0), length, safe)
        assert got[0].shape == (count, 6) and got[0].dtype == np.int32 and got[1].dtype == np.uint8
        assert _same_table(got, want), (length, count, kind)
        if count == cells and kind == 0 and length in ((96, 96, 96), (3, 4, 5)):
            # every cell stored: the peaks of the field itself by the count_peaks kernel
            n = 96 if length[0] == 96 else 8
            field = np.full((n, n, n), -np.inf, dtype=np.float32)
            sub = np.empty(cells, dtype=np.float32)
            sub[pos] = f
            field[:length[0], :length[1], :length[2]] = sub.reshape(length)
            region = None if n == 96 else ((0, 0, 0), length, safe)
            assert api.debug_peaks(field, -np.inf, region) == got[2]
            assert got[2][0] > 0 or n == 8


@pytest.mark.parametrize("ibox", [4, 5], ids=["17x9x70 mixed", "96^3"])
def test_the_plain_form_gives_the_same_arrays(api, monkeypatch, ibox):
    """PF_NEIGH_ROWS=0: one search of the whole of sorted_pos per neighbour, the form the row form is measured against"""
    length, safe = BOXES[ibox]
    count = int(round(0.5 * length[0] * length[1] * length[2]))
    for kind in (0, 1, 2):
        pos, f, want = _case(ibox, count, kind)
        rows = api.neighbours(pos, f, (0, 0, 0), length, safe)
        monkeypatch.setenv("PF_NEIGH_ROWS", "0")
        plain = api.neighbours(pos, f, (0, 0, 0), length, safe)
        monkeypatch.delenv("PF_NEIGH_ROWS")
        assert _same_table(plain, rows) and _same_table(plain, want)


def test_a_strided_fmax_and_a_count_only_call(api):
    """the Fmax field of a record array (stride 56) uploads the values alone; neigh and flags may be absent"""
    from pinocchio_amd import _lib
    L = _lib.load()
    pos, f, want = _case(4, 4097, 0)
    rec = np.zeros(len(pos), dtype=api.PRODUCT_DTYPE)
    rec["Fmax"] = f
    assert rec["Fmax"].strides[0] == 56
    assert _same_table(api.neighbours(pos, rec["Fmax"], (0, 0, 0), *BOXES[4]), want)
    rg = api._region(((0, 0, 0),) + BOXES[4])
    peaks = (C.c_ulonglong * 2)(7, 7)
    assert L.pf_neighbours(None, C.byref(rg), len(pos), pos.ctypes.data_as(C.POINTER(C.c_uint)), C.c_void_p(f.ctypes.data), 4, None, None, peaks) == 0
    assert (int(peaks[0]), int(peaks[1])) == want[2]
    flags = np.zeros(len(pos), dtype=np.uint8)
    assert L.pf_neighbours(None, C.byref(rg), len(pos), pos.ctypes.data_as(C.POINTER(C.c_uint)), C.c_void_p(f.ctypes.data), 4, None,
                           flags.ctypes.data_as(C.POINTER(C.c_ubyte)), peaks) == 0
    assert np.array_equal(flags, want[1])


# ------------------------------------------------------------------------------------------------------------------------
# the fused call on swept contexts
def _maps(f, n, rng):
    """(FragMap, what it is): the whole periodic box; a sub-box with a negative start and safe = 3 filled by create_map and committed;
    a mixed box (periodic in x alone) with every bit; the whole box with a random word pattern"""
    m = f.frag_map((0, 0, 0), (n, n, n), (0, 0, 0))
    m.set_words("current", np.full(m.nwords, 0xFFFFFFFF, dtype=np.uint32))
    yield m, "whole box"
    m = f.frag_map((-2, 3, 1), (n // 2, n // 2 + 1, n - 5), (3, 3, 3))
    m.fill_box()
    m.commit(False)
    yield m, "sub-box"
    m = f.frag_map((0, 5, -3), (n, 11, 9), (0, 3, 3))
    m.set_words("current", np.full(m.nwords, 0xFFFFFFFF, dtype=np.uint32))
    yield m, "mixed box"
    m = f.frag_map((0, 0, 0), (n, n, n), (0, 0, 0))
    m.set_words("current", rng.integers(0, 1 << 32, m.nwords, dtype=np.uint64).astype(np.uint32))
    yield m, "random words"


def _check_fused(api, f, n, flast=1.0, seed=0):
    rng = np.random.default_rng(seed + n)
    total = 0
    for m, what in _maps(f, n, rng):
        with m:
            pbc = tuple(v == n for v in m.length)
            rec, pos, spos, ind, cnt = f.distribute_sorted(flast, m.start, m.length, map=m)
            frec, fpos, fspos, find, neigh, flags, peaks, fcnt = f.distribute_sorted_neighbours(flast, m)
            assert fcnt == cnt == len(frec), what
            assert _same_records(frec, rec) and np.array_equal(fpos, pos) and np.array_equal(fspos, spos) and np.array_equal(find, ind), what
            want = npn.neighbours(pos, rec["Fmax"], m.length, m.safe, pbc)
            assert _same_table((neigh, flags, peaks), want), what
            # an existing, independent kernel: count_peaks over the stored set of the same map
            assert peaks == f.count_peaks(flast, map=m), what
            # the table on the host arrays, by the call that builds its own index
            assert _same_table(f.neighbours(pos, rec["Fmax"], m.start, m.length, m.safe), want), what
            # a capacity below the count: the table of the first third alone -- a neighbour beyond it is absent
            cap = cnt // 3
            frec, fpos, fspos, find, neigh, flags, peaks, fcnt = f.distribute_sorted_neighbours(flast, m, capacity=cap)
            crec, cpos, cspos, cind, ccnt = f.distribute_sorted(flast, m.start, m.length, map=m, capacity=cap)
            assert fcnt == cnt == ccnt and len(frec) == cap and _same_records(frec, crec)
            assert np.array_equal(fpos, cpos) and np.array_equal(fspos, cspos) and np.array_equal(find, cind), what
            assert _same_table((neigh, flags, peaks), npn.neighbours(pos[:cap], rec["Fmax"][:cap], m.length, m.safe, pbc)), what
            total += cnt
    assert total > 0
    # nothing taken
    with f.frag_map((0, 0, 0), (n, n, n), (0, 0, 0)) as m:
        out = f.distribute_sorted_neighbours(flast, m)          # no bit set
        assert out[7] == 0 and out[6] == (0, 0) and out[4].shape == (0, 6) and len(out[5]) == 0


@pytest.mark.parametrize("n", [24, 64])
def test_the_fused_call_is_distribute_sorted_plus_the_table(api, n):
    with _swept(api, n) as f:
        _check_fused(api, f, n)


def test_the_fused_call_with_fp32_fields(api):
    n = 32
    with _swept(api, n, lpt=False, field_bytes=4) as f:
        _check_fused(api, f, n, seed=3)


def test_the_fused_call_with_double_products(api):
    n = 24
    with _swept(api, n, double_products=True) as f:
        assert f.products().dtype.itemsize == 112
        _check_fused(api, f, n, seed=1)


def test_a_table_of_many_pieces(api, monkeypatch):
    """staging pieces of 1 MB: the table of every cell of the 64^3 box (6 MB) leaves in several pieces"""
    n = 64
    monkeypatch.setenv("PF_HANDOFF_CHUNK_MB", "1")
    with _swept(api, n) as f:
        with f.frag_map((0, 0, 0), (n, n, n), (0, 0, 0)) as m:
            m.set_words("current", np.full(m.nwords, 0xFFFFFFFF, dtype=np.uint32))
            rec, pos, spos, ind, neigh, flags, peaks, cnt = f.distribute_sorted_neighbours(-np.inf, m)
            assert cnt == n ** 3 and neigh.nbytes >= 6 << 20
            srec, spos_, sspos, sind, scnt = f.distribute_sorted(-np.inf, m.start, m.length, map=m)
            assert _same_records(rec, srec) and np.array_equal(pos, spos_) and np.array_equal(spos, sspos) and np.array_equal(ind, sind)
            want = npn.neighbours(pos, rec["Fmax"], m.length, m.safe, (True, True, True))
            assert _same_table((neigh, flags, peaks), want)
            assert peaks == f.count_peaks(-np.inf, map=m)
            assert _same_table(f.neighbours(pos, rec["Fmax"], m.start, m.length, m.safe), want)


# ------------------------------------------------------------------------------------------------------------------------
def test_refusals(api, capfd):
    """decided on the host: an error with a message, outputs untouched"""
    from pinocchio_amd import _lib
    L = _lib.load()
    up, ip, bp = C.POINTER(C.c_uint), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)
    length, safe = (6, 5, 64), (0, 2, 0)
    cells = 6 * 5 * 64
    pos, f, want = _case(3, 257, 0)

    def raw(ctx, rg, p, fm, stride):
        neigh = np.full((len(p), 6), 77, dtype=np.int32)
        flags = np.full(len(p), 77, dtype=np.uint8)
        peaks = (C.c_ulonglong * 2)(77, 77)
        rc = L.pf_neighbours(ctx, C.byref(rg), len(p), p.ctypes.data_as(up), C.c_void_p(fm.ctypes.data), stride, neigh.ctypes.data_as(ip),
                             flags.ctypes.data_as(bp), peaks)
        untouched = bool(np.all(neigh == 77) and np.all(flags == 77) and peaks[0] == 77 and peaks[1] == 77)
        return rc, untouched, L.pf_last_error().decode()

    rg = api._region(((0, 0, 0), length, safe))
    assert raw(None, rg, pos, f, 4)[:2] == (0, False)
    # a position equal to Lx Ly Lz
    bad = pos.copy()
    bad[200] = cells
    rc, untouched, msg = raw(None, rg, bad, f, 4)
    assert rc != 0 and untouched and "frag_pos[200] = 1920 lies outside the box of 1920 cells" in msg
    with pytest.raises(api.PinfmaxError, match="lies outside the box"):
        api.neighbours(bad, f, (0, 0, 0), length, safe)
    # a stride of 6
    wide = np.zeros(2 * len(f), dtype=np.float32)
    rc, untouched, msg = raw(None, rg, pos, wide, 6)
    assert rc != 0 and untouched and "a stride of 6 bytes is no multiple of the 4 bytes of an Fmax" in msg
    with api.Fmax(16) as f16, api.Fmax(16) as g16:
        # with a context the same two, decided while staging
        rg16 = api._region(((0, 0, 0), (16, 9, 16), (0, 2, 0)))
        p16 = np.arange(100, dtype=np.uint32)
        f100 = np.arange(100, 0, -1).astype(np.float32)
        assert raw(f16.h, rg16, p16, f100, 4)[:2] == (0, False)
        bad16 = p16.copy()
        bad16[99] = 16 * 9 * 16
        rc, untouched, msg = raw(f16.h, rg16, bad16, f100, 4)
        assert rc != 0 and untouched and "frag_pos[99] = 2304 lies outside the box of 2304 cells" in msg
        rc, untouched, msg = raw(f16.h, rg16, p16, np.zeros(200, dtype=np.float32), 6)
        assert rc != 0 and untouched and "a stride of 6 bytes" in msg
        # safe = 0 in a direction that is not periodic: the refusal of pf_map_create
        rc, untouched, msg = raw(f16.h, api._region(((0, 0, 0), (16, 9, 16), (0, 0, 0))), p16, f100, 4)
        assert rc != 0 and untouched and "pf_neighbours: safe[1] = 0 in a direction that is not periodic" in msg
        with pytest.raises(api.PinfmaxError, match="in a direction that is not periodic"):
            f16.neighbours(p16, f100, (0, 0, 0), (16, 9, 16), (0, 0, 0))
        # a map of another context
        with g16.frag_map((0, 0, 0), (16, 16, 16), (0, 0, 0)) as m:
            with pytest.raises(ValueError):
                f16.distribute_sorted_neighbours(1.0, m)
            lay, _ = f16.product_layout()
            neigh = np.full((8, 6), 77, dtype=np.int32)
            flags = np.full(8, 77, dtype=np.uint8)
            peaks = (C.c_ulonglong * 2)(77, 77)
            cnt = C.c_size_t(77)
            rc = L.pf_distribute_sorted_neighbours_map(f16.h, 1.0, m.h, 0, C.byref(lay), 8, None, None, None, None, neigh.ctypes.data_as(ip),
                                                       flags.ctypes.data_as(bp), peaks, C.byref(cnt))
            assert rc != 0 and "the map was not created with this context" in L.pf_last_error().decode()
            assert np.all(neigh == 77) and np.all(flags == 77) and peaks[0] == 77 and cnt.value == 77
    out = capfd.readouterr().out
    assert "ERROR on task 0: pf_neighbours: frag_pos[200]" in out and "ERROR on task 0: pf_distribute_sorted_neighbours_map: the map was not created" in out
