"""sort_and_organize() on the device (pf_distribute_sorted, pf_organize, pf_debug_organize; csrc/pf_organize.hip) against the numpy
restatement of what the reference's call leaves behind (tests/np_organize.py, pinned on the CPU by tests/test_organize_cpu.py).
Orders, positions and records are integers and bytes: every comparison is exact."""
import ctypes as C
import threading

import numpy as np
import pytest

import np_distribute as npd
import np_organize as npo
from pinocchio_amd import synth
from test_gpu_distribute import RADII, _padded_layout, _same_records, _subboxes_for_records, _swept
from test_gpu_multirank import run_ranks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


# ------------------------------------------------------------------------------------------------------------------------
# the ordering alone: the test tap on a caller's arrays
# 1: one record; 63 / 64 / 65: a wavefront; 255 / 256 / 257: a round of the gather; 4097: the 4096-cell group of distribute;
# 3 10^5: several blocks of the sort
COUNTS = (1, 63, 64, 65, 255, 256, 257, 4097, 300001)


def _inputs(rng, count, kind):
    """frag_pos: a random subset of a 96^3 index space in random input order.  Fmax kind 0: continuous; 1: seven distinct values (nearly
    every comparison is a tie and the stable rule decides); 2: zeros of both signs, infinities and NaN among the values"""
    pos = rng.choice(96 ** 3, size=count, replace=False).astype(np.uint32)
    f = (rng.random(count) * 4.0 - 0.5).astype(np.float32)
    if kind == 1:
        f = np.asarray([-0.5, 0.0, 0.5, 1.0, 1.5, 2.5, 3.0], dtype=np.float32)[rng.integers(0, 7, count)]
    if kind == 2:
        special = np.asarray([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1.0, -1e-40, 1e-40], dtype=np.float32)
        pick = rng.random(count) < 0.6
        f[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
        if count >= 63:
            assert np.isnan(f).any() and np.isinf(f).any() and (np.signbit(f) & (f == 0)).any()
    return f, pos


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["continuous", "seven values", "zeros infinities nan"])
def test_debug_organize_equals_the_restatement(api, kind):
    rng = np.random.default_rng(40 + kind)
    for count in COUNTS:
        f, pos = _inputs(rng, count, kind)
        worder, wspos, wind = npo.organize(f, pos)
        order, spos, ind = api.debug_organize(f, pos)
        assert np.array_equal(order, worder), (kind, count)
        assert np.array_equal(spos, wspos) and np.array_equal(ind, wind), (kind, count)
    order, spos, ind = api.debug_organize(np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.uint32))
    assert len(order) == len(spos) == len(ind) == 0


# ------------------------------------------------------------------------------------------------------------------------
# distribute + sort_and_organize from the columns
def _check_sorted(api, f, n, flast=1.0, seed=0, boxes=None):
    """pf_distribute_sorted = pf_distribute's output permuted by the restatement's order, with the restatement's index"""
    from pinocchio_amd import _lib
    pb = 8 if f.double_products else 4
    rng = np.random.default_rng(seed + n)
    total = 0
    for k, (start, length) in enumerate(boxes if boxes is not None else _subboxes_for_records(n, seed + n)):
        words = None if k % 2 == 0 else npd.pack_map(rng.random(tuple(length)) < 0.7)
        rec, pos, cnt = f.distribute(flast, start, length, map=words)
        o = npo.order(rec["Fmax"])
        wspos, wind = npo.index(pos[o])
        srec, spos_, sorted_pos, ind, scnt = f.distribute_sorted(flast, start, length, map=words)
        assert scnt == cnt == len(srec), (start, length)
        assert np.array_equal(spos_, pos[o]) and _same_records(srec, rec[o]), (start, length)
        assert np.array_equal(sorted_pos, wspos) and np.array_equal(ind, wind), (start, length)
        total += cnt
        # absent fields and padding; a record too long for the staged form (the plain gather)
        for stride in (16 + 52 * (pb // 4), 16 + 52 * (pb // 4) + 240):
            lay = _padded_layout(_lib, stride, pb // 4)
            rows, rpos, _ = f.distribute(flast, start, length, map=words, layout=lay)
            srows, spos_, sorted_pos, ind, scnt = f.distribute_sorted(flast, start, length, map=words, layout=lay)
            assert scnt == cnt and srows.shape == (cnt, stride) and np.array_equal(srows, rows[o]), (start, length, stride)
            assert np.array_equal(spos_, pos[o]) and np.array_equal(sorted_pos, wspos) and np.array_equal(ind, wind)
        # capacity below the count: the first records of the sorted order, the count of all, and the index of those records
        cap = cnt // 3
        srec, spos_, sorted_pos, ind, scnt = f.distribute_sorted(flast, start, length, map=words, capacity=cap)
        cspos, cind = npo.index(pos[o][:cap])
        assert scnt == cnt and len(srec) == cap and _same_records(srec, rec[o][:cap]) and np.array_equal(spos_, pos[o][:cap])
        assert np.array_equal(sorted_pos, cspos) and np.array_equal(ind, cind)
    assert total > 0
    # nothing taken
    srec, spos_, sorted_pos, ind, scnt = f.distribute_sorted(np.inf, (0, 0, 0), (n, n, n))
    assert scnt == 0 and len(srec) == len(spos_) == len(sorted_pos) == len(ind) == 0


@pytest.mark.parametrize("n", [24, 64, 96])
def test_distribute_sorted_is_distribute_in_the_order_of_the_restatement(api, n):
    with _swept(api, n) as f:
        _check_sorted(api, f, n)


def test_distribute_sorted_with_double_products(api):
    n = 24
    with _swept(api, n, double_products=True) as f:
        assert f.products().dtype.itemsize == 112
        _check_sorted(api, f, n, seed=1)


def test_distribute_sorted_with_fp32_fields_and_before_the_displacements(api):
    n = 32
    with _swept(api, n, lpt=False, field_bytes=4) as f:
        _check_sorted(api, f, n, seed=3, boxes=[((5, -4, 30), (20, n, 9)), ((0, 0, 0), (n, n, n))])


def test_the_plain_gather_gives_the_same_records(api, monkeypatch):
    """PF_DISTRIBUTE_LDS=0: one lane per record into a cleared buffer, the form the staged gather is measured against"""
    n = 64
    monkeypatch.setenv("PF_DISTRIBUTE_LDS", "0")
    with _swept(api, n) as f:
        _check_sorted(api, f, n, seed=2)


def test_a_sorted_result_of_many_pieces(api, monkeypatch):
    """staging pieces of 1 MB: every cell of the 64^3 box leaves in sixteen pieces"""
    n = 64
    monkeypatch.setenv("PF_HANDOFF_CHUNK_MB", "1")
    with _swept(api, n) as f:
        _check_sorted(api, f, n, flast=-np.inf, seed=4, boxes=[((0, 0, 0), (n, n, n)), ((-3, n - 2, 5), (n // 2, 7, n))])
        _check_sorted(api, f, n, flast=1.0, seed=4, boxes=[((0, 0, 0), (n, n, n))])


# ------------------------------------------------------------------------------------------------------------------------
# the arrays as count_peaks consumes them
@pytest.mark.parametrize("flast", [1.0, 1.5])
def test_peaks_counted_through_find_location_equal_pf_count_peaks(api, flast):
    """the whole periodic box on one rank, flast = 1 + z of an output at z = 0 and at z = 0.5: every neighbour of every stored cell is
    looked up in sorted_pos / indices the way the reference's count_peaks does (find_location, src/fragment.c:592-603), and the
    strict six-neighbour peaks are as many as the device's own count on the field"""
    n = 64
    with _swept(api, n, lpt=False) as f:
        rec, pos, sorted_pos, ind, cnt = f.distribute_sorted(flast, (0, 0, 0), (n, n, n))
        assert 0 < cnt < n ** 3
        got = npo.count_peaks(rec["Fmax"], pos, sorted_pos, ind, (n, n, n))
        assert got == f.count_peaks(flast)[0] > 0


# ------------------------------------------------------------------------------------------------------------------------
# contributions of several ranks, concatenated
# fp32 Fmax has 2^23 values per binade: among N stored cells about N^2 / 2^24 pairs are equal (hundreds at flast = 1), so the
# comparison with the single-rank context -- which holds only when no two stored cells of a sub-box have equal Fmax -- is made at
# FLAST_UNIQUE, where a sub-box stores between a hundred and two thousand cells, and with a density seed for which none of these
# sub-boxes holds an equal pair (the test asserts it); the comparison with the restatement is made at flast = 1 as well, ties and all
FLAST_UNIQUE = 6.0
SEED_UNIQUE = 71


@pytest.mark.parametrize("n,P,nbox", [(64, 2, (2, 1, 1)), (64, 8, (2, 2, 2)), (96, 3, (3, 1, 1))])
def test_organize_on_contributions_concatenated_in_the_order_of_distribute(api, n, P, nbox):
    """the virtual ranks of test_slabs_concatenated_in_the_order_of_distribute: every rank distributes to every sub-box, rank 0
    concatenates the contributions to each in distribute()'s order and organises them on its own context"""
    dk = synth.make_density(n, seed=SEED_UNIQUE + P)
    x, y = synth.invgrow_table("lcdm")
    nxl = n // P
    boxes = npd.subboxes(n, nbox, 3)
    maps = [npd.create_map(lgwbl, lgrid, safe, pbc) for (_, lgwbl, lgrid, safe, pbc) in boxes]
    flasts = (1.0, FLAST_UNIQUE)
    with api.Fmax(n) as f1:
        f1.set_density(dk); f1.set_invgrow(x, y); f1.sweep(RADII)
        single = {FLAST_UNIQUE: [f1.distribute_sorted(FLAST_UNIQUE, b[0], b[1], map=m) for b, m in zip(boxes, maps)]}
    shared = [None] * P
    gate = threading.Barrier(P)

    def body(f, r):
        f.set_density(dk[r * nxl:(r + 1) * nxl]); f.set_invgrow(x, y); f.sweep(RADII)
        shared[r] = {fl: [f.distribute(fl, b[0], b[1], map=m) for b, m in zip(boxes, maps)] for fl in flasts}
        gate.wait(timeout=300)
        if r:
            return None
        out = {}
        for fl in flasts:
            for t in range(len(boxes)):
                order = npd.hypercube_order(P, t)
                rec = np.concatenate([shared[q][fl][t][0] for q in order])
                pos = np.concatenate([shared[q][fl][t][1] for q in order])
                before = (rec.copy(), pos.copy())
                spos, ind = f.organize(rec, pos)
                out[fl, t] = before + (rec, pos, spos, ind)
        return out

    res = run_ranks(api, n, P, body)[0]
    for fl in flasts:
        for t in range(len(boxes)):
            rec0, pos0, rec, pos, spos, ind = res[fl, t]
            assert len(rec0) > 0
            o = npo.order(rec0["Fmax"])
            wspos, wind = npo.index(pos0[o])
            assert np.array_equal(pos, pos0[o]) and _same_records(rec, rec0[o]), (fl, t)
            assert np.array_equal(spos, wspos) and np.array_equal(ind, wind), (fl, t)
            if fl == FLAST_UNIQUE:
                assert len(np.unique(rec0["Fmax"])) == len(rec0), (t, len(rec0))       # the precondition: no ties to break
                srec, sfpos, sspos, sind, scnt = single[fl][t]
                assert scnt == len(rec)
                assert np.array_equal(pos, sfpos) and _same_records(rec, srec), t
                assert np.array_equal(spos, sspos) and np.array_equal(ind, sind), t


# ------------------------------------------------------------------------------------------------------------------------
def test_errors_in_the_house_format(api, capfd):
    n = 16
    with api.Fmax(n) as f:
        with pytest.raises(api.PinfmaxError, match="pf_distribute_sorted: products not computed"):
            f.distribute_sorted(1.0, (0, 0, 0), (n, n, n))
        f.set_density(synth.make_density(n, seed=5))
        f.set_invgrow(*synth.invgrow_table("lcdm"))
        f.sweep(RADII)
        lay, _ = f.product_layout()
        sub = api._subbox((0, 0, 0), (n, n, n))
        assert f.L.pf_distribute_sorted(f.h, 1.0, C.byref(sub), None, C.byref(lay), 0, None, None, None, None, None) != 0
        assert f.L.pf_last_error().decode() == "pf_distribute_sorted: null argument"
        with pytest.raises(api.PinfmaxError, match=r"pf_distribute_sorted: sub-box does not fit the box: len\[1\] = 17 outside \[1, 16\]"):
            f.distribute_sorted(1.0, (0, 0, 0), (n, n + 1, n))
        rec = np.zeros((4, lay.stride), dtype=np.uint8)
        pos = np.arange(4, dtype=np.uint32)
        lay.off_Fmax = -1
        with pytest.raises(api.PinfmaxError, match=r"pf_organize: the layout names no Fmax to sort by \(off_Fmax = -1\)"):
            f.organize(rec, pos, layout=lay)
        lay, _ = f.product_layout()
        lay.off_Vel = 6
        with pytest.raises(api.PinfmaxError, match="pf_organize: bad layout"):
            f.organize(rec, pos, layout=lay)
        with pytest.raises(api.PinfmaxError, match="pf_distribute_sorted: bad layout"):
            f.distribute_sorted(1.0, (0, 0, 0), (n, n, n), layout=lay)
        lay, _ = f.product_layout()
        lay.off_Vel_2LPT = lay.off_Vel + 8
        with pytest.raises(api.PinfmaxError, match="pf_distribute_sorted: fields of the layout overlap"):
            f.distribute_sorted(1.0, (0, 0, 0), (n, n, n), layout=lay)
        with pytest.raises(api.PinfmaxError, match="pf_organize: fields of the layout overlap"):
            f.organize(rec, pos, layout=lay)
        assert not rec.any() and np.array_equal(pos, np.arange(4))                      # a refused call has touched nothing
        lay, _ = f.product_layout()
        assert f.L.pf_organize(f.h, C.byref(lay), 4, None, None, None, None) != 0
        assert f.L.pf_last_error().decode() == "pf_organize: null argument"
    out = capfd.readouterr().out
    assert "ERROR on task 0: pf_distribute_sorted: products not computed" in out
    assert "ERROR on task 0: pf_organize: fields of the layout overlap" in out
