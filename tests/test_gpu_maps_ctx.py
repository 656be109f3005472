"""Resident fragmentation maps bound to a swept context (Fmax.frag_map; pf_distribute_map, pf_distribute_sorted_map,
pf_count_peaks_map): the distribute calls with a resident map return what the host-map calls return given the same words, byte for
byte; the mapped peak count is count_peaks() over the stored set (tests/np_maps.py count_peaks_stored); and one two-turn walk of
fragment() over the reference's tiling.  Every comparison is exact."""
import numpy as np
import pytest

import np_distribute as npd
import np_maps
import np_peaks
from pinocchio_amd import synth
from test_gpu_distribute import RADII, _same_records, _swept
from test_gpu_multirank import run_ranks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


def _tile(n, safe):
    """a sub-box that wraps the periodic box in x (negative start), is cut in x and y and periodic in z"""
    core = n // 2
    return (-safe, core - safe, 0), (core + 2 * safe, core + 2 * safe, n), (safe, safe, 0)


def _groups(length, pbc, count, seed, max_mass=2000):
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(0.0, length[d] - 0.6, count) for d in range(3)], axis=1)
    mass = np.maximum(np.exp(rng.uniform(np.log(10.0), np.log(max_mass), count)).astype(np.int32), 1)
    return pos, mass


def _turn_maps(m, box, seed):
    """turn 0 then spheres: CURRENT = the box of create_map, UPDATE = the spheres of seeded groups -> the restatement's two arrays"""
    start, length, safe = box
    pbc = [s == 0 for s in safe]
    m.fill_box()
    m.commit(False)
    pos, mass = _groups(length, pbc, 30, seed)
    cur = np_maps.create_map(length, safe, pbc)
    upd, nadd = np_maps.update_map(cur, pos, mass, 2.0, pbc)
    assert m.update(pos, mass, 2.0) == nadd
    assert upd.any() and not (upd & cur).any()
    return cur, upd


def _check_resident_distribute(f, n, seed=1):
    box = _tile(n, 3)
    start, length, safe = box
    seen = 0
    with f.frag_map(start, length, safe) as m:
        cur, upd = _turn_maps(m, box, seed)
        for which, bits in (("current", cur), ("update", upd)):
            words = m.words(which)
            assert np.array_equal(words, np_maps.words_of(bits))
            for flast in (1.0, 0.0):
                a = f.distribute(flast, start, length, map=words)
                b = f.distribute(flast, start, length, map=m, which=which)
                assert a[2] == b[2] <= m.count(which)
                assert np.array_equal(a[1], b[1]) and _same_records(b[0], a[0]), (which, flast)
                a = f.distribute_sorted(flast, start, length, map=words)
                b = f.distribute_sorted(flast, start, length, map=m, which=which)
                assert a[4] == b[4]
                assert _same_records(b[0], a[0]) and all(np.array_equal(a[k], b[k]) for k in (1, 2, 3)), (which, flast)
                assert np.all(b[2][:-1] < b[2][1:])
                seen += b[4]
            # a capacity below the count, and a count-only call
            few = f.distribute_sorted(0.0, start, length, map=m, which=which, capacity=7)
            full = f.distribute_sorted(0.0, start, length, map=words, capacity=7)
            assert few[4] == full[4] and all(np.array_equal(few[k], full[k]) for k in (1, 2, 3)) and _same_records(few[0], full[0])
        assert np.array_equal(m.words("current"), np_maps.words_of(cur)) and np.array_equal(m.words("update"), np_maps.words_of(upd))   # only read
    return seen


@pytest.mark.parametrize("n", [32, 64])
def test_distribute_with_a_resident_map_equals_the_host_map_call(api, n):
    with _swept(api, n) as f:
        assert _check_resident_distribute(f, n) > 0


def test_distribute_with_a_resident_map_and_double_products(api):
    n = 32
    with _swept(api, n, double_products=True) as f:
        assert f.products().dtype.itemsize == 112
        assert _check_resident_distribute(f, n) > 0


@pytest.mark.parametrize("n,P", [(32, 2), (64, 4)])
def test_distribute_with_a_resident_map_on_virtual_ranks(api, n, P):
    """every rank's own contribution to the sub-box, resident map against host words (the checks run inside each rank)"""
    dk = synth.make_density(n, seed=23 + P)
    x, y = synth.invgrow_table("lcdm")
    nxl = n // P

    def body(f, r):
        f.set_density(dk[r * nxl:(r + 1) * nxl]); f.set_invgrow(x, y); f.sweep(RADII)
        return _check_resident_distribute(f, n)

    res = run_ranks(api, n, P, body)
    assert sum(res) > 0 and sum(1 for s in res if s > 0) >= 2


# ------------------------------------------------------------------------------------------------------------------------
FLASTS = (1.0, 0.5, 0.0)


def _check_mapped_peaks(api, f, n, fmax, safe, seed=2):
    """the four maps of the issue on one tile; returns how often the turn-0 count differs from the unmapped region count"""
    box = _tile(n, safe)
    start, length, _ = box
    pbc = [False, False, True]
    rng = np.random.default_rng(seed + n)
    differ = 0
    with f.frag_map(*box) as m:
        assert f.count_peaks(1.0, map=m) == (0, 0) and f.count_peaks(0.0, map=m, which="update") == (0, 0)      # empty maps
        # turn 0
        cur = np_maps.create_map(length, box[2], pbc)
        m.fill_box()
        m.commit(False)
        for flast in FLASTS:
            got = f.count_peaks(flast, map=m)
            plain = f.count_peaks(flast, box)
            print(n, "turn 0", flast, got, "unmapped", plain)
            assert got == np_maps.count_peaks_stored(fmax, flast, box, cur)
            assert got[1] == plain[1]                   # every neighbour of a well resolved cell lies inside the map
            differ += got[0] != plain[0]
        # turn 1: spheres around the first peaks of the tile
        sub = np_peaks.cut(fmax, start, length).copy()
        sub[~np_maps.stored_mask(fmax, 1.0, box, cur)] = np.nan
        pk = np.argwhere(np_peaks.peak_mask_of_subbox(sub, 1.0, pbc))
        order = np.argsort(-sub[tuple(pk.T)].astype(np.float64), kind="stable")[:50]
        pos = pk[order].astype(np.float64) + rng.uniform(-0.4, 0.4, (len(order), 3))
        pos[:, 2] = np.clip(pos[:, 2], 0.0, n - 0.6)
        mass = rng.integers(10, 400, len(order)).astype(np.int32)
        assert len(order) > 0
        upd, nadd = np_maps.update_map(cur, pos, mass, 2.0, pbc)
        assert m.update(pos, mass, 2.0) == nadd
        m.commit(True)
        assert np.array_equal(m.words("current"), np_maps.words_of(cur | upd))
        for flast in FLASTS:
            assert f.count_peaks(flast, map=m) == np_maps.count_peaks_stored(fmax, flast, box, cur | upd), flast
            assert f.count_peaks(flast, map=m, which="update") == np_maps.count_peaks_stored(fmax, flast, box, upd), flast
        # a random map, every other bit on average
        half = rng.random(length) < 0.5
        m.set_words("update", np_maps.words_of(half))
        for flast in FLASTS:
            assert f.count_peaks(flast, map=m, which="update") == np_maps.count_peaks_stored(fmax, flast, box, half), flast
        # all bits set: the existing region count
        m.set_words("current", np.full(m.nwords, 0xFFFFFFFF, dtype=np.uint32))
        for flast in FLASTS:
            assert f.count_peaks(flast, map=m) == f.count_peaks(flast, box) == np_peaks.count_peaks(fmax, flast, box)
        with pytest.raises(ValueError, match="carries its own region"):
            f.count_peaks(1.0, box, map=m)
    return differ


@pytest.mark.parametrize("n", [16, 24, 64])
def test_count_peaks_over_the_stored_set(api, n):
    with _swept(api, n, lpt=False) as f:
        fmax = f.block("FMAX").reshape(n, n, n)
        differ = _check_mapped_peaks(api, f, n, fmax, 2 if n == 16 else 3)
        # the point of the mapped count: "found %d peaks" of turn 0 is NOT the count over every cell of the region
        assert differ > 0


def test_count_peaks_over_the_stored_set_with_fp32_fields(api):
    n = 24
    with _swept(api, n, lpt=False, field_bytes=4) as f:
        _check_mapped_peaks(api, f, n, f.block("FMAX").reshape(n, n, n), 3)


def test_count_peaks_over_the_stored_set_with_double_products(api):
    n = 24
    with _swept(api, n, lpt=False, double_products=True) as f:
        fmax = np.ascontiguousarray(f.products()["Fmax"])
        assert fmax.dtype == np.float64
        _check_mapped_peaks(api, f, n, fmax, 3)
    n = 18                                               # rows that are no multiple of the vector: one cell per lane
    with _swept(api, n, lpt=False) as f:
        _check_mapped_peaks(api, f, n, f.block("FMAX").reshape(n, n, n), 2)


@pytest.mark.parametrize("n,P", [(64, 2), (64, 4), (16, 4)])
def test_count_peaks_over_the_stored_set_on_virtual_ranks(api, n, P):
    """slabs through the in-process fabric: every rank holds the same words and gets the same, all-reduced counts"""
    dk = synth.make_density(n, seed=31 + P)
    x, y = synth.invgrow_table("lcdm")
    nxl = n // P
    box = _tile(n, 2 if n == 16 else 3)
    start, length, safe = box
    pbc = [False, False, True]
    cur = np_maps.create_map(length, safe, pbc)
    half = np.random.default_rng(P).random(length) < 0.5

    def body(f, r):
        f.set_density(dk[r * nxl:(r + 1) * nxl]); f.set_invgrow(x, y); f.sweep(RADII)
        out = {}
        with f.frag_map(*box) as m:
            m.fill_box()
            m.commit(False)
            m.set_words("update", np_maps.words_of(half))
            for flast in FLASTS:
                out[flast] = (f.count_peaks(flast, map=m), f.count_peaks(flast, map=m, which="update"), f.count_peaks(flast, box))
        return f.block("FMAX"), out

    res = run_ranks(api, n, P, body)
    fmax = np.concatenate([r[0] for r in res]).reshape(n, n, n)
    for flast in FLASTS:
        want = (np_maps.count_peaks_stored(fmax, flast, box, cur), np_maps.count_peaks_stored(fmax, flast, box, half), np_peaks.count_peaks(fmax, flast, box))
        for r in range(P):
            assert res[r][1][flast] == want, (flast, r)


# ------------------------------------------------------------------------------------------------------------------------
def test_a_two_turn_walk_over_the_tiles_of_the_reference(api):
    """fragment()'s two turns (src/fragment.c:193-346) with the resident map, nbox 2 x 2 x 1 (z periodic), boundary layer 3"""
    n, flast = 64, 1.0
    rng = np.random.default_rng(12)
    with _swept(api, n) as f:
        fmax = f.block("FMAX").reshape(n, n, n)
        good = 0
        for stabl, lgwbl, lgrid, safe, pbc in npd.subboxes(n, (2, 2, 1), 3):
            box = (stabl, lgwbl, safe)
            with f.frag_map(stabl, lgwbl, safe) as m:
                # turn 0
                m.fill_box()
                m.commit(False)
                cur = np_maps.create_map(lgwbl, safe, pbc)
                rec, pos, spos, ind, cnt = f.distribute_sorted(flast, stabl, lgwbl, map=m)
                stored = np_maps.stored_mask(fmax, flast, box, cur)
                assert cnt == len(pos) == int(stored.sum()) <= m.count("current")
                assert np.array_equal(np.sort(pos), np.flatnonzero(stored.ravel()))
                assert np.all(spos[:-1] < spos[1:]) and np.array_equal(spos, pos[ind])
                assert np.all(rec["Fmax"][:-1] >= rec["Fmax"][1:])
                peaks = f.count_peaks(flast, map=m)
                assert peaks == np_maps.count_peaks_stored(fmax, flast, box, cur) and peaks[0] > peaks[1] > 0
                good += peaks[1]
                # the "halos" of the quick catalogue: the first peaks of the tile
                sub = np_peaks.cut(fmax, stabl, lgwbl).copy()
                sub[~stored] = np.nan
                pk = np.argwhere(np_peaks.peak_mask_of_subbox(sub, flast, pbc))[:60]
                hpos = pk.astype(np.float64) + rng.uniform(-0.4, 0.4, pk.shape)
                hpos[:, 2] = np.clip(hpos[:, 2], 0.0, n - 0.6)
                mass = np.maximum(np.exp(rng.uniform(np.log(10.0), np.log(3000.0), len(pk))).astype(np.int32), 1)
                upd, nadd = np_maps.update_map(cur, hpos, mass, 2.0, pbc)
                assert m.update(hpos, mass, 2.0) == nadd and nadd[0] > 0
                # turn 1: the added particles alone, then everything after the merge
                add = f.distribute(flast, stabl, lgwbl, map=m, which="update")
                assert np.array_equal(np.sort(add[1]), np.flatnonzero(np_maps.stored_mask(fmax, flast, box, upd).ravel())) and add[2] <= m.count("update")
                m.commit(True)
                rec, pos, spos, ind, cnt = f.distribute_sorted(flast, stabl, lgwbl, map=m)
                stored1 = np_maps.stored_mask(fmax, flast, box, cur | upd)
                assert cnt == len(pos) == int(stored.sum()) + add[2] <= m.count("current")
                assert np.array_equal(np.sort(pos), np.flatnonzero(stored1.ravel()))
                assert np.all(spos[:-1] < spos[1:]) and np.array_equal(spos, pos[ind])
                assert f.count_peaks(flast, map=m) == np_maps.count_peaks_stored(fmax, flast, box, cur | upd)
        assert good == f.count_peaks(flast)[0]
