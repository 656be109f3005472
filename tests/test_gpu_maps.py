"""The fragmentation maps on the device (pf_map_*; csrc/pf_map.hip) against the numpy restatement of create_map() / update_map()
(tests/np_maps.py, held against the reference's triple loop by tests/test_maps_cpu.py).  Context-free maps: no sweep.  Every
comparison is exact: the outputs are bit words and integer counts."""
import numpy as np
import pytest

import np_maps

pytestmark = pytest.mark.gpu

# (len, safe); without a context a direction is periodic when safe == 0
BOX_A = ((20, 23, 37), (4, 4, 4))         # 17 020 cells: no multiple of 32, rows of 37 bits straddle words
BOX_A1 = ((20, 23, 37), (1, 1, 1))        # the range starts at 0
BOX_B = ((32, 22, 32), (0, 5, 0))         # x and z periodic
BOX_C = ((16, 16, 16), (0, 0, 0))         # all bits set
BOX_D = ((96, 80, 72), (6, 6, 6))         # rows longer than a wavefront and than four words


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


def _pbc(safe):
    return tuple(s == 0 for s in safe)


def _tail_is_zero(words, length):
    cells = int(np.prod(length))
    return cells % 32 == 0 or (int(words[-1]) >> (cells % 32)) == 0


@pytest.mark.parametrize("length,safe", [BOX_A, BOX_A1, BOX_B, BOX_C, ((7, 64, 5), (2, 3, 1))])
def test_fill_box_equals_create_map(api, length, safe):
    want = np_maps.create_map(length, safe, _pbc(safe))
    with api.FragMap((0, 0, 0), length, safe) as m:
        assert m.nwords == (int(np.prod(length)) + 31) // 32
        assert not m.words("current").any() and not m.words("update").any()      # both zero after create
        m.fill_box()
        w = m.words("update")
        assert np.array_equal(w, np_maps.words_of(want)) and _tail_is_zero(w, length)
        assert not m.words("current").any()
        assert m.count("update") == int(want.sum()) and m.count("current") == 0
        m.fill_box()                                                               # UPDATE is cleared first: the same again
        assert np.array_equal(m.words("update"), w)
    if (length, safe) == BOX_C:
        assert want.all()


def groups_for(length, safe, blf, seed=3, count=200):
    """200 seeded groups: masses 1 .. 5 10^4 log-uniform (size 0 -- BLF 0.5 only --, 1, ... 69 at BLF 3), centres anywhere and on
    faces and corners, positions that pin (int)(pos + 0.5); one group listed twice (the last repeats group 5).  No sphere larger
    than a periodic direction and no centre outside it (the library refuses those)"""
    rng = np.random.default_rng(seed)
    pbc = _pbc(safe)
    pos = np.empty((count, 3))
    for d in range(3):
        pos[:, d] = rng.uniform(0.0, length[d] - 0.6, count) if pbc[d] else rng.uniform(-2.0, length[d] + 2.0, count)
    mass = np.maximum(np.exp(rng.uniform(0.0, np.log(5e4), count)).astype(np.int32), 1)
    mass[:4] = (1, 2, 30, 50000)
    corners = [(0, 0, 0), (length[0] - 1, length[1] - 1, length[2] - 1), (0, length[1] - 1, 0), (length[0] // 2, 0, length[2] - 1)]
    for g, c in enumerate(corners):
        pos[10 + g] = c
        mass[10 + g] = 500
    pos[20] = (-0.3 if not pbc[0] else 0.3, length[1] - 0.4, 7.5)                  # -> 0, len (outside by one cell), 8
    if pbc[1]:
        pos[20, 1] = length[1] - 0.6
    mass[20] = 60
    for d in range(3):
        if pbc[d]:
            while max(np_maps.centre_and_size((0, 0, 0), int(v), blf)[1] for v in mass) > length[d]:
                mass = np.where(mass == mass.max(), mass // 2, mass)
    pos[-1], mass[-1] = pos[5], mass[5]
    return pos, mass


@pytest.fixture(scope="module")
def update_cases():
    """the restatement's answers, computed once: (box, blf) -> (pos, mass, current, update, nadd)"""
    out = {}
    for (length, safe), blf in ((BOX_A, 2.0), (BOX_A, 3.0), (BOX_B, 2.0), (BOX_B, 3.0), (BOX_D, 2.0), (BOX_D, 3.0)):
        pos, mass = groups_for(length, safe, blf)
        cur = np_maps.create_map(length, safe, _pbc(safe))
        upd, nadd = np_maps.update_map(cur, pos, mass, blf, _pbc(safe))
        out[(length, safe, blf)] = (pos, mass, cur, upd, nadd)
    return out


@pytest.mark.parametrize("blf", [2.0, 3.0])
@pytest.mark.parametrize("length,safe", [BOX_A, BOX_B, BOX_D])
def test_update_equals_update_map(api, update_cases, monkeypatch, length, safe, blf):
    pos, mass, cur, upd, nadd = update_cases[(length, safe, blf)]
    pbc = _pbc(safe)
    sizes = [np_maps.centre_and_size((0, 0, 0), int(v), blf)[1] for v in mass]
    assert min(sizes) == (1 if blf == 2.0 else 2)
    if (length, safe) == BOX_D and blf == 3.0:
        assert max(sizes) == 69                                                    # rows of 138 cells: three rounds of a wavefront, five words
    assert nadd[1] > 0                                                             # centres on faces and corners
    assert nadd[0] > upd.sum()                                                     # multiplicity: overlapping spheres count twice
    results = []
    for form in ("1", "0", "1"):                                                   # PF_MAP_WORDS is read when a map is created
        monkeypatch.setenv("PF_MAP_WORDS", form)
        with api.FragMap((0, 0, 0), length, safe) as m:
            m.fill_box()
            m.commit(False)
            got = m.update(pos, mass, blf)
            w = m.words("update")
            print(length, blf, form, got, "bits", m.count("update"))
            assert got == nadd
            assert np.array_equal(w, np_maps.words_of(upd)) and _tail_is_zero(w, length)
            assert np.array_equal(m.words("current"), np_maps.words_of(cur))       # CURRENT is only read
            assert not np.any(w & m.words("current"))                              # update never sets a bit CURRENT has
            results.append((got, w))
            if form == "0":
                continue
            # the group listed twice: without its second copy the words are the same and nadd[0] is smaller by its own count
            alone = np_maps.update_map(cur, pos[-1:], mass[-1:], blf, pbc)[1]
            got2 = m.update(pos[:-1], mass[:-1], blf)
            assert np.array_equal(m.words("update"), w)
            assert got2 == (nadd[0] - alone[0], nadd[1] - alone[1])
            # no groups: UPDATE is cleared
            assert m.update(np.zeros((0, 3)), np.zeros(0, dtype=np.int32), blf) == (0, 0)
            assert m.count("update") == 0 and m.count("current") == int(cur.sum())
    for got, w in results[1:]:                                                     # both forms, and two runs of one form
        assert got == results[0][0] and np.array_equal(w, results[0][1])


def test_sizes_zero_and_one(api):
    length, safe = BOX_A
    with api.FragMap((0, 0, 0), length, safe) as m:
        pos = np.array([[10.0, 11.0, 12.0], [3.2, 3.7, 30.5]])
        for blf, mass in ((0.5, [1, 1]), (2.0, [1, 1]), (0.5, [1, 30])):
            want, nadd = np_maps.update_map(np.zeros(length, dtype=bool), pos, mass, blf, _pbc(safe))
            assert m.update(pos, np.array(mass, dtype=np.int32), blf) == nadd
            assert np.array_equal(m.words("update"), np_maps.words_of(want))
        assert np_maps.centre_and_size(pos[0], 1, 0.5)[1] == 0 and np_maps.centre_and_size(pos[0], 1, 2.0)[1] == 1


def test_map_state(api):
    length, safe = BOX_B
    pbc = _pbc(safe)
    rng = np.random.default_rng(9)
    with api.FragMap((0, 0, 0), length, safe) as m:
        box = np_maps.create_map(length, safe, pbc)
        m.fill_box()
        m.commit(False)                                                            # turn 0: frag_map = frag_map_update
        assert np.array_equal(m.words("current"), np_maps.words_of(box))
        pos, mass = groups_for(length, safe, 2.0, seed=4, count=30)
        upd, nadd = np_maps.update_map(box, pos, mass, 2.0, pbc)
        assert m.update(pos, mass, 2.0) == nadd and upd.any()
        m.commit(True)                                                             # turn 1: frag_map |= frag_map_update
        assert np.array_equal(m.words("current"), np_maps.words_of(box | upd))
        assert np.array_equal(m.words("update"), np_maps.words_of(upd))
        assert m.count("current") == int((box | upd).sum()) == int(box.sum()) + int(upd.sum())
        m.commit(False)
        assert np.array_equal(m.words("current"), np_maps.words_of(upd))
        # get / set round trip of both arrays
        a = np_maps.words_of(rng.random(length) < 0.5)
        b = np_maps.words_of(rng.random(length) < 0.1)
        m.set_words("current", a)
        m.set_words("update", b)
        assert np.array_equal(m.words("current"), a) and np.array_equal(m.words("update"), b)
        assert m.count("current") == int(np.unpackbits(a.view(np.uint8)).sum()) and m.count("update") == int(np.unpackbits(b.view(np.uint8)).sum())
        m.commit(True)
        assert np.array_equal(m.words("current"), a | b)
    # the unused bits of the last word stay zero whatever set_words is given
    length, safe = BOX_A
    with api.FragMap((0, 0, 0), length, safe) as m:
        m.set_words("current", np.full(m.nwords, 0xFFFFFFFF, dtype=np.uint32))
        w = m.words("current")
        assert _tail_is_zero(w, length) and m.count("current") == int(np.prod(length))
        with pytest.raises(ValueError):
            m.set_words("current", np.zeros(m.nwords + 1, dtype=np.uint32))


def test_refusals(api, capfd):
    with pytest.raises(api.PinfmaxError, match=r"pf_map_create: box does not fit: len\[1\] = 0 outside \[1, 2048\]"):
        api.FragMap((0, 0, 0), (8, 0, 8), (1, 1, 1))
    with pytest.raises(api.PinfmaxError, match=r"pf_map_create: box does not fit: len\[2\] = 2049 outside \[1, 2048\]"):
        api.FragMap((0, 0, 0), (8, 8, 2049), (1, 1, 1))
    with pytest.raises(api.PinfmaxError, match=r"pf_map_create: safe\[0\] = -1 in a direction that is not periodic"):
        api.FragMap((0, 0, 0), (8, 8, 8), (-1, 1, 1))
    with pytest.raises(api.PinfmaxError, match=r"pf_map_create: safe\[2\] = 5, 2 \* safe > len\[2\] = 8"):
        api.FragMap((0, 0, 0), (8, 8, 8), (1, 1, 5))
    with pytest.raises(api.PinfmaxError, match="more than 2\\^32 cells"):
        api.FragMap((0, 0, 0), (2048, 2048, 2048), (1, 1, 1))
    # with a context a direction is periodic when len == n: safe = 0 elsewhere is refused, and so is a safety layer in a periodic one
    n = 16
    with api.Fmax(n) as f:
        with pytest.raises(api.PinfmaxError, match=r"pf_map_create: safe\[1\] = 0 in a direction that is not periodic \(len\[1\] = 12\)"):
            f.frag_map((0, 0, 0), (n, 12, n), (0, 0, 0))
        with pytest.raises(api.PinfmaxError, match=r"pf_map_create: safe\[2\] = 2 in a periodic direction"):
            f.frag_map((0, 0, 0), (12, 12, n), (2, 2, 2))
        with pytest.raises(api.PinfmaxError, match=r"pf_map_create: box does not fit: len\[0\] = 17 outside \[1, 16\]"):
            f.frag_map((0, 0, 0), (n + 1, 12, n), (2, 2, 0))
        with f.frag_map((-2, 3, 0), (12, 12, n), (2, 2, 0)) as m:
            with pytest.raises(api.PinfmaxError, match="pf_distribute_map: products not computed"):
                f.distribute(1.0, (-2, 3, 0), (12, 12, n), map=m)
            with pytest.raises(ValueError, match="disagree with the map's box"):
                f.distribute(1.0, (-2, 3, 1), (12, 12, n), map=m)
            with pytest.raises(ValueError, match="disagree with the map's box"):
                f.distribute_sorted(1.0, (-2, 3, 0), (12, 11, n), map=m)
    assert "ERROR on task 0: pf_map_create: safe[1] = 0" in capfd.readouterr().out
    length, safe = BOX_B
    with api.FragMap((0, 0, 0), length, safe) as m:
        m.fill_box()
        m.commit(False)
        m.update([[5.0, 5.0, 5.0]], [100], 2.0)
        before = (m.words("current"), m.words("update"))
        # size 33 > len[0] = 32 in a periodic direction
        big = 4.188790205 * (32.6 / 2.0) ** 3
        assert np_maps.centre_and_size((0, 0, 0), int(big), 2.0)[1] == 33
        with pytest.raises(api.PinfmaxError, match=r"pf_map_update: group 1: size 33 > len\[0\] = 32 in a periodic direction"):
            m.update([[5.0, 5.0, 5.0], [6.0, 6.0, 6.0]], [100, int(big)], 2.0)
        with pytest.raises(api.PinfmaxError, match=r"pf_map_update: group 0: centre\[2\] = 33 outside \[0, 32\] in a periodic direction"):
            m.update([[5.0, 5.0, 32.6]], [100], 2.0)
        with pytest.raises(api.PinfmaxError, match=r"pf_map_update: group 0: centre\[0\] = -1 outside"):
            m.update([[-1.6, 5.0, 5.0]], [100], 2.0)
        with pytest.raises(api.PinfmaxError, match="pf_map_update: group 0 of mass -5"):
            m.update([[5.0, 5.0, 5.0]], [-5], 2.0)
        with pytest.raises(api.PinfmaxError, match=r"pf_map_update: group 0: position\[1\] = nan"):
            m.update([[5.0, np.nan, 5.0]], [100], 2.0)
        for which in (2, -1):
            with pytest.raises(api.PinfmaxError, match=f"pf_map_get: which = {which} is neither"):
                m.words(which)
            with pytest.raises(api.PinfmaxError, match="pf_map_set: which"):
                m.set_words(which, before[0])
            with pytest.raises(api.PinfmaxError, match="pf_map_count: which"):
                m.count(which)
        # ... and nothing has changed
        assert np.array_equal(m.words("current"), before[0]) and np.array_equal(m.words("update"), before[1])
        m.update([[5.0, 5.0, 32.4]], [100], 2.0)                                   # centre = len: allowed, the cube wraps once


def test_a_context_closes_its_open_maps_first(api):
    """pf_map_destroy must come before pf_destroy of the map's context: Fmax.close() sees to it for maps that are still open"""
    f = api.Fmax(16)
    m = f.frag_map((0, 0, 0), (16, 16, 16), (0, 0, 0))
    m.fill_box()
    assert m.count("update") == 16 ** 3
    f.close()
    assert m.h is None                      # destroyed with its context
    m.close()                               # ... and closing it again does nothing
    with f.__class__(16) as g:
        with g.frag_map((0, 0, 0), (16, 16, 16), (0, 0, 0)) as m2:
            assert len(g._maps) == 1
        assert len(g._maps) == 0


def test_the_word_form_issues_one_atomic_per_touched_word(api, update_cases, monkeypatch):
    """PF_MAP_STATS=1 (read when a map is created) selects kernels that count their atomics: the per-bit form issues one per
    requested cell, the word form at most as many as there are (row, word) pairs with a requested cell -- fewer than one per cell as
    soon as two requested cells of a row share a word -- and the counting kernels give the words and counts of the plain ones"""
    length, safe = BOX_D
    pos, mass, cur, upd, nadd = update_cases[(length, safe, 3.0)]
    got = {}
    monkeypatch.setenv("PF_MAP_STATS", "1")
    for form in ("1", "0"):
        monkeypatch.setenv("PF_MAP_WORDS", form)
        with api.FragMap((0, 0, 0), length, safe) as m:
            m.fill_box()
            m.commit(False)
            assert m.update(pos, mass, 3.0) == nadd and np.array_equal(m.words("update"), np_maps.words_of(upd))
            got[form] = m.atomics()
    print("atomics", got, "requested", nadd[0])
    assert got["0"] == nadd[0]
    # a row's requested cells are consecutive in z but for the cells CURRENT holds: every 32 of them share a word
    assert nadd[0] // 32 <= got["1"] < nadd[0] // 4
    monkeypatch.delenv("PF_MAP_STATS")
    with api.FragMap((0, 0, 0), length, safe) as m:
        with pytest.raises(api.PinfmaxError, match="pf_debug_map_atomics: the map was created without PF_MAP_STATS=1"):
            m.atomics()
