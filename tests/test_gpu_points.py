"""The particle states at collapse time on the device (pf_point_states, pf_debug_point_states; csrc/pf_points.hip) against the numpy
restatement of the reference's lines (tests/np_points.py), under the pass criteria of tests/points_cases.py -- the ones
tests/test_points_cpu.py applies to the same arithmetic compiled for the host.  Every found particle is judged; none is excluded."""
import ctypes as C

import numpy as np
import pytest

import np_points as npo
import np_refresh as npr
import plc_cases as pc
import points_cases as qc
from pinocchio_amd import synth
from test_gpu_multirank import run_ranks

pytestmark = pytest.mark.gpu

RADII = np.array([2.0, 1.0, 0.5, 0.0])
G1 = synth.growth_multipliers()
G2 = G1 * np.array([0.75, 0.5, 0.625, 0.875])
BOX16 = ((-3, 0, 13), (7, 16, 5), (1, 0, 1))
BIG16 = ((-3, 0, 13), (12, 16, 10), (1, 0, 1))                  # the sub-box of points_cases.BOX16: y periodic, 1920 cells
PERIODIC16 = [False, True, False]
SIGMA0, K = 1.7, 0.1
Z_SEG, Z_PREV = 0.0, 0.3
FLAST = 1.0


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


@pytest.fixture(scope="module")
def tables(api):
    """a context per nk that holds the cosmology tables and nothing else"""
    ctx = {}
    for nk in (1, 10):
        ctx[nk] = api.Fmax(16)
        ctx[nk].plc_set_cosmology(**pc.cosmology_tables(nk))
    yield ctx
    for f in ctx.values():
        f.close()


def _tap(api, tables, c, hint=None):
    return api.debug_point_states(c.n, c.x0, c.fmax, c.cols, tables[c.nk], c.myseg, Z_SEG, (c.start, c.length, c.safe), c.pos, qc.SIGMA0, c.k_sigma, c.k_point,
                                  groups_order=c.order, z_prev=Z_PREV, use_v31=c.use_v31, order=hint)


# ------------------------------------------------------------------------------------------------------------------------
# the tap on prescribed columns
@pytest.mark.parametrize("name", qc.TAP_CASES)
def test_the_tap_against_the_restatement(api, tables, name):
    c = qc.case(name)
    index, st = _tap(api, tables, c)
    c.check(index, st, len(index), printer=print)
    # the hint changes which thread serves which particle and nothing else
    i2, s2 = _tap(api, tables, c, c.hint())
    assert i2.tobytes() == index.tobytes() and s2.tobytes() == st.tobytes(), name
    if c.count > 64:
        i3, s3 = _tap(api, tables, c, np.random.default_rng(3).permutation(c.count).astype(np.int32))
        assert i3.tobytes() == index.tobytes() and s3.tobytes() == st.tobytes(), name
    # ... and a second run gives the same bytes
    i4, s4 = _tap(api, tables, c)
    assert i4.tobytes() == index.tobytes() and s4.tobytes() == st.tobytes(), name


def test_found_below_count_and_a_miss(api, tables):
    a, b = qc.case("slab24"), qc.case("miss24")
    assert 0 < len(_tap(api, tables, a)[0]) < a.count
    index, st = _tap(api, tables, b)
    assert len(index) == 0 and st.shape == (0, 8)


@pytest.mark.parametrize("name", ["wrap_zero", "wrap_zero_f64_seg1"])
def test_without_velocities_x_is_q_to_the_byte(api, tables, name):
    c = qc.case(name)
    _, st = _tap(api, tables, c)
    q = c.oracle()["q"]
    assert st[:, 5:].tobytes() == q.tobytes() and (q[:, 1] == c.T(15.5)).any()


@pytest.mark.parametrize("name", ["wrap_both", "wrap_both_seg1_f64"])
def test_both_wrap_branches_are_taken(api, tables, name):
    c = qc.case(name)
    _, st = _tap(api, tables, c)
    o = c.oracle()
    y, q = st[:, 6].astype(np.float64), o["q"][:, 1].astype(np.float64)
    assert (y >= 0).all() and (y <= 16).all()
    assert (y[o["hi"][:, 1]] < q[o["hi"][:, 1]]).all() and o["hi"][:, 1].any()       # left through the upper face, came back below
    assert (y[o["lo"][:, 1]] > q[o["lo"][:, 1]]).all() and o["lo"][:, 1].any()


def test_line_1588_and_the_v31_switch_differ(api, tables):
    a, b = _tap(api, tables, qc.case("seg1_o3")), _tap(api, tables, qc.case("seg1_o3_v31"))
    assert len(a[0]) == len(b[0]) > 0 and not np.array_equal(a[1][:, 5:], b[1][:, 5:]) and np.array_equal(a[1][:, :5], b[1][:, :5])


# ------------------------------------------------------------------------------------------------------------------------
# with a context
def _first_segment(f, dk, order=3, nk=1):
    f.set_density(dk)
    f.set_invgrow(*synth.invgrow_table("lcdm"))
    f.set_lpt_order(order)
    f.sweep(RADII)
    f.set_growth(G1)
    f.compute_displacements(1, 0)
    f.plc_set_cosmology(**pc.cosmology_tables(nk))


def _next_segment(f, g):
    f.shift_displacements()
    f.set_growth(g)
    f.compute_displacements(0, 0)


def _cols_of(*products):
    out = []
    for p in products:
        p = p.reshape(-1)
        for name in ("Vel", "Vel_2LPT", "Vel_3LPT_1", "Vel_3LPT_2"):
            out += [np.ascontiguousarray(p[name][:, e]) for e in range(3)]
    return np.stack(out)


def _stored(A, box, n=16, fhi=None):
    """the positions of the sub-box whose cell has Fmax >= FLAST (and <= fhi), as distribute() stores them, some of them twice"""
    start, length, _ = box
    allpos = np.arange(int(np.prod(length)), dtype=np.uint32)
    _, cell = npr.cells(n, 0, n, start, length, allpos)
    F = A.reshape(-1)["Fmax"][cell]
    keep = (F >= FLAST) if fhi is None else ((F >= FLAST) & (F <= fhi))
    pos = allpos[keep]
    rng = np.random.default_rng(len(pos))
    return rng.permutation(np.concatenate([pos, pos[::7]])).astype(np.uint32)


def _want(nk, n, x0, nxl, box, pos, cur, prv, myseg, order, lpt, k_point=K, k_sigma=K, z_prev=Z_PREV):
    start, length, _ = box
    return npo.states(pc.cosmology(nk), n, x0, nxl, start, length, pos, np.ascontiguousarray(cur.reshape(-1)["Fmax"]), _cols_of(cur, prv), myseg, Z_SEG, z_prev, False,
                      order, SIGMA0, k_sigma, k_point, lpt)


def _band(o, length):
    L = float(max(length))
    if len(o["index"]):
        L = max(L, float(np.abs(o["states"][:, 5:].astype(np.float64)).max()))
    return 8.0 * float(np.spacing(np.float32(L)))


def _check(name, T, got, o, box, cap=None):
    index, st, found = got
    m = len(o["index"]) if cap is None else min(cap, len(o["index"]))
    assert found == len(o["index"]) and index.dtype == np.uint32 and np.array_equal(index, o["index"][:m]), name
    x = o["states"][:, 6].astype(np.float64)
    assert ((x >= 0) & (x <= 16)).all(), name               # the inputs' own condition: no displacement of a box length
    return qc.check_states(T, st, o["states"][:m], box[1], PERIODIC16, _band(o, box[1]), name, print)


@pytest.mark.parametrize("lpt", [1, 2, 3])
def test_orders_against_contexts_of_every_lpt_order(api, lpt):
    n = 16
    with api.Fmax(n) as f:
        _first_segment(f, synth.make_density(n, seed=5), lpt)
        A = f.products()
        pos = _stored(A, BOX16)
        assert len(pos) > 100
        hint = np.argsort(pos, kind="stable").astype(np.int32)
        for order in (1, 2, 3):
            got = f.point_states(0, Z_SEG, BOX16, pos, SIGMA0, K, K, groups_order=order)
            o = _want(1, n, 0, n, BOX16, pos, A, np.zeros_like(A), 0, order, lpt)
            _check(f"lpt {lpt} order {order}", np.float32, got, o, BOX16)
            for fam in range(4):
                assert (not got[1][:, fam].any()) == (fam >= {1: 1, 2: 2, 3: 4}[lpt]), (lpt, fam)
            again = f.point_states(0, Z_SEG, BOX16, pos, SIGMA0, K, K, groups_order=order, order=hint)
            assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()


@pytest.mark.parametrize("dp", [False, True])
def test_two_segments_on_one_rank(api, dp):
    """fragment.c:398-410 as tests/test_gpu_refresh.py sets it up: a first segment, pf_shift_displacements and a second pf_displacements;
    then myseg = 1 reads both sets of columns.  nk = 10 with the two k values in different bins"""
    n = 16
    T = np.float64 if dp else np.float32
    with api.Fmax(n, double_products=dp) as f:
        _first_segment(f, synth.make_density(n, seed=5), 3, nk=10)
        A = f.products()
        with pytest.raises(api.PinfmaxError, match="pf_point_states: myseg = 1 reads the Vel\\*_prev columns but there is no pf_shift_displacements yet"):
            f.point_states(1, Z_SEG, BIG16, _stored(A, BIG16), SIGMA0, K, K, z_prev=1.0)
        _next_segment(f, G2)
        B = f.products()
        assert np.any(B["Vel"] != A["Vel"]) and B["Fmax"].tobytes() == A["Fmax"].tobytes()
        pos = _stored(B, BIG16, fhi=2.0)                      # the collapse times of a segment z = 1 .. 0
        assert len(pos) > 100
        hint = np.argsort(pos, kind="stable").astype(np.int32)
        for order, kp, ks in ((2, 0.02, 1.2), (3, 1.2, 5e-4)):
            got = f.point_states(1, Z_SEG, BIG16, pos, SIGMA0, ks, kp, groups_order=order, z_prev=1.0, order=hint)
            o = _want(10, n, 0, n, BIG16, pos, B, A, 1, order, 3, kp, ks, z_prev=1.0)
            _check(f"two segments, order {order}", T, got, o, BIG16)
            plain = f.point_states(1, Z_SEG, BIG16, pos, SIGMA0, ks, kp, groups_order=order, z_prev=1.0)
            assert plain[0].tobytes() == got[0].tobytes() and plain[1].tobytes() == got[1].tobytes()
        # myseg = 0 on the same context reads the current columns alone
        pos0 = _stored(B, BIG16)
        got = f.point_states(0, Z_SEG, BIG16, pos0, SIGMA0, K, K)
        _check("two segments, myseg 0", T, got, _want(10, n, 0, n, BIG16, pos0, B, A, 0, 2, 3), BIG16)


@pytest.mark.parametrize("P", [1, 2, 4])
def test_every_rank_finds_its_own(api, P):
    """P ranks on one GPU through the in-process fabric; each rank's call finds the particles of its slab: disjoint sets, together all"""
    n = 16
    nxl = n // P
    dk = synth.make_density(n, seed=8)
    box = ((0, 0, 0), (16, 16, 16), (0, 0, 0))

    with api.Fmax(n) as f1:                                       # which particles are stored: from the one-rank context
        _first_segment(f1, dk, 2)
        pos = _stored(f1.products(), box)
    assert len(pos) > 500
    hint = np.argsort(pos, kind="stable").astype(np.int32)

    def body2(f, r):
        _first_segment(f, dk[r * nxl:(r + 1) * nxl], 2)
        return f.products(), f.point_states(0, Z_SEG, box, pos, SIGMA0, K, K), f.point_states(0, Z_SEG, box, pos, SIGMA0, K, K, order=hint)

    if P == 1:
        with api.Fmax(n) as f1:
            res = [body2(f1, 0)]
    else:
        res = run_ranks(api, n, P, body2)
    seen = np.zeros(len(pos), dtype=int)
    for r, (A, got, hinted) in enumerate(res):
        o = _want(1, n, r * nxl, nxl, box, pos, A, np.zeros_like(A), 0, 2, 2)
        index, st, found = got
        assert found == len(o["index"]) and np.array_equal(index, o["index"])
        qc.check_states(np.float32, st, o["states"], box[1], [True, True, True], _band(o, box[1]), f"P {P} rank {r}", print)
        assert hinted[0].tobytes() == index.tobytes() and hinted[1].tobytes() == st.tobytes()
        seen[index] += 1
    assert np.all(seen == 1)


def test_a_capacity_below_the_count(api):
    n = 16
    with api.Fmax(n) as f:
        _first_segment(f, synth.make_density(n, seed=5))
        A = f.products()
        pos = _stored(A, BIG16)
        o = _want(1, n, 0, n, BIG16, pos, A, np.zeros_like(A), 0, 2, 3)
        total = len(o["index"])
        assert total == len(pos) > 300
        full = f.point_states(0, Z_SEG, BIG16, pos, SIGMA0, K, K)
        _check("full", np.float32, full, o, BIG16)
        for hint in (None, np.argsort(pos, kind="stable").astype(np.int32)):
            for cap in (0, 1, 255, 256, 300, total - 1):
                index, st, found = f.point_states(0, Z_SEG, BIG16, pos, SIGMA0, K, K, order=hint, capacity=cap)
                assert found == total and len(index) == cap                       # the counting goes on
                assert index.tobytes() == full[0][:cap].tobytes() and st.tobytes() == full[1][:cap].tobytes()
        # a count alone, and either output alone, with canaries behind the capacity
        from pinocchio_amd import _lib
        L = _lib.load()
        rg = api._region(BIG16)
        seg, par = _lib.PlcSegment(0, 0, Z_SEG, Z_PREV), _lib.PointParams(SIGMA0, K, K, 2)
        up = C.POINTER(C.c_uint)
        found = C.c_size_t()
        assert L.pf_point_states(f.h, C.byref(seg), C.byref(rg), C.byref(par), len(pos), pos.ctypes.data_as(up), None, total, None, None, C.byref(found)) == 0
        assert found.value == total
        index = np.full(300 + 8, 0xDEADBEEF, dtype=np.uint32)
        st = np.full(8 * 300 + 8, -7.0, dtype=np.float32)
        assert L.pf_point_states(f.h, C.byref(seg), C.byref(rg), C.byref(par), len(pos), pos.ctypes.data_as(up), None, 300, index.ctypes.data_as(up), None, None) == 0
        assert L.pf_point_states(f.h, C.byref(seg), C.byref(rg), C.byref(par), len(pos), pos.ctypes.data_as(up), None, 300, None, C.c_void_p(st.ctypes.data), None) == 0
        assert index[:300].tobytes() == full[0][:300].tobytes() and st[:2400].tobytes() == full[1][:300].tobytes()
        assert np.all(index[300:] == 0xDEADBEEF) and np.all(st[2400:] == -7.0)


def test_refusals(api, tables, capfd):
    """decided on the host, before anything is launched: an error with a message, *found = 0, the context usable afterwards"""
    from pinocchio_amd import _lib
    L = _lib.load()
    n = 16
    start, length, safe = BOX16
    up, ip = C.POINTER(C.c_uint), C.POINTER(C.c_int)
    with api.Fmax(n) as f:
        f.set_density(synth.make_density(n, seed=5))
        f.set_invgrow(*synth.invgrow_table("lcdm"))
        f.sweep(RADII)
        f.set_growth(G1)
        f.compute_displacements(1, 0)
        A = f.products()
        pos = _stored(A, BOX16)
        count = len(pos)
        with pytest.raises(api.PinfmaxError, match="pf_point_states: no cosmology set \\(pf_plc_set_cosmology\\)"):
            f.point_states(0, Z_SEG, BOX16, pos, SIGMA0, K, K)
        f.plc_set_cosmology(**pc.cosmology_tables(1))
        good = f.point_states(0, Z_SEG, BOX16, pos, SIGMA0, K, K)
        assert good[2] == count

        def refused(match, call):
            with pytest.raises(api.PinfmaxError, match=match):
                call()
            again = f.point_states(0, Z_SEG, BOX16, pos, SIGMA0, K, K)
            assert again[2] == count and again[1].tobytes() == good[1].tobytes(), match

        refused("pf_point_states: myseg = 1 reads the Vel\\*_prev columns but there is no pf_shift_displacements yet",
                lambda: f.point_states(1, Z_SEG, BOX16, pos, SIGMA0, K, K, z_prev=Z_PREV))
        refused("pf_point_states: myseg = -1", lambda: f.point_states(-1, Z_SEG, BOX16, pos, SIGMA0, K, K))
        for order in (0, 4, -2):
            refused("pf_point_states: order = %d \\(1 to 3\\)" % order, lambda: f.point_states(0, Z_SEG, BOX16, pos, SIGMA0, K, K, groups_order=order))
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            refused("pf_point_states: sigma0 = .* must be positive and finite", lambda: f.point_states(0, Z_SEG, BOX16, pos, bad, K, K))
            refused("pf_point_states: k_sigma = .* must be positive and finite", lambda: f.point_states(0, Z_SEG, BOX16, pos, SIGMA0, bad, K))
            refused("pf_point_states: k_point = .* must be positive and finite", lambda: f.point_states(0, Z_SEG, BOX16, pos, SIGMA0, K, bad))
        refused("pf_point_states: box does not fit: len\\[0\\] = 17", lambda: f.point_states(0, Z_SEG, (start, (17, 16, 5), safe), pos, SIGMA0, K, K))
        refused("pf_point_states: safe\\[0\\] = 0 in a direction that is not periodic", lambda: f.point_states(0, Z_SEG, ((0, 0, 0), (8, 8, 8), (0, 0, 0)), pos, SIGMA0, K, K))
        bad = pos.copy()
        bad[250] = 2 ** 32 - 1
        bad[5] = 560
        refused(r"pf_point_states: frag_pos\[5\] = 560 lies outside the 560 cells of the box", lambda: f.point_states(0, Z_SEG, BOX16, bad, SIGMA0, K, K))
        hint = np.argsort(pos, kind="stable").astype(np.int32)
        hint[7] = count
        hint[200] = -1
        refused(r"pf_point_states: order\[7\] = %d is no index of the %d particles" % (count, count), lambda: f.point_states(0, Z_SEG, BOX16, pos, SIGMA0, K, K, order=hint))
        # through the C ABI: null arguments, 2^31 particles, and *found = 0 after each
        rg = api._region(BOX16)
        seg, par = _lib.PlcSegment(0, 0, Z_SEG, Z_PREV), _lib.PointParams(SIGMA0, K, K, 2)
        index, st = np.zeros(count, np.uint32), np.zeros((count, 8), np.float32)
        args = [f.h, C.byref(seg), C.byref(rg), C.byref(par), count, pos.ctypes.data_as(up), None, count, index.ctypes.data_as(up), C.c_void_p(st.ctypes.data)]
        for k in (0, 1, 2, 3, 5):
            a = list(args)
            a[k] = None
            found = C.c_size_t(99)
            assert L.pf_point_states(*a, C.byref(found)) == 1 and found.value == 0 and L.pf_last_error().decode() == "pf_point_states: null argument", k
        a = list(args)
        a[4] = 2 ** 31
        found = C.c_size_t(99)
        assert L.pf_point_states(*a, C.byref(found)) == 1 and found.value == 0
        assert L.pf_last_error().decode() == "pf_point_states: 2147483648 particles: indices[] is int as in the reference, 2^31 - 1 particles at most"
        found = C.c_size_t(99)
        assert L.pf_point_states(*args, C.byref(found)) == 0 and found.value == count and st.tobytes() == good[1].tobytes()
    with api.Fmax(n) as f:                                        # nothing computed
        f.plc_set_cosmology(**pc.cosmology_tables(1))
        with pytest.raises(api.PinfmaxError, match="pf_point_states: products not computed"):
            f.point_states(0, Z_SEG, BOX16, pos, SIGMA0, K, K)
    # the tap refuses the same
    c = qc.case("c777")
    box = (c.start, c.length, c.safe)
    with pytest.raises(api.PinfmaxError, match=r"pf_debug_point_states: frag_pos\[5\] = 1920 lies outside the 1920 cells"):
        p = c.pos.copy()
        p[5] = 1920
        api.debug_point_states(c.n, 0, c.fmax, c.cols, tables[1], 0, Z_SEG, box, p, SIGMA0, K, K)
    with pytest.raises(api.PinfmaxError, match=r"pf_debug_point_states: order\[7\] = 777"):
        h = c.hint()
        h[7] = 777
        api.debug_point_states(c.n, 0, c.fmax, c.cols, tables[1], 0, Z_SEG, box, c.pos, SIGMA0, K, K, order=h)
    with pytest.raises(api.PinfmaxError, match="pf_debug_point_states: order = 7"):
        api.debug_point_states(c.n, 0, c.fmax, c.cols, tables[1], 0, Z_SEG, box, c.pos, SIGMA0, K, K, groups_order=7)
    with pytest.raises(api.PinfmaxError, match="pf_debug_point_states: k_point = 0 must be positive"):
        api.debug_point_states(c.n, 0, c.fmax, c.cols, tables[1], 0, Z_SEG, box, c.pos, SIGMA0, K, 0.0)
    with api.Fmax(n) as bare:
        with pytest.raises(api.PinfmaxError, match="pf_debug_point_states: no cosmology set"):
            api.debug_point_states(c.n, 0, c.fmax, c.cols, bare, 0, Z_SEG, box, c.pos, SIGMA0, K, K)
    with pytest.raises(api.PinfmaxError, match="planes 12 .. 27 of a box of 16"):
        api.debug_point_states(c.n, 12, c.fmax, c.cols, tables[1], 0, Z_SEG, box, c.pos, SIGMA0, K, K)
    out = capfd.readouterr().out
    assert "ERROR on task 0: pf_point_states: frag_pos[5]" in out and "ERROR on task 0: pf_point_states: no cosmology set" in out


def test_the_times_are_off_without_the_switch(api):
    assert api.point_times() == (0.0, 0.0) or all(t >= 0.0 for t in api.point_times())
