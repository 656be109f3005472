"""pf_plc_cross on the device against the numpy restatement of the reference's light-cone test (tests/np_plc.py), on the cases of
tests/plc_cases.py -- the ones tests/test_plc_cpu.py runs through the host build of the same arithmetic and whose input conditions it
checks with the oracle alone.

Pass criteria (Case.check): the stored (candidate, replication) pairs are the oracle's, but for pairs whose oracle |aa| or |bb|
lies below 8 ulp32(L) cells (a position is a sum of at most eight fp32 terms of magnitude <= L, the largest coordinate of the
case); the oracle evaluated at the DEVICE's F gives |condition| < 1e-2 InterPartDist, and F_lo <= F <= Flast; x within
InterPartDist 8 ulp32(L) and v within 8 ulp32 of the sum of its terms' magnitudes of the oracle's store_PLC at that F; z, Mass and
name exact; *unconverged == 0; the n(z) histogram exact."""
import numpy as np
import pytest

import plc_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


@pytest.fixture(scope="module")
def ctx(api):
    """one context per PRODFLOAT; none of them ever runs a sweep"""
    made = {}

    def get(T):
        dp = np.dtype(T).itemsize == 8
        if dp not in made:
            made[dp] = api.Fmax(16, double_products=dp)
        return made[dp]
    yield get
    for f in made.values():
        f.close()


def run(api, ctx, c, capacity=None, groups=None, f_lo=None, layout=None, want_nz=True):
    f = ctx(c.T)
    f.set_lpt_order(c.order)
    f.plc_set_cosmology(**pc.cosmology_tables(c.nk))
    f.plc_set_geometry(**c.geometry_kwargs())
    nz = np.zeros(c.nzbins) if want_nz else None
    g = c.groups if groups is None else groups
    rec, cand, rep, count, unc = f.plc_cross(api.PLC_EVENTS if c.events else api.PLC_LAST_CHECK, c.myseg, c.z_seg, c.stabl, g, group_layout=layout, z_prev=c.z_prev,
                                             use_v31=c.use_v31, f_lo=(c.f_lo if f_lo is None else f_lo) if c.events else None, min_mass=c.min_mass,
                                             capacity=capacity, out_dtype=pc.out_dtype(c.T), nz=nz)
    return rec, cand, rep, count, unc, nz


@pytest.mark.parametrize("name", list(pc.CASES))
def test_against_the_oracle(api, ctx, name):
    c = pc.case(name)
    rec, cand, rep, count, unc, nz = run(api, ctx, c)
    print(name, "tried", int(c.oracle()["tried"].sum()), "stored", count, "unconverged", unc)
    c.check(rec, cand, rep, count, unc)
    assert np.array_equal(nz, c.nz_expected(rec))
    print(name, "x and v bit-equal to the oracle's:", getattr(c, "last_bit_equal", None))


def test_the_crossing_sets(api, ctx):
    count = lambda name: run(api, ctx, pc.case(name))[3]
    assert count("n0") == 0 and count("none") == 0 and count("n1_r1_all") == 1 and count("all_r65") == 64 * 65
    rec, cand, rep, n, _, _ = run(api, ctx, pc.case("last_r65"))
    assert n == 1 and cand.tolist() == [64] and rep.tolist() == [64]
    # Flast == F2 is tried at an event and not in the last check; F_lo == F1 is tried
    assert run(api, ctx, pc.case("equality_events"))[1].tolist() == [0, 1] and run(api, ctx, pc.case("equality_last_check"))[1].tolist() == [0]
    assert run(api, ctx, pc.case("equality_events_f64"))[1].tolist() == [0, 1]
    # a group of no extent (Mass 0: interp at its top, k > kmax) is among the stored records of the scale-dependent cases
    for name in ("nk10", "f64_nk10", "n1025_r65_events_seg1_nk10_o2"):
        assert (run(api, ctx, pc.case(name))[0]["Mass"] == 0).any(), name
    # the aperture: the groups at 25 degrees are stored, those at 35 are not
    assert run(api, ctx, pc.case("aperture"))[1].tolist() == list(range(0, 64, 2))


def test_the_filter(api, ctx):
    """Mass just below and at min_mass, good = 0, point = -1 (candidates 3..6 of the random cases), and absent good / point offsets"""
    c = pc.case("n63_r13")
    g = c.groups
    assert g["Mass"][3] == pc.MIN_MASS - 1 and g["Mass"][4] == pc.MIN_MASS and g["good"][5] == 0 and g["point"][6] == -1
    o = c.oracle()
    assert o["tried"][4].any() and not o["tried"][[3, 5, 6]].any()
    rec, cand, rep, count, unc, _ = run(api, ctx, c)
    assert not np.isin(cand, [3, 5, 6]).any()
    # make candidate 4 cross for certain: the same group once more, with a Mass of min_mass and of one less
    layout = api.plc_group_layout_of(g.dtype)
    layout.off_good = layout.off_point = -1
    rec2, cand2, rep2, count2, unc2, _ = run(api, ctx, c, layout=layout)
    o2 = c.oracle(False)
    want = set(zip(o2["cand"][o2["store"]["inside"]].tolist(), o2["rep"][o2["store"]["inside"]].tolist()))
    assert set(zip(cand2.tolist(), rep2.tolist())) == want and count2 >= count and unc2 == 0
    assert not (cand2 == 3).any() and o2["tried"][[5, 6]].any()
    # min_mass alone: one more and candidate 4 is out as well
    f = ctx(c.T)
    rec3, cand3, _, _, _ = f.plc_cross(api.PLC_LAST_CHECK, c.myseg, c.z_seg, c.stabl, g, min_mass=pc.MIN_MASS + 1, out_dtype=pc.out_dtype(c.T))
    assert not np.isin(cand3, [3, 4, 5, 6]).any() and set(cand3.tolist()) <= set(cand.tolist())


def test_capacity(api, ctx):
    c = pc.case("n63_r13")
    full = run(api, ctx, c)
    assert full[3] > 5
    for cap in (0, 5, full[3]):
        rec, cand, rep, count, unc, nz = run(api, ctx, c, capacity=cap)
        assert count == full[3] and len(rec) == min(cap, count)
        assert np.array_equal(rec, full[0][:cap]) and np.array_equal(cand, full[1][:cap]) and np.array_equal(rep, full[2][:cap])
        assert np.array_equal(nz, c.nz_expected(rec))
        c.check(rec, cand, rep, count, unc, capacity=cap)


@pytest.mark.parametrize("name", ["n4097_r13", "n1025_r65_events_seg1_nk10_o2", "f64_seg1_events_r65"])
def test_repeated_and_permuted_runs_are_bit_identical(api, ctx, name):
    c = pc.case(name)
    a = run(api, ctx, c)
    b = run(api, ctx, c)
    same = lambda r, q: all(r[k].tobytes() == q[k].tobytes() for k in ("Mass", "name", "z", "x", "v"))   # (field by field: the records have padding)
    assert same(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3:5] == b[3:5] and np.array_equal(a[5], b[5])
    perm = np.random.default_rng(99).permutation(c.ncand)
    p = run(api, ctx, c, groups=np.ascontiguousarray(c.groups[perm]), f_lo=np.ascontiguousarray(c.f_lo[perm]) if c.events else None)
    orig = perm[p[1]]                                      # the candidate of every record in the unpermuted numbering
    order = np.lexsort((p[2], orig))
    assert p[3] == a[3] and np.array_equal(orig[order], a[1]) and np.array_equal(p[2][order], a[2])
    assert same(p[0][order], a[0]) and np.array_equal(p[5], a[5])


def test_line_1588_and_the_v31_switch_differ(api, ctx):
    a, b = run(api, ctx, pc.case("n65_r13_seg1")), run(api, ctx, pc.case("n65_r13_seg1_v31"))
    assert a[3] > 0 and b[3] > 0
    same = min(a[3], b[3])
    assert a[3] != b[3] or not np.array_equal(a[0]["x"][:same], b[0]["x"][:same])


def test_refusals(api):
    c = pc.case("n63_r13")
    kw = pc.cosmology_tables(1)
    args = (c.myseg, c.z_seg, c.stabl, c.groups)
    with api.Fmax(16) as f:
        with pytest.raises(api.PinfmaxError, match="no cosmology"):
            f.plc_cross(api.PLC_LAST_CHECK, *args)
        f.plc_set_cosmology(**kw)
        with pytest.raises(api.PinfmaxError, match="no geometry"):
            f.plc_cross(api.PLC_LAST_CHECK, *args)
        f.plc_set_geometry(**c.geometry_kwargs())
        with pytest.raises(api.PinfmaxError, match="mode 7"):
            f.plc_cross(7, *args)
        with pytest.raises(api.PinfmaxError, match="f_lo"):
            f.plc_cross(api.PLC_EVENTS, *args)
        # the setters: knots that do not increase, nk out of range, no replications, a table that is not finite
        bad = dict(kw, x=kw["x"][::-1].copy())
        with pytest.raises(api.PinfmaxError, match="do not increase"):
            f.plc_set_cosmology(**bad)
        bad = dict(kw, grow=np.repeat(kw["grow"], 33, axis=1), fomega=np.repeat(kw["fomega"], 33, axis=1))
        with pytest.raises(api.PinfmaxError, match="nk = 33"):
            f.plc_set_cosmology(**bad)
        bad = dict(kw, hubble=np.where(np.arange(kw["x"].size) == 3, np.nan, kw["hubble"]))
        with pytest.raises(api.PinfmaxError, match="not finite"):
            f.plc_set_cosmology(**bad)
        with pytest.raises(api.PinfmaxError, match="no replications"):
            f.plc_set_geometry(**dict(c.geometry_kwargs(), repls=[]))
        L = f.L
        assert L.pf_plc_set_cosmology(f.h, None) == 1 and L.pf_plc_set_geometry(f.h, None) == 1
        # a refused call leaves what was set: the context still answers
        rec, cand, rep, count, unc = f.plc_cross(api.PLC_LAST_CHECK, *args, min_mass=c.min_mass)
        c.check(rec, cand, rep, count, unc)
