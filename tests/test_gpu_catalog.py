"""pf_catalog on the device against the numpy restatement of write_catalog() and compute_mf() (tests/np_catalog.py), on the cases of
tests/catalog_cases.py -- the ones tests/test_catalog_cpu.py runs through the host build of the same arithmetic and whose input
conditions it checks with the oracle alone.

Pass criteria (Case.check): count, order (ascending group_of) and the set of groups are the oracle's; name, n, M and all of q are
bit-equal to it (no transcendental function enters them); 0 <= x <= (T)(GSglobal InterPartDist hfactor), and x lies within
InterPartDist hfactor 8 ulp32(L) of the oracle's modulo the box (L the case's largest coordinate in cells: a position is a sum of at
most eight PRODFLOAT terms); v within 8 ulp32 of the sum of its terms' magnitudes; ninbin exact; massinbin bit-equal to
float64(sum of Mass) * ParticleMass and within (n_b + 1) 2^-53 relative of the oracle's running sum in batch order."""
import numpy as np
import pytest

import catalog_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


@pytest.fixture(scope="module")
def ctx(api):
    """one context per PRODFLOAT; none of them ever runs a sweep or sets a light-cone geometry"""
    made = {}

    def get(T):
        dp = np.dtype(T).itemsize == 8
        if dp not in made:
            made[dp] = api.Fmax(16, double_products=dp)
        return made[dp]
    yield get
    for f in made.values():
        f.close()


def layout_of(api, c, groups=None):
    gl = api.plc_group_layout_of((c.groups if groups is None else groups).dtype)
    if not c.flags:
        gl.off_good = gl.off_point = -1
    return gl


def run(api, ctx, c, capacity=None, groups=None, out=None, **over):
    f = ctx(c.T)
    f.set_lpt_order(c.order)
    f.plc_set_cosmology(**cc.pc.cosmology_tables(c.nk))
    g = c.groups if groups is None else groups
    kw = dict(c.call_kwargs(), **over)
    return f.catalog(groups=g, group_layout=layout_of(api, c, g), capacity=capacity, out_dtype=cc.catalog_dtype(c.T, c.light), out=out, **kw)


@pytest.mark.parametrize("name", list(cc.CASES))
def test_against_the_oracle(api, ctx, name):
    c = cc.case(name)
    rec, gof, count, nin, mas = run(api, ctx, c)
    c.check(rec, gof, count, nin, mas, printer=print)


@pytest.mark.parametrize("name", ["wrap", "wrap_f64"])
def test_wrap_case_in_closed_form(api, ctx, name):
    c = cc.case(name)
    rec, gof, count, _, _ = run(api, ctx, c)
    assert count == 4 and rec["x"].tobytes() == rec["q"].tobytes()
    assert np.array_equal(rec["q"], (c.expect_q_cells * (c.ipd * c.hfactor)).astype(c.T))


def test_the_filter(api, ctx):
    """Mass just below and at min_mass, good = 0, point = -1 (groups 3..6), and the same rows with good / point absent"""
    c, d = cc.case("n63"), cc.case("no_flags")
    gof = run(api, ctx, c)[1]
    assert 4 in gof and not np.isin([3, 5, 6], gof).any()
    gof = run(api, ctx, d)[1]
    assert np.isin([4, 5, 6], gof).all() and 3 not in gof
    gof = run(api, ctx, c, min_mass=cc.MIN_MASS + 1)[1]
    assert not np.isin([3, 4, 5, 6], gof).any()


@pytest.mark.parametrize("name", ["n63", "light", "f64_far_light"])
def test_unnamed_bytes_and_records_beyond_the_count_keep_the_callers(api, ctx, name):
    c = cc.case(name)
    dt = cc.catalog_dtype(c.T, c.light)
    full = run(api, ctx, c)
    for cap in (0, 5, c.n):
        buf = np.full(c.n * dt.itemsize, 0xA5, np.uint8)
        out = buf.view(dt)
        rec, gof, count, nin, mas = run(api, ctx, c, capacity=cap, out=out)
        m = min(cap, count)
        assert count == full[2] and len(rec) == m and count < c.n
        c.check(rec, gof, count, nin, mas, capacity=cap)
        raw = buf.reshape(c.n, dt.itemsize)
        assert (raw[m:] == 0xA5).all()
        named = np.zeros(dt.itemsize, bool)
        for k in ("name", "M", "x", "v", "q") + (() if c.light else ("n",)):
            named[dt.fields[k][1]:dt.fields[k][1] + dt.fields[k][0].itemsize] = True
        assert (~named).sum() == (0 if c.light else 4) and (raw[:m][:, ~named] == 0xA5).all()
        for k in ("name", "M", "x", "v", "q"):
            assert rec[k].tobytes() == full[0][k][:m].tobytes()
    # a layout that names x alone leaves everything else
    sub = np.dtype({"names": ["x"], "formats": [(np.dtype(c.T).str, 3)], "offsets": [dt.fields["x"][1]], "itemsize": dt.itemsize})
    buf = np.full(c.n * dt.itemsize, 0xA5, np.uint8)
    f = ctx(c.T)
    rec = f.catalog(groups=c.groups, group_layout=layout_of(api, c), out=buf.view(sub), **c.call_kwargs())[0]
    assert rec["x"].tobytes() == full[0]["x"].tobytes()
    xs = slice(dt.fields["x"][1], dt.fields["x"][1] + 3 * np.dtype(c.T).itemsize)
    raw = buf.reshape(c.n, dt.itemsize).copy()
    raw[:, xs] = 0xA5
    assert (raw == 0xA5).all()


@pytest.mark.parametrize("name", ["n4097", "n1025_seg1_nk10_o2", "f64_seg1_pbc", "hist_min1"])
def test_repeated_and_reversed_runs(api, ctx, name):
    c = cc.case(name)
    a, b = run(api, ctx, c), run(api, ctx, c)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3]) and a[4].tobytes() == b[4].tobytes()
    r = run(api, ctx, c, groups=np.ascontiguousarray(c.groups[::-1]))
    assert r[2] == a[2] and np.array_equal(r[3], a[3]) and r[4].tobytes() == a[4].tobytes()
    assert np.array_equal(c.n - 1 - r[1][::-1], a[1])
    for k in ("name", "M", "x", "v", "q"):
        assert r[0][k][::-1].tobytes() == a[0][k].tobytes(), k


def test_line_1588_and_the_v31_switch_differ(api, ctx):
    a, b = run(api, ctx, cc.case("n65_seg1")), run(api, ctx, cc.case("n65_seg1_v31"))
    assert a[2] == b[2] > 0 and not np.array_equal(a[0]["x"], b[0]["x"]) and np.array_equal(a[0]["v"], b[0]["v"])


def test_no_bins_and_no_flast(api, ctx):
    """bins = None skips the mass function; a group layout without Flast is taken"""
    c = cc.case("n63")
    full = run(api, ctx, c)
    names = [k for k in c.groups.dtype.names if k != "Flast"]
    g = np.zeros(c.n, dtype=np.dtype([(k, c.groups.dtype.fields[k][0]) for k in names], align=True))
    for k in names:
        g[k] = c.groups[k]
    f = ctx(c.T)
    rec, gof, count, nin, mas = f.catalog(groups=g, **dict(c.call_kwargs(), bins=None))
    assert nin is None and mas is None and count == full[2] and np.array_equal(gof, full[1])
    for k in ("name", "M", "x", "v", "q", "n"):
        assert rec[k].tobytes() == full[0][k].tobytes()
    rec, gof, count, nin, mas = f.catalog(groups=g, **dict(c.call_kwargs(), bins=(0, c.mmin, c.deltam)))
    assert count == full[2] and nin.size == 0 and mas.size == 0


def test_refusals(api):
    c = cc.case("n63")
    kw = c.call_kwargs()
    import ctypes as C
    from pinocchio_amd import _lib
    with api.Fmax(16) as f:
        def refused(match, **over):
            with pytest.raises(api.PinfmaxError, match=match):
                f.catalog(groups=c.groups, **dict(kw, **over))
        refused("no cosmology")
        f.plc_set_cosmology(**cc.pc.cosmology_tables(1))
        refused("myseg = -1", myseg=-1)
        for bad in (float("nan"), float("inf"), 0.0, -1.0):
            refused("F = ", F=bad)
        refused("InterPartDist", InterPartDist=0.0)
        refused("hfactor", hfactor=-0.5)
        refused("ParticleMass", ParticleMass=0.0)
        refused("deltam", bins=(c.nbin, c.mmin, 0.0))
        refused("bins", bins=(-1, c.mmin, c.deltam))
        refused("bins", bins=(2 ** 20 + 1, c.mmin, c.deltam))
        refused("len", Lgwbl=(64, 0, 64))
        refused("GSglobal", GSglobal=(128, 128, -1))
        gl = api.plc_group_layout_of(c.groups.dtype)
        gl.off_Vel_3LPT_2_prev = gl.stride - 4
        refused("leaves the record", group_layout=gl)
        # ParticleMass is not read without bins
        assert f.catalog(groups=c.groups, **dict(kw, ParticleMass=0.0, bins=None))[2] == len(c.oracle()["index"])
        # straight through the C ABI: null arguments and too many groups; every refusal leaves *count = 0
        L = f.L
        seg, rg = _lib.PlcSegment(0, 0, 0.0, 0.0), api._region((c.stabl, c.lgwbl, (0, 0, 0)))
        par = _lib.CatalogParams(F=1.15, InterPartDist=c.ipd, ParticleMass=c.pmass, hfactor=1.0, GSglobal=(C.c_longlong * 3)(128, 128, 128), pbc=(C.c_int * 3)(0, 0, 0), min_mass=10)
        gl = api.plc_group_layout_of(c.groups.dtype)
        gp = c.groups.ctypes.data_as(C.c_void_p)
        cnt = C.c_size_t(77)
        call = lambda seg_, rg_, par_, n_, gp_, gl_, bins_=None: L.pf_catalog(f.h, seg_, rg_, par_, n_, gp_, gl_, 0, None, None, None, bins_, None, None, C.byref(cnt))
        for args in ((None, C.byref(rg), C.byref(par), c.n, gp, C.byref(gl)), (C.byref(seg), None, C.byref(par), c.n, gp, C.byref(gl)),
                     (C.byref(seg), C.byref(rg), None, c.n, gp, C.byref(gl)), (C.byref(seg), C.byref(rg), C.byref(par), c.n, None, C.byref(gl)),
                     (C.byref(seg), C.byref(rg), C.byref(par), c.n, gp, None), (C.byref(seg), C.byref(rg), C.byref(par), 2 ** 31, gp, C.byref(gl)),
                     (C.byref(seg), C.byref(rg), C.byref(par), c.n, gp, C.byref(gl), C.byref(_lib.MfBins(10, c.mmin, c.deltam)))):
            cnt.value = 77
            assert call(*args) == 1 and cnt.value == 0
        # an output layout whose q leaves the record (numpy makes no such dtype)
        buf, ol = np.full(c.n * 48, 0xA5, np.uint8), _lib.CatalogOutLayout(48, 0, 8, 12, 24, 40, -1)
        cnt.value = 77
        assert L.pf_catalog(f.h, C.byref(seg), C.byref(rg), C.byref(par), c.n, gp, C.byref(gl), c.n, buf.ctypes.data_as(C.c_void_p), C.byref(ol), None, None, None, None,
                            C.byref(cnt)) == 1 and cnt.value == 0 and (buf == 0xA5).all() and "leaves the record" in L.pf_last_error().decode()
        par.F = float("nan")
        cnt.value = 77
        assert call(C.byref(seg), C.byref(rg), C.byref(par), c.n, gp, C.byref(gl)) == 1 and cnt.value == 0
        assert L.pf_debug_catalog_times(None) == 1
        # a refused call leaves the context as it was: it still answers
        rec, gof, count, nin, mas = f.catalog(groups=c.groups, **kw)
        c.check(rec, gof, count, nin, mas)
