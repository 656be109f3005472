"""The matter-density call on slabs (include/pinfmax.h: pf_matter_power_slabs, pf_debug_matter_slabs, pf_debug_matter_exchange): P
contexts on one GPU through the in-process fabric (run_ranks of tests/test_gpu_multirank.py).  The contract is exact: on any number
of ranks every rank receives the bits one rank returns for the same box.  So every comparison here is an equality of integers or of
the bits of doubles -- the grids against the one-rank restatement of the whole box (tests/np_matter.py), the plan against its
brute-force statement (tests/np_matter_slabs.py), the whole call against pf_matter_power on a one-rank context."""
import ctypes as C
import functools

import numpy as np
import pytest

import np_matter as npm
import np_matter_slabs as nps
from pinocchio_amd import synth
from test_gpu_multirank import run_ranks
from test_gpu_power import same_bits

pytestmark = pytest.mark.gpu

INT_KEYS = ("deposited", "nonfinite", "outside", "empty_cells", "max_cell", "sum_hi32", "sum_lo32")
INFO_KEYS = INT_KEYS + ("modes", "nonfinite_modes")
NAMES = ("Vel", "Vel_2LPT", "Vel_3LPT_1", "Vel_3LPT_2")
# The densities of the whole-call cases, (n, P, field bytes, sigma(R = 0) of synth.make_density, keywords).  The sigma0 decide how far
# the particles go, and so which form of the exchange a case takes; the common reach (below, above) in planes, from one-rank products
# through np_matter_slabs.box_reach before the values were fixed here (the test asserts every one of them again from `exchange`):
#   (32, 2) 2.5 -> (16, 15): the whole box;  (64, 4) 1.0 -> (5, 5): ghost planes, B = 5;  (48, 3) 2.5 -> (16, 18): the whole box;
#   (64, 8) 0.4 -> (2, 2): ghost planes, B = 2, the production-like case, which cannot pass with nothing crossing;
#   (16, 16) 1.0 -> (2, 3): slabs of one plane, every ghost region spans several owners
WHOLE = [(32, 2, 8, 2.5, {}), (64, 4, 8, 1.0, {"deconvolve": True, "weight": (1.0, 1.0, 0.0, 0.0)}), (48, 3, 8, 2.5, {}), (64, 8, 4, 0.4, {}),
         (16, 16, 8, 1.0, {"ngp": True})]


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


class DoubleProducts:
    """what run_ranks asks of the module, with contexts that keep fp64 products"""

    def __init__(self, api):
        self.api = api

    def Fmax(self, *a, **k):
        return self.api.Fmax(*a, double_products=True, **k)


@functools.lru_cache(maxsize=None)
def planted(n, P, pb):
    """the planted boxes with what one rank makes of them, computed once: [(name, vel12, weight, ngp, expect, grid, info, exchange)]"""
    dt = np.float64 if pb == 8 else np.float32
    out = []
    for name, v, w, ngp, expect in nps.shift_cases(n, P, dt):
        grid, info = npm.deposit(v, w, ngp)
        out.append((name, v, w, ngp, expect, grid, info, nps.exchange(n, P, *nps.box_reach(v, P, w, ngp))))
    return out


def tap_body(api, n, P, pb):
    nxl = n // P

    def body(f, r):
        before = f.device_bytes
        res = []
        for name, v, w, ngp, _, _, _, _ in planted(n, P, pb):
            grid, info = f.debug_matter_slabs(v[:, r * nxl:(r + 1) * nxl], ngp=ngp, weight=w)
            res.append((grid, info, api.matter_exchange(), api.matter_form()[0]))
        assert f.device_bytes == before
        return res
    return body


def check_tap(n, P, pb, res, lds):
    nxl = n // P
    forms = set()
    for k, (name, v, w, ngp, expect, grid, info, exch) in enumerate(planted(n, P, pb)):
        for r in range(P):
            g, i, e, form = res[r][k]
            assert g.dtype == np.uint64 and np.array_equal(g, grid[r * nxl:(r + 1) * nxl]), (name, n, P, pb, r)
            assert {key: i[key] for key in INT_KEYS} == info and i["modes"] == 0 == i["nonfinite_modes"], (name, r, i, info)
            assert e == exch, (name, r, e, exch)
            assert form == (1 if lds else 0), (name, r, form)
        if expect is not None:
            assert (exch["reach_below"], exch["reach_above"]) == expect, (name, exch)
        if name.startswith("zero"):
            assert exch["form"] == 0 and exch["bytes_per_peer"] == 0
        if name.startswith("one_far") and nxl + n // 2 - 1 >= n:
            assert exch["form"] == 2
        forms.add(exch["form"])
    assert {0, 1} <= forms or {0, 2} <= forms


# (16, 2): both neighbours are one peer; (16, 16): nxl = 1, every reach spans several owners; (32, 4): the LDS form; (24, 3): the plain
# form, nxl = 8; (48, 3): no power of two.  The LDS form runs where n is a multiple of 16 and nxl one of 4
@pytest.mark.parametrize("pb", [4, 8])
@pytest.mark.parametrize("n,P,lds", [(16, 2, True), (16, 16, False), (32, 4, True), (24, 3, False), (48, 3, True)])
def test_planted_columns_through_the_tap(api, n, P, lds, pb):
    planted(n, P, pb)
    res = run_ranks(DoubleProducts(api) if pb == 8 else api, n, P, tap_body(api, n, P, pb))
    check_tap(n, P, pb, res, lds)


def test_the_plain_deposit_gives_the_same_slabs(api, monkeypatch):
    """PF_MATTER_LDS is read per call: the same contexts' worth of columns with the one-particle-per-lane deposit"""
    n, P, pb = 32, 4, 4
    planted(n, P, pb)
    default = run_ranks(api, n, P, tap_body(api, n, P, pb))
    check_tap(n, P, pb, default, True)
    monkeypatch.setenv("PF_MATTER_LDS", "0")
    plain = run_ranks(api, n, P, tap_body(api, n, P, pb))
    check_tap(n, P, pb, plain, False)
    for r in range(P):
        for a, b in zip(default[r], plain[r]):
            assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2]


def as_power(m):
    """a matter result in the shape test_gpu_power.same_bits compares: cross in the place of variance, nonfinite_modes of nonfinite"""
    return {"nmodes": m["nmodes"], "k2sum": m["k2sum"], "power": m["power"], "variance": m["cross"] if m["cross"] is not None else np.zeros(0),
            "modes": m["modes"], "nonfinite": m["nonfinite_modes"]}


def bits_equal(a, b):
    return same_bits(as_power(a), as_power(b)) and all(a[k] == b[k] for k in INFO_KEYS) and (a["cross"] is None) == (b["cross"] is None)


def columns_of(prod, dtype):
    return np.ascontiguousarray(np.stack([prod[name][..., j] for name in NAMES for j in range(3)]).astype(dtype))


def prepare(f, dk_slab):
    f.set_density(dk_slab)
    f.set_invgrow(*synth.invgrow_table("lcdm"))
    f.set_growth(synth.growth_multipliers())
    f.compute_fmax(np.array([1.0, 0.0]), do_lpt=True)


@functools.lru_cache(maxsize=None)
def one_rank(n, seed, fb, sigma0, kw_items):
    """the density of a case and what one rank makes of it, computed once and left unchanged: (dk, matter_power, products)"""
    from pinocchio_amd import api
    dk = synth.make_density(n, seed=seed, sigma0=sigma0)
    with api.Fmax(n, field_bytes=fb) as f1:
        prepare(f1, dk)
        return dk, f1.matter_power(density=True, **dict(kw_items)), f1.products()


def whole_call(api, n, P, fb, sigma0, kw, delay_us=0):
    """-> (one rank's matter_power and products, [every rank's matter_power_slabs and products])"""
    nxl = n // P
    dk, one, p1 = one_rank(n, 70 + n + P, fb, sigma0, tuple(sorted(kw.items())))

    def body(f, r):
        prepare(f, dk[r * nxl:(r + 1) * nxl])
        before = f.device_bytes
        got = f.matter_power_slabs(density=True, **kw)
        assert f.device_bytes == before
        return got, f.products()

    return one, p1, run_ranks(api, n, P, body, field_bytes=fb, delay_us=delay_us)


def check_whole(n, P, one, p1, res):
    nxl = n // P
    for r in range(P):
        got, p = res[r]
        sl = slice(r * nxl, (r + 1) * nxl)
        # what the contract presumes: the same columns on P ranks as on one
        same_columns = all(np.array_equal(p[name], p1[name][sl]) for name in NAMES)
        assert bits_equal(got, res[0][0]) and got["exchange"] == res[0][0]["exchange"], r              # between the ranks
        assert bits_equal(got, one), (r, same_columns, {k: (got[k], one[k]) for k in INFO_KEYS})
        assert np.array_equal(got["density"], one["density"][sl]), (r, same_columns)
    return res[0][0]["exchange"]


@pytest.mark.parametrize("replicate", [1, 0])
@pytest.mark.parametrize("n,P,fb,sigma0,kw", WHOLE)
def test_the_whole_call_against_one_rank(api, n, P, fb, sigma0, kw, replicate, monkeypatch):
    """synthetic density, a sweep with 3LPT displacements, then the call on P ranks and pf_matter_power on one: nmodes, k2sum, power,
    cross and every field of info bit-equal on every rank, the contrast slabs equal.  So that the (64, 8) case cannot pass with
    nothing crossing, its sigma0 is such that the common reach is at least 2 planes one way: asserted from `exchange`"""
    monkeypatch.setenv("PF_REPLICATE_DK", str(replicate))
    one, p1, res = whole_call(api, n, P, fb, sigma0, kw)
    ex = check_whole(n, P, one, p1, res)
    print(n, P, fb, replicate, ex)
    assert ex["form"] in (1, 2) and ex["bytes_per_peer"] == ex["block_planes"] * n * n * 8 > 0
    cols = columns_of(p1, np.float32)
    assert (ex["reach_below"], ex["reach_above"]) == nps.box_reach(cols, P, kw.get("weight"), kw.get("ngp", False))
    if (n, P) == (64, 8):
        assert max(ex["reach_below"], ex["reach_above"]) >= 2


def test_a_scan_per_sum_on_slabs(api, monkeypatch):
    """PF_MATTER_SCAN_EACH=1 (read per call): the way of the largest grids, a scan per sum before the maxima are taken over the ranks"""
    monkeypatch.setenv("PF_MATTER_SCAN_EACH", "1")
    one, p1, res = whole_call(api, 32, 2, 8, 1.0, {})
    check_whole(32, 2, one, p1, res)
    assert api.matter_form()[1] == 3


def test_one_rank_is_pf_matter_power(api):
    n = 32
    radii = np.array([1.0, 0.0])
    with api.Fmax(n) as f:
        f.synth_density(seed=77, sigma0=0.4)
        f.set_invgrow(*synth.invgrow_table("lcdm"))
        f.set_growth(synth.growth_multipliers())
        tv = f.compute_fmax(radii, do_lpt=True)
        prod = f.products().tobytes()
        before = f.device_bytes
        for kw in ({}, {"ngp": True, "cross": False}, {"deconvolve": True, "weight": (1.0, 0.5, 0.0, 0.0)}):
            exchange = api.matter_exchange()                # (from the second turn on: what the slab call of the turn before left)
            one = f.matter_power(density=True, **kw)
            assert api.matter_exchange() == exchange        # the one-rank entry point shares its body with the slab call and reports no exchange
            form = api.matter_form()
            got = f.matter_power_slabs(density=True, **kw)
            assert bits_equal(got, one) and np.array_equal(got["density"], one["density"]) and api.matter_form() == form
            ex = got["exchange"]
            assert (ex["form"], ex["window_planes"], ex["block_planes"], ex["bytes_per_peer"]) == (0, n, 0, 0)
            cols = columns_of(f.products(), np.float32)
            assert (ex["reach_below"], ex["reach_above"]) == nps.box_reach(cols, 1, kw.get("weight"), kw.get("ngp", False))
        assert f.device_bytes == before and f.products().tobytes() == prod
        assert np.array_equal(f.compute_fmax(radii, do_lpt=True), tv) and f.products().tobytes() == prod      # a sweep after the call


def test_late_exchange(api):
    """the fabric idles every exchange's stream for 2 ms before it pulls (the delay of the delayed tests of
    tests/test_gpu_multirank.py at four ranks): a fold that does not wait for the blocks, or blocks packed late, change the bits"""
    one, p1, res = whole_call(api, 64, 4, 8, 1.0, {}, delay_us=2000)
    check_whole(64, 4, one, p1, res)


def test_refusals_on_every_rank(api, capfd):
    """every rank makes the same mistake, so no rank waits for another: each returns 1 with the message naming the call, device_bytes
    as before; then the same contexts complete a good call"""
    from pinocchio_amd import _lib
    n, P = 16, 2
    nxl = n // P
    nb = api.power_bins(n)
    dk = synth.make_density(n, seed=5, sigma0=1.0)
    up, dp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_ulonglong))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double)))

    def body(f, r):
        L = f.L
        nm, ks = np.full(nb + 1, 0xABCDEF, np.uint64), np.full(nb + 1, 0xABCDEF, np.uint64)
        pw, cr, dens = np.full(nb + 1, 123.5), np.full(nb + 1, 123.5), np.full(nxl * n * n + 1, 123.5)
        info = (_lib.MatterInfo * 2)()
        info[0].deposited = info[1].deposited = 0xABCDEF
        w = np.array([1.0, 1.0, 1.0, 1.0])

        def untouched():
            return np.all(nm == 0xABCDEF) and np.all(ks == 0xABCDEF) and np.all(pw == 123.5) and np.all(cr == 123.5) and np.all(dens == 123.5) and \
                info[0].deposited == info[1].deposited == 0xABCDEF

        call = lambda **k: L.pf_matter_power_slabs(f.h, k.get("flags", 0), k.get("w", dp(w)), up(nm), up(ks), dp(pw), k.get("cr", dp(cr)), dp(dens), info)
        before = f.device_bytes
        seen = []

        def refused(what, **k):
            assert call(**k) == 1, (r, what)
            msg = L.pf_last_error()
            assert b"pf_matter_power_slabs" in msg and what in msg, (r, msg)
            assert untouched() and f.device_bytes == before, (r, what)
            seen.append(what)

        refused(b"density not set")                           # cross without a density
        refused(b"products not computed", cr=None)
        f.set_density(dk[r * nxl:(r + 1) * nxl])
        f.set_invgrow(*synth.invgrow_table("lcdm"))
        refused(b"products not computed")
        f.set_growth(synth.growth_multipliers())
        f.compute_fmax(np.array([1.0, 0.0]), do_lpt=True)
        before = f.device_bytes
        refused(b"unknown flag bits", flags=4)
        refused(b"is not finite", w=dp(np.array([1.0, np.nan, 0.0, 0.0])))
        with pytest.raises(api.PinfmaxError, match="pf_debug_matter_slabs: unknown flag bits"):
            f._chk(f.L.pf_debug_matter_slabs(f.h, dens.ctypes.data_as(C.c_void_p), 8, None, up(nm), info))
        assert untouched() and f.device_bytes == before
        good = f.matter_power_slabs()
        assert f.device_bytes == before
        return good, len(seen)

    res = run_ranks(api, n, P, body)
    assert "ERROR on task 1: pf_matter_power_slabs" in capfd.readouterr().out
    assert res[0][1] == res[1][1] == 5 and bits_equal(res[0][0], res[1][0])
    with api.Fmax(n) as f1:
        prepare(f1, dk)
        assert bits_equal(res[0][0], f1.matter_power())
