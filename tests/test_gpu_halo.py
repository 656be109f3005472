"""The halo-power call on the device (include/pinfmax.h: pf_halo_power, pf_debug_halo_deposit) against the numpy restatement
(tests/np_halo.py): the planted lists of tests/halo_cases.py through the tap, the lattice whose power is exactly zero, the unit list
that is the matter call, a random catalogue in three bins on both field types, the order of the list, any number of ranks through the
in-process fabric (run_ranks of tests/test_gpu_multirank.py), the state the call must leave alone, and the refusals.

What is equal and what is bounded.  Grids, counters, nmodes and k2sum are integers: equal.  The contrast is one division and one
difference of exact integers: the restatement forms the same doubles.  `power` and `cross` of a bin are then held TWICE:
  bit for bit (same_bits of tests/test_gpu_power.py) against the restatement's contrast taken through the context's own forward
    transform (Fmax.forward_transform, the field and the passes pf_halo_power uses) and the production shell passes
    (pf_debug_matter_shells) -- selection, positions, deposit and contrast are numpy's, and any difference in them changes bits;
  against numpy's own transform of that contrast through the shell restatement (np_halo.spectra: np.fft.rfftn, np_matter.shells),
    within the bounds tests/test_gpu_matter.py derives from the forward transform's asserted error (spectra_bound) -- two transforms
    that order their roundings differently cannot agree to the bit, and the fixed-point shell sums differ from math.fsum by up to
    TOL_POWER = 1e-14 (tests/test_matter_cpu.py), so this second comparison is a bound and cannot be an equality.
The figures of the second comparison are printed before they are asserted."""
import ctypes as C

import numpy as np
import pytest

import halo_cases as hc
import np_halo as nph
import np_matter as npm
import np_power as npp
from pinocchio_amd import synth
from test_gpu_multirank import run_ranks
from test_gpu_power import same_bits
from test_halo_cpu import check, window_of, WINDOWS

pytestmark = pytest.mark.gpu

NAMES = ("Vel", "Vel_2LPT", "Vel_3LPT_1", "Vel_3LPT_2")
RANGES = [(10, 2 ** 31 - 1), (100, 2 ** 31 - 1), (1000, 2 ** 31 - 1)]        # cumulative thresholds


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


def raw_deposit(n, case, lo, hi, ngp, x0=0, nxl=None):
    """pf_debug_halo_deposit with a guard element behind every output -> (grid, the integer counters); (None, counters as they were) when refused"""
    from pinocchio_amd import _lib
    L = _lib.load()
    nxl = n - x0 if nxl is None else nxl
    grid = np.full(nxl * n * n + 1, 0x5A5A5A, np.uint64)
    info = (_lib.HaloInfo * 2)()
    info[0].selected = info[1].selected = info[1].nonfinite_modes = 0xABCDEF
    flags = (1 if ngp else 0) | (4 if case["mass_weight"] else 0)
    rc = L.pf_debug_halo_deposit(n, x0, nxl, flags, len(case["mass"]), case["pos"].ctypes.data_as(C.POINTER(C.c_double)), case["scale"],
                                 case["mass"].ctypes.data_as(C.POINTER(C.c_int)), lo, hi, grid.ctypes.data_as(C.POINTER(C.c_ulonglong)), info)
    assert grid[-1] == 0x5A5A5A and info[1].selected == info[1].nonfinite_modes == 0xABCDEF
    if rc:
        assert b"pf_debug_halo_deposit: the weights of bin 0 add up to" in L.pf_last_error(), L.pf_last_error()
        assert np.all(grid == 0x5A5A5A) and info[0].selected == 0xABCDEF
        return None, None
    assert info[0].modes == 0 == info[0].nonfinite_modes
    return grid[:-1].reshape(nxl, n, n), {k: int(getattr(info[0], k)) for k in nph.INT_KEYS}


@pytest.mark.parametrize("n", [16, 24])
def test_planted_lists_through_the_tap(api, n):
    """rows shorter than a wavefront (16) and no multiple of one (24); the whole box, three planes inside it and its last plane"""
    for case in hc.cases(n):
        for r, (lo, hi) in enumerate(case["ranges"]):
            for ngp in (False, True):
                whole = nph.deposit(n, case["pos"], case["mass"], lo, hi, case["scale"], case["mass_weight"], ngp)
                for x0, nxl in WINDOWS(n):
                    name = (case["name"], n, r, ngp, x0, nxl)
                    got = raw_deposit(n, case, lo, hi, ngp, x0, nxl)
                    if whole[0] is None:
                        assert got[0] is None and case["what"][r] == ("refused",), name
                        continue
                    check(got, window_of(whole, n, x0, nxl), name, case["what"][r], n, x0, nxl, ngp)
    case = next(c for c in hc.cases(n) if c["name"] == "random_777_weighted")
    g, info = api.debug_halo_deposit(n, case["pos"], case["mass"], 100, 2 ** 31 - 1, mass_weight=True, x0=5, nxl=3)      # the binding, and the same bits from run to run
    again = raw_deposit(n, case, 100, 2 ** 31 - 1, False, 5, 3)
    assert np.array_equal(g, again[0]) and {k: info[k] for k in nph.INT_KEYS} == again[1] and info["weight2"] == info["weight2_lo"]


def test_one_halo_on_every_cell_centre(api):
    n = 16
    q = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), axis=-1).reshape(-1, 3)
    pos = (q + 0.5) * 2.5                       # in units of 2.5 to the cell: scale = 0.4 brings them to cells, and (q + 0.5) 2.5 0.4 stays inside cell q
    assert np.array_equal(np.floor(nph.positions(pos, 0.4, n)), q)
    with api.Fmax(n) as f:
        for mw in (False, True):
            got = f.halo_power(pos, np.full(n ** 3, 7), [(7, 7), (1, 6)], scale=0.4, ngp=True, cross=False, mass_weight=mw)
            assert got["cross"] is None and not np.any(got["power"]) and got["power"].shape == (2, npp.bins(n))
            assert got["empty_cells"].tolist() == [0, n ** 3] and got["selected"].tolist() == [n ** 3, 0] and got["max_cell"].tolist() == [(7 if mw else 1) << 30, 0]
            assert got["modes"].tolist() == [n ** 3, n ** 3] and int(got["nmodes"].sum()) == n ** 3
            assert got["shot"][0] == 1.0 / n ** 3 and np.isnan(got["shot"][1])
        # every bin empty: nmodes and k2sum all the same
        none = f.halo_power(pos, np.full(n ** 3, 7), [(1, 6), (8, 9)], scale=0.4, cross=False)
        ref = npp.power(np.zeros((n, n, n // 2 + 1), np.complex128))
        assert np.array_equal(none["nmodes"], ref["nmodes"]) and np.array_equal(none["k2sum"], ref["k2sum"]) and np.array_equal(none["nmodes"], got["nmodes"])
        assert not np.any(none["power"]) and none["selected"].tolist() == [0, 0]


def columns_of(prod, dtype):
    return np.ascontiguousarray(np.stack([prod[name][..., j] for name in NAMES for j in range(3)]).astype(dtype))


def as_power(out, b):
    """bin b of a halo_power dict under the keys same_bits of tests/test_gpu_power.py compares (`variance` carries cross)"""
    return {"nmodes": out["nmodes"], "k2sum": out["k2sum"], "power": out["power"][b], "variance": out["cross"][b], "modes": int(out["modes"][b]),
            "nonfinite": int(out["nonfinite_modes"][b])}


def matter_as_power(m):
    return {"nmodes": m["nmodes"], "k2sum": m["k2sum"], "power": m["power"], "variance": m["cross"], "modes": m["modes"], "nonfinite": m["nonfinite_modes"]}


def test_the_unit_list_of_the_particles_is_the_matter_call(api):
    """the LPT particles as a list of unit masses, nearest grid point: the same grid, so the same contrast (cell / 2^30 against cell /
    2^48 of the matter call's units: the same doubles) and, through the same transform and shell passes, the same bits"""
    n = 32
    with api.Fmax(n) as f:
        f.synth_density(seed=91, sigma0=0.4)
        f.set_invgrow(*synth.invgrow_table("lcdm"))
        f.set_growth(synth.growth_multipliers())
        f.compute_fmax(np.array([1.0, 0.0]), do_lpt=True)
        cols = columns_of(f.products(), np.float32)
        p = npm.positions(cols)
        assert np.all(npm.classes(p, n) == 0)
        pos = np.stack([a.astype(np.float64).ravel() for a in p], axis=1)
        for dec in (False, True):
            m = f.matter_power(ngp=True, deconvolve=dec)
            h = f.halo_power(pos, np.ones(n ** 3, np.int32), [(1, 1)], ngp=True, deconvolve=dec)
            assert same_bits(as_power(h, 0), matter_as_power(m)), dec
            assert np.count_nonzero(h["power"][0]) > n // 4 and np.all(h["cross"][0][1:3] > 0)
            assert (int(h["selected"][0]), int(h["empty_cells"][0]), int(h["max_cell"][0])) == (m["deposited"], m["empty_cells"], m["max_cell"] >> 18)
        g, _ = npm.deposit(cols, None, True)
        assert np.array_equal(nph.contrast(g >> np.uint64(18), n ** 3, n), npm.contrast(g))


@pytest.fixture(scope="module")
def catalogue():
    n = 32
    pos, mass = hc.random_list(21, 2000, n)
    pos = pos * 3.7                                    # "Mpc/h": scale = 1 / 3.7 brings them to cells
    want = {}
    for mw in (False, True):
        for b, (lo, hi) in enumerate(RANGES):
            want[mw, b] = nph.deposit(n, pos, mass, lo, hi, 1.0 / 3.7, mw)
    assert want[False, 0][1]["selected"] > want[False, 1][1]["selected"] > want[False, 2][1]["selected"] > 20
    return n, pos, mass, want


@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("mw", [False, True])
def test_a_random_catalogue_in_three_bins(api, catalogue, fb, mw):
    from test_gpu_matter import spectra_bound
    n, pos, mass, want = catalogue
    perm = np.random.default_rng(5).permutation(len(mass))
    with api.Fmax(n, field_bytes=fb) as f:
        f.synth_density(seed=33, sigma0=0.4)
        dk = f.density()
        lin = npp.from_x_slab(dk)
        for dec in (False, True):
            got = f.halo_power(pos, mass, RANGES, scale=1.0 / 3.7, mass_weight=mw, deconvolve=dec)
            again = f.halo_power(pos[perm], mass[perm], RANGES, scale=1.0 / 3.7, mass_weight=mw, deconvolve=dec)
            ref = npp.power(lin)
            assert np.array_equal(got["nmodes"], ref["nmodes"]) and np.array_equal(got["k2sum"], ref["k2sum"])
            for b in range(3):
                g, info = want[mw, b]
                assert {k: int(got[k][b]) for k in nph.INT_KEYS} == info and got["weight2"][b] == (info["weight2_hi"] << 64) | info["weight2_lo"], (b, dec)
                assert int(got["modes"][b]) == n ** 3 and int(got["nonfinite_modes"][b]) == 0 and got["shot"][b] == nph.shot(info)
                assert same_bits(as_power(got, b), as_power(again, b)), (b, dec)                 # the order of the list changes no bit
                assert {k: int(again[k][b]) for k in nph.INT_KEYS} == info
                dens = nph.contrast(g, info["weight_sum"], n, fb)
                # bit for bit: the restated contrast through the context's transform and the production shell passes
                spec = npp.from_x_slab(f.forward_transform(dens))
                chain = api.debug_matter_shells(spec, lin, 0, fb, False, dec)
                assert same_bits(as_power(got, b), matter_as_power(chain)), (b, dec)
                # within the transform's bound: numpy's transform and the shell restatement
                full = nph.spectra(dens, dk, False, dec)
                _, bound_p, bound_c = spectra_bound(n, fb, dens, lin, dec)
                dp_, dc_ = np.abs(got["power"][b] - full["power"]), np.abs(got["cross"][b] - full["cross"])
                nz = bound_p > 0
                print(fb, mw, dec, b, "power / bound", float(np.max(dp_[nz] / bound_p[nz])), "cross / bound", float(np.max(dc_[nz] / np.maximum(bound_c[nz], 1e-300))),
                      "power rel", npp.rel(got["power"][b], full["power"]))
                assert np.all(got["power"][b][~nz] == 0) and np.all(dp_ <= bound_p) and np.all(dc_ <= bound_c), (b, dec)
                assert np.count_nonzero(got["power"][b]) > n // 4
            if not dec:
                only = f.halo_power(pos, mass, RANGES, scale=1.0 / 3.7, mass_weight=mw, cross=False)
                assert only["cross"] is None and np.array_equal(only["power"], got["power"])


def test_the_tap_on_a_production_size_of_list(api):
    """20000 haloes, more than PF_HALO_SLOTS workgroups: every copy of the selection counters is in use"""
    n = 24
    pos, mass = hc.random_list(31, 20000, n, mmax=200000)
    case = {"pos": pos, "mass": mass, "scale": 1.0, "mass_weight": True}
    for ngp in (False, True):
        want = nph.deposit(n, pos, mass, 50, 150000, 1.0, True, ngp)
        got = raw_deposit(n, case, 50, 150000, ngp)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1] and want[1]["weight2_lo"] >> 32 > 0


def ranks_body(api, n, P, pos, mass, dk, short_rank):
    nxl = n // P

    def body(f, r):
        f.set_density(dk[r * nxl:(r + 1) * nxl])
        before = f.device_bytes
        k = len(mass) - 1 if r == short_rank else len(mass)     # one rank is handed a shortened list: every rank must return 1
        with pytest.raises(api.PinfmaxError, match="pf_halo_power: rank"):
            f.halo_power(pos[:k], mass[:k], RANGES, mass_weight=True)
        order = np.random.default_rng(100 + r).permutation(len(mass))      # every rank its own order
        out = [f.halo_power(pos[order], mass[order], RANGES, mass_weight=True, deconvolve=True), f.halo_power(pos, mass, RANGES, ngp=True, cross=False)]
        assert f.device_bytes == before
        return out

    return body


@pytest.mark.parametrize("n,P", [(16, 2), (32, 4), (16, 16), (48, 3)])
def test_every_rank_returns_the_bits_of_one_rank(api, n, P):
    pos, mass = hc.random_list(40 + P, 1500, n)
    pos[:4] = [[n - 1e-13, 1.0, 1.0], [-1e-20, 2.0, 2.0], [np.nan, 1.0, 1.0], [0.25, 0.25, 0.25]]      # the planes at both ends of the box, and one that is no position
    dk = synth.make_density(n, seed=50 + P)
    with api.Fmax(n) as f:
        f.set_density(dk)
        one = [f.halo_power(pos, mass, RANGES, mass_weight=True, deconvolve=True), f.halo_power(pos, mass, RANGES, ngp=True, cross=False)]
    assert int(one[0]["nonfinite"][0]) == 1 and np.count_nonzero(one[0]["cross"][0]) > n // 4
    res = run_ranks(api, n, P, ranks_body(api, n, P, pos, mass, dk, P - 1))
    for r in range(P):
        for got, want in zip(res[r], one):
            assert np.array_equal(got["nmodes"], want["nmodes"]) and np.array_equal(got["k2sum"], want["k2sum"]), r
            assert np.array_equal(got["power"].view(np.uint64), want["power"].view(np.uint64)), r
            assert (got["cross"] is None and want["cross"] is None) or np.array_equal(got["cross"].view(np.uint64), want["cross"].view(np.uint64)), r
            for k in nph.INT_KEYS + ("modes", "nonfinite_modes"):
                assert np.array_equal(got[k], want[k]), (r, k)
            assert got["weight2"] == want["weight2"] and np.array_equal(got["shot"], want["shot"])


def test_the_call_leaves_the_context_as_it_was(api, catalogue):
    n, pos, mass, _ = catalogue

    def run(with_call):
        with api.Fmax(n) as f:
            f.synth_density(seed=77, sigma0=0.4)
            f.set_invgrow(*synth.invgrow_table("lcdm"))
            f.set_growth(synth.growth_multipliers())
            if with_call:
                f.halo_power(pos, mass, RANGES, scale=1.0 / 3.7)
            f.compute_fmax(np.array([1.0, 0.0]), do_lpt=True)
            state = (f.device_bytes, f.arithmetic, f.L.pf_replicated_spectrum(f.h))
            prod = f.products().tobytes()
            if with_call:
                f.halo_power(pos, mass, RANGES, scale=1.0 / 3.7, mass_weight=True, deconvolve=True)
                f.halo_power(pos, mass, RANGES[:1], scale=1.0 / 3.7, ngp=True, cross=False)
                assert state == (f.device_bytes, f.arithmetic, f.L.pf_replicated_spectrum(f.h))
                assert prod == f.products().tobytes()
            f.sweep(np.array([2.0, 1.0]))
            return f.products()["Fmax"].tobytes(), prod, f.power_spectrum("density", (1.0,)), f.density()

    a, b = run(False), run(True)
    assert a[0] == b[0] and a[1] == b[1]
    assert all(np.array_equal(a[2][k], b[2][k]) for k in ("nmodes", "k2sum", "power", "variance")) and np.array_equal(a[3], b[3])


def test_refusals_on_a_live_context(api, capfd):
    from pinocchio_amd import _lib
    n = 16
    nb = api.power_bins(n)
    nm, ks = np.full(nb + 1, 0xABCDEF, np.uint64), np.full(nb + 1, 0xABCDEF, np.uint64)
    pw, cr = np.full(2 * nb + 1, 123.5), np.full(2 * nb + 1, 123.5)
    info = (_lib.HaloInfo * 3)()
    for k in range(3):
        info[k].selected = 0xABCDEF
    pos, mass = hc.random_list(7, 50, n)
    rg = np.array([[1, 100], [50, 5000]], np.int32)
    up, dp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_ulonglong))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int)))
    big = next(c for c in hc.cases(n) if c["name"] == "headroom_16")

    def untouched():
        return np.all(nm == 0xABCDEF) and np.all(ks == 0xABCDEF) and np.all(pw == 123.5) and np.all(cr == 123.5) and all(info[k].selected == 0xABCDEF for k in range(3))

    with api.Fmax(n) as f:
        L = f.L
        call = lambda **k: L.pf_halo_power(k.get("h", f.h), k.get("flags", 0), k.get("count", len(mass)), k.get("pos", dp(pos)), k.get("scale", 1.0), k.get("mass", ip(mass)),
                                           k.get("nbins", 2), k.get("rg", ip(rg)), k.get("nm", up(nm)), k.get("ks", up(ks)), k.get("pw", dp(pw)), k.get("cr", dp(cr)),
                                           k.get("info", info))
        before = f.device_bytes
        assert call() != 0 and b"pf_halo_power: density not set" in L.pf_last_error() and untouched()       # cross without a density
        f.synth_density(seed=3)
        before = f.device_bytes
        bad_rg, bad_rg2 = np.array([[1, 100], [0, 5]], np.int32), np.array([[7, 6], [1, 5]], np.int32)
        for kw, what in (({"h": None}, b"null argument"), ({"pos": None}, b"null argument"), ({"mass": None}, b"null argument"), ({"rg": None}, b"null argument"),
                         ({"nm": None}, b"null argument"), ({"ks": None}, b"null argument"), ({"pw": None}, b"null argument"), ({"info": None}, b"null argument"),
                         ({"flags": 8}, b"unknown flag bits"), ({"flags": -1}, b"unknown flag bits"), ({"nbins": 0}, b"0 bins"), ({"nbins": 9}, b"9 bins"),
                         ({"rg": ip(bad_rg)}, b"bin 1 takes the masses 0 to 5"), ({"rg": ip(bad_rg2)}, b"bin 0 takes the masses 7 to 6"),
                         ({"scale": 0.0}, b"a scale of 0"), ({"scale": float("nan")}, b"a scale of"), ({"scale": -2.0}, b"a scale of -2"),
                         ({"count": 2 ** 31 + 1}, b"more than 2^31")):
            assert call(**kw) != 0, kw
            assert what in L.pf_last_error() and b"pf_halo_power" in L.pf_last_error(), (kw, L.pf_last_error())
            assert untouched() and before == f.device_bytes, kw
        # the headroom: refused after the selection pass, the message names the bin, nothing is deposited or returned
        one_bin = np.array([[1, 5], [hc.BIG, hc.BIG]], np.int32)
        assert call(flags=4, count=16, pos=dp(big["pos"]), mass=ip(big["mass"]), rg=ip(one_bin)) != 0
        assert b"pf_halo_power: the weights of bin 1 add up to 17179869184" in L.pf_last_error() and untouched() and before == f.device_bytes
        assert "ERROR on task 0: pf_halo_power" in capfd.readouterr().out
        assert call(count=16, pos=dp(big["pos"]), mass=ip(big["mass"]), rg=ip(one_bin), cr=None) == 0             # unweighted the same list is sixteen unit weights
        assert info[1].selected == 16 == info[1].weight_sum and info[0].selected == 0 and info[2].selected == 0xABCDEF and np.all(cr == 123.5)
        assert nm[-1] == ks[-1] == 0xABCDEF and pw[-1] == 123.5 and not np.any(pw[:nb]) and np.count_nonzero(pw[nb:2 * nb]) > 4 and before == f.device_bytes


def test_more_than_one_rank_without_an_exchange_is_refused(api):
    pos, mass = hc.random_list(7, 50, 16)
    with api.Fmax(16, rank=0, nranks=2) as f:
        with pytest.raises(api.PinfmaxError, match="pf_halo_power: no exchange installed for 2 ranks"):
            f.halo_power(pos, mass, RANGES, cross=False)
