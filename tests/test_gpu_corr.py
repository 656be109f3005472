"""The two-point correlation function of the haloes on the device (include/pinfmax.h: pf_halo_correlation) against the numpy
restatement (tests/np_corr.py): the form tap and the separation-space shell tap bit for bit and within the fixed point's TOL_POWER,
the call against its own pieces chained through the taps bit for bit on every transform path, closed forms and numpy's transform
within a bound derived before the run, the ranks against one rank bit for bit, the state of the context, the refusals.

The bound (corr_bound): tests/test_gpu_parity.py::test_transforms_vs_pocketfft holds one transform of fp64 fields within e = 1e-13
log2(n) of the largest output, tests/test_gpu_matter.py (spectra_bound) uses e = 3e-5 for fp32 fields.  With numpy's spectrum S of
the restated contrast, M = max |S|, c the deconvolution factor of a mode and u the unit roundoff of the field type:
  a mode of the forward transform is off by at most e M, so its auto term c^2 |S|^2 by c^2 (2 e M |S| + e^2 M^2) and its cross term
  c Re(S conj L) by c e M |L|; the division by N^3 and the rounding to the field type add u |Q| to the formed element Q;
  a cell of the reverse transform is off by at most the sum over the modes (Hermitian weights w) of those errors over N^3 -- the
  transform is linear with coefficients of modulus one -- plus (e + u) times the largest cell, itself at most sum w |Q| / N^3;
  a shell sum of ncells cells with |L_l| <= 1 is off by at most ncells times that, plus TOL_POWER (positive + negative) for the
  fixed point.
Every quantity is numpy's own; nothing of the library's output enters."""
import ctypes as C
import math

import numpy as np
import pytest

import corr_cases as cc
import halo_cases as hc
import np_corr as npc
import np_halo as nph
import np_matter as npm
import np_multipoles as npl
import np_power as npp
from pinocchio_amd import synth
from test_gpu_multirank import run_ranks
from test_gpu_power import TOL_POWER

pytestmark = pytest.mark.gpu

RANGES = [(10, 2 ** 31 - 1), (100, 2 ** 31 - 1), (1000, 2 ** 31 - 1)]
INFO_KEYS = nph.INT_KEYS + ("modes", "nonfinite_modes", "cells", "nonfinite_cells")
PATHS = [(16, 8, 0), (16, 4, 0), (48, 8, 1), (48, 4, 1), (36, 8, 2)]      # (n, field bytes, pf_transform_path); the general path has fp64 fields only
SCALE = 1.0 / 3.7


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(a, b, keys=("ncells", "r2sum", "xi", "xi_cross")):
    return all((a[k] is None and b[k] is None) or np.array_equal(bits(a[k]), bits(b[k])) for k in keys)


def list_for(n, seed=21, count=2000):
    pos, mass = hc.random_list(seed, count, n)
    vel = np.random.default_rng(seed + 1).normal(0.0, 1.5 * 3.7, size=pos.shape)          # N(0, 1.5 cells) in the units of the positions
    return pos * 3.7, vel, mass


def corr_bound(n, fb, dens, lin_slab, ngp, dec, absum, absum_cross=None):
    """per-shell bounds [3][nb] of xi and of xi_cross (None without lin_slab), see the head of the file; absum: positive + negative
    sums [3][nb] of the reference"""
    spec = npp.from_x_slab(np.fft.rfftn(dens, axes=(0, 1, 2)))
    e, u = (1e-13 * math.log2(n), 2.0 ** -53) if fb == 8 else (3e-5, 2.0 ** -24)
    M, N3 = float(np.max(np.abs(spec))), float(n) ** 3
    _, _, w = npp.geometry(n)
    c = np.ones(spec.shape)
    if dec:
        tab = npm.deconv_table(n, ngp)
        a = np.abs(npp.signed(np.arange(n), n))
        c = tab[a][:, None, None] * tab[a][None, :, None] * tab[np.arange(n // 2 + 1)][None, None, :]
    ncells = npc.shells(np.zeros((n, n, n)))["ncells"].astype(np.float64)

    def per_cell(dq, q):
        largest = float((w * q).sum()) / N3
        return float((w * (dq + u * q)).sum()) / N3 + (e + u) * largest

    cell = per_cell(c * c * (2 * e * M * np.abs(spec) + e * e * M * M) / N3, c * c * np.abs(spec) ** 2 / N3)
    out = [ncells[None, :] * cell + TOL_POWER * absum, None]
    if lin_slab is not None:
        cell = per_cell(c * e * M * np.abs(lin_slab) / N3, c * np.abs(spec) * np.abs(lin_slab) / N3)
        out[1] = ncells[None, :] * cell + TOL_POWER * absum_cross
    return out


def absums(parts):
    return parts[0::2] + parts[1::2]


# ------------------------------------------------------------------------------------------------------------ 1. the form tap
@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("n", [16, 24])
def test_form_tap(api, n, fb):
    for a, b in (cc.planted_spectra(n), cc.random_spectra(n, 3 + n)):
        a = a.copy()
        a[2, 3, 4] = np.inf + 0j                  # a mode that is not finite: zeroed and counted with its weight 2
        for y0, nyl in ((0, n), (n // 2, n // 2), (3, 5)):
            sa, sb = np.ascontiguousarray(a[y0:y0 + nyl]), np.ascontiguousarray(b[y0:y0 + nyl])
            for which, ngp, dec in ((0, False, False), (1, False, False), (0, False, True), (1, True, True)):
                got, info = api.debug_corr_form(sa, sb if which else None, y0, fb, ngp, dec, which)
                want, nonfin = npc.form(sa, sb, y0, fb, ngp, dec, which)
                name = (n, fb, y0, which, ngp, dec)
                assert np.array_equal(bits(got.real), bits(want)) and not np.any(got.imag), name
                assert info == {"modes": nyl * n * n, "nonfinite_modes": nonfin} and nonfin == (2 if y0 <= 2 < y0 + nyl else 0), name
                if y0 == 0:
                    assert got[0, 0, 0] == 0 and got[2, 3, 4] == 0 and np.count_nonzero(got) >= 4, name


# ------------------------------------------------------------------------------------------------------------ 2. the shell tap, one point
@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("n", [16, 24])
def test_shell_tap_on_one_cell(api, n, fb):
    nb = npp.bins(n)
    for los in range(3):
        for d in (1, 3, n // 2):
            on = api.debug_corr_shells(cc.on_los(n, los, d), 0, fb, los)
            assert np.array_equal(bits(on["xi"][0]), bits(on["xi"][1])) and np.array_equal(bits(on["xi"][0]), bits(on["xi"][2])), (los, d)     # L2 = L4 = 1
            assert on["xi"][0, d] == 3.0 and np.count_nonzero(on["xi"]) == 3 and on["nonfinite_cells"] == 0
            for dd in (d, n - d):                 # either sign of the separation
                ac = api.debug_corr_shells(cc.across_los(n, los, dd), 0, fb, los)
                assert list(ac["xi"][:, d]) == [3.0, -1.5, 1.125] and np.count_nonzero(ac["xi"]) == 3, (los, dd)                               # L2 = -1/2, L4 = 3/8, exact
                assert list(ac["parts"][:, d]) == [3.0, 0.0, 0.0, 1.5, 1.125, 0.0]
        origin = api.debug_corr_shells(cc.one_cell(n, (0, 0, 0), -2.0), 0, fb, los)
        assert list(origin["parts"][:, 0]) == [0.0, 2.0, 0.0, 0.0, 0.0, 0.0] and np.count_nonzero(origin["parts"]) == 1       # r = 0: l = 0 alone
        assert origin["xi"].shape == (3, nb) and int(origin["ncells"].sum()) == n ** 3


# ------------------------------------------------------------------------------------------------------------ 3. the shell tap, random fields
@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("n", [16, 24])
def test_shell_tap_on_random_fields(api, n, fb, monkeypatch):
    f = cc.random_field(n, 5 + n)
    f[3, 2, 1] = np.inf                           # a cell that is not finite: in ncells and r2sum, in no other sum
    half = npp.power(np.zeros((n, n, n // 2 + 1), np.complex128))
    for los in range(3):
        want = npc.shells(f, 0, fb, los)
        got = api.debug_corr_shells(f, 0, fb, los)
        assert np.array_equal(got["ncells"], want["ncells"]) and np.array_equal(got["r2sum"], want["r2sum"]) and got["nonfinite_cells"] == 1
        assert np.array_equal(got["ncells"], half["nmodes"]) and np.array_equal(got["r2sum"], half["k2sum"])
        rp = npp.rel(got["parts"], want["parts"])
        print(n, fb, los, "positive sums against fsum", rp)
        assert rp <= TOL_POWER
        assert np.all(np.abs(got["xi"] - want["xi"]) <= TOL_POWER * absums(want["parts"]))
        assert np.array_equal(bits(got["xi"]), bits(got["parts"][0::2] - got["parts"][1::2]))
        # x-windows that split the box: integers add up; each window's sums are those of the restatement on its planes
        for wins in cc.x_windows(n)[1:]:
            win = [api.debug_corr_shells(f[x0:x0 + nxl], x0, fb, los) for x0, nxl in wins]
            assert np.array_equal(np.sum([p["ncells"] for p in win], axis=0, dtype=np.uint64), got["ncells"])
            assert np.array_equal(np.sum([p["r2sum"] for p in win], axis=0, dtype=np.uint64), got["r2sum"]) and sum(p["nonfinite_cells"] for p in win) == 1
            for (x0, nxl), p in zip(wins, win):
                assert npp.rel(p["parts"], npc.shells(f[x0:x0 + nxl], x0, fb, los)["parts"]) <= TOL_POWER, (los, x0)
        # one sum per pass (PF_CORR_SCAN_EACH, tests only): the grouping changes no bit
        monkeypatch.setenv("PF_CORR_SCAN_EACH", "1")
        each = api.debug_corr_shells(f, 0, fb, los)
        monkeypatch.delenv("PF_CORR_SCAN_EACH")
        assert all(np.array_equal(bits(each[k]), bits(got[k])) for k in ("ncells", "r2sum", "xi", "parts")) and each["nonfinite_cells"] == 1


# ------------------------------------------------------------------------------------------------------------ 4. the call against its pieces
def chain(api, f, n, fb, pos, vel, mass, lo, hi, vfac, los, mw, ngp, dec, lin):
    """the pieces through the taps: deposit, restated contrast, the context's forward transform, the form tap, the context's reverse
    transform, the shell tap -> (auto, cross or None, the deposit's counters, the contrast)"""
    g, info = api.debug_halo_deposit_rsd(n, pos, vel, mass, lo, hi, SCALE, vfac, los, mw, ngp)
    dens = nph.contrast(g, info["weight_sum"], n, fb)
    spec = npp.from_x_slab(f.forward_transform(dens))
    out = []
    for which in ((0, 1) if lin is not None else (0,)):
        q, _ = api.debug_corr_form(spec, lin if which else None, 0, fb, ngp, dec, which)
        out.append(api.debug_corr_shells(f.reverse_transform(npp.from_x_slab(q)), 0, fb, los))
    return out[0], (out[1] if lin is not None else None), info, dens


@pytest.mark.parametrize("n,fb,path", PATHS)
def test_the_call_is_its_pieces(api, n, fb, path):
    pos, vel, mass = list_for(n, seed=40 + n, count=3000)
    perm = np.random.default_rng(5).permutation(len(mass))
    with api.Fmax(n, field_bytes=fb) as f:
        assert f.L.pf_transform_path(f.h) == path
        f.synth_density(seed=60 + n, sigma0=0.4)
        lin = npp.from_x_slab(f.density())
        kw = dict(scale=SCALE, vfac=1.0, los=1, mass_weight=True, deconvolve=True)
        got = f.halo_correlation(pos, vel, mass, RANGES, **kw)
        again = f.halo_correlation(pos[perm], vel[perm], mass[perm], RANGES, **kw)
        assert same(got, again) and all(np.array_equal(got[k], again[k]) for k in INFO_KEYS)                # the order of the list changes no bit
        only = f.halo_correlation(pos, vel, mass, RANGES, cross=False, **kw)
        assert only["xi_cross"] is None and np.array_equal(bits(only["xi"]), bits(got["xi"]))
        multi = f.halo_multipoles(pos, vel, mass, RANGES, **kw)
        for k in nph.INT_KEYS + ("modes",):
            assert np.array_equal(got[k], multi[k]), k                                                        # info[b].halo is the multipole call's
        assert np.all(got["cells"] == n ** 3) and not np.any(got["nonfinite_cells"]) and not np.any(got["nonfinite_modes"])
        for b, (lo, hi) in enumerate(RANGES):
            auto, cross, info, _ = chain(api, f, n, fb, pos, vel, mass, lo, hi, 1.0, 1, True, False, True, lin)
            assert {k: int(got[k][b]) for k in nph.INT_KEYS} == {k: info[k] for k in nph.INT_KEYS}, b
            assert np.array_equal(bits(got["xi"][b]), bits(auto["xi"])) and np.array_equal(bits(got["xi_cross"][b]), bits(cross["xi"])), (n, fb, b)
            assert np.array_equal(got["ncells"], auto["ncells"]) and np.array_equal(got["r2sum"], auto["r2sum"])
            assert np.count_nonzero(got["xi"][b, 1]) > n // 4 and np.count_nonzero(got["xi_cross"][b, 2]) > n // 4
        # real space: the l = 0 rows know no line of sight
        real = [f.halo_correlation(pos, None, mass, RANGES, scale=SCALE, los=los, cross=False) for los in range(3)]
        assert np.array_equal(bits(real[0]["xi"][:, 0]), bits(real[1]["xi"][:, 0])) and np.array_equal(bits(real[0]["xi"][:, 0]), bits(real[2]["xi"][:, 0]))
        assert not np.array_equal(real[0]["xi"][:, 1], real[1]["xi"][:, 1]) and not np.array_equal(real[0]["xi"][:, 0], only["xi"][:, 0])


# ------------------------------------------------------------------------------------------------------------ 5. closed forms
@pytest.mark.parametrize("n,fb,path", PATHS)
def test_closed_forms(api, n, fb, path):
    N3 = float(n ** 3)
    nb = npp.bins(n)
    with api.Fmax(n, field_bytes=fb) as f:
        assert f.L.pf_transform_path(f.h) == path
        # one halo, NGP, unit weight: N^3 - 1 at r = 0 and -1 elsewhere
        pos, mass = cc.one_halo(n)
        for los in (0, 2):
            got = f.halo_correlation(pos, None, mass, [cc.ONE], los=los, ngp=True, cross=False)
            g, info = npl.deposit(n, pos, None, mass, 1, 2 ** 31 - 1, ngp=True)
            dens = nph.contrast(g, info["weight_sum"], n, fb)
            assert abs(dens.max() - (N3 - 1)) <= 2.0 ** (-50 if fb == 8 else -22) * N3 and np.count_nonzero(dens == -1.0) == n ** 3 - 1      # (the one rounding of the contrast)
            base = npc.shells(-np.ones((n, n, n)), 0, 8, los)                                # the field that is -1 everywhere: minus the sums of the weights
            want = base["xi"].copy()
            want[0, 0] = N3 - 1
            absum = absums(base["parts"])
            absum[0, 0] = N3 - 1
            bound = corr_bound(n, fb, dens, None, True, False, absum)[0]
            err = np.abs(got["xi"][0] - want)
            print(n, fb, "one halo, los", los, "largest error / bound", float(np.max(err / bound)), "largest bound", float(bound.max()), "largest error", float(err.max()))
            assert np.all(err <= bound)
            assert np.array_equal(want[0, 1:], -got["ncells"][1:].astype(np.float64))
            total = abs(float(got["xi"][0, 0].sum()))
            print(n, fb, "the l = 0 sums over all shells", total, "bound", float(bound[0].sum()))
            assert total <= bound[0].sum()
        # two haloes at cell centres d cells apart, along the line of sight and across it
        for los in range(3):
            for d in (3, n // 2):
                for along, gain in ((True, (N3 / 2, N3 / 2, N3 / 2)), (False, (N3 / 2, -N3 / 4, 3 * N3 / 16))):
                    pos, mass = cc.pair(n, los, d, along)
                    got = f.halo_correlation(pos, None, mass, [cc.ONE], los=los, ngp=True, cross=False)
                    g, info = npl.deposit(n, pos, None, mass, 1, 2 ** 31 - 1, ngp=True)
                    dens = nph.contrast(g, info["weight_sum"], n, fb)
                    base = npc.shells(-np.ones((n, n, n)), 0, 8, los)
                    want, absum = base["xi"].copy(), absums(base["parts"])
                    want[0, 0] += N3 / 2
                    want[:, d] += np.array(gain)
                    absum[0, 0] += N3 / 2
                    absum[:, d] += np.abs(np.array(gain))
                    bound = corr_bound(n, fb, dens, None, True, False, absum)[0]
                    err = np.abs(got["xi"][0] - want)
                    print(n, fb, "pair", los, d, along, "largest error / bound", float(np.max(err / bound)), "largest error", float(err.max()))
                    assert np.all(err <= bound), (los, d, along)
                    assert abs(float(got["xi"][0, 0].sum())) <= bound[0].sum()
        # Parseval: the zero-lag cell is the sum over the shells of the halo power
        pos, vel, mass = list_for(n, seed=40 + n, count=3000)
        got = f.halo_correlation(pos, None, mass, RANGES, scale=SCALE, cross=False)
        power = f.halo_power(pos, mass, RANGES, scale=SCALE, cross=False)
        ref = npc.correlation(n, pos, None, mass, RANGES, SCALE, field_bytes=fb)
        for b, (lo, hi) in enumerate(RANGES):
            g, info = npl.deposit(n, pos, None, mass, lo, hi, SCALE)
            dens = nph.contrast(g, info["weight_sum"], n, fb)
            bound = corr_bound(n, fb, dens, None, False, False, absums(ref["parts"][b, :6]))[0]
            diff = abs(float(got["xi"][b, 0, 0]) - float(power["power"][b, 1:].sum()))
            print(n, fb, "Parseval, bin", b, diff, "bound", float(2 * bound[0, 0]))
            assert diff <= 2 * bound[0, 0]                                                    # (either side carries one transform's error)
            assert abs(float(got["xi"][b, 0].sum())) <= bound[0].sum()


# ------------------------------------------------------------------------------------------------------------ 6. numpy end to end
@pytest.mark.parametrize("fb,ngp,dec,mw,rsd,los", [(8, False, True, True, True, 0), (8, True, False, False, False, 2), (4, False, False, True, True, 1), (4, True, True, False, False, 0),
                                                   (8, True, True, True, True, 2), (8, False, False, False, False, 1)])
def test_against_numpy_end_to_end(api, fb, ngp, dec, mw, rsd, los):
    n = 32
    pos, vel, mass = list_for(n)
    v, vfac = (vel, 1.0) if rsd else (None, 0.0)
    with api.Fmax(n, field_bytes=fb) as f:
        f.synth_density(seed=33, sigma0=0.4)
        dk = f.density()
        got = f.halo_correlation(pos, v, mass, RANGES, scale=SCALE, vfac=vfac, los=los, mass_weight=mw, ngp=ngp, deconvolve=dec)
    ref = npc.correlation(n, pos, v, mass, RANGES, SCALE, vfac, los, mw, ngp, dec, dk, fb)
    assert np.array_equal(got["ncells"], ref["ncells"]) and np.array_equal(got["r2sum"], ref["r2sum"])
    lin = npp.from_x_slab(dk)
    for b, (lo, hi) in enumerate(RANGES):
        info = ref["info"][b]
        assert {k: int(got[k][b]) for k in nph.INT_KEYS} == info and int(got["cells"][b]) == n ** 3 and int(got["nonfinite_cells"][b]) == 0
        g, _ = npl.deposit(n, pos, v, mass, lo, hi, SCALE, vfac, los, mw, ngp)
        dens = nph.contrast(g, info["weight_sum"], n, fb)
        ba, bc = corr_bound(n, fb, dens, lin, ngp, dec, absums(ref["parts"][b, :6]), absums(ref["parts"][b, 6:]))
        ea, ec = np.abs(got["xi"][b] - ref["xi"][b]), np.abs(got["xi_cross"][b] - ref["xi_cross"][b])
        print(fb, ngp, dec, mw, rsd, los, b, "xi error / bound", float(np.max(ea / ba)), "xi_cross error / bound", float(np.max(ec / bc)))
        assert np.all(ea <= ba) and np.all(ec <= bc), b
        assert np.count_nonzero(got["xi"][b, 1]) > n // 4
    assert np.array_equal(got["variance"], got["xi"][:, 0, 0]) and np.allclose(got["xi_l"][:, 1] * got["ncells"], 5 * got["xi"][:, 1], equal_nan=True)


# ------------------------------------------------------------------------------------------------------------ 7. ranks
def ranks_body(api, n, P, pos, vel, mass, dk, odd_rank):
    nxl = n // P

    def body(f, r):
        f.set_density(dk[r * nxl:(r + 1) * nxl])
        before = f.device_bytes
        for kw in (dict(vfac=0.5 if r == odd_rank else 1.0, los=0), dict(vfac=1.0, los=1 if r == odd_rank else 0),       # one rank with another vfac, another los,
                   dict(vfac=1.0, los=0, scale=0.0 if r == odd_rank else 1.0)):                                           # one rank that refuses on its own
            with pytest.raises(api.PinfmaxError, match="pf_halo_correlation: (r|a scale of 0)"):
                f.halo_correlation(pos, vel, mass, RANGES, **kw)
        order = np.random.default_rng(100 + r).permutation(len(mass))      # every rank its own order
        out = [f.halo_correlation(pos[order], vel[order], mass[order], RANGES, vfac=1.0, los=0, mass_weight=True, deconvolve=True),
               f.halo_correlation(pos, vel, mass, RANGES, vfac=-1.0, los=2, ngp=True, cross=False)]
        assert f.device_bytes == before
        return out

    return body


@pytest.mark.parametrize("n,P", [(32, 2), (64, 4), (48, 3)])
def test_every_rank_returns_the_bits_of_one_rank(api, n, P):
    pos, mass = hc.random_list(40 + P, 1500, n)
    vel = np.random.default_rng(41 + P).normal(0.0, 1.5, size=pos.shape)
    pos[:4, 0], vel[:4, 0] = [n - 0.5, 0.25, n - 1.0, 3.0], [2.0, -1.0, 1.0, np.nan]
    dk = synth.make_density(n, seed=50 + P)
    with api.Fmax(n) as f:
        f.set_density(dk)
        one = [f.halo_correlation(pos, vel, mass, RANGES, vfac=1.0, los=0, mass_weight=True, deconvolve=True),
               f.halo_correlation(pos, vel, mass, RANGES, vfac=-1.0, los=2, ngp=True, cross=False)]
    assert int(one[0]["nonfinite"][0]) == 1 and np.count_nonzero(one[0]["xi_cross"][0, 1]) > n // 4
    res = run_ranks(api, n, P, ranks_body(api, n, P, pos, vel, mass, dk, P - 1))
    for r in range(P):
        for got, want in zip(res[r], one):
            assert same(got, want), r
            for k in INFO_KEYS:
                assert np.array_equal(got[k], want[k]), (r, k)
            assert got["weight2"] == want["weight2"]


# ------------------------------------------------------------------------------------------------------------ 8. state and refusals
def test_the_call_leaves_the_context_as_it_was(api):
    n = 32
    pos, vel, mass = list_for(n)

    def run(with_call):
        with api.Fmax(n) as f:
            if with_call:                                                   # no density yet: xi alone
                first = f.halo_correlation(pos, vel, mass, RANGES, scale=SCALE, vfac=1.0, cross=False)
            f.synth_density(seed=77, sigma0=0.4)
            f.set_invgrow(*synth.invgrow_table("lcdm"))
            f.set_growth(synth.growth_multipliers())
            if with_call:
                full = f.halo_correlation(pos, vel, mass, RANGES, scale=SCALE, vfac=1.0)
                assert np.array_equal(bits(first["xi"]), bits(full["xi"]))
            f.compute_fmax(np.array([1.0, 0.0]), do_lpt=True)
            state = (f.device_bytes, f.arithmetic, f.L.pf_replicated_spectrum(f.h))
            prod = f.products().tobytes()
            if with_call:
                f.halo_correlation(pos, vel, mass, RANGES, scale=SCALE, vfac=1.0, los=0, mass_weight=True, deconvolve=True)
                f.halo_correlation(pos, None, mass, RANGES[:1], scale=SCALE, ngp=True, cross=False)
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
    nc, r2 = np.full(nb + 1, 0xABCDEF, np.uint64), np.full(nb + 1, 0xABCDEF, np.uint64)
    xi, xc = np.full(6 * nb + 1, 123.5), np.full(6 * nb + 1, 123.5)
    info = (_lib.CorrInfo * 3)()
    for k in range(3):
        info[k].halo.selected = 0xABCDEF
    pos, mass = hc.random_list(7, 50, n)
    vel = np.ones_like(pos)
    rg = np.array([[1, 100], [50, 5000]], np.int32)
    up, dp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_ulonglong))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int)))
    big = next(c for c in hc.cases(n) if c["name"] == "headroom_16")

    def untouched():
        return np.all(nc == 0xABCDEF) and np.all(r2 == 0xABCDEF) and np.all(xi == 123.5) and np.all(xc == 123.5) and all(info[k].halo.selected == 0xABCDEF for k in range(3))

    with api.Fmax(n) as f:
        L = f.L
        call = lambda **k: L.pf_halo_correlation(k.get("h", f.h), k.get("flags", 0), k.get("count", len(mass)), k.get("pos", dp(pos)), k.get("vel", dp(vel)), k.get("scale", 1.0),
                                                 k.get("vfac", 0.5), k.get("los", 2), k.get("mass", ip(mass)), k.get("nbins", 2), k.get("rg", ip(rg)), k.get("nc", up(nc)),
                                                 k.get("r2", up(r2)), k.get("xi", dp(xi)), k.get("xc", dp(xc)), k.get("info", info))
        assert call() != 0 and b"pf_halo_correlation: density not set" in L.pf_last_error() and untouched()       # xi_cross without a density
        f.synth_density(seed=3)
        before = f.device_bytes
        bad_rg = np.array([[1, 100], [0, 5]], np.int32)
        for kw, what in (({"h": None}, b"null argument"), ({"pos": None}, b"null argument"), ({"mass": None}, b"null argument"), ({"rg": None}, b"null argument"),
                         ({"nc": None}, b"null argument"), ({"r2": None}, b"null argument"), ({"xi": None}, b"null argument"), ({"info": None}, b"null argument"),
                         ({"flags": 8}, b"unknown flag bits"), ({"nbins": 0}, b"0 bins"), ({"nbins": 9}, b"9 bins"), ({"rg": ip(bad_rg)}, b"bin 1 takes the masses 0 to 5"),
                         ({"scale": 0.0}, b"a scale of 0"), ({"scale": float("nan")}, b"a scale of"), ({"count": 2 ** 31 + 1}, b"more than 2^31"),
                         ({"los": 3}, b"a line of sight along axis 3"), ({"los": -1}, b"a line of sight along axis -1"), ({"vfac": float("nan")}, b"a vfac of"),
                         ({"vfac": float("inf")}, b"a vfac of inf"), ({"vel": None}, b"a vfac of 0.5 without velocities")):
            assert call(**kw) != 0, kw
            assert what in L.pf_last_error() and b"pf_halo_correlation" in L.pf_last_error(), (kw, L.pf_last_error())
            assert untouched() and before == f.device_bytes, kw
        one_bin = np.array([[1, 5], [hc.BIG, hc.BIG]], np.int32)
        bigvel = np.zeros_like(big["pos"])
        assert call(flags=4, count=16, pos=dp(big["pos"]), vel=dp(bigvel), mass=ip(big["mass"]), rg=ip(one_bin)) != 0
        assert b"pf_halo_correlation: the weights of bin 1 add up to 17179869184" in L.pf_last_error() and untouched() and before == f.device_bytes
        assert "ERROR on task 0: pf_halo_correlation" in capfd.readouterr().out
        assert call(count=16, pos=dp(big["pos"]), vel=None, vfac=0.0, mass=ip(big["mass"]), rg=ip(one_bin), xc=None) == 0          # real space, no cross: vel may be null
        assert info[1].halo.selected == 16 == info[1].halo.weight_sum and info[0].halo.selected == 0 and info[2].halo.selected == 0xABCDEF and np.all(xc == 123.5)
        assert info[1].cells == n ** 3 == info[0].cells and info[1].nonfinite_cells == 0
        assert nc[-1] == r2[-1] == 0xABCDEF and xi[-1] == 123.5 and not np.any(xi[:3 * nb]) and np.count_nonzero(xi[3 * nb:4 * nb]) > 4 and before == f.device_bytes
        assert int(nc[:nb].sum()) == n ** 3
        # every bin empty: zeros, and the counts all the same
        none = np.array([[hc.BIG + 1, hc.BIG + 2]], np.int32)
        assert call(count=16, pos=dp(big["pos"]), vel=None, vfac=0.0, mass=ip(big["mass"]), nbins=1, rg=ip(none), xc=None) == 0
        assert info[0].halo.selected == 0 and info[0].cells == n ** 3 and not np.any(xi[:3 * nb]) and int(nc[:nb].sum()) == n ** 3


def test_more_than_one_rank_without_an_exchange_is_refused(api):
    pos, mass = hc.random_list(7, 50, 16)
    with api.Fmax(16, rank=0, nranks=2) as f:
        with pytest.raises(api.PinfmaxError, match="pf_halo_correlation: no exchange installed for 2 ranks"):
            f.halo_correlation(pos, np.zeros_like(pos), mass, RANGES, cross=False)
