"""The bispectrum of the haloes on the device (include/pinfmax.h: pf_halo_bispectrum) against the numpy restatement
(tests/np_bispec.py): the mask tap bit for bit, the triple tap on planted cosines and, on random fields, bit for bit against the
restatement's integers and within the fixed point's TOL_POWER of math.fsum, the call against its own pieces chained through the taps
bit for bit on every transform path, numpy's own transforms within a bound derived before the run, the ranks against one rank bit for
bit, the state of the context, the refusals.

The bound (bispec_bound): tests/test_gpu_parity.py::test_transforms_vs_pocketfft holds one transform of fp64 fields within e = 1e-13
log2(n) of the largest output, tests/test_gpu_matter.py (spectra_bound) uses e = 3e-5 for fp32 fields.  With numpy's spectrum S of the
restated contrast, M = max |S|, c the window factor of a mode (1 without deconvolution), u the unit roundoff of the field type, w the
Hermitian weight and N3 = n^3:
  a mode of the forward transform is off by at most e M, the masked mode c S of the data field by c e M + u c |S| (the product and
  its rounding to the field type); the count field's N3 is exact in either type;
  a cell of the reverse transform of k-bin i is off by at most d_i = sum over the bin's modes of w times that over N3 -- the
  transform is linear with coefficients of modulus one -- plus (e + u) times the largest cell, itself at most A_i = sum w c |S| / N3
  (for the count field A_i = kmodes[i] and d_i = (e + u) kmodes[i]);
  the sum over the cells of a triple is then off by at most sum_x [(|D_i| + d_i)(|D_j| + d_j)(|D_l| + d_l) - |D_i D_j D_l|], the error
  to first and higher order through the three factors, with numpy's own fields D; the two roundings of a term add 2^-52, and the fixed
  point TOL_POWER, of the absolute sum (itself at most sum_x (|D_i| + d_i)(|D_j| + d_j)(|D_l| + d_l)); psum likewise through two factors.
Every quantity is numpy's own; nothing of the library's output enters."""
import ctypes as C
import math

import numpy as np
import pytest

import bispec_cases as bc
import halo_cases as hc
import np_bispec as npb
import np_halo as nph
import np_power as npp
from pinocchio_amd import synth
from test_gpu_corr import PATHS
from test_gpu_multirank import run_ranks
from test_gpu_power import TOL_POWER

pytestmark = pytest.mark.gpu

RANGES = [(10, 2 ** 31 - 1), (100, 2 ** 31 - 1), (1000, 2 ** 31 - 1)]
INFO_KEYS = nph.INT_KEYS + ("modes", "nonfinite_modes", "cells", "nonfinite_cells")
OUT_KEYS = ("kmodes", "ntri", "bsum", "psum")
SCALE = 1.0 / 3.7


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(a, b, keys=OUT_KEYS):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys)


def list_for(n, seed=21, count=2000):
    pos, mass = hc.random_list(seed, count, n)
    vel = np.random.default_rng(seed + 1).normal(0.0, 1.5 * 3.7, size=pos.shape)          # N(0, 1.5 cells) in the units of the positions
    return pos * 3.7, vel, mass


def cell_error(n, fb, spec, kmin, dk, nk, ngp, dec, kmodes=None):
    """d_i of the head of the file for every k-bin: of the data fields of the spectrum `spec` (a ky-slab), or with spec None of the
    count fields"""
    e, u = (1e-13 * math.log2(n), 2.0 ** -53) if fb == 8 else (3e-5, 2.0 ** -24)
    if spec is None:
        return (e + u) * kmodes.astype(np.float64)
    k2, _, w = npp.geometry(n)
    which = npb.bin_of(k2, kmin, dk, nk)
    c = npb.window(n, 0, n, ngp) if dec else np.ones(k2.shape)
    M, N3 = float(np.max(np.abs(spec))), float(n) ** 3
    d = np.zeros(nk)
    for i in range(nk):
        m = which == i
        A = float((w[m] * c[m] * np.abs(spec[m])).sum()) / N3
        d[i] = float((w[m] * c[m] * (e * M + u * np.abs(spec[m]))).sum()) / N3 + (e + u) * A
    return d


def bispec_bound(fields, d, tri):
    """the bounds of the sums of the closed triples [nt] and of the pair sums [nk] from numpy's fields [nk][n][n][n] and the per-cell
    errors d[nk], see the head of the file"""
    a = np.abs(fields)
    out, pair = np.zeros(len(tri)), np.zeros(len(d))
    for t, (i, j, l) in enumerate(tri):
        plain = float((a[i] * a[j] * a[l]).sum())
        off = float(((a[i] + d[i]) * (a[j] + d[j]) * (a[l] + d[l])).sum())
        out[t] = (off - plain) + (2.0 ** -52 + TOL_POWER) * off
    for i in range(len(d)):
        plain, off = float((a[i] * a[i]).sum()), float(((a[i] + d[i]) ** 2).sum())
        pair[i] = (off - plain) + (2.0 ** -53 + TOL_POWER) * off
    return out, pair


# ------------------------------------------------------------------------------------------------------------ 1. the mask tap
@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("n", [16, 24])
def test_mask_tap(api, n, fb):
    kmin, dk, nk = bc.BY_N[n]
    rng = np.random.default_rng(3 + n)
    shape = (n, n, n // 2 + 1)
    a = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.exp2(rng.integers(-8, 9, shape).astype(np.float64))
    a[2, 1, 1] = np.inf + 0j                      # ky 2, kx 1, kz 1: k2 = 6, inside a bin of either case; weight 2
    planted = int(npb.bin_of(np.array([6]), kmin, dk, nk)[0])
    assert planted >= 0
    for y0, nyl in ((0, n), (n // 2, n // 2), (3, 5)):
        sa = np.ascontiguousarray(a[y0:y0 + nyl])
        k2, _, w = npp.geometry(n, y0, nyl)
        for which in range(nk):
            for kind, ngp, dec in ((0, False, False), (1, False, False), (0, False, True), (0, True, True), (1, True, True)):
                got, info = api.debug_bispec_mask(sa, kmin, dk, nk, which, y0, fb, ngp, dec, kind)
                want, km, nonfin = npb.mask(sa, kmin, dk, nk, which, y0, fb, ngp, dec, kind)
                name = (n, fb, y0, which, kind, ngp, dec)
                assert np.array_equal(bits(got.real), bits(want.real)) and np.array_equal(bits(got.imag), bits(want.imag)), name
                assert info == {"kmodes": km, "nonfinite_modes": nonfin}, name
                inside = npb.bin_of(k2, kmin, dk, nk) == which
                assert km == int(w[inside].sum()) and nonfin == (2 if which == planted and y0 <= 2 < y0 + nyl else 0), name    # the Hermitian-weighted count
                assert not np.any(got[~inside]) and (kind == 0 or np.all(got[inside & np.isfinite(sa)] == float(n) ** 3)), name
                if y0 == 0:
                    assert got[0, 0, 0] == 0 and got[2, 1, 1] == 0 and np.count_nonzero(got) == np.count_nonzero(inside) - (which == planted), name


# ------------------------------------------------------------------------------------------------------------ 2. the triple tap
@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("case", [c for c in bc.CASES if c[3] >= 3 and c[0] <= 24])
def test_triple_tap_on_planted_cosines(api, case, fb):
    n, kmin, dk, nk = case
    (bi, bj, bl), k1, k2, k3 = bc.planted_triangle(n, kmin, dk, nk)
    tri = npb.triangles(kmin, dk, nk)
    A, B, Cc = 1.5, -0.75, 2.25
    u = 2.0 ** -24 if fb == 4 else 2.0 ** -53 * (2.0 * math.pi * 3 * (kmin + nk * dk) + 2.0)      # of a factor: the field type's rounding, or that of the cosine's argument
    for phi in (0.0, 1.0, math.pi / 2, 2.5):
        f = np.zeros((nk, n, n, n))
        # the three parts of A cos(k1.x) + B cos(k2.x) + C cos(k3.x + phi), each in the field of its own k-bin
        f[bi], f[bj], f[bl] = bc.cosines(n, k1, k2, k3, A, 0.0, 0.0, phi), bc.cosines(n, k1, k2, k3, 0.0, B, 0.0, phi), bc.cosines(n, k1, k2, k3, 0.0, 0.0, Cc, phi)
        amp = {bi: abs(A), bj: abs(B), bl: abs(Cc)}
        got = api.debug_bispec_triples(f, kmin, dk, nk, 0, fb)
        for t, (i, j, l) in enumerate(tri):
            want = n ** 3 * A * B * Cc * math.cos(phi) / 4 if (i, j, l) == (bi, bj, bl) else 0.0
            absum = n ** 3 * amp.get(i, 0.0) * amp.get(j, 0.0) * amp.get(l, 0.0)
            assert abs(got["sums"][t] - want) <= (TOL_POWER + 3 * u) * absum, (case, fb, phi, (i, j, l), got["sums"][t], want)
        assert np.array_equal(got["maxima"], np.abs(npb.as_stores(f, fb)[0]).max(axis=(1, 2, 3))) and got["nonfinite_cells"] == 0
        assert np.allclose(got["pair"][[bi, bj, bl]], [n ** 3 * A * A / 2, n ** 3 * B * B / 2, n ** 3 * Cc * Cc / 2], rtol=1e-6)


@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("case", bc.SMALL)
def test_triple_tap_on_random_fields(api, case, fb):
    n, kmin, dk, nk = case
    f = bc.random_fields(nk, n, n, 5 + n)
    f[nk - 1, 3, 2, 1] = np.inf                   # a cell that is not finite: stored as zero and counted
    f[0, 0, 0, :2] = [0.0, -0.0]
    for wins in bc.x_windows(n):
        for x0, nxl in wins:
            part = np.ascontiguousarray(f[:, x0:x0 + nxl])
            got = api.debug_bispec_triples(part, kmin, dk, nk, x0, fb)
            want = npb.triples(part, kmin, dk, nk, fb)
            name = (case, fb, x0, nxl)
            assert got["nonfinite_cells"] == want["nonfinite_cells"] == (1 if x0 <= 3 < x0 + nxl else 0), name
            assert np.array_equal(bits(got["maxima"]), bits(want["maxima"])), name
            for k in ("parts", "sums", "pair"):                                               # the restatement's Python integers: bit for bit
                assert np.array_equal(bits(got[k]), bits(want[k])), (name, k)
            rp, rq = npp.rel(got["parts"], want["parts_fsum"]), npp.rel(got["pair"], want["pair_fsum"])
            print(name, "positive sums against fsum", rp, "pair sums", rq)
            assert rp <= TOL_POWER and rq <= TOL_POWER
            assert np.array_equal(bits(got["sums"]), bits(got["parts"][0] - got["parts"][1])) and np.all(got["parts"] > 0)


# ------------------------------------------------------------------------------------------------------------ 3. the call against its pieces
def chain(api, f, n, fb, pos, vel, mass, lo, hi, vfac, los, mw, ngp, dec, kmin, dk, nk):
    """the pieces through the taps: deposit, restated contrast, the context's forward transform, the mask tap per k-bin, the context's
    reverse transform, the triple tap -> (the tap's columns, kmodes, nonfinite modes, the deposit's counters)"""
    g, info = api.debug_halo_deposit_rsd(n, pos, vel, mass, lo, hi, SCALE, vfac, los, mw, ngp)
    dens = nph.contrast(g, info["weight_sum"], n, fb)
    spec = npp.from_x_slab(f.forward_transform(dens))
    fields, km, bad = [], [], 0
    for i in range(nk):
        q, m = api.debug_bispec_mask(spec, kmin, dk, nk, i, 0, fb, ngp, dec, 0)
        fields.append(f.reverse_transform(npp.from_x_slab(q)))
        km.append(m["kmodes"])
        bad += m["nonfinite_modes"]
    return api.debug_bispec_triples(np.array(fields), kmin, dk, nk, 0, fb), km, bad, info


def count_chain(api, f, n, fb, kmin, dk, nk):
    fields = []
    for i in range(nk):
        q, _ = api.debug_bispec_mask(np.zeros((n, n, n // 2 + 1), np.complex128), kmin, dk, nk, i, 0, fb, False, False, 1)
        fields.append(f.reverse_transform(npp.from_x_slab(q)))
    return api.debug_bispec_triples(np.array(fields), kmin, dk, nk, 0, fb)


@pytest.mark.parametrize("n,fb,path", PATHS)
def test_the_call_is_its_pieces(api, n, fb, path):
    kmin, dk, nk = bc.BY_N[n]
    pos, vel, mass = list_for(n, seed=40 + n, count=3000)
    perm = np.random.default_rng(5).permutation(len(mass))
    with api.Fmax(n, field_bytes=fb) as f:
        assert f.L.pf_transform_path(f.h) == path
        kw = dict(scale=SCALE, vfac=1.0, los=1, mass_weight=True, deconvolve=True)
        got = f.halo_bispectrum(pos, vel, mass, RANGES, kmin, dk, nk, **kw)
        again = f.halo_bispectrum(pos[perm], vel[perm], mass[perm], RANGES, kmin, dk, nk, **kw)
        assert same(got, again) and all(np.array_equal(got[k], again[k]) for k in INFO_KEYS)                # the order of the list changes no bit
        corr = f.halo_correlation(pos, vel, mass, RANGES, cross=False, **kw)
        for k in nph.INT_KEYS + ("modes", "cells"):
            assert np.array_equal(got[k], corr[k]), k                                                         # info[b].halo is the correlation call's
        assert np.all(got["cells"] == n ** 3) and not np.any(got["nonfinite_cells"]) and not np.any(got["nonfinite_modes"])
        cnt = count_chain(api, f, n, fb, kmin, dk, nk)
        assert np.array_equal(bits(got["ntri"]), bits(cnt["sums"] / float(n) ** 3))
        assert [tuple(r) for r in got["triangles"]] == npb.triangles(kmin, dk, nk)
        for b, (lo, hi) in enumerate(RANGES):
            tap, km, bad, info = chain(api, f, n, fb, pos, vel, mass, lo, hi, 1.0, 1, True, False, True, kmin, dk, nk)
            assert {k: int(got[k][b]) for k in nph.INT_KEYS} == {k: info[k] for k in nph.INT_KEYS}, b
            assert np.array_equal(bits(got["bsum"][b]), bits(tap["sums"])) and np.array_equal(bits(got["psum"][b]), bits(tap["pair"])), (n, fb, b)
            assert list(got["kmodes"]) == km and bad == 0
            assert np.count_nonzero(got["bsum"][b]) == len(got["triangles"]) and np.all(got["psum"][b] > 0)
        # real space: another answer, the same counts
        real = f.halo_bispectrum(pos, None, mass, RANGES, kmin, dk, nk, scale=SCALE)
        assert np.array_equal(bits(real["ntri"]), bits(got["ntri"])) and np.array_equal(real["kmodes"], got["kmodes"]) and not np.array_equal(real["bsum"], got["bsum"])


# ------------------------------------------------------------------------------------------------------------ 4. numpy end to end
@pytest.mark.parametrize("case,fb,ngp,dec,mw,rsd,los", [(bc.CASES[0], 8, False, True, True, True, 0), (bc.CASES[0], 4, True, False, False, False, 2),
                                                        (bc.CASES[1], 8, True, True, False, True, 1), (bc.CASES[1], 4, False, True, True, False, 0),
                                                        (bc.CASES[2], 8, False, False, False, False, 2), (bc.CASES[2], 4, False, True, True, True, 1),
                                                        (bc.CASES[3], 8, False, True, True, True, 0),
                                                        (bc.CASES[4], 8, True, False, False, False, 1), (bc.CASES[4], 4, False, True, False, True, 2)])
def test_against_numpy_end_to_end(api, case, fb, ngp, dec, mw, rsd, los):
    n, kmin, dk, nk = case
    pos, vel, mass = list_for(n)
    v, vfac = (vel, 1.0) if rsd else (None, 0.0)
    ref = npb.bispectrum(n, pos, v, mass, RANGES, kmin, dk, nk, SCALE, vfac, los, mw, ngp, dec, fb)
    tri = ref["triangles"]
    counts = npb.count_triangles(kmin, dk, nk)
    assert np.all(np.abs(ref["ntri"] - counts) < 1e-6)                                       # numpy's own transforms give the integers
    # the bounds, before the run
    cb, _ = bispec_bound(ref["count_fields"], cell_error(n, fb, None, kmin, dk, nk, ngp, dec, ref["kmodes"]), tri)
    cb = cb / float(n) ** 3
    bounds = [None if ref["spec"][b] is None else bispec_bound(ref["data_fields"][b], cell_error(n, fb, ref["spec"][b], kmin, dk, nk, ngp, dec), tri) for b in range(len(RANGES))]
    with api.Fmax(n, field_bytes=fb) as f:
        got = f.halo_bispectrum(pos, v, mass, RANGES, kmin, dk, nk, scale=SCALE, vfac=vfac, los=los, mass_weight=mw, ngp=ngp, deconvolve=dec, box=100.0)
    assert np.array_equal(got["kmodes"], ref["kmodes"]) and [tuple(r) for r in got["triangles"]] == tri
    en = np.abs(got["ntri"] - counts)
    print(case, fb, "ntri error", float(en.max()), "error / bound", float(np.max(en / cb)), "largest bound", float(cb.max()))
    assert np.all(en <= cb)
    if fb == 8:
        assert np.array_equal(np.round(got["ntri"]).astype(np.int64), counts)
    for b in range(len(RANGES)):
        info = ref["info"][b]
        assert {k: int(got[k][b]) for k in nph.INT_KEYS} == info and int(got["cells"][b]) == n ** 3 and int(got["nonfinite_cells"][b]) == 0
        bb, pb = bounds[b]
        eb, ep = np.abs(got["bsum"][b] - ref["bsum"][b]), np.abs(got["psum"][b] - ref["psum"][b])
        print(case, fb, ngp, dec, mw, rsd, los, b, "bsum error / bound", float(np.max(eb / bb)), "psum error / bound", float(np.max(ep / pb)),
              "bound / absolute sum", float(np.max(bb / ref["babs"][b])))
        assert np.all(eb <= bb) and np.all(ep <= pb), b
    N3 = float(n) ** 3
    assert np.allclose(got["B"], 100.0 ** 6 * got["bsum"] / (N3 * got["ntri"])) and np.allclose(got["pk"], 100.0 ** 3 * got["psum"] / (N3 * got["kmodes"]))
    assert got["Q"].shape == got["B"].shape and np.all(np.isfinite(got["Q"]))


# ------------------------------------------------------------------------------------------------------------ 5. ranks
def ranks_body(api, n, P, pos, vel, mass, kmin, dk, nk, odd_rank):
    def body(f, r):
        before = f.device_bytes
        for kw, kb in ((dict(vfac=1.0, los=0), (kmin, dk, nk - 1 if r == odd_rank else nk)),                       # one rank with other k-bins,
                       (dict(vfac=1.0, los=0), (kmin + 1 if r == odd_rank else kmin, dk, nk - 1)),
                       (dict(vfac=0.5 if r == odd_rank else 1.0, los=0), (kmin, dk, nk)),                          # with another vfac,
                       (dict(vfac=1.0, los=0, scale=0.0 if r == odd_rank else 1.0), (kmin, dk, nk))):              # one rank that refuses on its own
            with pytest.raises(api.PinfmaxError, match="pf_halo_bispectrum: (r|a scale of 0)"):
                f.halo_bispectrum(pos, vel, mass, RANGES, *kb, **kw)
        order = np.random.default_rng(100 + r).permutation(len(mass))      # every rank its own order
        out = [f.halo_bispectrum(pos[order], vel[order], mass[order], RANGES, kmin, dk, nk, vfac=1.0, los=0, mass_weight=True, deconvolve=True),
               f.halo_bispectrum(pos, vel, mass, RANGES, kmin, dk, nk, vfac=-1.0, los=2, ngp=True)]
        assert f.device_bytes == before
        return out

    return body


@pytest.mark.parametrize("n,P", [(32, 2), (64, 4), (48, 3)])
def test_every_rank_returns_the_bits_of_one_rank(api, n, P):
    kmin, dk, nk = bc.BY_N[n]
    pos, mass = hc.random_list(40 + P, 1500, n)
    vel = np.random.default_rng(41 + P).normal(0.0, 1.5, size=pos.shape)
    pos[:4, 0], vel[:4, 0] = [n - 0.5, 0.25, n - 1.0, 3.0], [2.0, -1.0, 1.0, np.nan]
    with api.Fmax(n) as f:
        one = [f.halo_bispectrum(pos, vel, mass, RANGES, kmin, dk, nk, vfac=1.0, los=0, mass_weight=True, deconvolve=True),
               f.halo_bispectrum(pos, vel, mass, RANGES, kmin, dk, nk, vfac=-1.0, los=2, ngp=True)]
    assert int(one[0]["nonfinite"][0]) == 1 and np.count_nonzero(one[0]["bsum"]) == one[0]["bsum"].size
    res = run_ranks(api, n, P, ranks_body(api, n, P, pos, vel, mass, kmin, dk, nk, P - 1))
    for r in range(P):
        for got, want in zip(res[r], one):
            assert same(got, want), r
            for k in INFO_KEYS:
                assert np.array_equal(got[k], want[k]), (r, k)
            assert got["weight2"] == want["weight2"]


# ------------------------------------------------------------------------------------------------------------ 6. state
def test_the_call_leaves_the_context_as_it_was(api):
    n = 32
    kmin, dk, nk = bc.BY_N[n]
    pos, vel, mass = list_for(n)

    def run(with_call):
        with api.Fmax(n) as f:
            if with_call:                                                   # no density yet: the call needs none
                first = f.halo_bispectrum(pos, vel, mass, RANGES, kmin, dk, nk, scale=SCALE, vfac=1.0)
            f.synth_density(seed=77, sigma0=0.4)
            f.set_invgrow(*synth.invgrow_table("lcdm"))
            f.set_growth(synth.growth_multipliers())
            if with_call:
                full = f.halo_bispectrum(pos, vel, mass, RANGES, kmin, dk, nk, scale=SCALE, vfac=1.0)
                assert same(first, full)
            f.compute_fmax(np.array([1.0, 0.0]), do_lpt=True)
            state = (f.device_bytes, f.arithmetic, f.L.pf_replicated_spectrum(f.h))
            prod = f.products().tobytes()
            if with_call:
                f.halo_bispectrum(pos, vel, mass, RANGES, kmin, dk, nk, scale=SCALE, vfac=1.0, los=0, mass_weight=True, deconvolve=True)
                f.halo_bispectrum(pos, None, mass, RANGES[:1], 1, 1, 2, scale=SCALE, ngp=True)
                assert state == (f.device_bytes, f.arithmetic, f.L.pf_replicated_spectrum(f.h))
                assert prod == f.products().tobytes()
            f.sweep(np.array([2.0, 1.0]))
            return f.products()["Fmax"].tobytes(), prod, f.power_spectrum("density", (1.0,)), f.density()

    a, b = run(False), run(True)
    assert a[0] == b[0] and a[1] == b[1]
    assert all(np.array_equal(a[2][k], b[2][k]) for k in ("nmodes", "k2sum", "power", "variance")) and np.array_equal(a[3], b[3])


# ------------------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_on_a_live_context(api, capfd):
    from pinocchio_amd import _lib
    n, kmin, dk, nk = 16, 1, 2, 2
    nt = len(npb.triangles(kmin, dk, nk))
    km = np.full(nk + 1, 0xABCDEF, np.uint64)
    ntri, bsum, psum = np.full(nt + 1, 123.5), np.full(3 * nt + 1, 123.5), np.full(3 * nk + 1, 123.5)
    info = (_lib.BispecInfo * 3)()
    for k in range(3):
        info[k].halo.selected = 0xABCDEF
    pos, mass = hc.random_list(7, 50, n)
    vel = np.ones_like(pos)
    rg = np.array([[1, 100], [50, 5000]], np.int32)
    up, dp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_ulonglong))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int)))
    big = next(c for c in hc.cases(n) if c["name"] == "headroom_16")

    def untouched():
        return np.all(km == 0xABCDEF) and np.all(ntri == 123.5) and np.all(bsum == 123.5) and np.all(psum == 123.5) and all(info[k].halo.selected == 0xABCDEF for k in range(3))

    with api.Fmax(n) as f:
        L = f.L
        call = lambda **k: L.pf_halo_bispectrum(k.get("h", f.h), k.get("flags", 0), k.get("count", len(mass)), k.get("pos", dp(pos)), k.get("vel", dp(vel)), k.get("scale", 1.0),
                                                k.get("vfac", 0.5), k.get("los", 2), k.get("mass", ip(mass)), k.get("nbins", 2), k.get("rg", ip(rg)), k.get("kmin", kmin),
                                                k.get("dk", dk), k.get("nk", nk), k.get("km", up(km)), k.get("ntri", dp(ntri)), k.get("bsum", dp(bsum)), k.get("psum", dp(psum)),
                                                k.get("info", info))
        before = f.device_bytes
        bad_rg = np.array([[1, 100], [0, 5]], np.int32)
        for kw, what in (({"h": None}, b"null argument"), ({"pos": None}, b"null argument"), ({"mass": None}, b"null argument"), ({"rg": None}, b"null argument"),
                         ({"km": None}, b"null argument"), ({"ntri": None}, b"null argument"), ({"bsum": None}, b"null argument"), ({"psum": None}, b"null argument"),
                         ({"info": None}, b"null argument"),
                         ({"flags": 8}, b"unknown flag bits"), ({"nbins": 0}, b"0 bins"), ({"nbins": 9}, b"9 bins"), ({"rg": ip(bad_rg)}, b"bin 1 takes the masses 0 to 5"),
                         ({"scale": 0.0}, b"a scale of 0"), ({"count": 2 ** 31 + 1}, b"more than 2^31"),
                         ({"los": 3}, b"a line of sight along axis 3"), ({"vfac": float("nan")}, b"a vfac of"), ({"vel": None}, b"a vfac of 0.5 without velocities"),
                         ({"kmin": 0}, b"a kmin of 0"), ({"kmin": -3}, b"a kmin of -3"), ({"dk": 0}, b"a dk of 0"), ({"nk": 0}, b"0 k-bins (1 to 32)"),
                         ({"nk": 33, "dk": 1}, b"33 k-bins (1 to 32)"), ({"nk": 3}, b"3 kmax = 3 (1 + 3 * 2) = 21 is above the grid of 16"),
                         ({"kmin": 2, "dk": 2, "nk": 2}, b"3 kmax = 3 (2 + 2 * 2) = 18 is above the grid of 16")):
            assert call(**kw) != 0, kw
            assert what in L.pf_last_error() and b"pf_halo_bispectrum" in L.pf_last_error(), (kw, L.pf_last_error())
            assert untouched() and before == f.device_bytes, kw
        one_bin = np.array([[1, 5], [hc.BIG, hc.BIG]], np.int32)
        bigvel = np.zeros_like(big["pos"])
        assert call(flags=4, count=16, pos=dp(big["pos"]), vel=dp(bigvel), mass=ip(big["mass"]), rg=ip(one_bin)) != 0
        assert b"pf_halo_bispectrum: the weights of bin 1 add up to 17179869184" in L.pf_last_error() and untouched() and before == f.device_bytes
        assert "ERROR on task 0: pf_halo_bispectrum" in capfd.readouterr().out
        assert call(count=16, pos=dp(big["pos"]), vel=None, vfac=0.0, mass=ip(big["mass"]), rg=ip(one_bin)) == 0          # real space: vel may be null; 3 kmax = 15 <= 16
        assert info[1].halo.selected == 16 == info[1].halo.weight_sum and info[0].halo.selected == 0 and info[2].halo.selected == 0xABCDEF
        assert info[1].cells == n ** 3 == info[0].cells and info[1].nonfinite_cells == 0
        assert km[-1] == 0xABCDEF and ntri[-1] == 123.5 and bsum[2 * nt] == 123.5 and psum[2 * nk] == 123.5 and before == f.device_bytes
        assert not np.any(bsum[:nt]) and not np.any(psum[:nk]) and np.all(psum[nk:2 * nk] > 0)                            # the empty bin: zeros
        assert list(np.round(ntri[:nt]).astype(np.int64)) == [3798, 4418, 17508, 39504] and np.all(km[:nk] > 0)
        # every mass bin empty: zeros, and the counts all the same
        counts, modes = ntri[:nt].copy(), km[:nk].copy()
        none = np.array([[hc.BIG + 1, hc.BIG + 2]], np.int32)
        assert call(count=16, pos=dp(big["pos"]), vel=None, vfac=0.0, mass=ip(big["mass"]), nbins=1, rg=ip(none)) == 0
        assert info[0].halo.selected == 0 and info[0].cells == n ** 3 and not np.any(bsum[:nt]) and not np.any(psum[:nk])
        assert np.array_equal(bits(ntri[:nt]), bits(counts)) and np.array_equal(km[:nk], modes)


def test_more_than_one_rank_without_an_exchange_is_refused(api):
    pos, mass = hc.random_list(7, 50, 16)
    with api.Fmax(16, rank=0, nranks=2) as f:
        with pytest.raises(api.PinfmaxError, match="pf_halo_bispectrum: no exchange installed for 2 ranks"):
            f.halo_bispectrum(pos, np.zeros_like(pos), mass, RANGES, 1, 2, 2)
