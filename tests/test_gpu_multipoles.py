"""The redshift-space multipoles on the device (include/pinfmax.h: pf_halo_multipoles, pf_debug_halo_deposit_rsd,
pf_debug_multipole_shells) against the numpy restatement (tests/np_multipoles.py): the planted velocities of
tests/multipole_cases.py through the deposit tap, planted and random spectra through the shell tap, the real-space identity with
pf_halo_power, a random catalogue in three bins, plane waves whose multipole ratios are known in closed form, the three transform
paths, any number of ranks through the in-process fabric, the state the call must leave alone, and the refusals.

What is equal and what is bounded, as in tests/test_gpu_halo.py.  Grids, counters, nmodes and k2sum are integers: equal.  The
eleven positive sums of a shell are fixed-point sums of the terms the restatement forms bit for bit: within TOL_POWER = 1e-14 of
math.fsum, and `power` / `cross`, differences of two such sums, within TOL_POWER times (positive + negative part).  The call itself is
held bit for bit against the restated contrast taken through the context's own transform and the shell tap, and against numpy's
transform within spectra_bound of tests/test_gpu_matter.py, which stands for every l since |L_l| <= 1."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import halo_cases as hc
import multipole_cases as mc
import np_halo as nph
import np_multipoles as npl
import np_power as npp
from pinocchio_amd import synth
from test_gpu_multirank import run_ranks
from test_gpu_power import TOL_POWER
from test_halo_cpu import WINDOWS, window_of

pytestmark = pytest.mark.gpu

RANGES = [(10, 2 ** 31 - 1), (100, 2 ** 31 - 1), (1000, 2 ** 31 - 1)]
ONE = (1, 2 ** 31 - 1)
INFO_KEYS = nph.INT_KEYS + ("modes", "nonfinite_modes")


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(a, b, keys=("nmodes", "k2sum", "power", "cross")):
    return all((a[k] is None and b[k] is None) or np.array_equal(bits(a[k]), bits(b[k])) for k in keys)


# ------------------------------------------------------------------------------------------------------------ 1. the deposit tap
@pytest.mark.parametrize("n", [16, 24])
def test_deposit_tap(api, n):
    """without velocities the grids of pf_debug_halo_deposit; with the planted velocities the restatement's, for every line of sight"""
    for case in hc.cases(n):
        for r, (lo, hi) in enumerate(case["ranges"]):
            if case["what"][r] == ("refused",):
                with pytest.raises(api.PinfmaxError, match="pf_debug_halo_deposit_rsd: the weights of bin 0 add up to"):
                    api.debug_halo_deposit_rsd(n, case["pos"], None, case["mass"], lo, hi, case["scale"], 0.0, r % 3, case["mass_weight"])
                continue
            for ngp in (False, True):
                a = api.debug_halo_deposit(n, case["pos"], case["mass"], lo, hi, case["scale"], case["mass_weight"], ngp)
                b = api.debug_halo_deposit_rsd(n, case["pos"], None, case["mass"], lo, hi, case["scale"], 0.0, r % 3, case["mass_weight"], ngp)
                assert np.array_equal(a[0], b[0]) and a[1] == b[1], (case["name"], r, ngp)
    for los in range(3):
        for case in mc.velocity_cases(n, los):
            for ngp in (False, True):
                for mw in (False, True):
                    whole = npl.deposit(n, case["pos"], case["vel"], case["mass"], *ONE, case["scale"], case["vfac"], los, mw, ngp)
                    for x0, nxl in WINDOWS(n):
                        g, info = api.debug_halo_deposit_rsd(n, case["pos"], case["vel"], case["mass"], *ONE, case["scale"], case["vfac"], los, mw, ngp, x0, nxl)
                        w, wi = window_of(whole, n, x0, nxl)
                        name = (case["name"], n, los, ngp, mw, x0, nxl)
                        assert np.array_equal(g, w) and {k: info[k] for k in nph.INT_KEYS} == wi, name
                        assert (info["selected"], info["nonfinite"], info["outside"]) == case["counts"] and info["modes"] == 0, name


# ------------------------------------------------------------------------------------------------------------ 2. planted spectra
@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("n", [16, 24])
def test_shell_tap_on_planted_spectra(api, n, fb):
    nb = npp.bins(n)
    for los in range(3):
        on, across = [0, 0, 0], [0, 0, 0]
        on[los], across[(los + 1) % 3] = 3, 5
        lin = mc.planted_spectrum(n, on, 2.0 + 1.0j) + mc.planted_spectrum(n, across, -1.0 + 0.5j) + mc.planted_spectrum(n, (0, 0, 0), -2.0)
        # on the line of sight: mu = 1, every weight is 1
        got = api.debug_multipole_shells(mc.planted_spectrum(n, on), lin, 0, fb, los=los)
        p = got["parts"]
        assert p[0, 3] > 0 and np.count_nonzero(p[0]) == 1
        for a, b in ((1, 0), (3, 0), (7, 5), (9, 5)):
            assert np.array_equal(bits(p[a]), bits(p[b])), (los, a, b)
        assert not np.any(p[[2, 4, 6, 8, 10]]) and p[5, 3] > 0                      # cross term (3 - 4i) conj(2 + i) = 2 > 0
        assert np.array_equal(bits(got["power"]), bits(p[[0, 1, 3]])) and np.array_equal(bits(got["cross"]), bits(p[[5, 7, 9]]))
        # transverse: mu = 0, L2 = -1/2 and L4 = 3/8, both exact in binary
        got = api.debug_multipole_shells(mc.planted_spectrum(n, across), lin, 0, fb, los=los)
        p = got["parts"]
        # (the term 25 and the cross term (3 - 4i) conj(-1 + i/2) = -5 times the weights are exact; w = 2 where the mode lies off the planes kz = 0, n/2)
        w, n6 = (2.0 if (los + 1) % 3 == 2 else 1.0), float(n ** 6)
        want = np.zeros((11, nb))
        want[[0, 2, 3, 6, 7, 10], 5] = np.array([25.0, 12.5, 9.375, 5.0, 2.5, 1.875]) * w / n6
        assert np.array_equal(bits(p), bits(want)), (los, p[:, 5] * n6)
        assert np.array_equal(bits(got["power"][:, 5]), bits(np.array([25.0, -12.5, 9.375]) * w / n6)) and np.count_nonzero(got["power"]) == 3
        assert np.array_equal(bits(got["cross"][:, 5]), bits(np.array([-5.0, 2.5, -1.875]) * w / n6)) and np.count_nonzero(got["cross"]) == 3
        # ... and so l2 = -1/2 l0 and l4 = 3/8 l0 of the outputs themselves (for these values the division by N^6 keeps them at both sizes)
        # (equal as numbers, which is equal bits for what is not zero: -1/2 of an empty shell's +0 is -0)
        assert np.array_equal(got["power"][1], -0.5 * got["power"][0]) and np.array_equal(got["power"][2], 0.375 * got["power"][0])
        assert np.array_equal(p[2], 0.5 * p[0]) and np.array_equal(p[3], 0.375 * p[0])
        # k = 0: only l = 0
        got = api.debug_multipole_shells(mc.planted_spectrum(n, (0, 0, 0)), lin, 0, fb, los=los)
        p = got["parts"]
        assert p[0, 0] == 25.0 / n ** 6 and p[6, 0] == 6.0 / n ** 6 and np.count_nonzero(p) == 2 and got["power"].shape == (3, nb)


# ------------------------------------------------------------------------------------------------------------ 3. random spectra
def check_shells(got, want, name):
    assert np.array_equal(got["nmodes"], want["nmodes"]) and np.array_equal(got["k2sum"], want["k2sum"]), name
    assert (got["modes"], got["nonfinite_modes"]) == (want["modes"], want["nonfinite_modes"]), name
    r = npp.rel(got["parts"], want["parts"])
    print(name, "parts rel", r)
    assert r <= TOL_POWER, (name, r)
    P = want["parts"]
    assert np.all(np.abs(got["power"] - want["power"]) <= TOL_POWER * np.stack([P[0], P[1] + P[2], P[3] + P[4]])), name
    if want["cross"] is not None:
        assert np.all(np.abs(got["cross"] - want["cross"]) <= TOL_POWER * np.stack([P[5] + P[6], P[7] + P[8], P[9] + P[10]])), name
    else:
        assert got["cross"] is None and not np.any(got["parts"][5:]), name


@pytest.fixture(scope="module")
def random_shells():
    """the spectra and their restatement, computed once: (n, los, half, fb, ngp, dec) -> dict"""
    out = {}
    for n in (16, 24):
        a, b = mc.random_spectra(n, 70 + n)
        a[3, 2, 1] = np.nan
        out[n] = (a, b, {})
    return out


@pytest.mark.parametrize("n", [16, 24])
def test_random_spectra_through_the_tap(api, random_shells, n):
    a, b, _ = random_shells[n]
    for los in range(3):
        for k, (y0, nyl) in enumerate(((0, n // 2), (n // 2, n // 2), (0, n))):
            fb, ngp, dec = ((8, False, True), (4, True, True), (8, False, False))[(k + los) % 3]
            sa, sb = a[y0:y0 + nyl], b[y0:y0 + nyl]
            name = (n, los, y0, nyl, fb, ngp, dec)
            want = npl.shells(sa, sb, y0, fb, ngp, dec, los)
            got = api.debug_multipole_shells(sa, sb, y0, fb, ngp, dec, los)
            assert want["nonfinite_modes"] == (2 if y0 == 0 else 0)
            check_shells(got, want, name)
            again = api.debug_multipole_shells(sa, sb, y0, fb, ngp, dec, los)
            assert same(got, again, ("nmodes", "k2sum", "power", "cross", "parts")), name                     # the same bits from run to run
        only = api.debug_multipole_shells(a, None, 0, 8, False, True, los)
        check_shells(only, npl.shells(a, None, 0, 8, False, True, los), (n, los, "auto alone"))


FORM_CHILD = """
import sys
import numpy as np
from pinocchio_amd import api
data = np.load(sys.argv[1])
out = {}
for los in range(3):
    for fb in (8, 4):
        for two in (1, 0):
            got = api.debug_multipole_shells(data["m"], data["lin"] if two else None, 0, fb, False, True, los)
            for k in ("nmodes", "k2sum", "power", "parts"):
                out["%s_%d_%d_%d" % (k, los, fb, two)] = got[k]
            out["form_%d_%d_%d" % (los, fb, two)] = np.array(api.multipole_form())
np.savez(sys.argv[2], **out)
"""


def test_the_grouping_of_the_sums_changes_no_bit(api, random_shells, tmp_path):
    """as many sums per pass as the LDS tables hold, or (PF_MULTIPOLE_SCAN_EACH=1) one: each in a fresh child process -- the passes
    that ran, and identical bits"""
    n = 24
    a, b, _ = random_shells[n]
    np.savez(tmp_path / "in.npz", m=a, lin=b)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    got = {}
    for each in ("0", "1"):
        env = dict(os.environ, PF_MULTIPOLE_SCAN_EACH=each, PYTHONPATH=root)
        r = subprocess.run([sys.executable, "-c", FORM_CHILD, str(tmp_path / "in.npz"), str(tmp_path / ("out%s.npz" % each))], env=env, capture_output=True, text=True, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        got[each] = np.load(tmp_path / ("out%s.npz" % each))
    for los in range(3):
        for fb in (8, 4):
            for two in (1, 0):
                key = "_%d_%d_%d" % (los, fb, two)
                total = 11 if two else 5
                assert got["1"]["form" + key].tolist() == [total, total] and got["0"]["form" + key].tolist() == [1, 1]         # a small grid: every sum in one pass
                for k in ("nmodes", "k2sum", "power", "parts"):
                    assert np.array_equal(bits(got["0"][k + key]), bits(got["1"][k + key])), (k, key)
    here = api.debug_multipole_shells(a, b, 0, 8, False, True, 1)
    assert np.array_equal(bits(here["parts"]), bits(got["1"]["parts_1_8_1"])) and api.multipole_form() == (1, 1)


# ------------------------------------------------------------------------------------------------------------ 4. real space
def real_space_identity(api, f, n, pos, vel, mass, los_list, combos):
    for ngp, dec, mw in combos:
        kw = dict(scale=1.0 / 3.7, mass_weight=mw, ngp=ngp, deconvolve=dec)
        want = f.halo_power(pos, mass, RANGES, **kw)
        for los in los_list:
            for v, vfac in ((None, 0.0), (vel, 0.0)):
                got = f.halo_multipoles(pos, v, mass, RANGES, vfac=vfac, los=los, **kw)
                name = (n, ngp, dec, mw, los, v is None)
                assert got["power"].shape == (3, 3, npp.bins(n)) and np.array_equal(bits(got["power"][:, 0]), bits(want["power"])), name
                assert np.array_equal(bits(got["cross"][:, 0]), bits(want["cross"])), name
                assert np.array_equal(got["nmodes"], want["nmodes"]) and np.array_equal(got["k2sum"], want["k2sum"]), name
                for k in INFO_KEYS:
                    assert np.array_equal(got[k], want[k]), (name, k)
                assert got["weight2"] == want["weight2"] and np.array_equal(got["shot"], want["shot"]), name
                assert np.count_nonzero(got["power"][0, 1]) > n // 4 and np.count_nonzero(got["cross"][0, 2]) > n // 4, name
    only = f.halo_multipoles(pos, None, mass, RANGES, scale=1.0 / 3.7, cross=False, ngp=combos[0][0], deconvolve=combos[0][1], mass_weight=combos[0][2])
    full = f.halo_multipoles(pos, None, mass, RANGES, scale=1.0 / 3.7, ngp=combos[0][0], deconvolve=combos[0][1], mass_weight=combos[0][2])
    assert only["cross"] is None and np.array_equal(bits(only["power"]), bits(full["power"]))


def list_for(n, seed=21, count=2000):
    pos, mass = hc.random_list(seed, count, n)
    vel = np.random.default_rng(seed + 1).normal(0.0, 1.5 * 3.7, size=pos.shape)          # N(0, 1.5 cells) in the units of the positions
    return pos * 3.7, vel, mass


@pytest.mark.parametrize("fb", [8, 4])
def test_real_space_is_the_halo_power(api, fb):
    n = 32
    pos, vel, mass = list_for(n)
    with api.Fmax(n, field_bytes=fb) as f:
        f.synth_density(seed=33, sigma0=0.4)
        real_space_identity(api, f, n, pos, vel, mass, (0, 1, 2), [(False, False, False), (False, True, True), (True, False, True), (True, True, False)])


# ------------------------------------------------------------------------------------------------------------ 5. a random catalogue
def restated_chain(api, f, n, fb, pos, vel, mass, vfac, los, mw, dec, got, lin, dk, bound=True):
    """the call's bins against the restated contrast through the context's transform and the shell tap (bits), and through numpy's
    transform and the restated shells (the transform's bound)"""
    from test_gpu_matter import spectra_bound
    for b, (lo, hi) in enumerate(RANGES):
        g, info = npl.deposit(n, pos, vel, mass, lo, hi, 1.0 / 3.7, vfac, los, mw)
        assert {k: int(got[k][b]) for k in nph.INT_KEYS} == info and got["weight2"][b] == (info["weight2_hi"] << 64) | info["weight2_lo"], (b, los)
        assert int(got["modes"][b]) == n ** 3 and int(got["nonfinite_modes"][b]) == 0 and got["shot"][b] == nph.shot(info)
        dens = nph.contrast(g, info["weight_sum"], n, fb)
        chain = api.debug_multipole_shells(npp.from_x_slab(f.forward_transform(dens)), lin, 0, fb, False, dec, los)
        assert np.array_equal(bits(got["power"][b]), bits(chain["power"])) and np.array_equal(bits(got["cross"][b]), bits(chain["cross"])), (b, los, dec)
        assert np.array_equal(got["nmodes"], chain["nmodes"]) and np.array_equal(got["k2sum"], chain["k2sum"])
        if not bound:
            continue
        full = npl.shells(npp.from_x_slab(np.fft.rfftn(dens, axes=(0, 1, 2))), lin, 0, 8, False, dec, los)
        _, bound_p, bound_c = spectra_bound(n, fb, dens, lin, dec)
        for l in range(3):
            dp_, dc_ = np.abs(got["power"][b, l] - full["power"][l]), np.abs(got["cross"][b, l] - full["cross"][l])
            nz = bound_p > 0
            print(n, fb, mw, dec, los, b, 2 * l, "power / bound", float(np.max(dp_[nz] / bound_p[nz])), "cross / bound", float(np.max(dc_[nz] / np.maximum(bound_c[nz], 1e-300))))
            assert np.all(got["power"][b, l][~nz] == 0) and np.all(dp_ <= bound_p) and np.all(dc_ <= bound_c), (b, l, los, dec)
        assert np.count_nonzero(got["power"][b, 1]) > n // 4


@pytest.mark.parametrize("fb,mw", [(8, False), (4, True)])
def test_a_random_catalogue_in_three_bins(api, fb, mw):
    n = 32
    pos, vel, mass = list_for(n)
    perm = np.random.default_rng(5).permutation(len(mass))
    with api.Fmax(n, field_bytes=fb) as f:
        f.synth_density(seed=33, sigma0=0.4)
        dk = f.density()
        lin = npp.from_x_slab(dk)
        for los, dec in ((0, True), (2, False)):
            kw = dict(scale=1.0 / 3.7, vfac=1.0, los=los, mass_weight=mw, deconvolve=dec)
            got = f.halo_multipoles(pos, vel, mass, RANGES, **kw)
            again = f.halo_multipoles(pos[perm], vel[perm], mass[perm], RANGES, **kw)
            assert same(got, again) and all(np.array_equal(got[k], again[k]) for k in INFO_KEYS)            # the order of the list changes no bit
            real = f.halo_power(pos, mass, RANGES, scale=1.0 / 3.7, mass_weight=mw, deconvolve=dec)
            assert not np.array_equal(got["power"][:, 0], real["power"])                                   # ... and the velocities do move the list
            restated_chain(api, f, n, fb, pos, vel, mass, 1.0, los, mw, dec, got, lin, dk)


# ------------------------------------------------------------------------------------------------------------ 6. plane waves
def test_plane_waves(api):
    """one unit halo per cell centre, displaced by 0.3 cos(2 pi 3 x_d / n) cells along axis d.  Displaced along the line of sight
    (by velocity) every mode of the pattern has mu = 1: l2 / l0 = l4 / l0 = 1; displaced across it (in position) mu = 0: -1/2 and 3/8"""
    n = 16
    q = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64) + 0.5
    mass = np.ones(n ** 3, np.int32)
    with api.Fmax(n) as f:
        for los in range(3):
            wave = 0.3 * np.cos(2.0 * np.pi * 3.0 * q[:, los] / n)
            vel = np.zeros_like(q)
            vel[:, los] = wave / 0.25
            along = f.halo_multipoles(q, vel, mass, [(1, 1)], vfac=0.25, los=los, cross=False)
            d = (los + 1) % 3
            moved = q.copy()
            moved[:, d] += 0.3 * np.cos(2.0 * np.pi * 3.0 * q[:, d] / n)
            across = f.halo_multipoles(moved, np.zeros_like(q), mass, [(1, 1)], vfac=0.25, los=los, cross=False)
            for got, r2, r4 in ((along, 1.0, 1.0), (across, -0.5, 0.375)):
                p0, p2, p4 = got["power"][0]
                big = p0 > 1e-6 * p0.max()
                assert int(got["selected"][0]) == n ** 3 and big[3] and np.count_nonzero(big) >= 2
                print(los, r2, "l2 / l0", float(np.max(np.abs(p2[big] / p0[big] - r2))), "l4 / l0", float(np.max(np.abs(p4[big] / p0[big] - r4))))
                assert np.all(np.abs(p2[big] / p0[big] - r2) <= 1e-10) and np.all(np.abs(p4[big] / p0[big] - r4) <= 1e-10), (los, r2)


# ------------------------------------------------------------------------------------------------------------ 7. transform paths
@pytest.mark.parametrize("n,path", [(16, 0), (24, 1), (18, 2)])
def test_transform_paths(api, n, path):
    pos, vel, mass = list_for(n, seed=40 + n, count=1200)
    with api.Fmax(n) as f:
        assert f.L.pf_transform_path(f.h) == path
        f.synth_density(seed=60 + n, sigma0=0.4)
        dk = f.density()
        lin = npp.from_x_slab(dk)
        real_space_identity(api, f, n, pos, vel, mass, (1,), [(False, True, False)])
        got = f.halo_multipoles(pos, vel, mass, RANGES, scale=1.0 / 3.7, vfac=1.0, los=1, deconvolve=True)
        restated_chain(api, f, n, 8, pos, vel, mass, 1.0, 1, False, True, got, lin, dk, bound=False)


# ------------------------------------------------------------------------------------------------------------ 8. ranks
def ranks_body(api, n, P, pos, vel, mass, dk, odd_rank, los_list):
    nxl = n // P

    def body(f, r):
        f.set_density(dk[r * nxl:(r + 1) * nxl])
        before = f.device_bytes
        for kw in (dict(vfac=0.5 if r == odd_rank else 1.0, los=0), dict(vfac=1.0, los=1 if r == odd_rank else 0)):      # one rank with another vfac, another los
            with pytest.raises(api.PinfmaxError, match="pf_halo_multipoles: r"):
                f.halo_multipoles(pos, vel, mass, RANGES, **kw)
        order = np.random.default_rng(100 + r).permutation(len(mass))      # every rank its own order
        out = [f.halo_multipoles(pos[order], vel[order], mass[order], RANGES, vfac=1.0, los=los, mass_weight=True, deconvolve=True) for los in los_list]
        out.append(f.halo_multipoles(pos, vel, mass, RANGES, vfac=-1.0, los=0, ngp=True, cross=False))
        assert f.device_bytes == before
        return out

    return body


@pytest.mark.parametrize("n,P", [(16, 2), (32, 4), (16, 16), (48, 3)])
def test_every_rank_returns_the_bits_of_one_rank(api, n, P):
    pos, mass = hc.random_list(40 + P, 1500, n)
    vel = np.random.default_rng(41 + P).normal(0.0, 1.5, size=pos.shape)
    # the shift decides the owning plane: across both ends of the box along x, onto n exactly, and one that is no velocity
    pos[:4, 0], vel[:4, 0] = [n - 0.5, 0.25, n - 1.0, 3.0], [2.0, -1.0, 1.0, np.nan]
    los_list = (0, 2) if (n, P) == (16, 2) else (0,)
    dk = synth.make_density(n, seed=50 + P)
    with api.Fmax(n) as f:
        f.set_density(dk)
        one = [f.halo_multipoles(pos, vel, mass, RANGES, vfac=1.0, los=los, mass_weight=True, deconvolve=True) for los in los_list]
        one.append(f.halo_multipoles(pos, vel, mass, RANGES, vfac=-1.0, los=0, ngp=True, cross=False))
    assert int(one[0]["nonfinite"][0]) == 1 and np.count_nonzero(one[0]["cross"][0, 1]) > n // 4
    res = run_ranks(api, n, P, ranks_body(api, n, P, pos, vel, mass, dk, P - 1, los_list))
    for r in range(P):
        for got, want in zip(res[r], one):
            assert same(got, want), r
            for k in INFO_KEYS:
                assert np.array_equal(got[k], want[k]), (r, k)
            assert got["weight2"] == want["weight2"] and np.array_equal(got["shot"], want["shot"])


# ------------------------------------------------------------------------------------------------------------ 9. state and refusals
def test_the_call_leaves_the_context_as_it_was(api):
    n = 32
    pos, vel, mass = list_for(n)

    def run(with_call):
        with api.Fmax(n) as f:
            f.synth_density(seed=77, sigma0=0.4)
            f.set_invgrow(*synth.invgrow_table("lcdm"))
            f.set_growth(synth.growth_multipliers())
            if with_call:
                f.halo_multipoles(pos, vel, mass, RANGES, scale=1.0 / 3.7, vfac=1.0)
            f.compute_fmax(np.array([1.0, 0.0]), do_lpt=True)
            state = (f.device_bytes, f.arithmetic, f.L.pf_replicated_spectrum(f.h))
            prod = f.products().tobytes()
            if with_call:
                f.halo_multipoles(pos, vel, mass, RANGES, scale=1.0 / 3.7, vfac=1.0, los=0, mass_weight=True, deconvolve=True)
                f.halo_multipoles(pos, None, mass, RANGES[:1], scale=1.0 / 3.7, ngp=True, cross=False)
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
    pw, cr = np.full(6 * nb + 1, 123.5), np.full(6 * nb + 1, 123.5)
    info = (_lib.HaloInfo * 3)()
    for k in range(3):
        info[k].selected = 0xABCDEF
    pos, mass = hc.random_list(7, 50, n)
    vel = np.ones_like(pos)
    rg = np.array([[1, 100], [50, 5000]], np.int32)
    up, dp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_ulonglong))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int)))
    big = next(c for c in hc.cases(n) if c["name"] == "headroom_16")

    def untouched():
        return np.all(nm == 0xABCDEF) and np.all(ks == 0xABCDEF) and np.all(pw == 123.5) and np.all(cr == 123.5) and all(info[k].selected == 0xABCDEF for k in range(3))

    with api.Fmax(n) as f:
        L = f.L
        call = lambda **k: L.pf_halo_multipoles(k.get("h", f.h), k.get("flags", 0), k.get("count", len(mass)), k.get("pos", dp(pos)), k.get("vel", dp(vel)), k.get("scale", 1.0),
                                                k.get("vfac", 0.5), k.get("los", 2), k.get("mass", ip(mass)), k.get("nbins", 2), k.get("rg", ip(rg)), k.get("nm", up(nm)),
                                                k.get("ks", up(ks)), k.get("pw", dp(pw)), k.get("cr", dp(cr)), k.get("info", info))
        assert call() != 0 and b"pf_halo_multipoles: density not set" in L.pf_last_error() and untouched()       # cross without a density
        f.synth_density(seed=3)
        before = f.device_bytes
        bad_rg = np.array([[1, 100], [0, 5]], np.int32)
        for kw, what in (({"h": None}, b"null argument"), ({"pos": None}, b"null argument"), ({"mass": None}, b"null argument"), ({"rg": None}, b"null argument"),
                         ({"nm": None}, b"null argument"), ({"ks": None}, b"null argument"), ({"pw": None}, b"null argument"), ({"info": None}, b"null argument"),
                         ({"flags": 8}, b"unknown flag bits"), ({"nbins": 0}, b"0 bins"), ({"nbins": 9}, b"9 bins"), ({"rg": ip(bad_rg)}, b"bin 1 takes the masses 0 to 5"),
                         ({"scale": 0.0}, b"a scale of 0"), ({"scale": float("nan")}, b"a scale of"), ({"count": 2 ** 31 + 1}, b"more than 2^31"),
                         ({"los": 3}, b"a line of sight along axis 3"), ({"los": -1}, b"a line of sight along axis -1"), ({"vfac": float("nan")}, b"a vfac of"),
                         ({"vfac": float("inf")}, b"a vfac of inf"), ({"vel": None}, b"a vfac of 0.5 without velocities")):
            assert call(**kw) != 0, kw
            assert what in L.pf_last_error() and b"pf_halo_multipoles" in L.pf_last_error(), (kw, L.pf_last_error())
            assert untouched() and before == f.device_bytes, kw
        one_bin = np.array([[1, 5], [hc.BIG, hc.BIG]], np.int32)
        bigvel = np.zeros_like(big["pos"])
        assert call(flags=4, count=16, pos=dp(big["pos"]), vel=dp(bigvel), mass=ip(big["mass"]), rg=ip(one_bin)) != 0
        assert b"pf_halo_multipoles: the weights of bin 1 add up to 17179869184" in L.pf_last_error() and untouched() and before == f.device_bytes
        assert "ERROR on task 0: pf_halo_multipoles" in capfd.readouterr().out
        assert call(count=16, pos=dp(big["pos"]), vel=None, vfac=0.0, mass=ip(big["mass"]), rg=ip(one_bin), cr=None) == 0          # real space, no cross: vel may be null
        assert info[1].selected == 16 == info[1].weight_sum and info[0].selected == 0 and info[2].selected == 0xABCDEF and np.all(cr == 123.5)
        assert nm[-1] == ks[-1] == 0xABCDEF and pw[-1] == 123.5 and not np.any(pw[:3 * nb]) and np.count_nonzero(pw[3 * nb:4 * nb]) > 4 and before == f.device_bytes


def test_more_than_one_rank_without_an_exchange_is_refused(api):
    pos, mass = hc.random_list(7, 50, 16)
    with api.Fmax(16, rank=0, nranks=2) as f:
        with pytest.raises(api.PinfmaxError, match="pf_halo_multipoles: no exchange installed for 2 ranks"):
            f.halo_multipoles(pos, np.zeros_like(pos), mass, RANGES, cross=False)
