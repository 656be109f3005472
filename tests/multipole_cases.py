"""Planted inputs for the redshift-space multipoles (include/pinfmax.h: pf_halo_multipoles) -- TEST INFRASTRUCTURE shared by the CPU
and the device tests.

velocity_cases(n, los) yields dicts: name, pos and vel [count][3] float64, mass [count] int32, scale, vfac, los and
  p_los    what the position along the line of sight must come out as, per halo (None: nothing beyond the restatement)
  counts   (selected, nonfinite, outside) of the range (1, 2^31 - 1)
planted_spectrum(n, mode) is a ky-slab [n][n][n/2+1] complex128 of exact zeros with one mode (kx, ky, kz) set.
random_spectra(n, seed) are two Hermitian-free random half-spectra (the taps take any numbers) with a steep fall-off."""
import numpy as np

import halo_cases as hc

ONE = (1, 2 ** 31 - 1)


def _case(name, los, pos_los, vel_los, vfac, p_los, counts, scale=1.0, other=(3.5, 7.25)):
    count = len(pos_los)
    pos = np.empty((count, 3))
    vel = np.empty((count, 3))
    axes = [j for j in range(3) if j != los]
    pos[:, los], vel[:, los] = pos_los, vel_los
    for j, x in zip(axes, other):
        pos[:, j] = x / scale
        vel[:, j] = np.nan                       # the other components are never read: anything may stand there
    return {"name": name, "pos": np.ascontiguousarray(pos), "vel": np.ascontiguousarray(vel), "mass": np.arange(5, 5 + count, dtype=np.int32), "scale": scale, "vfac": vfac,
            "los": los, "p_los": p_los, "counts": counts}


def velocity_cases(n, los):
    out = []
    # across the upper and the lower edge of the box (all numbers exact in binary)
    out.append(_case("crosses_the_edge", los, [n - 0.25, 0.25, n - 0.5], [1.0, -1.0, 8.0], 0.5, [0.25, n - 0.25, 3.5], (3, 0, 0)))
    # exactly on n: wraps to 0; exactly on 0 from above: stays
    out.append(_case("lands_on_n", los, [n - 1.0, 1.0, 0.0], [2.0, -2.0, 2.0 * n], 0.5, [0.0, 0.0, 0.0], (3, 0, 0)))
    # no velocity at all: vfac = 0 moves nothing, but NaN 0 and inf 0 are NaN
    out.append(_case("not_finite_with_vfac_0", los, [1.5, 2.5, 3.5, 4.5], [np.nan, np.inf, -np.inf, 1e300], 0.0, [np.nan, np.nan, np.nan, 4.5], (1, 3, 0)))
    # a negative vfac turns the shift round
    out.append(_case("vfac_negative", los, [2.0, n - 1.0, 0.25], [4.0, -8.0, 2.0], -0.25, [1.0, 1.0, n - 0.25], (3, 0, 0)))
    # more than a box away: one wrap does not bring it back
    out.append(_case("more_than_a_box", los, [1.0, n - 1.0, 2.0], [2.0 * (2 * n + 1), -2.0 * (2 * n + 1), 2.0 * n], 0.5, [n + 2.0, -2.0, 2.0], (1, 0, 2)))
    # the shift is in the units of the positions: moved first, scaled after
    out.append(_case("scaled", los, [2.0 * (n - 0.25), 0.5, 5.0], [1.0, -1.0, 0.0], 1.0, [0.25, n - 0.25, 2.5], (3, 0, 0), scale=0.5))
    # a list over more than one workgroup, shifts of a cell or two both ways, a product and a sum that round
    pos, mass = hc.random_list(13 + los, 777, n)
    vel = np.random.default_rng(17 + los).normal(0.0, 150.0, size=pos.shape)
    out.append({"name": "random_777", "pos": pos * (1.0 / 0.37), "vel": vel, "mass": mass, "scale": 0.37, "vfac": 0.0271, "los": los, "p_los": None, "counts": (777, 0, 0)})
    return out


def planted_spectrum(n, mode, value=3.0 - 4.0j):
    spec = np.zeros((n, n, n // 2 + 1), np.complex128)
    kx, ky, kz = mode
    spec[ky % n, kx % n, kz] = value
    return spec


def random_spectra(n, seed):
    rng = np.random.default_rng(seed)
    shape = (n, n, n // 2 + 1)
    fall = np.exp(-0.4 * rng.uniform(0.0, n, size=shape))                     # a dynamic range of many decades inside a shell
    a = (rng.normal(size=shape) + 1j * rng.normal(size=shape)) * fall
    b = (rng.normal(size=shape) + 1j * rng.normal(size=shape)) * fall
    return a, 0.6 * a + b
