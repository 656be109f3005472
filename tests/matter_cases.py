"""Planted displacement columns for the matter-density tests -- TEST INFRASTRUCTURE.  cases(n, dtype) -> [(name, vel12 [12][n][n][n] of
dtype, weight or None, ngp, what)], `what` naming what the grid must be where that can be said without any implementation:
"uniform" (every cell exactly 2^48), ("one_cell", (x, y, z)) (everything in that cell), ("counts", nonfinite, outside) or None."""
import numpy as np

ONE = 1 << 48


def zeros(n, dtype):
    return np.zeros((12, n, n, n), dtype=dtype)


def smooth_random(n, dtype, seed, rms=3.0):
    """twelve different smooth columns: a few long waves with random phases each, scaled to `rms` cells for the Zel'dovich ones and a
    tenth, a hundredth of that for the higher orders"""
    rng = np.random.default_rng(seed)
    x = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")).astype(np.float64)
    v = np.zeros((12, n, n, n))
    for k in range(12):
        for _ in range(4):
            kv = rng.integers(-2, 3, size=3)
            v[k] += rng.standard_normal() * np.cos(2.0 * np.pi * np.tensordot(kv, x, axes=1) / n + rng.uniform(0, 2 * np.pi))
        s = np.sqrt(np.mean(v[k] ** 2))
        v[k] *= (rms / (10.0 ** (k // 3))) / (s if s > 0 else 1.0)
    return v.astype(dtype)


def cases(n, dtype):
    T = np.dtype(dtype).type
    out = [("zero_columns", zeros(n, dtype), None, False, "uniform")]
    # whole cells: the lattice moves onto itself.  The shift is spread over the orders so that every statement of the position adds
    for name, s in (("plus_one", 1), ("minus_one", -1), ("plus_half_box", n // 2), ("minus_half_box", -(n // 2)), ("n_minus_one", n - 1)):
        v = zeros(n, dtype)
        v[0] = s                       # x through V1
        v[1] = s; v[4] = -s; v[7] = s  # y through V1 + V2 + V31: +s again
        v[11] = s                      # z through V32
        out.append(("shift_" + name, v, None, False, "uniform"))
    # pos = 0 exactly, then a hair below: + n gives n itself in float (15.999999999 in double)
    v = zeros(n, dtype)
    for j in range(3):
        sl = [slice(None)] * 3
        sl[j] = 0
        v[j][tuple(sl)] = -0.5
        v[3 + j][tuple(sl)] = -1e-9
    out.append(("wrap_to_exactly_n", v, None, False, None))
    v = zeros(n, dtype)
    v[0:3] = -0.25                     # the particles of plane 0 sit below 0.5: i0 = -1
    out.append(("below_half_a_cell", v, None, False, None))
    v = zeros(n, dtype)
    v[0:3] = -np.finfo(dtype).epsneg   # cell 0: u = -epsneg, d = 1 - epsneg, one ulp below 1; the other cells whatever the sum rounds to
    out.append(("d_one_ulp_below_one", v, None, False, None))
    v = zeros(n, dtype)
    q = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    target = (5, n - 1, 0)
    for j in range(3):
        v[j] = target[j] - q[j]
    out.append(("all_into_one_cell", v, None, False, ("one_cell", target)))
    v = smooth_random(n, dtype, 5, rms=0.5)
    v[4, 1, 2, 3] = np.nan
    v[0, 2, 2, 2] = np.inf
    v[8, 3, 0, n - 1] = -np.inf
    v[2, 4, 4, 4] = 2.5 * n
    v[6, 5, 5, 5] = -2.5 * n
    out.append(("nonfinite_and_outside", v, None, False, ("counts", 3, 2)))
    out.append(("smooth_random_rms3", smooth_random(n, dtype, 7), None, False, None))
    out.append(("smooth_random_rms3_ngp", smooth_random(n, dtype, 7), None, True, None))
    out.append(("weighted_zeldovich_only", smooth_random(n, dtype, 9), (1.0, 0.0, 0.0, 0.0), False, None))
    out.append(("weighted_all_ones", smooth_random(n, dtype, 9), (1.0, 1.0, 1.0, 1.0), False, None))
    out.append(("weighted_fractions", smooth_random(n, dtype, 9), (0.5, -1.0, 1.0 / 3.0, 2.0), False, None))
    assert all(c[1].dtype == np.dtype(dtype) and c[1].shape == (12, n, n, n) for c in out)
    return out


def zeroed_by_hand(vel12, weight):
    """the columns whose weight is 0 cleared, for the comparison of a 0 / 1 weight against no weight"""
    v = vel12.copy()
    for o in range(4):
        if weight[o] == 0.0:
            v[3 * o:3 * o + 3] = 0
        else:
            assert weight[o] == 1.0
    return v


def planted_modes(n=16):
    """spectra for the shell sums: [(name, spec_m, spec_lin, expect)] as ky-slabs [n][n][n/2+1]; expect: {shell: (power, cross_pos,
    cross_neg)} times N^6, exact, or None"""
    nzh = n // 2 + 1
    z = lambda: np.zeros((n, n, nzh), dtype=np.complex128)
    out = []
    # one mode: (ix, iy, iz) = (3, 4, 0): shell 5, weight 1; |m|^2 = 2.125, Re(m conj l) = 0.75 * 2 + (-1.25) * 0.5 = 0.875
    m, l = z(), z()
    m[4, 3, 0] = 0.75 - 1.25j
    l[4, 3, 0] = 2.0 + 0.5j
    out.append(("single_positive", m, l, {5: (2.125, 0.875, 0.0)}))
    l2 = z()
    l2[4, 3, 0] = -2.0 - 0.5j
    out.append(("single_negative", m, l2, {5: (2.125, 0.0, 0.875)}))
    # (1, 2, 2): shell 3, weight 2
    m, l = z(), z()
    m[2, 1, 2] = 1.5 + 0.5j
    l[2, 1, 2] = 0.5 + 2.0j
    out.append(("single_weight_two", m, l, {3: (2 * 2.5, 2 * 1.75, 0.0)}))
    # a shell whose cross terms all cancel: k2 = 1, shell 1, the modes (1, 0, 0) and (15, 0, 0) (weight 1 each) and (0, 1, 0), (0, 15, 0)
    m, l = z(), z()
    for (ix, iy), sgn in (((1, 0), 1.0), ((15, 0), -1.0), ((0, 1), 1.0), ((0, 15), -1.0)):
        m[iy, ix, 0] = 3.0 + 1.0j
        l[iy, ix, 0] = sgn * (0.25 + 0.5j)
    out.append(("cross_cancels", m, l, {1: (4 * 10.0, 2 * 1.25, 2 * 1.25)}))
    return out
