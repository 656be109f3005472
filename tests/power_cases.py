"""Planted spectra for the power-spectrum tests -- TEST INFRASTRUCTURE.  Every case is a whole box [ky][kx][kz] complex128 of
n = 16 whose expected columns are known exactly; `expect` names, where it can be said in a line, the one shell that is touched:
(shell, weight, k2, term)."""
import numpy as np

N = 16
NZH = N // 2 + 1

# (ix, iy, iz) -> shell, weight, k2 by the definitions: signed wavenumbers (15 -> -1, 8 stays 8), nearest integer to |k|
SINGLE = {
    (0, 0, 0): (0, 1, 0),
    (0, 0, 1): (1, 2, 1),
    (0, 0, 8): (8, 1, 64),
    (8, 8, 8): (14, 1, 192),      # sqrt(192) = 13.86
    (15, 0, 0): (1, 1, 1),
    (3, 4, 0): (5, 1, 25),
    (1, 2, 2): (3, 2, 9),
    # the edge between shells 3 and 4 is 4 k2 = 49: k2 = 12 (48, one below) and k2 = 13 (52, the first even number above)
    (2, 2, 2): (3, 2, 12),
    (0, 2, 3): (4, 2, 13),
}
VALUE = 0.75 - 1.25j    # |v|^2 = 2.125 exactly


def empty():
    return np.zeros((N, N, NZH), dtype=np.complex128)


def random_box(seed, n=N, scale=1.0):
    rng = np.random.default_rng(seed)
    return scale * (rng.standard_normal((n, n, n // 2 + 1)) + 1j * rng.standard_normal((n, n, n // 2 + 1)))


def cases():
    """-> [(name, spectrum, expect or None)]"""
    out = []
    for (ix, iy, iz), (b, w, k2) in SINGLE.items():
        s = empty()
        s[iy, ix, iz] = VALUE
        out.append(("mode_%d_%d_%d" % (ix, iy, iz), s, (b, w, k2, 2.125)))
    out.append(("all_ones", np.full((N, N, NZH), 1.0 + 1.0j), None))
    s = random_box(5)
    s[3, 7, 2] = complex(np.nan, 1.0)        # weight 2
    s[9, 1, 0] = complex(2.0, np.inf)        # weight 1
    s[0, 0, 8] = complex(-np.inf, np.nan)    # weight 1
    out.append(("nan_and_inf", s, None))
    s = np.full((N, N, NZH), complex(-0.0, -0.0))
    s[5, 5, 5] = complex(-0.0, 3.0)
    out.append(("minus_zero", s, None))
    # subnormal parts and nothing else: doubles whose squares vanish or are themselves subnormal, and values that are subnormal only
    # as floats (their squares are ordinary doubles; with fp32 fields the smallest ones arrive as zeros)
    s = empty()
    s[1, 0, 0] = complex(5e-324, 1e-310)
    s[0, 1, 1] = complex(1.5e-160, -1.2e-161)
    s[2, 3, 4] = complex(1e-40, 3e-42)
    s[15, 15, 7] = complex(-7e-45, 1.4e-45)
    out.append(("subnormal_parts", s, None))
    # one enormous and many tiny terms in different shells: every shell keeps its own precision
    s = random_box(6, scale=1e-12)
    s[0, 1, 0] = 3e15
    out.append(("dynamic_range", s, None))
    out.append(("random", random_box(7), None))
    return out
