"""What the bispectrum tests plant (tests/test_bispec_cpu.py, tests/test_abi_bispec.py, tests/test_gpu_bispec.py): the k-bin cases,
Gaussian fields for the enumeration, real fields and planted cosines for the triple pass."""
import numpy as np

# (n, kmin, dk, nk): 3 (kmin + nk dk) <= n in every one
CASES = [(16, 1, 1, 4),      # kmax 5; of the 20 ordered triples some are open, (0, 0, 3) among them
         (16, 1, 2, 2),
         (24, 1, 2, 3),      # kmax 7; 10 closed triples
         (36, 2, 3, 3),      # kmax 11; the general transform path, fp64 fields only
         (48, 2, 4, 3)]      # kmax 14
SMALL = CASES[:3]            # what the direct enumeration of all pairs of modes takes in seconds
BY_N = {16: (1, 1, 4), 24: (1, 2, 3), 36: (2, 3, 3), 48: (2, 4, 3), 32: (1, 3, 3), 64: (2, 4, 3)}
ALIASED = (16, 1, 2, 3)      # kmax 7, 3 kmax = 21 > 16: what the call refuses


def gaussian_field(n, seed):
    return np.random.default_rng(seed).standard_normal((n, n, n))


def random_fields(nk, nxl, n, seed, spread=6):
    """both signs, a dynamic range of 2^(2 spread) per field and another between the fields, a handful of exact zeros"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((nk, nxl, n, n)) * np.exp2(rng.integers(-spread, spread + 1, (nk, nxl, n, n)).astype(np.float64))
    f *= np.exp2(3.0 * np.arange(nk))[:, None, None, None]
    f[rng.integers(0, nk, 9), rng.integers(0, nxl, 9), rng.integers(0, n, 9), rng.integers(0, n, 9)] = 0.0
    return f


def x_windows(n):
    """windows of planes that split the box, each list covering it once"""
    return [[(0, n)], [(0, n // 2), (n // 2, n // 2)], [(0, 3), (3, n - 4), (n - 1, 1)]]


def cosines(n, k1, k2, k3, A, B, Cc, phi):
    """A cos(k1.x) + B cos(k2.x) + C cos(k3.x + phi) on the grid, k in units of the fundamental"""
    x = np.arange(n)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    ph = lambda k: (2.0 * np.pi / n) * (k[0] * X + k[1] * Y + k[2] * Z)
    return A * np.cos(ph(k1)) + B * np.cos(ph(k2)) + Cc * np.cos(ph(k3) + phi)


def planted_triangle(n, kmin, dk, nk):
    """three wavevectors with k1 + k2 + k3 = 0 in three different bins of the case (nk >= 3), or None"""
    import np_bispec as npb
    r = range(-(kmin + nk * dk), kmin + nk * dk + 1)
    ks = [(a, b, c) for a in r for b in r for c in r]
    bins = npb.bin_of(np.array([a * a + b * b + c * c for a, b, c in ks]), kmin, dk, nk)
    by = {i: [k for k, b in zip(ks, bins) if b == i] for i in range(nk)}
    sets = {i: set(by[i]) for i in range(nk)}
    for i, j, l in npb.triangles(kmin, dk, nk):
        if i < j < l:
            for k1 in by[i][:40]:
                for k2 in by[j]:
                    k3 = tuple(-(p + q) for p, q in zip(k1, k2))
                    if k3 in sets[l]:
                        return (i, j, l), k1, k2, k3
    return None
