"""What the correlation tests plant (tests/test_corr_cpu.py, tests/test_gpu_corr.py): real fields for the separation-space shell
pass, spectra for the form pass, and the small catalogues of the closed forms.  Every planted number is exact in binary."""
import numpy as np

ONE = (1, 2 ** 31 - 1)
BINS = ((10, 60), (61, 600), (10, 5000))      # two disjoint ranges and one that takes all of halo_cases.random_list


def one_cell(n, cell, value=3.0):
    f = np.zeros((n, n, n))
    f[cell] = value
    return f


def on_los(n, los, d, value=3.0):
    """a single cell d steps along axis los from the origin: mu = 1, so L2 = L4 = 1"""
    cell = [0, 0, 0]
    cell[los] = d % n
    return one_cell(n, tuple(cell), value)


def across_los(n, los, d, value=3.0):
    """a single cell d steps along the axis after los: mu = 0, so L2 = -1/2 and L4 = 3/8"""
    cell = [0, 0, 0]
    cell[(los + 1) % 3] = d % n
    return one_cell(n, tuple(cell), value)


def random_field(n, seed, spread=6):
    """both signs, a dynamic range of 2^(2 spread), a handful of exact zeros"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((n, n, n)) * np.exp2(rng.integers(-spread, spread + 1, (n, n, n)).astype(np.float64))
    f[rng.integers(0, n, 7), rng.integers(0, n, 7), rng.integers(0, n, 7)] = 0.0
    return f


def x_windows(n):
    """windows of planes that split the box, each list covering it once"""
    return [[(0, n)], [(0, n // 2), (n // 2, n // 2)], [(0, 3), (3, n - 4), (n - 1, 1)]]


def random_spectra(n, seed):
    rng = np.random.default_rng(seed)
    shape = (n, n, n // 2 + 1)
    a = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.exp2(rng.integers(-8, 9, shape).astype(np.float64))
    b = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.exp2(rng.integers(-8, 9, shape).astype(np.float64))
    return a, b


def planted_spectra(n):
    """one mode each at the corners of the layout [ky][kx][kz], the k = 0 mode among them, with a cross term of either sign"""
    a = np.zeros((n, n, n // 2 + 1), np.complex128)
    b = np.zeros_like(a)
    for i, (ky, kx, kz) in enumerate(((0, 0, 0), (0, 0, n // 2), (n - 1, 0, 0), (0, n - 1, 1), (n // 2, n // 2, n // 2), (3, 5, 2))):
        a[ky, kx, kz] = (3.0 + i) - 4.0j
        b[ky, kx, kz] = (-1.0) ** i * (1.0 + 0.5j)
    return a, b


def one_halo(n):
    return np.array([[2.5, 5.5, 7.5]]), np.array([100], np.int32)


def pair(n, los, d, along):
    """two haloes at cell centres, d cells apart along los, or along the axis after it"""
    p = np.array([[2.5, 5.5, 7.5], [2.5, 5.5, 7.5]])
    p[1, los if along else (los + 1) % 3] += d
    return p, np.array([100, 100], np.int32)
