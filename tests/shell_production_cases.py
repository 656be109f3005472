"""What the tests of the shell passes at production shell counts plant (tests/test_shells_fast_cpu.py,
tests/test_gpu_shells_production.py) -- TEST INFRASTRUCTURE.  A case is one thin window of a grid of 512 to 2048: its shell count,
LDS tables, grouping of the sums, column groups and strides are those of the full box, at one or two planes' worth of cells.

  plane 0        holds the k = 0 mode (the r = 0 cell) and the shells 0 .. n / sqrt 2
  plane n/2      the signed index stays +n/2; reaches the top shell nb - 1
  plane n - 1    signed -1 (512 and 1024)
  n/2 - 1 .. n/2 + 1   three planes across the change of sign (512)
Fields and spectra follow corr_cases.random_field and multipole_cases.random_spectra: both signs, amplitudes over 2^-30 .. 2^30 cell
by cell, so that shells hold terms 36 decades apart and the per-shell exponent of the fixed point decides what survives; exact zeros;
one value per window that is not finite."""
import numpy as np

GRIDS = (512, 1024, 1536, 2048)
RAGGED = 136                                   # a full box of 136: 18496 rows over 8192 workgroups -> 3 rows each and a last one of 1
RADII13 = tuple(np.linspace(0.0, 2.0, 13))     # more than one batch of twelve
RADII3 = (RADII13[12], RADII13[6], RADII13[0])
FLAGS = ((False, False), (False, True), (True, True))     # (ngp, deconvolve), as the small-grid tests


def windows(n):
    """(first plane, planes)"""
    out = [(0, 1), (n // 2, 1)]
    if n <= 1024:
        out.append((n - 1, 1))
    if n == 512:
        out.append((n // 2 - 1, 3))
    return out


def cases():
    """(n, first plane, planes, field bytes, lines of sight): fp64 everywhere, fp32 on plane 0; all three lines of sight at 512, one
    per window elsewhere, rotated, the fp32 case taking the next -- so that each of the three occurs at every grid"""
    out = []
    for g, n in enumerate(GRIDS):
        w = windows(n)
        for k, (p0, np_) in enumerate(w):
            out.append((n, p0, np_, 8, (0, 1, 2) if n == 512 else ((g + k) % 3,)))
        out.append((n, 0, 1, 4, ((g + len(w)) % 3,)))
    return out


def case_id(c):
    return "n%d_p%d+%d_fp%d" % (c[0], c[1], c[2], 8 * c[3])


def seed_of(n, p0, planes):
    return 1000 * n + 10 * p0 + planes


def spectra(n, y0, nyl, seed=None):
    """two ky-slabs [nyl][n][n/2+1]; the first has one mode that is not finite, of weight 2"""
    rng = np.random.default_rng(seed_of(n, y0, nyl) if seed is None else seed)
    shape = (nyl, n, n // 2 + 1)
    a = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.exp2(rng.integers(-30, 31, shape).astype(np.float64))
    b = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.exp2(rng.integers(-30, 31, shape).astype(np.float64))
    a[rng.integers(0, nyl, 7), rng.integers(0, n, 7), rng.integers(0, n // 2 + 1, 7)] = 0.0
    a[nyl - 1, 5, 7] = complex(np.nan, 1.0) if (y0 + n) % 3 else complex(2.0, -np.inf)
    with np.errstate(invalid="ignore"):
        return a, 0.6 * a + b


def field(n, x0, nxl, seed=None):
    """planes [nxl][n][n] of a real field; one cell is not finite"""
    rng = np.random.default_rng(seed_of(n, x0, nxl) + 1 if seed is None else seed)
    shape = (nxl, n, n)
    f = rng.standard_normal(shape) * np.exp2(rng.integers(-30, 31, shape).astype(np.float64))
    f[rng.integers(0, nxl, 7), rng.integers(0, n, 7), rng.integers(0, n, 7)] = 0.0
    f[nxl - 1, 3, n - 2] = np.inf if (x0 + n) % 3 else np.nan
    return f
