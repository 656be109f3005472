"""numpy restatement of the redshift-space multipoles of the halo power (include/pinfmax.h: pf_halo_multipoles) -- TEST
INFRASTRUCTURE.  It shares no code with the library: the list moved along the line of sight (one product, one sum), then the halo
restatement of tests/np_halo.py; the Legendre weights from int64 integers with one division each; the eleven positive sums of a
shell by math.fsum over the terms as the library rounds them (the terms of tests/np_matter.py times the weight: one product; times
the mode weight w, a power of two: exact)."""
import math

import numpy as np

import np_halo as nph
import np_matter as npm
import np_power as npp

ORDERS, SUMS = 3, 11


def moved(pos, vel, vfac, los):
    """s [count][3]: pos, and on axis los pos + vel * vfac (the product, then the sum); vel None: pos"""
    s = np.array(pos, dtype=np.float64).reshape(-1, 3)
    if vel is not None:
        v = np.asarray(vel, dtype=np.float64).reshape(-1, 3)
        with np.errstate(invalid="ignore", over="ignore"):
            shift = v[:, los] * np.float64(vfac)
            s[:, los] = s[:, los] + shift
    return s


def deposit(n, pos, vel, mass, lo, hi, scale=1.0, vfac=0.0, los=2, mass_weight=False, ngp=False, x0=0, nxl=None):
    return nph.deposit(n, moved(pos, vel, vfac, los), mass, lo, hi, scale, mass_weight, ngp, x0, nxl)


def legendre(n, los, y0=0, nyl=None):
    """L2 and L4 of every mode of the slab, each [nyl][n][n/2+1] float64, and the integers they come from"""
    nyl = n if nyl is None else nyl
    k2, _, _ = npp.geometry(n, y0, nyl)
    sy = npp.signed(np.arange(y0, y0 + nyl), n)[:, None, None]
    sx = npp.signed(np.arange(n), n)[None, :, None]
    sz = np.arange(n // 2 + 1, dtype=np.int64)[None, None, :]
    a = np.broadcast_to((sx, sy, sz)[los] ** 2, k2.shape).astype(np.int64)
    n2, d2 = 3 * a - k2, 2 * k2
    n4, d4 = 35 * a * a - 30 * a * k2 + 3 * k2 * k2, 8 * k2 * k2
    assert max(int(np.abs(n4).max()), int(d4.max())) < 2 ** 50
    zero = k2 == 0
    L2 = np.where(zero, 0.0, n2.astype(np.float64) / np.where(zero, 1, d2).astype(np.float64))
    L4 = np.where(zero, 0.0, n4.astype(np.float64) / np.where(zero, 1, d4).astype(np.float64))
    return L2, L4, (a, k2)


def mode_parts(ta, tc, L2, L4):
    """the eleven non-negative terms of every mode (zeros where it has no part); tc None: the first five"""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        signed_terms = [ta * L2, ta * L4] + ([] if tc is None else [tc, tc * L2, tc * L4])
    out = [ta]
    for x in signed_terms:
        with np.errstate(invalid="ignore"):
            out += [np.where(x > 0, x, 0.0), np.where(x < 0, -x, 0.0)]
    return out


def shells(spec_m, spec_lin=None, y0=0, field_bytes=8, ngp=False, deconvolve=False, los=2):
    """the columns of pf_debug_multipole_shells for this slab: nmodes, k2sum, parts [11][nb], power [3][nb], cross [3][nb] or None"""
    nyl, n = spec_m.shape[:2]
    k2, sh, w = npp.geometry(n, y0, nyl)
    ta, tc = npm.mode_terms(spec_m, spec_lin, y0, field_bytes, ngp, deconvolve)
    fin = np.isfinite(ta) & (np.isfinite(tc) if tc is not None else True)
    L2, L4, _ = legendre(n, los, y0, nyl)
    terms = mode_parts(ta, tc, L2, L4)
    nb = npp.bins(n)
    n6 = float(n ** 6)
    sums = np.zeros((SUMS, nb))
    out = {"nmodes": np.zeros(nb, np.uint64), "k2sum": np.zeros(nb, np.uint64), "modes": nyl * n * n, "nonfinite_modes": int(w[~fin].sum())}
    for b in range(nb):
        m = sh == b
        out["nmodes"][b] = int(w[m].sum())
        out["k2sum"][b] = int((w[m] * k2[m]).sum())
        mf = m & fin
        for i, t in enumerate(terms):
            sums[i, b] = math.fsum((w[mf] * t[mf]).tolist())
    out["parts"] = sums / n6
    out["power"] = np.stack([sums[0], sums[1] - sums[2], sums[3] - sums[4]]) / n6
    out["cross"] = None if tc is None else np.stack([sums[5] - sums[6], sums[7] - sums[8], sums[9] - sums[10]]) / n6
    return out
