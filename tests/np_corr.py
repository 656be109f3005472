"""numpy restatement of the two-point correlation function of the haloes (include/pinfmax.h: pf_halo_correlation) -- TEST
INFRASTRUCTURE.  It shares no code with the library: the form rule on the mode terms of tests/np_matter.py (one division by N^3, one
rounding to the field type, zero at k = 0 and for a term that is not finite); the shell rule of a real field in separation space
(signed separations, the shell of tests/np_power.py with r2 for k2, the Legendre weights from int64 integers with one division each,
the six positive sums of a shell by math.fsum over the terms as the library rounds them); and the whole call through numpy.fft on
the deposit and the contrast of tests/np_halo.py / tests/np_multipoles.py."""
import math

import numpy as np

import np_halo as nph
import np_matter as npm
import np_multipoles as npl
import np_power as npp

ORDERS, SUMS, FIELD_SUMS = 3, 12, 6


def form(spec_m, spec_lin=None, y0=0, field_bytes=8, ngp=False, deconvolve=False, which=0):
    """the formed slab [nyl][n][n/2+1] float64 (the real parts; the imaginary parts are zero) and the weight of the modes whose term
    is not finite"""
    nyl, n = spec_m.shape[:2]
    ta, tc = npm.mode_terms(spec_m, spec_lin if which else None, y0, field_bytes, ngp, deconvolve)
    t = tc if which else ta
    k2, _, w = npp.geometry(n, y0, nyl)
    bad = ~np.isfinite(t)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        q = np.where(bad | (k2 == 0), 0.0, np.where(bad, 0.0, t) / np.float64(float(n) * float(n) * float(n)))
        if field_bytes == 4:
            q = q.astype(np.float32).astype(np.float64)
    return q, int(w[bad].sum())


def geometry(n, los, x0=0, nxl=None):
    """r2, shell, L2 and L4 of every cell of the planes [x0, x0 + nxl), each [nxl][n][n], and a = s_los^2"""
    nxl = n - x0 if nxl is None else nxl
    sx = npp.signed(np.arange(x0, x0 + nxl), n)[:, None, None]
    sy = npp.signed(np.arange(n), n)[None, :, None]
    sz = npp.signed(np.arange(n), n)[None, None, :]
    r2 = sx * sx + sy * sy + sz * sz
    a = np.broadcast_to((sx, sy, sz)[los] ** 2, r2.shape).astype(np.int64)
    n2, d2 = 3 * a - r2, 2 * r2
    n4, d4 = 35 * a * a - 30 * a * r2 + 3 * r2 * r2, 8 * r2 * r2
    assert max(int(np.abs(n4).max()), int(d4.max())) < 2 ** 50
    zero = r2 == 0
    L2 = np.where(zero, 0.0, n2.astype(np.float64) / np.where(zero, 1, d2).astype(np.float64))
    L4 = np.where(zero, 0.0, n4.astype(np.float64) / np.where(zero, 1, d4).astype(np.float64))
    return r2, npp.shell_of(r2), L2, L4, a


def as_field(real, field_bytes):
    real = np.ascontiguousarray(real, dtype=np.float64)
    if field_bytes == 8:
        return real
    with np.errstate(over="ignore", invalid="ignore"):
        return real.astype(np.float32).astype(np.float64)


def cell_terms(real, los, x0=0, field_bytes=8):
    """the three signed terms of every cell, v, v L2, v L4 (one product each), and which cells are finite"""
    nxl, n = real.shape[:2]
    _, _, L2, L4, _ = geometry(n, los, x0, nxl)
    v = as_field(real, field_bytes)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return [v, v * L2, v * L4], np.isfinite(v)


def sum_index(real, los, x0=0, field_bytes=8):
    """[3][nxl][n][n]: the sum (0 .. 5) that term k of a cell enters, -1 for none (a term of zero, a value that is not finite)"""
    x, fin = cell_terms(real, los, x0, field_bytes)
    out = np.full((ORDERS,) + real.shape, -1, np.int32)
    for k in range(ORDERS):
        with np.errstate(invalid="ignore"):
            out[k] = np.where(fin & (x[k] > 0), 2 * k, np.where(fin & (x[k] < 0), 2 * k + 1, -1))
    return out


def shells(real, x0=0, field_bytes=8, los=2):
    """the columns of pf_debug_corr_shells for the planes [x0, x0 + nxl) of a real field [nxl][n][n]"""
    nxl, n = real.shape[:2]
    r2, sh, _, _, _ = geometry(n, los, x0, nxl)
    x, fin = cell_terms(real, los, x0, field_bytes)
    nb = npp.bins(n)
    parts = np.zeros((FIELD_SUMS, nb))
    out = {"ncells": np.zeros(nb, np.uint64), "r2sum": np.zeros(nb, np.uint64), "nonfinite_cells": int((~fin).sum())}
    for b in range(nb):
        m = sh == b
        out["ncells"][b] = int(m.sum())
        out["r2sum"][b] = int(r2[m].sum())
        mf = m & fin
        for k in range(ORDERS):
            t = x[k][mf]
            parts[2 * k, b] = math.fsum(t[t > 0].tolist())
            parts[2 * k + 1, b] = math.fsum((-t[t < 0]).tolist())
    out["parts"] = parts
    out["xi"] = parts[0::2] - parts[1::2]
    return out


def add(parts):
    """the box's columns from those of its x-windows: integers exactly, the positive sums in window order"""
    out = {"nonfinite_cells": sum(p["nonfinite_cells"] for p in parts)}
    for k in ("ncells", "r2sum"):
        out[k] = np.sum([p[k] for p in parts], axis=0, dtype=np.uint64)
    out["parts"] = np.sum([p["parts"] for p in parts], axis=0)
    return out


def field_of(spec_x_slab, n):
    """a formed half-spectrum [kx][ky][kz] -> the real field [n][n][n] with numpy's 1 / N^3"""
    return np.fft.irfftn(spec_x_slab, s=(n, n, n), axes=(0, 1, 2))


def correlation(n, pos, vel, mass, ranges, scale=1.0, vfac=0.0, los=2, mass_weight=False, ngp=False, deconvolve=False, lin=None, field_bytes=8):
    """the whole call through numpy.fft: per bin xi [3][nb] and xi_cross [3][nb] (None without lin, the resident spectrum as an
    x-slab [kx][ky][n/2+1]) with their positive sums, and ncells, r2sum; a bin without haloes gives zeros"""
    nb = npp.bins(n)
    out = {"xi": np.zeros((len(ranges), ORDERS, nb)), "xi_cross": None if lin is None else np.zeros((len(ranges), ORDERS, nb)),
           "parts": np.zeros((len(ranges), SUMS, nb)), "info": []}
    lin_slab = None if lin is None else npp.from_x_slab(lin)
    geo = shells(np.zeros((n, n, n)), 0, 8, los)
    out["ncells"], out["r2sum"] = geo["ncells"], geo["r2sum"]
    for b, (lo, hi) in enumerate(ranges):
        grid, info = npl.deposit(n, pos, vel, mass, int(lo), int(hi), scale, vfac, los, mass_weight, ngp)
        out["info"].append(info)
        if grid is None or not info["weight_sum"]:
            continue
        delta = nph.contrast(grid, info["weight_sum"], n, field_bytes)
        spec = npp.from_x_slab(np.fft.rfftn(delta, axes=(0, 1, 2)))
        for which, key in ((0, "xi"), (1, "xi_cross")):
            if which and lin is None:
                continue
            q, _ = form(spec, lin_slab, 0, field_bytes, ngp, deconvolve, which)
            s = shells(field_of(np.transpose(q, (1, 0, 2)).astype(np.complex128), n), 0, field_bytes, los)
            out[key][b] = s["xi"]
            out["parts"][b, 6 * which:6 * which + 6] = s["parts"]
    return out
