"""numpy restatement of the matter-power call (include/pinfmax.h: pf_matter_power) -- TEST INFRASTRUCTURE.  It shares no code with
the library: positions as the reference's initialize_POS forms them (src/write_snapshot.c:907-954), cloud-in-cell weights as integers,
the grid by np.add.at on uint64, the shell sums as math.fsum over the terms of a shell (shells and weights from tests/np_power.py).

Columns are [12][nxl][n][n] of the PRODFLOAT type (float32 or float64), column 3 o + j = axis j of order o (0 Zel'dovich, 1 2LPT,
2 3LPT(a), 3 3LPT(b)); a spectrum is a ky-slab [nyl][n (kx)][n/2+1] complex128 as in np_power."""
import math

import numpy as np

import np_power as npp

ONE = 1 << 48


def positions(vel12, weight=None, x0=0):
    """pos[3] of every particle, each [nxl][n][n] of the columns' type"""
    T = vel12.dtype.type
    nxl, n = vel12.shape[1], vel12.shape[2]
    q = np.meshgrid(np.arange(x0, x0 + nxl), np.arange(n), np.arange(n), indexing="ij")
    pos = []
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(3):
            v = [vel12[3 * o + j] for o in range(4)]
            if weight is not None:
                v = [(np.float64(weight[o]) * v[o].astype(np.float64)).astype(T) for o in range(4)]
            p = (q[j].astype(np.float64) + 0.5 + v[0].astype(np.float64)).astype(T)
            p = p + v[1]
            p = p + (v[2] + v[3])
            p = np.where(p >= T(n), p - T(n), p)
            p = np.where(p < T(0), p + T(n), p)
            assert p.dtype == vel12.dtype
            pos.append(p)
    return pos


def classes(pos, n):
    """0 deposited, 1 not finite, 2 outside [0, n]"""
    T = pos[0].dtype.type
    bad = ~(np.isfinite(pos[0]) & np.isfinite(pos[1]) & np.isfinite(pos[2]))
    with np.errstate(invalid="ignore"):
        inside = np.ones(pos[0].shape, dtype=bool)
        for p in pos:
            inside &= (p >= T(0)) & (p <= T(n))
    return np.where(bad, 1, np.where(inside, 0, 2))


def cic_axis(p, n):
    """cells [2] and integer weights [2] of positions in [0, n]"""
    T = p.dtype.type
    u = p - T(0.5)
    f = np.floor(u)
    d = u - f
    t = np.floor(d * T(65536)).astype(np.int64)
    i0 = f.astype(np.int64)
    assert np.all((i0 >= -1) & (i0 <= n - 1)) and np.all((t >= 0) & (t <= 65536))
    return (np.mod(i0, n), np.mod(i0 + 1, n)), (65536 - t, t)


def deposit(vel12, weight=None, ngp=False, x0=0):
    """-> (grid [nxl][n][n] uint64, info dict); one rank: x0 = 0 and nxl = n"""
    nxl, n = vel12.shape[1], vel12.shape[2]
    assert nxl == n and x0 == 0
    pos = positions(vel12, weight, x0)
    cls = classes(pos, n)
    ok = cls == 0
    grid = np.zeros(n * n * n, dtype=np.uint64)
    p = [a[ok] for a in pos]
    if ngp:
        c = [np.mod(np.floor(a).astype(np.int64), n) for a in p]
        np.add.at(grid, (c[0] * n + c[1]) * n + c[2], np.uint64(ONE))
    else:
        ax = [cic_axis(a, n) for a in p]
        for a in range(2):
            for b in range(2):
                for c in range(2):
                    w = (ax[0][1][a] * ax[1][1][b] * ax[2][1][c]).astype(np.uint64)
                    np.add.at(grid, (ax[0][0][a] * n + ax[1][0][b]) * n + ax[2][0][c], w)
    g = grid.reshape(n, n, n)
    total = sum(int(v) for v in g.ravel().tolist())
    info = {"deposited": int(ok.sum()), "nonfinite": int((cls == 1).sum()), "outside": int((cls == 2).sum()), "empty_cells": int((g == 0).sum()),
            "max_cell": int(g.max()), "sum_hi32": int((g >> np.uint64(32)).sum(dtype=np.uint64)), "sum_lo32": int((g & np.uint64(0xffffffff)).sum(dtype=np.uint64))}
    assert total == info["deposited"] * ONE == info["sum_hi32"] * (1 << 32) + info["sum_lo32"]
    return g, info


def contrast(grid, field_bytes=8):
    """delta = cell / 2^48 - 1 in double, rounded to the field type, widened back"""
    d = np.ldexp(grid.astype(np.float64), -48) - 1.0
    return d if field_bytes == 8 else d.astype(np.float32).astype(np.float64)


def deconv_table(n, ngp=False):
    j = np.arange(n // 2 + 1)
    x = math.pi * j[1:].astype(np.float64) / float(n)
    s = np.sin(x) / x
    return np.concatenate([[1.0], 1.0 / s if ngp else 1.0 / (s * s)])


def mode_terms(spec_m, spec_lin=None, y0=0, field_bytes=8, ngp=False, deconvolve=False):
    """auto and cross term of every mode of the slab (cross None without spec_lin), as the library forms them: the parts widened to
    double, two products and a sum, then the deconvolution factor (c[|kx|] c[|ky|]) c[kz], squared for auto"""
    nyl, n = spec_m.shape[:2]
    a, b = npp.as_field(spec_m, field_bytes)
    c = None
    if deconvolve:
        tab = deconv_table(n, ngp)
        ay = np.abs(npp.signed(np.arange(y0, y0 + nyl), n))[:, None, None]
        ax = np.abs(npp.signed(np.arange(n), n))[None, :, None]
        c = (tab[ax] * tab[ay]) * tab[np.arange(n // 2 + 1)][None, None, :]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        ta = a * a + b * b
        if c is not None:
            ta = ta * (c * c)
        tc = None
        if spec_lin is not None:
            p, q = npp.as_field(spec_lin, field_bytes)
            tc = a * p + b * q
            if c is not None:
                tc = tc * c
    return ta, tc


def shells(spec_m, spec_lin=None, y0=0, field_bytes=8, ngp=False, deconvolve=False):
    """the columns of pf_debug_matter_shells for this slab, and the two parts of cross (cross_pos, cross_neg: positive sums / N^6)"""
    nyl, n = spec_m.shape[:2]
    assert spec_m.shape == (nyl, n, n // 2 + 1)
    k2, sh, w = npp.geometry(n, y0, nyl)
    ta, tc = mode_terms(spec_m, spec_lin, y0, field_bytes, ngp, deconvolve)
    fin = np.isfinite(ta) & (np.isfinite(tc) if tc is not None else True)
    nb = npp.bins(n)
    n6 = float(n ** 6)
    out = {"nmodes": np.zeros(nb, np.uint64), "k2sum": np.zeros(nb, np.uint64), "power": np.zeros(nb), "cross": None, "cross_pos": np.zeros(nb),
           "cross_neg": np.zeros(nb), "modes": nyl * n * n, "nonfinite_modes": int(w[~fin].sum())}
    for b in range(nb):
        m = sh == b
        out["nmodes"][b] = int(w[m].sum())
        out["k2sum"][b] = int((w[m] * k2[m]).sum())
        mf = m & fin
        out["power"][b] = math.fsum((w[mf] * ta[mf]).tolist()) / n6
        if tc is not None:
            x = w[mf] * tc[mf]
            out["cross_pos"][b] = math.fsum(x[x > 0].tolist()) / n6
            out["cross_neg"][b] = math.fsum((-x[x < 0]).tolist()) / n6
    if tc is not None:
        out["cross"] = out["cross_pos"] - out["cross_neg"]
    return out


def cross_masks(spec_m, spec_lin, y0=0, field_bytes=8, ngp=False, deconvolve=False):
    """spec_lin with every mode removed whose cross term is not positive, and with every mode removed whose term is not negative:
    fed to the library in place of spec_lin, its `cross` is +cross_pos and -cross_neg -- the two parts on their own"""
    _, tc = mode_terms(spec_m, spec_lin, y0, field_bytes, ngp, deconvolve)
    with np.errstate(invalid="ignore"):
        return np.where(tc > 0, spec_lin, 0.0), np.where(tc < 0, spec_lin, 0.0)
