"""The four shell restatements (np_power.power, np_matter.shells, np_multipoles.shells, np_corr.shells) at production shell counts --
TEST INFRASTRUCTURE.  It shares no code with the library.  The slow versions walk the shells with a boolean mask of the whole
window, O(nb cells): minutes at nb = 1775.  Here the cells are put in the order of their shells by ONE stable sort, the integer
columns are differences of a running uint64 sum, and math.fsum runs once per (sum, shell) over that shell's slice.  fsum is exact, so
the order of the terms cannot matter: the dictionaries are those of the slow versions bit for bit (tests/test_shells_fast_cpu.py).

Every rule -- signed wavenumbers, shells, weights, terms, Legendre weights, which sum a term enters -- is the slow restatement's own
function, called, not restated: npp.geometry / npp.shell_of / npp.terms, npm.mode_terms, npl.legendre / npl.mode_parts,
npc.geometry / npc.cell_terms / npc.sum_index."""
import math

import numpy as np

import np_corr as npc
import np_matter as npm
import np_multipoles as npl
import np_power as npp


class Groups:
    """the cells of a window in the order of their shells"""

    def __init__(self, sh, nb):
        flat = np.asarray(sh).ravel()
        assert flat.min() >= 0 and flat.max() < nb
        self.nb = nb
        self.order = np.argsort(flat, kind="stable")
        self.bounds = np.searchsorted(flat[self.order], np.arange(nb + 1))
        self.filled = np.nonzero(np.diff(self.bounds))[0].tolist()

    def ints(self, vals):
        """per shell the sum of non-negative integers, in uint64"""
        v = np.asarray(vals)
        assert v.min() >= 0 and float(v.max()) * v.size < 2.0 ** 63          # the running sum cannot wrap
        run = np.concatenate([np.zeros(1, np.uint64), np.cumsum(v.ravel()[self.order].astype(np.uint64), dtype=np.uint64)])
        return run[self.bounds[1:]] - run[self.bounds[:-1]]

    def fsums(self, vals, keep):
        """per shell math.fsum of vals where keep; the others enter as exact zeros"""
        lst = np.where(keep, vals, 0.0).ravel()[self.order].tolist()
        out = np.zeros(self.nb)
        for b in self.filled:
            out[b] = math.fsum(lst[self.bounds[b]:self.bounds[b + 1]])
        return out


def power(spec, y0=0, radii_cells=(), field_bytes=8):
    """np_power.power"""
    nyl, n = spec.shape[0], spec.shape[1]
    assert spec.shape == (nyl, n, n // 2 + 1)
    k2, sh, w = npp.geometry(n, y0, nyl)
    t = npp.terms(spec, field_bytes)
    fin = np.isfinite(t)
    nb = npp.bins(n)
    n6 = float(n ** 6)
    g = Groups(sh, nb)
    with np.errstate(invalid="ignore", over="ignore"):
        wt = w * t
    kf = 2.0 * math.pi / n
    var = np.zeros(len(radii_cells))
    mv = fin & (k2 > 0)
    wv, kk = wt[mv], k2[mv].astype(np.float64)
    for i, r in enumerate(radii_cells):
        a = (kf * kf) * (float(r) * float(r))
        with np.errstate(under="ignore"):
            var[i] = math.fsum((wv * np.exp(-(a * kk))).tolist()) / n6
    return {"nmodes": g.ints(w), "k2sum": g.ints(w * k2), "power": g.fsums(wt, fin) / n6, "variance": var, "modes": nyl * n * n, "nonfinite": int(w[~fin].sum())}


def matter_shells(spec_m, spec_lin=None, y0=0, field_bytes=8, ngp=False, deconvolve=False):
    """np_matter.shells"""
    nyl, n = spec_m.shape[:2]
    assert spec_m.shape == (nyl, n, n // 2 + 1)
    k2, sh, w = npp.geometry(n, y0, nyl)
    ta, tc = npm.mode_terms(spec_m, spec_lin, y0, field_bytes, ngp, deconvolve)
    fin = np.isfinite(ta) & (np.isfinite(tc) if tc is not None else True)
    nb = npp.bins(n)
    n6 = float(n ** 6)
    g = Groups(sh, nb)
    out = {"nmodes": g.ints(w), "k2sum": g.ints(w * k2), "cross": None, "cross_pos": np.zeros(nb), "cross_neg": np.zeros(nb), "modes": nyl * n * n,
           "nonfinite_modes": int(w[~fin].sum())}
    with np.errstate(invalid="ignore", over="ignore"):
        out["power"] = g.fsums(w * ta, fin) / n6
        if tc is not None:
            x = w * tc
            out["cross_pos"] = g.fsums(x, fin & (x > 0)) / n6
            out["cross_neg"] = g.fsums(-x, fin & (x < 0)) / n6
            out["cross"] = out["cross_pos"] - out["cross_neg"]
    return out


def multipole_shells(spec_m, spec_lin=None, y0=0, field_bytes=8, ngp=False, deconvolve=False, los=2):
    """np_multipoles.shells"""
    nyl, n = spec_m.shape[:2]
    k2, sh, w = npp.geometry(n, y0, nyl)
    ta, tc = npm.mode_terms(spec_m, spec_lin, y0, field_bytes, ngp, deconvolve)
    fin = np.isfinite(ta) & (np.isfinite(tc) if tc is not None else True)
    L2, L4, _ = npl.legendre(n, los, y0, nyl)
    terms = npl.mode_parts(ta, tc, L2, L4)
    nb = npp.bins(n)
    n6 = float(n ** 6)
    g = Groups(sh, nb)
    sums = np.zeros((npl.SUMS, nb))
    for i, t in enumerate(terms):
        with np.errstate(invalid="ignore", over="ignore"):
            sums[i] = g.fsums(w * t, fin)
    out = {"nmodes": g.ints(w), "k2sum": g.ints(w * k2), "modes": nyl * n * n, "nonfinite_modes": int(w[~fin].sum())}
    out["parts"] = sums / n6
    out["power"] = np.stack([sums[0], sums[1] - sums[2], sums[3] - sums[4]]) / n6
    out["cross"] = None if tc is None else np.stack([sums[5] - sums[6], sums[7] - sums[8], sums[9] - sums[10]]) / n6
    return out


def corr_shells(real, x0=0, field_bytes=8, los=2):
    """np_corr.shells"""
    nxl, n = real.shape[:2]
    r2, sh, _, _, _ = npc.geometry(n, los, x0, nxl)
    x, fin = npc.cell_terms(real, los, x0, field_bytes)
    which = npc.sum_index(real, los, x0, field_bytes)
    nb = npp.bins(n)
    g = Groups(sh, nb)
    parts = np.zeros((npc.FIELD_SUMS, nb))
    for k in range(npc.ORDERS):
        with np.errstate(invalid="ignore"):
            parts[2 * k] = g.fsums(x[k], which[k] == 2 * k)
            parts[2 * k + 1] = g.fsums(-x[k], which[k] == 2 * k + 1)
    out = {"ncells": g.ints(np.ones(sh.shape, np.int64)), "r2sum": g.ints(r2), "nonfinite_cells": int((~fin).sum()), "parts": parts}
    out["xi"] = parts[0::2] - parts[1::2]
    return out
