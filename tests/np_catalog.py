"""The output step of build_groups() restated in numpy, vectorised over groups: one record of write_catalog()
(src/write_halos.c:285-317) and the histograms of compute_mf() (:56-65).  Built on tests/np_plc.py, which has set_obj, set_weight,
q2x and the growth interpolation; added here are q2x's periodic wrap (src/build_groups.c:1595-1600), the shift to the global box
with its two wraps and the conversion to Mpc (write_halos.c:300-313), and vel (:1607-1643) with set_obj_vel's factors (:1446-1460),
formed as np_plc.store_at forms them.  np.float32 / np.float64 stand where the reference has PRODFLOAT / double: a product of two
PRODFLOATs is rounded to PRODFLOAT, anything with a double operand is a double, an assignment to a PRODFLOAT rounds."""
import numpy as np

import np_plc as npp

f64 = np.float64
D = lambda a: np.asarray(a).astype(f64)


class Box:
    """what write_catalog reads beside the groups: subbox.stabl, subbox.Lgwbl, subbox.pbc, GSglobal, InterPartDist, ParticleMass, hfactor"""

    def __init__(self, stabl, lgwbl, pbc, gs, ipd, pmass, hfactor):
        self.stabl, self.lgwbl, self.pbc, self.gs = np.asarray(stabl, f64), np.asarray(lgwbl, f64), [bool(p) for p in pbc], np.asarray(gs, f64)
        self.ipd, self.pmass, self.hfactor = f64(ipd), f64(pmass), f64(hfactor)


def passing(M, good, point, min_mass):
    """write_halos.c:286-287; good / point None: absent, passes"""
    ok = np.asarray(M) >= min_mass
    if good is not None:
        ok &= np.asarray(good) != 0
    if point is not None:
        ok &= np.asarray(point) >= 0
    return ok


def to_global(a, j, box, T):
    """sub-box cells -> the global box in Mpc (write_halos.c:300-305, :308-313), wrapped[0] / [1]: where the two wraps fired"""
    G = box.gs[j]
    q = (D(a) + box.stabl[j]).astype(T)
    neg = q < 0
    q = np.where(neg, (D(q) + G).astype(T), q)
    big = q >= G
    q = np.where(big, (D(q) - G).astype(T), q)
    return (D(q) * (box.ipd * box.hfactor)).astype(T), neg, big


def vel(cos, seg, G, K, w, F, ipd):
    """vel (:1607-1643) of the three axes with set_obj_vel's factors at z = F - 1 -> (v [N][3] PRODFLOAT, vscale [N]: the sum of the
    magnitudes of v's terms)"""
    T = G.T
    z = D(F) - 1.0
    fac = (cos.hubble(z) / (1. + z) * ipd).astype(T)
    Dv = [(D(fac) * cos.growth(4 + f, K, z)).astype(T)[:, None] for f in range(4)]
    W = [a[:, None] for a in w]
    v = G.vel
    if not seg.myseg:
        t = [((v[o] * Dv[o]).astype(T) * W[o]).astype(T) for o in range(4)]
        vv = t[0]
        if seg.order > 1:
            vv = (vv + t[1]).astype(T)
        if seg.order > 2:
            vv = (vv + (t[2] + t[3]).astype(T)).astype(T)
        terms = t
    else:
        t = [(D(v[4 + o]) * (1. - D(W[o])) + D((v[o] * W[o]).astype(T))) * D(Dv[o]) for o in range(4)]
        vv = t[0].astype(T)
        if seg.order > 1:
            vv = (D(vv) + t[1]).astype(T)
        if seg.order > 2:
            vv = (D(vv) + (t[2] + t[3])).astype(T)
        terms = [np.abs(D(v[4 + o]) * (1. - D(W[o])) * D(Dv[o])) + np.abs(D(v[o]) * D(W[o]) * D(Dv[o])) for o in range(4)]
    nterm = {1: 1, 2: 2}.get(seg.order, 4)
    vscale = sum(np.abs(D(a)).max(axis=1) for a in terms[:nterm]) if G.M.size else np.zeros(0)
    return vv, vscale


def records(cos, seg, G, F, box):
    """the records of the groups G (all of them: the caller filters) at F -> dict M [N], x, v, q [N][3] PRODFLOAT, vscale [N], and
    which of the wraps fired: pbc_hi, pbc_lo, xneg, xbig, qneg, qbig [N][3]"""
    T = G.T
    N = G.M.size
    Fa = np.full(N, T(F), T)
    K = cos.group_k(G.M, box.ipd, T)
    w = npp.weights(cos, seg, K, Fa, T)
    pos = npp.q2x(G, w, seg)
    out = {k: np.zeros((N, 3), bool) for k in ("pbc_hi", "pbc_lo", "xneg", "xbig", "qneg", "qbig")}
    x, q = np.zeros((N, 3), T), np.zeros((N, 3), T)
    for j in range(3):
        p = pos[:, j]
        if box.pbc[j]:
            hi = p >= box.lgwbl[j]
            p = np.where(hi, (D(p) - box.lgwbl[j]).astype(T), p)
            lo = p < 0.0
            p = np.where(lo, (D(p) + box.lgwbl[j]).astype(T), p)
            out["pbc_hi"][:, j], out["pbc_lo"][:, j] = hi, lo
        x[:, j], out["xneg"][:, j], out["xbig"][:, j] = to_global(p, j, box, T)
        q[:, j], out["qneg"][:, j], out["qbig"][:, j] = to_global(G.q[:, j], j, box, T)
    v, vscale = vel(cos, seg, G, K, w, Fa, box.ipd)
    out.update(M=(D(G.M) * box.pmass * box.hfactor).astype(T), x=x, v=v, q=q, vscale=vscale)
    return out


def bin_quotient(M, pmass, mmin, deltam):
    """(log10(Mass * ParticleMass) - mmin) / DELTAM of write_halos.c:59-60, before the cast"""
    return (np.log10(D(M) * f64(pmass)) - f64(mmin)) / f64(deltam)


def mass_function(M, pmass, nbin, mmin, deltam):
    """compute_mf's two local arrays of the (passing) masses M in their order -> (ninbin int32, massinbin: the reference's running sum
    of doubles, sum_mass: the integer sum of Mass per bin).  Masses below 1 are left out."""
    M = np.asarray(M, np.int64)
    M = M[M >= 1]
    nin, run, tot = np.zeros(nbin, np.int32), np.zeros(nbin, f64), [0] * nbin
    if M.size and nbin:
        b = bin_quotient(M, pmass, mmin, deltam).astype(int)   # (the cast truncates toward zero, as C's does)
        for m, k in zip(M.tolist(), b.tolist()):
            if 0 <= k < nbin:
                nin[k] += 1
                run[k] += f64(m) * f64(pmass)
                tot[k] += m
    return nin, run, tot
