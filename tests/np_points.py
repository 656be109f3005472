"""The state of a stored particle at its own collapse time restated in numpy, vectorised over particles, from the lines of the
reference that condition_for_accretion() (src/build_groups.c:1286-1317) runs for the particle the loop works on:
  * virial() (:1023-1051): sigmaD = sqrt(TrueVariance[S]) * GrowingMode(F - 1, k) assigned to a PRODFLOAT, k = Smoothing.k_GM_dens[S]
    in a scale-dependent build and params.k_for_GM otherwise (:1040-1045);
  * set_point() (:1464-1520): z = F - 1, myk = Smoothing.k_GM_displ[S] or params.k_for_GM (:1470-1475), q = the sub-box coordinate
    + SHIFT (:1480-1482, SHIFT = 0.5: src/pinocchio.h:73), the velocities of frag[ind];
  * set_weight() (:1411-1444): w, w2, w31, w32 -- growing mode at z over the one at the segment's end with myseg == 0 (:1418-1423),
    the linear weight between the two ends of the segment otherwise (:1430-1439) -- each assigned to a PRODFLOAT;
  * q2x() (:1554-1603) of the three axes at `order`, with line :1588 as written unless use_v31, and its periodic wraps (:1595-1600:
    `>= Box` first, then `< 0`);
  * InterpolateGrowth (src/cosmo.c:1737-1749) for a given k: below kmin the first k-bin alone, above kmax the last alone, the two
    around log10 k otherwise; GrowingMode_3LPT_1 carries a minus sign (cosmo.c:1810).
np.float32 / np.float64 stand where the reference has PRODFLOAT / double: a product of two PRODFLOATs is a PRODFLOAT, `1. - w` is a
double, an assignment to a PRODFLOAT rounds.  Which particles there are and where their cells lie is np_refresh.cells.  The spline
tables are np_plc.Cosmology.  Shares no code with pinocchio_amd."""
import numpy as np

import np_refresh as npr

f64 = np.float64
SHIFT = 0.5


def k_branch(cos, k, shape):
    """InterpolateGrowth's branch for the k value `k` -> (myk, kk, dk, both) as np_plc.Cosmology.growth takes them, broadcast to shape"""
    z = np.zeros(shape)
    if cos.nk == 1:
        return np.full(shape, f64(k)), z.astype(int), z, z.astype(bool)
    k = f64(k)
    if k < cos.kmin:
        kk, dk, both = 0, 0.0, False
    elif k > cos.kmax:
        kk, dk, both = cos.nk - 1, 0.0, False
    else:
        dk = (np.log10(k) - cos.logkmin) / cos.dlogk
        kk = min(int(dk), cos.nk - 2)      # (k == kmax exactly: the reference reads bin nk with weight zero)
        dk, both = dk - kk, True
    return np.full(shape, k), np.full(shape, kk, int), np.full(shape, dk), np.full(shape, both, bool)


def weights(cos, myseg, z_seg, z_prev, k_point, F, T, nfam=4):
    """set_weight at z = F - 1 -> w [4][N] PRODFLOAT; the families from nfam on (LPT orders that are not computed) are zero"""
    F = np.asarray(F, T)
    z = F.astype(f64) - 1.0
    K = k_branch(cos, k_point, z.shape)
    w = []
    for o in range(4):
        if o >= nfam:
            w.append(np.zeros(z.shape, T))
            continue
        g, gs = cos.mode(o, K, z), cos.mode(o, K, np.full(z.shape, f64(z_seg)))
        if myseg:
            gp = cos.mode(o, K, np.full(z.shape, f64(z_prev)))
            w.append(((g - gp) / (gs - gp)).astype(T))
        else:
            w.append((g / gs).astype(T))
    return w


def sigma_d(cos, sigma0, k_sigma, F, T):
    F = np.asarray(F, T)
    z = F.astype(f64) - 1.0
    return (f64(sigma0) * cos.mode(0, k_branch(cos, k_sigma, z.shape), z)).astype(T)


def q2x(q, v, w, myseg, order, use_v31, pbc, box, T):
    """q [N][3], v [8][N][3] (v, v2, v31, v32 and their _prev twins), w [4][N] -> (x [N][3] PRODFLOAT, hi [N][3], lo [N][3]: which
    wrap fired)"""
    q, v = np.asarray(q, T), np.asarray(v, T)
    W = [a[:, None] for a in w]
    D = lambda a: a.astype(f64)
    if not myseg:
        pos = (q + (W[0] * v[0]).astype(T)).astype(T)
        if order > 1:
            pos = (pos + (W[1] * v[1]).astype(T)).astype(T)
        if order > 2:
            pos = (pos + ((W[2] * v[2]).astype(T) + (W[3] * v[3]).astype(T)).astype(T)).astype(T)
    else:
        pos = ((D(q) + (1. - D(W[0])) * D(v[4])) + D((W[0] * v[0]).astype(T))).astype(T)
        if order > 1:
            pos = (D(pos) + ((1. - D(W[1])) * D(v[5]) + D((W[1] * v[1]).astype(T)))).astype(T)
        if order > 2:
            third = v[2] if use_v31 else v[3]
            pos = (D(pos) + ((((1. - D(W[2])) * D(v[6]) + D((W[2] * third).astype(T))) + (1. - D(W[3])) * D(v[7])) + D((W[3] * v[3]).astype(T)))).astype(T)
    box = np.asarray(box, f64)[None, :]
    per = np.asarray(pbc, bool)[None, :]
    hi = per & (D(pos) >= box)
    pos = np.where(hi, (D(pos) - box).astype(T), pos)
    lo = per & (D(pos) < 0.0)
    pos = np.where(lo, (D(pos) + box).astype(T), pos)
    return pos.astype(T), hi, lo


def states(cos, n, x0, nxl, start, length, frag_pos, fmax_col, cols24, myseg, z_seg, z_prev, use_v31, order, sigma0, k_sigma, k_point, lpt_order=3):
    """fmax_col [nxl n n], cols24 [24][nxl n n] PRODFLOAT -> dict: index [found] (ascending particle index), states [found][8], and what the
    tests ask of the inputs: F, q, unwrapped hi / lo flags"""
    T = np.asarray(fmax_col).dtype.type
    found, fftpos = npr.cells(n, x0, nxl, start, length, frag_pos)
    index = np.flatnonzero(found)
    if not index.size:
        e = np.zeros((0, 3), T)
        return {"index": index.astype(np.uint32), "states": np.zeros((0, 8), T), "F": np.zeros(0, T), "q": e, "hi": e.astype(bool), "lo": e.astype(bool)}
    cell = fftpos[index]
    F = np.asarray(fmax_col)[cell]
    c = npr.coords(np.asarray(frag_pos)[index], length)
    q = np.stack([(c[d].astype(f64) + SHIFT).astype(T) for d in range(3)], axis=1)
    vals = np.asarray(cols24)[:, cell]                      # [24][found]
    v = np.stack([vals[3 * s:3 * s + 3].T for s in range(8)])   # [8][found][3]
    eff = min(int(order), int(lpt_order))
    nfam = {1: 1, 2: 2}.get(int(lpt_order), 4)
    w = weights(cos, myseg, z_seg, z_prev, k_point, F, T, nfam)
    sd = sigma_d(cos, sigma0, k_sigma, F, T)
    pbc = [int(length[d]) == int(n) for d in range(3)]
    x, hi, lo = q2x(q, v, w, myseg, eff, use_v31, pbc, [float(l) for l in length], T)
    st = np.concatenate([np.stack(w, axis=1), sd[:, None], x], axis=1).astype(T)
    return {"index": index.astype(np.uint32), "states": st, "F": F, "q": q, "hi": hi, "lo": lo}
