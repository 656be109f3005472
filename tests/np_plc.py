"""The past-light-cone test of build_groups() restated in numpy, vectorised over groups: set_obj, set_weight, set_obj_vel
(src/build_groups.c:1354-1460), q2x and vel (:1554-1643), condition_PLC, store_PLC and the polar transformation (:1738-1841), with
InterpolateGrowth (src/cosmo.c:1728-1755) and my_spline_eval (:2016-2027).  np.float32 / np.float64 stand where the reference has
PRODFLOAT / double: a product of two PRODFLOATs is rounded to PRODFLOAT, `1. - w` is a double, an assignment to a PRODFLOAT rounds.
The root is found by bisection in fp64 down to adjacent PRODFLOAT values.  Hubble(z) comes from a table at the same knots, as on the
device."""
import numpy as np

PI = 3.14159265358979323846
f64 = np.float64


def cspline(x, y):
    """GSL's natural cubic spline: (y, c, b, d) per interval"""
    x, y = np.asarray(x, f64), np.asarray(y, f64)
    n = x.size
    h = np.diff(x)
    c = np.zeros(n)
    if n > 2:
        A = np.zeros((n - 2, n - 2))
        g = 3.0 * (np.diff(y)[1:] / h[1:] - np.diff(y)[:-1] / h[:-1])
        for i in range(n - 2):
            A[i, i] = 2.0 * (h[i] + h[i + 1])
            if i + 1 < n - 2:
                A[i, i + 1] = A[i + 1, i] = h[i + 1]
        c[1:-1] = np.linalg.solve(A, g)
    b, d = np.zeros(n), np.zeros(n)
    b[:-1] = np.diff(y) / h - h * (c[1:] + 2.0 * c[:-1]) / 3.0
    d[:-1] = (c[1:] - c[:-1]) / (3.0 * h)
    return np.stack([y, c, b, d])


class Cosmology:
    """the tables of pf_plc_set_cosmology: x [n]; comvdist, hubble [n]; grow, fomega [4][nk][n]"""

    def __init__(self, x, comvdist, hubble, grow, fomega, k_for_GM=0.0, logkmin=-3.0, deltalogk=0.5, rad_gm0=0.0, k_gm_displ=None):
        self.x = np.asarray(x, f64)
        self.n = self.x.size
        self.comv, self.hub = cspline(x, comvdist), cspline(x, hubble)
        grow, fomega = np.asarray(grow, f64), np.asarray(fomega, f64)
        if grow.ndim == 2:
            grow, fomega = grow[:, None, :], fomega[:, None, :]
        self.nk = grow.shape[1]
        # fam[f][j] -> (4, n); f = 0..3 growth, 4..7 fomega
        self.fam = np.array([[cspline(x, t[j]) for j in range(self.nk)] for t in list(grow) + list(fomega)])   # [8][nk][4][n]
        self.k_for_GM, self.logkmin, self.dlogk, self.rad_gm0 = k_for_GM, logkmin, deltalogk, rad_gm0
        self.kmin, self.kmax = 10.0 ** f64(logkmin), np.power(10.0, f64(logkmin) + (self.nk - 1) * f64(deltalogk))
        self.kgm = None if k_gm_displ is None else np.asarray(k_gm_displ, f64)

    def locate(self, z):
        v = -np.log10(1.0 + np.asarray(z, f64))
        i = np.clip(np.searchsorted(self.x, v, side="right") - 1, 0, self.n - 2)
        return v, i

    def _eval(self, tab, v, i):
        """tab [..., 4, n] broadcast against v: my_spline_eval"""
        x = self.x
        y, c, b, d = tab[..., 0, :], tab[..., 1, :], tab[..., 2, :], tab[..., 3, :]

        def pick(a, j):
            if a.ndim == 1:
                return a[j]
            return np.take_along_axis(a, np.broadcast_to(j, a.shape[:-1])[..., None], -1)[..., 0]
        dx = v - x[i]
        inside = pick(y, i) + dx * (pick(b, i) + dx * (pick(c, i) + dx * pick(d, i)))
        below = y[..., 0] + (v - x[0]) * (y[..., 1] - y[..., 0]) / (x[1] - x[0])
        above = y[..., -1] + (v - x[-1]) * (y[..., -1] - y[..., -2]) / (x[-1] - x[-2])
        return np.where(v < x[0], below, np.where(v > x[-1], above, inside))

    def comvdist(self, z):
        v, i = self.locate(z)
        return self._eval(self.comv, v, i)

    def hubble(self, z):
        v, i = self.locate(z)
        return self._eval(self.hub, v, i)

    def group_k(self, M, ipd, T):
        """(myk, kk, dk, both) of groups of M particles: set_obj :1361-1378 and the branch of InterpolateGrowth"""
        M = np.asarray(M)
        if self.nk == 1:
            z = np.zeros(M.shape)
            return np.full(M.shape, self.k_for_GM), z.astype(int), z, z.astype(bool)
        ns = self.kgm.size
        R = (np.power(M.astype(f64) * 3. / 4. / PI, 1. / 3.) * ipd).astype(T).astype(f64)
        interp = np.maximum((1. - R / self.rad_gm0) * f64(ns - 1), 0.0)
        indx = np.minimum(interp.astype(int), ns - 2)
        w = interp - indx
        myk = np.power(10., np.log10(self.kgm[indx]) * (1. - w) + np.log10(self.kgm[indx + 1]) * w)
        dk = (np.log10(myk) - self.logkmin) / self.dlogk
        kk = np.clip(dk.astype(int), 0, self.nk - 2)
        dk = dk - kk
        lo, hi = myk < self.kmin, myk > self.kmax
        both = ~(lo | hi)
        kk = np.where(lo, 0, np.where(hi, self.nk - 1, kk))
        return myk, kk, np.where(both, dk, 0.0), both

    def growth(self, f, K, z):
        """InterpolateGrowth of family f (0..3 log10 growth, 4..7 fomega) at z for groups with K = group_k(...)"""
        _, kk, dk, both = K
        v, i = self.locate(z)
        a = self._eval(self.fam[f][kk], v, i)
        b = self._eval(self.fam[f][np.minimum(kk + 1, self.nk - 1)], v, i)
        return np.where(both, dk * b + (1 - dk) * a, a)

    def mode(self, o, K, z):
        g = np.power(10., self.growth(o, K, z))
        return -g if o == 2 else g


class Geometry:
    def __init__(self, center, zvers, aperture, Fstop, ipd, gs, repls, stabl, lastz=0.0, delta_z=1.0, nzbins=0):
        self.center, self.zvers = np.asarray(center, f64), np.asarray(zvers, f64)
        self.aperture, self.Fstop, self.ipd, self.gs = f64(aperture), f64(Fstop), f64(ipd), np.asarray(gs, np.int64)
        r = np.asarray(repls, f64).reshape(-1, 5)
        self.shift = r[:, :3].astype(np.int64)
        self.F1, self.F2 = r[:, 3], r[:, 4]
        self.stabl = np.asarray(stabl, np.int64)
        self.lastz, self.delta_z, self.nzbins = f64(lastz), f64(delta_z), int(nzbins)
        self.observer = self.center[None, :] - (self.gs[None, :] * self.shift).astype(f64)   # [nrep][3]


class Segment:
    def __init__(self, myseg, z_seg, z_prev=0.0, use_v31=False, order=3):
        self.myseg, self.z_seg, self.z_prev, self.use_v31, self.order = int(myseg), f64(z_seg), f64(z_prev), bool(use_v31), int(order)


class Groups:
    """M [N] int; q [N][3]; vel [8][N][3] (v, v2, v31, v32 and their _prev twins), PRODFLOAT"""

    def __init__(self, M, q, vel, T):
        self.T = T
        self.M, self.q, self.vel = np.asarray(M, np.int32), np.asarray(q, T), np.asarray(vel, T)


def weights(cos, seg, K, F, T):
    """set_weight (:1411-1444) at z = F - 1 -> w [4][N] PRODFLOAT"""
    z = F.astype(f64) - 1.0
    w = []
    for o in range(4):
        g, gs = cos.mode(o, K, z), cos.mode(o, K, seg.z_seg)
        if seg.myseg:
            gp = cos.mode(o, K, seg.z_prev)
            w.append(((g - gp) / (gs - gp)).astype(T))
        else:
            w.append((g / gs).astype(T))
    return w


def q2x(G, w, seg):
    """q2x (:1554-1603) of the three axes without periodic wrapping -> [N][3] PRODFLOAT"""
    T, v, q = G.T, G.vel, G.q
    W = [a[:, None] for a in w]
    D = lambda a: a.astype(f64)
    if not seg.myseg:
        pos = (q + (W[0] * v[0]).astype(T)).astype(T)
        if seg.order > 1:
            pos = (pos + (W[1] * v[1]).astype(T)).astype(T)
        if seg.order > 2:
            pos = (pos + ((W[2] * v[2]).astype(T) + (W[3] * v[3]).astype(T)).astype(T)).astype(T)
        return pos
    pos = ((D(q) + (1. - D(W[0])) * D(v[4])) + D((W[0] * v[0]).astype(T))).astype(T)
    if seg.order > 1:
        pos = (D(pos) + ((1. - D(W[1])) * D(v[5]) + D((W[1] * v[1]).astype(T)))).astype(T)
    if seg.order > 2:
        third = v[2] if seg.use_v31 else v[3]          # :1588 as written multiplies w31 with v32
        pos = (D(pos) + ((((1. - D(W[2])) * D(v[6]) + D((W[2] * third).astype(T))) + (1. - D(W[3])) * D(v[7])) + D((W[3] * v[3]).astype(T)))).astype(T)
    return pos


def ends(cos, geo, seg, G, K, F):
    """what condition_PLC needs of every group at its F: P [N][3] PRODFLOAT (stabl added in PRODFLOAT), D [N] = distance / InterPartDist"""
    T = G.T
    F = np.asarray(F, T)
    w = weights(cos, seg, K, F, T)
    P = (q2x(G, w, seg) + geo.stabl.astype(T)[None, :]).astype(T)
    return P, cos.comvdist(F.astype(f64) - 1.0) / geo.ipd, w


def condition(geo, P, D, reps=None):
    """condition_PLC of every (group, replication): [N][nrep] (reps: one replication index per group -> [N])"""
    if reps is None:
        diff = P.astype(f64)[:, None, :] - geo.observer[None, :, :]
        s = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
        return np.sqrt(s) - D[:, None]
    diff = P.astype(f64) - geo.observer[reps]
    s = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
    return np.sqrt(s) - D


def subset(G, idx):
    return Groups(G.M[idx], G.q[idx], G.vel[:, idx], G.T)


def condition_at(cos, geo, seg, G, idx, reps, F):
    """condition_PLC of the pairs (idx[p], reps[p]) at F[p]"""
    g = subset(G, idx)
    K = cos.group_k(g.M, geo.ipd, G.T)
    P, D, _ = ends(cos, geo, seg, g, K, F)
    return condition(geo, P, D, reps)


def store_at(cos, geo, seg, G, idx, reps, F):
    """store_PLC of the pairs at F -> dict: inside (the aperture test), z, x [P][3], v [P][3], vscale [P] (sum of |terms| of v), bin"""
    T = G.T
    g = subset(G, idx)
    F = np.asarray(F, T)
    K = cos.group_k(g.M, geo.ipd, T)
    P, _, w = ends(cos, geo, seg, g, K, F)
    D = lambda a: a.astype(f64)
    x = (geo.ipd * (D(P) - geo.observer[reps])).astype(T)
    rho = np.sqrt(D(((x[:, 0] * x[:, 0]).astype(T) + (x[:, 1] * x[:, 1]).astype(T)).astype(T) + (x[:, 2] * x[:, 2]).astype(T)))
    dot = (D(x[:, 0]) * geo.zvers[0] + D(x[:, 1]) * geo.zvers[1]) + D(x[:, 2]) * geo.zvers[2]
    with np.errstate(invalid="ignore", divide="ignore"):
        theta = np.where(rho > 0, -np.arccos(np.clip(dot / rho, -1, 1)) * 180. / PI + 90., 90.0)
    inside = (90. - theta) < geo.aperture
    z = D(F) - 1.0
    fac = (cos.hubble(z) / (1. + z) * geo.ipd).astype(T)
    Dv = [(D(fac) * cos.growth(4 + f, K, z)).astype(T)[:, None] for f in range(4)]
    W = [a[:, None] for a in w]
    v = g.vel
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
    vscale = sum(np.abs(D(a)).max(axis=1) for a in terms[:nterm])
    zT = z.astype(T)
    b = ((D(zT) - geo.lastz) / geo.delta_z).astype(int) if geo.nzbins else np.zeros(len(idx), int)
    b = np.where(b == geo.nzbins, b - 1, b)
    return {"inside": inside, "angle": 90. - theta, "z": zT, "x": x, "v": vv, "vscale": vscale, "bin": b}


def tried(mode_events, Flo, Flast, geo, T):
    """[N][nrep]: the range test of a replication, :819 in the last check and :394-395 at an event"""
    F1, F2 = geo.F1.astype(T)[None, :], geo.F2.astype(T)[None, :]
    if mode_events:
        return ~((Flo[:, None] > F1) | (Flast[:, None] < F2))
    return Flast[:, None] > F2


def bisect(cos, geo, seg, G, idx, reps, Flo, Flast):
    """the crossing F of every pair (condition > 0 at Flo, < 0 at Flast): fp64 bisection down to adjacent PRODFLOAT values; of the two
    the one with the smaller |condition|"""
    T = G.T
    a, b = np.array(Flo, T), np.array(Flast, T)
    fa = condition_at(cos, geo, seg, G, idx, reps, a)
    fb = condition_at(cos, geo, seg, G, idx, reps, b)
    for _ in range(80):
        m = (0.5 * (a.astype(f64) + b.astype(f64))).astype(T)
        live = (m != a) & (m != b)
        if not live.any():
            break
        fm = condition_at(cos, geo, seg, G, idx, reps, m)
        up = live & (fm > 0)
        dn = live & ~(fm > 0)
        a, fa = np.where(up, m, a), np.where(up, fm, fa)
        b, fb = np.where(dn, m, b), np.where(dn, fm, fb)
    return np.where(np.abs(fa) <= np.abs(fb), a, b), np.minimum(np.abs(fa), np.abs(fb))


def cross(cos, geo, seg, G, Flast, events=False, Flo=None, passes=None, min_mass=0):
    """the whole test -> dict: tried [N][nrep], bb, aa [N][nrep] (nan where not tried / not passing), cand, rep of the crossing pairs in
    (candidate, replication) order, kind (1 at F_lo, 2 a root), F, resid (|condition| at F), and store_at(...) of them"""
    T = G.T
    N = G.M.size
    Flast = np.asarray(Flast, T)
    Flo = np.asarray(Flo, T) if events else np.full(N, T(geo.Fstop), T)
    ok = (G.M >= min_mass) if passes is None else (np.asarray(passes, bool) & (G.M >= min_mass))
    K = cos.group_k(G.M, geo.ipd, T)
    Plo, Dlo, _ = ends(cos, geo, seg, G, K, Flo)
    Phi, Dhi, _ = ends(cos, geo, seg, G, K, Flast)
    tr = tried(events, Flo, Flast, geo, T) & ok[:, None]
    bb = np.where(tr, condition(geo, Plo, Dlo), np.nan)
    aa = np.where(tr, condition(geo, Phi, Dhi), np.nan)
    with np.errstate(invalid="ignore"):
        kind = np.where(bb == 0.0, 1, np.where((bb > 0.) & (aa < 0.), 2, 0))
    cand, rep = np.nonzero(kind)
    kd = kind[cand, rep]
    F = Flo[cand].copy()
    resid = np.zeros(len(cand))
    r = kd == 2
    if r.any():
        F[r], resid[r] = bisect(cos, geo, seg, G, cand[r], rep[r], Flo[cand[r]], Flast[cand[r]])
    out = {"tried": tr, "bb": bb, "aa": aa, "cand": cand, "rep": rep, "kind": kd, "F": F, "resid": resid, "Flo": Flo}
    out["store"] = store_at(cos, geo, seg, G, cand, rep, F) if len(cand) else None
    return out
