"""numpy / plain-Python restatement of the plan of the slab form of the matter call (include/pinfmax.h: pf_matter_power_slabs) -- TEST
INFRASTRUCTURE.  It shares no code with the library: the reach of a slab from the positions of tests/np_matter.py, windows as lists
of planes, block lists by brute force over sets.  Columns of a slab are [12][nxl][n][n]; planes are global x indices."""
import numpy as np

import np_matter as npm

EXCHANGE_KEYS = ("form", "reach_below", "reach_above", "window_planes", "block_planes", "bytes_per_peer")


def reach(vel12_slab, x0, weight=None, ngp=False):
    """(Hlo, Hhi) of the particles of one slab: over every particle whose x position is finite and inside [0, n], the planes it adds
    to as signed minimal-image offsets from its own plane"""
    nxl, n = vel12_slab.shape[1], vel12_slab.shape[2]
    p = npm.positions(vel12_slab, weight, x0)[0]
    T = p.dtype.type
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(p) & (p >= T(0)) & (p <= T(n))
    q0 = np.broadcast_to(np.arange(x0, x0 + nxl)[:, None, None], p.shape)[ok]
    p = p[ok]
    if p.size == 0:
        return 0, 0
    if ngp:
        planes, used = [np.mod(np.floor(p).astype(np.int64), n)], [np.ones(p.shape, bool)]
    else:
        (c0, c1), (_, t) = npm.cic_axis(p, n)
        planes, used = [c0, c1], [np.ones(p.shape, bool), t != 0]
    lo = hi = 0
    for c, u in zip(planes, used):
        s = np.mod(c[u] - q0[u] + n // 2, n) - n // 2
        if s.size:
            lo, hi = max(lo, int(-s.min())), max(hi, int(s.max()))
    return lo, hi


def box_reach(vel12, P, weight=None, ngp=False):
    """the common reach of the P slabs of a box [12][n][n][n]"""
    n = vel12.shape[1]
    nxl = n // P
    r = [reach(vel12[:, k * nxl:(k + 1) * nxl], k * nxl, weight, ngp) for k in range(P)]
    return max(a for a, _ in r), max(b for _, b in r)


def window(n, P, r, hlo, hhi):
    """the planes rank r deposits into, in the order of its window"""
    nxl = n // P
    if nxl + hlo + hhi >= n:
        return list(range(n))
    return [(r * nxl - hlo + k) % n for k in range(nxl + hlo + hhi)]


def block_lists(n, P, hlo, hhi):
    """L[r][q]: ascending local planes of rank q inside the window of rank r (q != r; L[r][r] is empty), and B"""
    nxl = n // P
    L = [[[] for _ in range(P)] for _ in range(P)]
    for r in range(P):
        w = set(window(n, P, r, hlo, hhi))
        for q in range(P):
            if q != r:
                L[r][q] = sorted(l for l in range(nxl) if q * nxl + l in w)
    B = max([len(L[r][q]) for r in range(P) for q in range(P)] + [0])
    return L, B


def exchange(n, P, hlo, hhi):
    """what pf_debug_matter_exchange reports for this reach"""
    nxl = n // P
    form = 0 if P == 1 or (hlo == 0 and hhi == 0) else 2 if nxl + hlo + hhi >= n else 1
    B = block_lists(n, P, hlo, hhi)[1] if form else 0
    return dict(zip(EXCHANGE_KEYS, (form, hlo, hhi, len(window(n, P, 0, hlo, hhi)), B, B * n * n * 8)))


def shift_cases(n, P, dtype):
    """planted columns of a box for the slab tests: [(name, vel12 [12][n][n][n], weight, ngp, expect)], expect = the common (Hlo,
    Hhi) where it can be said without any implementation, else None"""
    from matter_cases import cases, zeros
    nxl = n // P
    out = []
    for ngp in (False, True):
        tag = "_ngp" if ngp else ""
        out.append(("zero" + tag, zeros(n, dtype), None, ngp, (0, 0)))
        v = zeros(n, dtype); v[0] = 0.25
        out.append(("plus_quarter" + tag, v, None, ngp, (0, 0) if ngp else (0, 1)))
        v = zeros(n, dtype); v[0] = -0.25
        out.append(("minus_quarter" + tag, v, None, ngp, (0, 0) if ngp else (1, 0)))
        v = zeros(n, dtype); v[0] = nxl + 0.5
        out.append(("two_slabs_on" + tag, v, None, ngp, None))
        rng = np.random.default_rng(3 + n + P)
        v = zeros(n, dtype)
        v[0:3] = (1.5 * rng.standard_normal((3, n, n, n))).astype(dtype)
        out.append(("normal_1p5" + tag, v, None, ngp, None))
        v = zeros(n, dtype); v[0, 1, 2, 3] = n // 2 - 1
        out.append(("one_far" + tag, v, None, ngp, (0, n // 2 - 1)))
        v = zeros(n, dtype); v[0, n - 2, 0, 1] = -(n // 2 - 1)
        out.append(("one_far_below" + tag, v, None, ngp, (n // 2 - 1, 0)))
    for name, v, w, ngp, _ in cases(n, dtype):
        if name in ("nonfinite_and_outside", "wrap_to_exactly_n", "below_half_a_cell", "weighted_fractions", "shift_n_minus_one"):
            out.append((name, v, w, ngp, None))
    return out
