"""numpy restatement of the halo-power call (include/pinfmax.h: pf_halo_power) -- TEST INFRASTRUCTURE.  It shares no code with the
library: the positions in cells, their classes, the selection by mass with its integer sums (Python integers: no width to
overflow), the integer cloud-in-cell / nearest-grid-point factors, the grid by np.add.at on uint64, the contrast with the bin's own
mean.  The shell sums of a contrast come through tests/np_matter.py and tests/np_power.py (spectra()).

pos is [count][3] float64, mass [count] int32; a grid is [nxl][n][n] uint64 in units of 2^-30 of a unit weight."""
import numpy as np

import np_matter as npm
import np_power as npp

SHIFT = 30
UNIT = 1024
WEIGHT_LIMIT = 1 << 34
INT_KEYS = ("selected", "weight_sum", "weight2_hi", "weight2_lo", "nonfinite", "outside", "empty_cells", "max_cell")


def positions(pos, scale, n):
    """p [count][3]: one double product and one wrap"""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        p = pos * np.float64(scale)
        p = np.where(p >= np.float64(n), p - np.float64(n), p)
        p = np.where(p < 0.0, p + np.float64(n), p)
    return p


def classes(p, n):
    """0 deposited, 1 not finite, 2 outside [0, n]"""
    bad = ~np.all(np.isfinite(p), axis=1)
    with np.errstate(invalid="ignore"):
        inside = np.all((p >= 0.0) & (p <= np.float64(n)), axis=1)
    return np.where(bad, 1, np.where(inside, 0, 2))


def cic_axis(p, n):
    """cells [2] and integer factors [2] of positions in [0, n]"""
    u = p - 0.5
    f = np.floor(u)
    d = u - f
    t = np.floor(d * 1024.0).astype(np.int64)
    i0 = f.astype(np.int64)
    assert np.all((i0 >= -1) & (i0 <= n - 1)) and np.all((t >= 0) & (t <= UNIT))
    return (np.mod(i0, n), np.mod(i0 + 1, n)), (UNIT - t, t)


def select(pos, mass, lo, hi, n, scale=1.0, mass_weight=False):
    """-> (p, the index of the selected haloes, their weights as int64, the list-derived counters of the bin)"""
    mass = np.asarray(mass, dtype=np.int32)
    p = positions(pos, scale, n)
    cls = classes(p, n)
    rng = (mass >= lo) & (mass <= hi)
    sel = np.flatnonzero(rng & (cls == 0))
    w = mass[sel].astype(np.int64) if mass_weight else np.ones(len(sel), dtype=np.int64)
    w2 = sum(int(x) * int(x) for x in w.tolist())
    info = {"selected": len(sel), "weight_sum": sum(int(x) for x in w.tolist()), "weight2_hi": w2 >> 64, "weight2_lo": w2 & ((1 << 64) - 1),
            "nonfinite": int((rng & (cls == 1)).sum()), "outside": int((rng & (cls == 2)).sum())}
    return p, sel, w, info


def deposit(n, pos, mass, lo, hi, scale=1.0, mass_weight=False, ngp=False, x0=0, nxl=None):
    """-> (grid [nxl][n][n] uint64 of the planes [x0, x0 + nxl), info dict), or (None, info) where the bin has no headroom"""
    nxl = n - x0 if nxl is None else nxl
    p, sel, w, info = select(pos, mass, lo, hi, n, scale, mass_weight)
    if info["weight_sum"] >= WEIGHT_LIMIT:
        return None, info
    grid = np.zeros(n * n * n, dtype=np.uint64)
    q = p[sel]
    wu = w.astype(np.uint64)
    if ngp:
        c = [np.mod(np.floor(q[:, j]).astype(np.int64), n) for j in range(3)]
        np.add.at(grid, (c[0] * n + c[1]) * n + c[2], wu << np.uint64(SHIFT))
    else:
        ax = [cic_axis(q[:, j], n) for j in range(3)]
        for a in range(2):
            for b in range(2):
                for c in range(2):
                    f = (ax[0][1][a] * ax[1][1][b] * ax[2][1][c]).astype(np.uint64)
                    np.add.at(grid, (ax[0][0][a] * n + ax[1][0][b]) * n + ax[2][0][c], wu * f)
    whole = grid.reshape(n, n, n)
    assert sum(int(v) for v in whole.ravel().tolist()) == info["weight_sum"] << SHIFT
    g = whole[x0:x0 + nxl]
    info["empty_cells"] = int((g == 0).sum())
    info["max_cell"] = int(g.max())
    return g.copy(), info


def mean(weight_sum, n):
    return np.float64(weight_sum << SHIFT) / np.float64(n ** 3)


def contrast(grid, weight_sum, n, field_bytes=8):
    """delta = cell / mean - 1 in double, rounded to the field type, widened back"""
    d = grid.astype(np.float64) / mean(weight_sum, n) - 1.0
    return d if field_bytes == 8 else d.astype(np.float32).astype(np.float64)


def spectra(delta, lin=None, ngp=False, deconvolve=False):
    """the shell columns of a whole-box contrast [n][n][n] through numpy's transform and the shell restatement of np_matter; lin: the
    linear spectrum as an x-slab [n (kx)][n (ky)][n/2+1] (Fmax.density())"""
    spec = npp.from_x_slab(np.fft.rfftn(delta, axes=(0, 1, 2)))
    return npm.shells(spec, None if lin is None else npp.from_x_slab(lin), 0, 8, ngp, deconvolve)


def shot(info):
    w2 = (info["weight2_hi"] << 64) | info["weight2_lo"]
    return w2 / (info["weight_sum"] * info["weight_sum"]) if info["weight_sum"] else float("nan")


def brute_force(n, pos, mass, lo, hi, scale=1.0, mass_weight=False, ngp=False):
    """the same grid and counters halo by halo in Python integers and floats -- what deposit() is held against"""
    import math
    grid = {}
    info = {k: 0 for k in ("selected", "weight_sum", "nonfinite", "outside")}
    w2 = 0
    for x, m in zip(np.asarray(pos, dtype=np.float64).reshape(-1, 3).tolist(), np.asarray(mass).tolist()):
        if not lo <= m <= hi:
            continue
        p = []
        for v in x:
            v = v * float(scale)
            if v >= n:
                v -= n
            if v < 0:
                v += n
            p.append(v)
        if not all(math.isfinite(v) for v in p):
            info["nonfinite"] += 1
            continue
        if not all(0.0 <= v <= n for v in p):
            info["outside"] += 1
            continue
        W = m if mass_weight else 1
        info["selected"] += 1
        info["weight_sum"] += W
        w2 += W * W
        if ngp:
            axes = [[(int(math.floor(v)) % n, UNIT)] for v in p]
        else:
            axes = []
            for v in p:
                u = v - 0.5
                i0 = math.floor(u)
                t = int((u - i0) * 1024.0)
                axes.append([(int(i0) % n, UNIT - t), ((int(i0) + 1) % n, t)])
        for cx, fx in axes[0]:
            for cy, fy in axes[1]:
                for cz, fz in axes[2]:
                    grid[cx, cy, cz] = grid.get((cx, cy, cz), 0) + W * fx * fy * fz
    info["weight2_hi"], info["weight2_lo"] = w2 >> 64, w2 & ((1 << 64) - 1)
    return grid, info
