"""numpy restatement of the bispectrum of the haloes (include/pinfmax.h: pf_halo_bispectrum) -- TEST INFRASTRUCTURE.  It shares no
code with the library: the k-bin of a mode from int64 integers, the closed triples from the triangle inequality on the bin edges, the
mask rule on a ky-slab, the terms (a b) c as numpy rounds them, the fixed point of the sums in Python integers (floor(|t| 2^(95 - e))
exactly, the carry and the three roundings of pf_power_from_limbs restated), the same sums by math.fsum, the whole call through
numpy.fft on the deposit and the contrast of tests/np_halo.py / tests/np_multipoles.py, and the direct enumeration of all ordered
pairs of modes that the estimator is held against."""
import math

import numpy as np

import np_halo as nph
import np_matter as npm
import np_multipoles as npl
import np_power as npp

MAX_KBINS = 32


def bin_of(k2, kmin, dk, nk):
    """the k-bin of every k2 (int64), -1 for none: (kmin + i dk)^2 <= k2 < (kmin + (i + 1) dk)^2"""
    k2 = np.asarray(k2, dtype=np.int64)
    out = np.full(k2.shape, -1, np.int64)
    for i in range(nk):
        lo, hi = (kmin + i * dk) ** 2, (kmin + (i + 1) * dk) ** 2
        out[(k2 >= lo) & (k2 < hi)] = i
    return out


def triangles(kmin, dk, nk):
    """the ordered triples i <= j <= l that can close: the smallest side of bin l below the supremum of the sum of the other two"""
    return [(i, j, l) for i in range(nk) for j in range(i, nk) for l in range(j, nk) if kmin + l * dk < (kmin + (i + 1) * dk) + (kmin + (j + 1) * dk)]


def window(n, y0, nyl, ngp):
    tab = npm.deconv_table(n, ngp)
    ay = np.abs(npp.signed(np.arange(y0, y0 + nyl), n))[:, None, None]
    ax = np.abs(npp.signed(np.arange(n), n))[None, :, None]
    return (tab[ax] * tab[ay]) * tab[np.arange(n // 2 + 1)][None, None, :]


def mask(spec, kmin, dk, nk, which, y0=0, field_bytes=8, ngp=False, deconvolve=False, kind=0, read=True):
    """the field of k-bin `which` on the ky-slab [nyl][n][n/2+1]: (complex128 field, kmodes, nonfinite_modes).  read False: the
    count field of a call, which reads no spectrum"""
    nyl, n = spec.shape[:2]
    k2, _, w = npp.geometry(n, y0, nyl)
    inside = bin_of(k2, kmin, dk, nk) == which
    re, im = npp.as_field(spec, field_bytes)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if deconvolve:
            c = window(n, y0, nyl, ngp)
            re, im = re * c, im * c
        if field_bytes == 4:
            re, im = re.astype(np.float32).astype(np.float64), im.astype(np.float32).astype(np.float64)
    bad = inside & ~(np.isfinite(re) & np.isfinite(im)) if read else np.zeros(inside.shape, bool)
    keep = inside & ~bad
    out = np.zeros(inside.shape, np.complex128)
    out.real = np.where(keep, float(n) ** 3 if kind else re, 0.0)
    out.imag = np.where(keep, 0.0 if kind else im, 0.0)
    return out, int(w[inside].sum()), int(w[bad].sum())


def as_stores(fields, field_bytes):
    """the kept fields: rounded to the field type, a cell that is not finite as zero -> (fields, nonfinite cells)"""
    f = np.ascontiguousarray(fields, dtype=np.float64)
    if field_bytes == 4:
        with np.errstate(over="ignore", invalid="ignore"):
            f = f.astype(np.float32).astype(np.float64)
    bad = ~np.isfinite(f)
    return np.where(bad, 0.0, f), int(bad.sum())


def exponent(m):
    """e with 2^(e-1) <= m < 2^e"""
    return math.frexp(m)[1]


def fixed_sum(t, e):
    """sum over the terms t >= 0 of floor(t 2^(95 - e)), a Python integer"""
    t = t[t > 0]
    if not len(t):
        return 0
    m, ex = np.frexp(t)
    mi = (m * 2.0 ** 53).astype(np.int64)                       # exact: t = mi 2^(ex - 53)
    shift = ex.astype(np.int64) - 53 + 95 - e
    total = 0
    down = shift < 0
    if np.any(down):
        v = mi[down] >> np.minimum(-shift[down], 63)
        total += (int((v >> 26).sum()) << 26) + int((v & ((1 << 26) - 1)).sum())
    for s in np.unique(shift[~down]):
        v = mi[shift == s]
        total += ((int((v >> 26).sum()) << 26) + int((v & ((1 << 26) - 1)).sum())) << int(s)
    return total


def from_fixed(total, e):
    """pf_power_from_limbs on the three carried limbs of `total`: three roundings"""
    v0, v1, top = total & 0xffffffff, (total >> 32) & 0xffffffff, total >> 64
    d = float(top)
    d = d * 4294967296.0 + float(v1)
    d = d * 4294967296.0 + float(v0)
    return math.ldexp(d, e - 95)


def term(a, b, c):
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return (a * b) * c


def triples(fields, kmin, dk, nk, field_bytes=8):
    """the columns of pf_debug_bispec_triples for nk real fields [nk][nxl][n][n], bit for bit (sums, parts, pair, maxima), and the
    same positive sums by math.fsum (parts_fsum, pair_fsum)"""
    f, bad = as_stores(fields, field_bytes)
    tri = triangles(kmin, dk, nk)
    M = [float(np.max(np.abs(f[i]))) for i in range(nk)]
    out = {"sums": np.zeros(len(tri)), "parts": np.zeros((2, len(tri))), "pair": np.zeros(nk), "maxima": np.array(M), "nonfinite_cells": bad,
           "parts_fsum": np.zeros((2, len(tri))), "pair_fsum": np.zeros(nk)}
    for t, (i, j, l) in enumerate(tri):
        x = term(f[i], f[j], f[l]).ravel()
        m = float(term(np.float64(M[i]), np.float64(M[j]), np.float64(M[l])))
        e = exponent(m) if m > 0 else 0
        for s, part in enumerate((x[x > 0], -x[x < 0])):
            out["parts"][s, t] = from_fixed(fixed_sum(part, e), e)
            out["parts_fsum"][s, t] = math.fsum(part.tolist())
        out["sums"][t] = out["parts"][0, t] - out["parts"][1, t]
    for i in range(nk):
        x = (f[i] * f[i]).ravel()
        m = M[i] * M[i]
        e = exponent(m) if m > 0 else 0
        out["pair"][i] = from_fixed(fixed_sum(x, e), e)
        out["pair_fsum"][i] = math.fsum(x.tolist())
    return out


def fields_of(spec_slab, kmin, dk, nk, field_bytes=8, ngp=False, deconvolve=False, kind=0, read=True):
    """the nk band-filtered real fields [nk][n][n][n] of a whole ky-slab through numpy's reverse transform (with its 1 / N^3), and
    kmodes[nk]"""
    n = spec_slab.shape[1]
    out, km = [], []
    for i in range(nk):
        q, k, _ = mask(spec_slab, kmin, dk, nk, i, 0, field_bytes, ngp, deconvolve, kind, read)
        out.append(np.fft.irfftn(np.transpose(q, (1, 0, 2)), s=(n, n, n), axes=(0, 1, 2)))
        km.append(k)
    return np.array(out), np.array(km, dtype=np.uint64)


def estimator(fields, kmin, dk, nk):
    """sum over the cells of the product of three fields for every closed triple, by math.fsum: (sums, absolute sums)"""
    tri = triangles(kmin, dk, nk)
    sums, absum = np.zeros(len(tri)), np.zeros(len(tri))
    for t, (i, j, l) in enumerate(tri):
        x = term(fields[i], fields[j], fields[l]).ravel()
        sums[t], absum[t] = math.fsum(x.tolist()), math.fsum(np.abs(x).tolist())
    return sums, absum


def bispectrum(n, pos, vel, mass, ranges, kmin, dk, nk, scale=1.0, vfac=0.0, los=2, mass_weight=False, ngp=False, deconvolve=False, field_bytes=8):
    """the whole call through numpy.fft: kmodes, ntri, per mass bin bsum [nt] and psum [nk] with their absolute sums, the deposit's
    counters, and the fields themselves (data [b] -> [nk][n][n][n] or None, count [nk][n][n][n]) for the bound of the GPU test"""
    tri = triangles(kmin, dk, nk)
    count, km = fields_of(np.zeros((n, n, n // 2 + 1), np.complex128), kmin, dk, nk, field_bytes, kind=1, read=False)
    cs, cabs = estimator(count, kmin, dk, nk)
    out = {"triangles": tri, "kmodes": km, "ntri": cs / float(n) ** 3, "ntri_abs": cabs / float(n) ** 3, "bsum": np.zeros((len(ranges), len(tri))),
           "babs": np.zeros((len(ranges), len(tri))), "psum": np.zeros((len(ranges), nk)), "info": [], "count_fields": count, "data_fields": [], "spec": [], "dens": []}
    for b, (lo, hi) in enumerate(ranges):
        grid, info = npl.deposit(n, pos, vel, mass, int(lo), int(hi), scale, vfac, los, mass_weight, ngp)
        out["info"].append(info)
        if grid is None or not info["weight_sum"]:
            out["data_fields"].append(None); out["spec"].append(None); out["dens"].append(None)
            continue
        delta = nph.contrast(grid, info["weight_sum"], n, field_bytes)
        spec = npp.from_x_slab(np.fft.rfftn(delta, axes=(0, 1, 2)))
        data, _ = fields_of(spec, kmin, dk, nk, field_bytes, ngp, deconvolve)
        out["bsum"][b], out["babs"][b] = estimator(data, kmin, dk, nk)
        out["psum"][b] = [math.fsum((data[i] * data[i]).ravel().tolist()) for i in range(nk)]
        out["data_fields"].append(data); out["spec"].append(spec); out["dens"].append(delta)
    return out


def count_triangles(kmin, dk, nk):
    """the number of ordered (k1 in i, k2 in j, k3 in l) with k1 + k2 + k3 = 0 for every closed triple, in exact integers on the
    unbounded lattice.  The bins are invariant under the 48 symmetries of the cube, so k1 runs over one representative per orbit
    (kx >= ky >= kz >= 0) with the size of its orbit as its weight; k2 runs over the whole bin"""
    kmax = kmin + nk * dk
    s = np.arange(-kmax, kmax + 1)
    kx, ky, kz = np.meshgrid(s, s, s, indexing="ij")
    K = np.stack([kx.ravel(), ky.ravel(), kz.ravel()], axis=1)
    b = bin_of((K * K).sum(axis=1), kmin, dk, nk)
    sel = [K[b == i] for i in range(nk)]
    out = []
    for i, j, l in triangles(kmin, dk, nk):
        total = 0
        for k1 in sel[i]:
            if not (k1[0] >= k1[1] >= k1[2] >= 0):
                continue
            orbit = {tuple(sg * k1[list(p)]) for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
                     for sg in (np.array(q) for q in ((1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1), (-1, 1, 1), (-1, 1, -1), (-1, -1, 1), (-1, -1, -1)))}
            k3 = -(k1[None, :] + sel[j])
            total += len(orbit) * int((bin_of((k3 * k3).sum(axis=1), kmin, dk, nk) == l).sum())
        out.append(total)
    return np.array(out, dtype=np.int64)


def enumerate_pairs(delta, kmin, dk, nk, all_triples=False):
    """direct enumeration: for every ordered triple of bins the sum over all ordered pairs (k1 in i, k2 in j) with k3 = -(k1 + k2) in l
    of delta(k1) delta(k2) delta(k3) / N3^2, and their number -- true triangles of integer wavevectors, nothing modulo the grid.
    delta: the real field [n][n][n].  all_triples: every i <= j <= l, the open ones too -> (list of triples, sums, counts)"""
    n = delta.shape[0]
    full = np.fft.fftn(delta)
    s = npp.signed(np.arange(n), n)
    kx, ky, kz = np.meshgrid(s, s, s, indexing="ij")
    k2 = kx * kx + ky * ky + kz * kz
    b = bin_of(k2, kmin, dk, nk)
    # (a Nyquist plane has one sign here; bins that reach it are not used: kmax <= n / 2 in every case of the tests)
    assert kmin + nk * dk <= n // 2
    sel = [np.nonzero(b.ravel() == i)[0] for i in range(nk)]
    K = np.stack([kx.ravel(), ky.ravel(), kz.ravel()], axis=1)
    val = full.ravel()
    tri = [(i, j, l) for i in range(nk) for j in range(i, nk) for l in range(j, nk)] if all_triples else triangles(kmin, dk, nk)
    sums, counts = np.zeros(len(tri)), np.zeros(len(tri), np.int64)
    for t, (i, j, l) in enumerate(tri):
        K1, K2 = K[sel[i]], K[sel[j]]
        k3 = -(K1[:, None, :] + K2[None, :, :])                   # true integers: up to 2 kmax in magnitude
        inl = bin_of((k3 * k3).sum(axis=2), kmin, dk, nk) == l
        a, c = np.nonzero(inl)
        q = k3[a, c]
        assert np.all(np.abs(q) <= n // 2)
        v3 = full[q[:, 0] % n, q[:, 1] % n, q[:, 2] % n]
        prod = val[sel[i]][a] * val[sel[j]][c] * v3
        counts[t] = len(a)
        sums[t] = float(np.sum(prod.real)) / float(n) ** 6
    return tri, sums, counts
