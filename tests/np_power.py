"""numpy restatement of the power-spectrum call (include/pinfmax.h: pf_power_spectrum) -- TEST INFRASTRUCTURE.  The integer columns in
integer arithmetic, `power` as math.fsum over the terms of a shell, `variance` as math.fsum with numpy.exp.

A spectrum here is a ky-slab [nyl][n (kx)][n/2+1] complex128, rows y0 .. y0 + nyl - 1 of the box: the layout of
pf_debug_power_spectrum.  Fmax.density() / kvector() of one rank return [kx][ky][kz]: from_x_slab() swaps the two."""
import math

import numpy as np


def signed(i, n):
    i = np.asarray(i, dtype=np.int64)
    return np.where(i > n // 2, i - n, i)


def shell_of(k2):
    """b with (2b - 1)^2 <= 4 k2 < (2b + 1)^2: 2b - 1 <= isqrt(4 k2), so b = (isqrt(4 k2) + 1) // 2"""
    q = 4 * np.asarray(k2, dtype=np.int64)
    s = np.floor(np.sqrt(q.astype(np.float64))).astype(np.int64)
    s = np.where(s * s > q, s - 1, s)          # the float root is a guess: the decision is the integers'
    s = np.where((s + 1) * (s + 1) <= q, s + 1, s)
    assert np.all(s * s <= q) and np.all((s + 1) * (s + 1) > q)
    b = (s + 1) // 2
    assert np.all(((2 * b - 1) ** 2 <= q) | (q == 0)) and np.all(q < (2 * b + 1) ** 2)   # (k = 0 alone is shell 0)
    return b


def bins(n):
    """1 + the largest b with (2b - 1)^2 <= 3 n^2"""
    b = (math.isqrt(3 * n * n) + 1) // 2
    assert (2 * b - 1) ** 2 <= 3 * n * n < (2 * b + 1) ** 2
    return b + 1


def geometry(n, y0=0, nyl=None):
    """k2, shell and weight of every mode of the slab, each [nyl][n][n/2+1] int64"""
    nyl = n if nyl is None else nyl
    sy = signed(np.arange(y0, y0 + nyl), n)[:, None, None]
    sx = signed(np.arange(n), n)[None, :, None]
    iz = np.arange(n // 2 + 1)[None, None, :]
    k2 = sx * sx + sy * sy + signed(iz, n) ** 2
    w = np.broadcast_to(np.where((iz > 0) & (iz < n // 2), 2, 1), k2.shape)
    return k2, shell_of(k2), w


def from_x_slab(spec):
    return np.ascontiguousarray(np.transpose(spec, (1, 0, 2)))


def as_field(spec, field_bytes):
    """the parts as the device holds them, widened back to double"""
    spec = np.ascontiguousarray(spec, dtype=np.complex128)
    if field_bytes == 8:
        return spec.real.copy(), spec.imag.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        return spec.real.astype(np.float32).astype(np.float64), spec.imag.astype(np.float32).astype(np.float64)


def terms(spec, field_bytes=8):
    re, im = as_field(spec, field_bytes)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return re * re + im * im


def power(spec, y0=0, radii_cells=(), field_bytes=8):
    """the columns of pf_debug_power_spectrum for this slab (of the whole box with y0 = 0 and nyl = n)"""
    nyl, n = spec.shape[0], spec.shape[1]
    assert spec.shape == (nyl, n, n // 2 + 1)
    k2, sh, w = geometry(n, y0, nyl)
    t = terms(spec, field_bytes)
    fin = np.isfinite(t)
    nb = bins(n)
    n6 = float(n ** 6)
    nm = np.zeros(nb, dtype=np.uint64)
    ks = np.zeros(nb, dtype=np.uint64)
    pw = np.zeros(nb)
    for b in range(nb):
        m = sh == b
        nm[b] = int(w[m].sum())
        ks[b] = int((w[m] * k2[m]).sum())
        mf = m & fin
        pw[b] = math.fsum((w[mf] * t[mf]).tolist()) / n6      # (w t is exact: w is a power of two)
    kf = 2.0 * math.pi / n
    var = np.zeros(len(radii_cells))
    mv = fin & (k2 > 0)
    wt, kk = (w[mv] * t[mv]), k2[mv].astype(np.float64)
    for i, r in enumerate(radii_cells):
        a = (kf * kf) * (float(r) * float(r))
        with np.errstate(under="ignore"):
            var[i] = math.fsum((wt * np.exp(-(a * kk))).tolist()) / n6
    return {"nmodes": nm, "k2sum": ks, "power": pw, "variance": var, "modes": nyl * n * n, "nonfinite": int(w[~fin].sum())}


def add(parts):
    """the box's columns from those of its slabs: integers exactly, doubles in slab order"""
    out = {k: sum(int(p[k]) for p in parts) for k in ("modes", "nonfinite")}
    for k in ("nmodes", "k2sum"):
        out[k] = np.sum([p[k] for p in parts], axis=0, dtype=np.uint64)
    for k in ("power", "variance"):
        out[k] = np.sum([p[k] for p in parts], axis=0)
    return out


def rel(got, want):
    """largest |got - want| / want over the entries with want != 0; entries with want == 0 must be exactly 0"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    z = want == 0
    if np.any(got[z] != 0):
        return np.inf
    return float(np.max(np.abs(got[~z] - want[~z]) / want[~z])) if np.any(~z) else 0.0
