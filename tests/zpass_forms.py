"""References, comparisons and the tap's wrappers for the z-pass forms the library itself launches (tests/test_gpu_zpass_forms.py, held to
definitions of their own in tests/test_zpass_forms_cpu.py): plain numpy, nothing of the device path.

The forms (zpass_c2r, csrc/pf_api.hip): several jobs in one launch, product rows (float, or packed field-type rows), spectra rows of
nzp = n/2 + 64/fb complex and real rows of 2 nzp, norm = 1/n^3, a DC constant from device memory, in place or not, and the 3LPT(b)
contraction inside the six-row z-pass (pf_launch_c2r_invariants, mode 1: acc -= 2 phi2_ab h_ab; mode 2: acc formed from h first)."""
import ctypes as C

import numpy as np

MUL6 = (0, 0, 2, 0, 1, 1)          # the kz factors of the six components 11, 22, 33, 12, 13, 23 (hess_yz, csrc/pf_api.hip)
ORDER = (0, 3, 4, 1, 5, 2)         # the reference's order 11, 12, 13, 22, 23, 33 in storage indices (src/LPT.c:134-137)
FACTOR = (2.0, 2.0, 2.0, 4.0, 4.0, 4.0)
EXACT_FRAC = 1e-3                  # float rows: cells that may differ from the rounded reference (the cap of tests/test_lpt_analytic.py)


def signed(n):
    e = np.arange(n)
    return np.where(e > n // 2, e - n, e).astype(np.float64)  # Nyquist stays +n/2 (src/fmax-pfft.c:306-339)


def kfactor(mul, k):
    return {0: np.ones_like(k) + 0j, 1: k + 0j, 2: k * k + 0j, 3: 1j * k}[mul]


def tol(fb, n):
    """the bound of the line tests (tests/test_gpu_lines.py), relative to max |want|"""
    return (2e-15 if fb == 8 else 1e-6) * np.log2(n)


def ftype(fb):
    return np.float64 if fb == 8 else np.float32


def nzp(fb, n):
    """complex columns of a spectrum row on the device (csrc/pf_api.hip: whole 128-byte lines)"""
    return n // 2 + 64 // fb


# ---- references ----
def expected_rows(x, mul, n, norm=1.0, dc=0.0, band=1 << 30, irfft=np.fft.irfft):
    """x: [..., n/2+1] Hermitian rows -> [..., n] real rows: columns above `band` are zeros, the factor `mul` in kz, pocketfft's inverse
    (which divides by n: the library's does not), norm and the DC constant"""
    h = n // 2 + 1
    kz = 2 * np.pi / n * np.arange(h)
    xb = np.where(np.arange(h) <= band, x, 0) if band < n // 2 else x
    return irfft(xb * kfactor(mul, kz), n=n, axis=-1) * n * norm + dc


def dft_rows(x, mul, n, norm=1.0, dc=0.0, band=1 << 30):
    """expected_rows from the definition, O(n^2) in longdouble: r[c] = sum over the n signed wavenumbers of X[s] exp(2 pi i s c / n), with
    X[-s] = conj(X[s]) and only the real parts of X[0] and X[n/2]"""
    LD, h = np.longdouble, n // 2 + 1
    x = np.asarray(x)
    kz = 2 * np.pi / LD(n) * np.arange(h).astype(LD)
    f = {0: (np.ones(h, LD), np.zeros(h, LD)), 1: (kz, np.zeros(h, LD)), 2: (kz * kz, np.zeros(h, LD)), 3: (np.zeros(h, LD), kz)}[mul]
    keep = (np.arange(h) <= band) if band < n // 2 else np.ones(h, bool)
    re = (x.real.astype(LD) * f[0] - x.imag.astype(LD) * f[1]) * keep
    im = (x.real.astype(LD) * f[1] + x.imag.astype(LD) * f[0]) * keep
    # exact angles: (s c) mod n before the multiplication by 2 pi / n
    ang = 2 * np.pi / LD(n) * ((np.arange(h)[:, None] * np.arange(n)[None, :]) % n).astype(LD)
    w = np.full(h, 2.0, LD)
    w[0] = 1.0
    w[n // 2] = 1.0
    im = im.copy()
    im[..., 0] = 0
    im[..., n // 2] = 0
    r = (re * w) @ np.cos(ang) - (im * w) @ np.sin(ang)
    return r * LD(norm) + LD(dc)


def expected_acc(s0, d, h):
    """s0 - sum_c f_c d_c h_c in longdouble (f = 2 on the diagonal, 4 off it); d, h: [6][...]"""
    LD = np.longdouble
    s = np.asarray(s0).astype(LD)
    for c in range(6):
        s = s - LD(FACTOR[c]) * np.asarray(d[c]).astype(LD) * np.asarray(h[c]).astype(LD)
    return s


def acc_scale(s0, d, h):
    """B = |s0| + sum_c f_c |d_c| |h_c| per cell: what the errors of the contraction are relative to"""
    b = np.abs(np.asarray(s0, dtype=np.float64))
    for c in range(6):
        b = b + FACTOR[c] * np.abs(d[c]) * np.abs(h[c])
    return b


def restated_acc(s0, d, h, F):
    """pf_lpt3b_accumulate (csrc/pf_collapse_core.h) operation by operation in float64 -- the reference's order of the components, the
    factor times phi2 first, then times h, one subtraction each, nothing fused -- and the kernel's cast to the field type"""
    s = np.asarray(s0, dtype=np.float64).copy()
    for c in ORDER:
        f = 2.0 * (1.0 if c < 3 else 2.0)
        s = s - (f * np.asarray(d[c], dtype=np.float64)) * np.asarray(h[c], dtype=np.float64)
    return s.astype(F)


def restated_start(h, F):
    """src32 of pf_lpt_sources_cell (csrc/pf_collapse_core.h): 2 (h11 + h22 + h33) S2(h), the same way; cast to the field type"""
    d = [np.asarray(v, dtype=np.float64) for v in h]
    src2 = ((((d[0] * d[1] + d[0] * d[2]) + d[1] * d[2]) - d[3] * d[3]) - d[4] * d[4]) - d[5] * d[5]
    return ((2.0 * ((d[0] + d[1]) + d[2])) * src2).astype(F)


def expected_start(h):
    LD = np.longdouble
    d = [np.asarray(v).astype(LD) for v in h]
    src2 = d[0] * d[1] + d[0] * d[2] + d[1] * d[2] - d[3] * d[3] - d[4] * d[4] - d[5] * d[5]
    return 2 * (d[0] + d[1] + d[2]) * src2


# ---- which sizes have a contracting z-pass: pf_c2r_invariants_supported (csrc/pf_fft_kernels.hip, csrc/pf_mixed_kernels.hip) ----
def radices(n, allow4):
    """pf_radices: the stage plan of n points, or None"""
    r0 = 8 if n % 8 == 0 else (4 if allow4 and n % 4 == 0 else 0)
    if not r0 or n < r0:
        return None
    rest, r = n // r0, [r0]
    while rest % 8 == 0:
        r.append(8)
        rest //= 8
    if rest % 4 == 0:
        r.append(4)
        rest //= 4
    if rest % 2 == 0:
        r.append(2)
        rest //= 2
    for q in (5, 3):
        while rest % q == 0:
            r.append(q)
            rest //= q
    return r if rest == 1 and len(r) <= 12 else None


def supported(fb, n):
    if n & (n - 1) == 0:
        return 16 <= n <= (1024 if fb == 8 else 2048)   # (the six lines of a 2048-point fp64 row do not fit a workgroup's LDS)
    if not (8 <= n <= 2048 and n % 8 == 0 and radices(n, False) and radices(n // 2, True)):   # pf_mixed_supported
        return False
    nt = (n // 2) // radices(n // 2, True)[0]
    return 6 * nt <= 1024 and 6 * (n // 2 + 1) * (16 if fb == 8 else 8) <= 128 * 1024


# ---- launch rules a test sizes its rows by ----
def persistent_tiles(n, nrows, njobs):
    """launch_c2r_n (csrc/pf_fft_kernels.hip): rows per tile TL = 256 / NT with NT = n / 16 threads per row (one row from 4096 points on),
    tiles = ceil(nrows / TL) * njobs, tile t is job t % njobs; the persistent kernel serves n >= 64"""
    nt = n // 16
    tl = 1 if nt >= 256 else 256 // nt
    return tl, -(-nrows // tl) * njobs


# ---- comparisons ----
def check_rel(got, want, bound):
    err, amp = np.max(np.abs(got - want)), np.max(np.abs(want))
    assert err <= bound * amp, (float(err / amp), bound)
    return float(err / amp / bound)


def check_float_rows(got, want):
    """float product rows of fp64 fields: within one fp32 ulp of the rounded reference everywhere, the rounded reference itself on all but
    EXACT_FRAC of the cells.  Returns (worst ulps, fraction differing)"""
    w32 = np.asarray(want).astype(np.float32)
    g32 = np.asarray(got).astype(np.float32)
    assert np.array_equal(g32.astype(np.float64), np.asarray(got, dtype=np.float64)), "not float values"
    ulp = np.spacing(np.abs(w32)).astype(np.float64)
    ulps = float(np.max(np.abs(g32.astype(np.float64) - w32.astype(np.float64)) / ulp))
    frac = float(np.mean(g32 != w32))
    assert ulps <= 1.0, ulps
    assert frac <= EXACT_FRAC, frac
    return ulps, frac


def check_acc(got, s0, d, h, bound):
    """|got - expected_acc| <= 2 bound max(B): one bound B for the transforms' error carried through the six products, a second one above
    the thirteen fp64 operations and the rounding to the field type"""
    want = expected_acc(s0, d, h)
    err = float(np.max(np.abs(np.asarray(got).astype(np.longdouble) - want)))
    lim = 2 * bound * float(np.max(acc_scale(s0, d, h)))
    assert err <= lim, (err / lim,)
    return err / lim


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- sizes and inputs ----
POW2 = [16, 64, 128, 256, 512, 1024, 2048]
MIXED = [24, 40, 96, 120, 200, 384, 768, 1000, 1536, 400, 640, 800, 1280, 1600, 2000, 144, 360, 720, 1080, 1440, 1800, 1944]
ALL_SIZES = POW2 + MIXED           # SIZES + MIXED of tests/test_gpu_lines.py, and 128 and 512
DISP_MUL = (0, 0, 3)               # the displacement z-pass: one, one, i k
DISP_ROWS = 37


def disp_inputs(n, fb, rows=DISP_ROWS):
    """the spectra of the displacement form's tests, and its norm"""
    return spectrum_rows(np.random.default_rng(1000 * n + fb), (3, rows), n, fb), 1.0 / float(n) ** 3



def spectrum_rows(rng, shape, n, fb):
    """random Hermitian rows [shape..., n/2+1] with real DC and Nyquist columns, exactly representable in the field type"""
    h = n // 2 + 1
    x = rng.standard_normal(tuple(shape) + (h,)) + 1j * rng.standard_normal(tuple(shape) + (h,))
    x[..., 0] = x[..., 0].real
    x[..., n // 2] = x[..., n // 2].real
    return x.astype(np.complex64).astype(np.complex128) if fb == 4 else x


def real_rows(rng, shape, fb, scale=1.0):
    return (scale * rng.standard_normal(shape)).astype(ftype(fb)).astype(np.float64)


# ---- the tap ----
def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def zpass_rc(L, fb, n, form, x, mul=(), f32=(), in_place=False, band=1 << 30, norm=1.0, dc=None, ncu=0, hess=None, acc=None):
    """pf_debug_zpass_jobs -> (return code, rows, sentinels intact)"""
    x = np.ascontiguousarray(x, dtype=np.complex128)
    njobs, nrows = x.shape[0], x.shape[1]
    assert x.shape[2] == n // 2 + 1
    mul_a, f32_a = np.asarray(mul, dtype=np.int32), np.asarray(f32, dtype=np.int32)
    out = np.zeros((njobs, nrows, n) if form == 0 else (nrows, n))
    if form:
        hess, acc = np.ascontiguousarray(hess, dtype=np.float64), np.ascontiguousarray(acc, dtype=np.float64)
        assert hess.shape == (6, nrows, n) and acc.shape == (nrows, n) and njobs == 6
    else:
        assert len(mul_a) == len(f32_a) == njobs
    dcv = None if dc is None else np.array([dc], dtype=np.float64)
    ok = C.c_int(-1)
    rc = L.pf_debug_zpass_jobs(fb, n, form, njobs, _ip(mul_a), _ip(f32_a), int(in_place), nrows, band, norm, _dp(dcv), ncu, _dp(x.view(np.float64)),
                               _dp(hess), _dp(acc), _dp(out), C.byref(ok))
    return rc, out, ok.value


def zpass(L, *a, **k):
    rc, out, ok = zpass_rc(L, *a, **k)
    assert rc == 0, L.pf_last_error()
    assert ok == 1, "a row's padding, a guard region or a read-only field changed"
    return out


def xfuse(L, fb, n, x, mul, pre, rs, growth, outer_offset=0):
    """pf_debug_strided_xfuse: x [nouter][n][ncols] -> (fused, forward then plain inverse), each [njobs][nouter][n][ncols]"""
    x = np.ascontiguousarray(x, dtype=np.complex128)
    nouter, ncols = x.shape[0], x.shape[2]
    mul_a = np.asarray(mul, dtype=np.int32)
    a, b = (np.zeros((len(mul_a),) + x.shape, dtype=np.complex128) for _ in range(2))
    rc = L.pf_debug_strided_xfuse(fb, n, len(mul_a), _ip(mul_a), nouter, ncols, pre, rs, growth, outer_offset, _dp(x.view(np.float64)),
                                  _dp(a.view(np.float64)), _dp(b.view(np.float64)))
    assert rc == 0, L.pf_last_error()
    return a, b
