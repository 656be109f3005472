"""The z-pass c2r in the forms the library itself launches (zpass_c2r, csrc/pf_api.hip), a few rows at a time through pf_debug_zpass_jobs,
at every line length of tests/test_gpu_lines.py and 128 and 512 -- the line tests reach these kernels with one job, rows of pitch n,
norm = 1 and no DC constant only, whole-box runs at a handful of sizes:
  A  the displacement z-pass: three jobs (one, one, i k) into float rows or packed fp64 rows, spectra at the padded pitch, norm = 1/n^3
     -- the product-row stores of k_c2r, k_c2r_persistent and k_mixed_c2r (one kernel per built-in plan), and tiles of several jobs
     walked by one persistent workgroup
  B  the Hessian z-pass: six jobs, rows at the fields' pitch, a DC constant from device memory, out of place and in place, pruned or not
  C  the 3LPT(b) contraction inside the six-row z-pass (k_c2r_invariants<F, N, 1>, k_mixed_c2r_invariants<F, R0, PLAN, 1>): against the
     definition in longdouble, and bit for bit against the restated accumulation of the six-job output of the same input
  D  the same with the start value formed in the kernel (mode 2, powers of two)
  E  the inverse x-pass with the forward x-transform in front (pf_debug_strided_xfuse): the same bits as the two launches it replaces
References, bounds and comparisons: tests/zpass_forms.py (held to definitions of their own in tests/test_zpass_forms_cpu.py).
Every test prints the ratio of what it measured to its bound (profiles/zpass_forms_notes.md)."""
import numpy as np
import pytest

import band_ladder as B
import test_gpu_lines as TL
import zpass_forms as Z

pytestmark = pytest.mark.gpu

assert sorted(Z.ALL_SIZES) == sorted(TL.SIZES + TL.MIXED + [128, 512])
PAIRS = [(n, fb) for n in Z.ALL_SIZES for fb in (8, 4)]


@pytest.fixture(scope="module")
def L():
    from pinocchio_amd import _lib
    return _lib.load()


def set_persist(monkeypatch, persist):
    if persist == "default":
        monkeypatch.delenv("PF_ZPASS_PERSIST", raising=False)
    else:
        monkeypatch.setenv("PF_ZPASS_PERSIST", persist)


def pruned_band(n):
    """a band of production: the ladder's own where it names one, else that of a six-cell radius (the rule behind the 2048 entry)"""
    if n == 1024:
        return B.PRODUCTION_1024[2]
    if n == 2048:
        return B.PRODUCTION_2048[0]
    band = B.hess_band(n, 6.0)
    assert 1 <= band < n // 2
    return band


_refs = {}


def disp_case(n, fb):
    """inputs and the pocketfft rows of the displacement form, computed once per (n, fb)"""
    if (n, fb) not in _refs:
        x, norm = Z.disp_inputs(n, fb)
        want = np.array([Z.expected_rows(x[j], Z.DISP_MUL[j], n, norm) for j in range(3)])
        want.setflags(write=False)
        _refs[(n, fb)] = (x, norm, want)
    return _refs[(n, fb)]


def hess_case(n, fb, rows, band=1 << 30):
    key = ("h", n, fb, rows, band)
    if key not in _refs:
        x = Z.spectrum_rows(np.random.default_rng(2000 * n + fb + rows), (6, rows), n, fb)
        norm = 1.0 / float(n) ** 3
        dc = float(np.sqrt(n)) * norm                       # of the size of the rows' own amplitude
        want = np.array([Z.expected_rows(x[j], Z.MUL6[j], n, norm, dc, band) for j in range(6)])
        want.setflags(write=False)
        _refs[key] = (x, norm, dc, want)
    return _refs[key]


def report(form, n, fb, **ratios):
    print("RATIO form=%s n=%d fb=%d " % (form, n, fb) + " ".join("%s=%.4g" % kv for kv in sorted(ratios.items())))


# ---- A: the displacement form ----
def check_disp(got, want, n, fb, f32, what):
    worst = {}
    for j in range(3):
        if f32[j] == 1 and fb == 8:
            ulps, frac = Z.check_float_rows(got[j], want[j])
            worst["ulps"], worst["frac_over_cap"] = max(worst.get("ulps", 0), ulps), max(worst.get("frac_over_cap", 0), frac / Z.EXACT_FRAC)
        else:
            if f32[j] == 1:
                assert np.array_equal(got[j], got[j].astype(np.float32).astype(np.float64)), (n, fb, j, "not float values")
            worst["tol"] = max(worst.get("tol", 0), Z.check_rel(got[j], want[j], Z.tol(fb, n)))
    report(what, n, fb, **worst)


@pytest.mark.parametrize("persist", ["default", "0"])
@pytest.mark.parametrize("n,fb", PAIRS)
def test_displacement_form(L, n, fb, persist, monkeypatch):
    """37 rows (the last tile ragged), float rows for both field types and packed fp64 rows for fp64 fields, with the persistent kernel
    (PF_ZPASS_PERSIST at its default) and the one-shot kernel (0)"""
    set_persist(monkeypatch, persist)
    x, norm, want = disp_case(n, fb)
    for f32 in ((1, 1, 1),) + (((2, 2, 2), (1, 2, 1)) if fb == 8 else ()):
        got = Z.zpass(L, fb, n, 0, x, mul=Z.DISP_MUL, f32=f32, norm=norm)
        check_disp(got, want, n, fb, f32, "A%s" % "".join(map(str, f32)))


@pytest.mark.parametrize("n,fb", PAIRS)
def test_displacement_form_with_workgroups_that_walk_tiles_of_several_jobs(L, n, fb, monkeypatch):
    """launch_c2r_n (csrc/pf_fft_kernels.hip): the persistent grid is min(ncu * PF_ZPASS_PERSIST, tiles) workgroups, workgroup b takes the
    tiles b, b + grid, ... and tile t belongs to job t % njobs.  One CU and four workgroups for nine tiles and more of three jobs: workgroup 0
    walks tiles 0, 4, 8 -- jobs 0, 1, 2.  (The one-shot and mixed-radix kernels take one tile per workgroup: several tiles per job here.)"""
    monkeypatch.setenv("PF_ZPASS_PERSIST", "4")
    ncu, grid = 1, 4
    if n & (n - 1) == 0:
        tl, _ = Z.persistent_tiles(n, 1, 3)
    else:
        nt = B.zpass_threads(n)
        tl = max(256 // nt, 1)                             # pf_mixed_rows_per_wg (csrc/pf_mixed_kernels.hip)
    rows = 2 * tl + 1
    ntiles = -(-rows // tl) * 3
    if n & (n - 1) == 0 and n >= 64:
        assert Z.persistent_tiles(n, rows, 3) == (tl, ntiles)
        assert ntiles >= 2 * grid + 1 and grid % 3 != 0    # tiles t and t + grid of a workgroup are of different jobs
    x, norm = Z.disp_inputs(n, fb, rows)
    want = [Z.expected_rows(x[j], Z.DISP_MUL[j], n, norm) for j in range(3)]
    got = Z.zpass(L, fb, n, 0, x, mul=Z.DISP_MUL, f32=(1, 1, 1), norm=norm, ncu=ncu)
    check_disp(got, want, n, fb, (1, 1, 1), "Awalk")


# ---- B: the Hessian form ----
@pytest.mark.parametrize("persist", ["default", "0"])
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("n,fb", PAIRS)
def test_hessian_form(L, n, fb, in_place, persist, monkeypatch):
    """six jobs with the kz factors of hess_yz into rows at the fields' pitch, DC constant, norm = 1/n^3; unpruned and at a band of
    production; the padding of every row as it was (in place: the Nyquist column of the input and the padding behind it)"""
    set_persist(monkeypatch, persist)
    worst = 0.0
    for band in (n, pruned_band(n)):
        x, norm, dc, want = hess_case(n, fb, 37, band)
        got = Z.zpass(L, fb, n, 0, x, mul=Z.MUL6, f32=(0,) * 6, in_place=in_place, band=band, norm=norm, dc=dc)
        for j in range(6):
            worst = max(worst, Z.check_rel(got[j], want[j], Z.tol(fb, n)))
    report("B", n, fb, tol=worst)


@pytest.mark.parametrize("n,fb", [(16, 8), (64, 4), (1024, 8), (2048, 4), (24, 8), (200, 8), (768, 4), (1080, 8)])
def test_jobs_of_both_kinds_in_one_launch(L, n, fb):
    """rows at the fields' pitch and float rows from one launch: the flag is the job's own"""
    x, norm, dc, want = hess_case(n, fb, 37)
    f32 = (0, 1, 0, 1, 1, 0)
    got = Z.zpass(L, fb, n, 0, x, mul=Z.MUL6, f32=f32, norm=norm, dc=dc)
    worst = {}
    for j in range(6):
        if f32[j] == 1 and fb == 8:
            worst["ulps"] = max(worst.get("ulps", 0), Z.check_float_rows(got[j], want[j])[0])
        else:
            worst["tol"] = max(worst.get("tol", 0), Z.check_rel(got[j], want[j], Z.tol(fb, n)))
    report("Bmix", n, fb, **worst)


# ---- C, D: the contraction ----
def contraction_case(L, n, fb, rows, band, hscale=None):
    """-> spectra, norm, dc, the six rows by pocketfft, the six rows by the six-job launch of the same input, h, s0; h of the
    amplitude of the rows, or of hscale(that amplitude)"""
    x, norm, dc, d_ref = hess_case(n, fb, rows, band)
    d_dev = Z.zpass(L, fb, n, 0, x, mul=Z.MUL6, f32=(0,) * 6, band=band, norm=norm, dc=dc)
    amp = float(np.max(np.abs(d_ref)))
    rng = np.random.default_rng(3000 * n + fb)
    hs = amp if hscale is None else hscale(amp)
    h = Z.real_rows(rng, (6, rows, n), fb, hs)
    s0 = Z.real_rows(rng, (rows, n), fb, amp * hs)
    return x, norm, dc, d_ref, d_dev, h, s0


@pytest.mark.parametrize("walk", [False, True])
@pytest.mark.parametrize("n,fb", PAIRS)
def test_contraction_in_the_zpass(L, n, fb, walk, monkeypatch):
    """mode 1 at every (field type, size) with such a kernel; the tap refuses exactly the others (and mode 2 off the powers of two).
    walk: one CU and PF_ZPASS_INV_WG_PER_CU=1 -- one workgroup (powers of two), at most eight (mixed radix: pf_launch_mixed_c2r_invariants
    caps the grid at 8 per CU) -- for 19 rows: every workgroup walks two rows and more"""
    if not Z.supported(fb, n):
        x = Z.spectrum_rows(np.random.default_rng(n), (6, 3), n, fb)
        z = np.zeros((3, n))
        for form in (1, 2):
            rc, _, ok = Z.zpass_rc(L, fb, n, form, x, hess=np.zeros((6, 3, n)), acc=z)
            assert rc != 0 and ok != 1, (n, fb, form)
        return
    rows, ncu = (19, 1) if walk else (5, 0)
    if walk:
        monkeypatch.setenv("PF_ZPASS_INV_WG_PER_CU", "1")
        assert rows >= 2 * 8 + 1
    F = Z.ftype(fb)
    worst = 0.0
    for band in (n, pruned_band(n)):
        x, norm, dc, d_ref, d_dev, h, s0 = contraction_case(L, n, fb, rows, band, None)
        got = Z.zpass(L, fb, n, 1, x, band=band, norm=norm, dc=dc, ncu=ncu, hess=h, acc=s0)   # (h and every padding unchanged: the tap's flag)
        worst = max(worst, Z.check_acc(got, s0, d_ref, h, Z.tol(fb, n)))
        assert Z.same_bits(got, Z.restated_acc(s0, d_dev, h, F)), (n, fb, band, "the accumulation of the six-job rows, bit for bit")
    report("C", n, fb, acc=worst)
    if n & (n - 1):
        rc, _, ok = Z.zpass_rc(L, fb, n, 2, x, hess=h, acc=s0)
        assert rc != 0 and ok != 1, (n, fb, "mode 2 of a mixed-radix size")


@pytest.mark.parametrize("walk", [False, True])
@pytest.mark.parametrize("n,fb", [(n, fb) for n, fb in PAIRS if n & (n - 1) == 0 and Z.supported(fb, n)])
def test_contraction_that_forms_its_start_value(L, n, fb, walk, monkeypatch):
    """mode 2: the source field is written only (it comes in as NaN) -- bit for bit mode 1 started from the restated
    2 (h11 + h22 + h33) S2(h) in the field type, and within the bound of the definition in longdouble"""
    rows, ncu = (19, 1) if walk else (5, 0)
    if walk:
        monkeypatch.setenv("PF_ZPASS_INV_WG_PER_CU", "1")
    F = Z.ftype(fb)
    band = n
    x, norm, dc, d_ref, d_dev, h, _ = contraction_case(L, n, fb, rows, band, np.sqrt)   # h^3 and d h of one size
    got2 = Z.zpass(L, fb, n, 2, x, band=band, norm=norm, dc=dc, ncu=ncu, hess=h, acc=np.full((rows, n), np.nan))
    assert np.all(np.isfinite(got2))
    start = Z.restated_start(h, F).astype(np.float64)
    got1 = Z.zpass(L, fb, n, 1, x, band=band, norm=norm, dc=dc, ncu=ncu, hess=h, acc=start)
    assert Z.same_bits(got2, got1), (n, fb)
    assert Z.same_bits(got2, Z.restated_acc(start, d_dev, h, F)), (n, fb)
    # the bound of mode 1 with the start value from the definition (its own rounding: twelve fp64 operations and the cast, far below tol B)
    s_ld = Z.expected_start(h)
    err = float(np.max(np.abs(got2.astype(np.longdouble) - Z.expected_acc(s_ld, d_ref, h))))
    lim = 2 * Z.tol(fb, n) * float(np.max(Z.acc_scale(s_ld.astype(np.float64), d_ref, h)))
    assert err <= lim, (n, fb, err / lim)
    report("D", n, fb, acc=err / lim)


# ---- E: the fused forward + inverse x-pass ----
XF_PAIRS = [(n, 8) for n in (16, 64, 128, 256, 512, 1024, 2048)] + [(n, 4) for n in (16, 64, 128, 256, 512)]


@pytest.mark.parametrize("n,fb", XF_PAIRS)
def test_fused_x_pass_is_its_two_launches_bit_for_bit(L, n, fb):
    """the two-job displacement form (one, i k; the filter without a window, a growth factor) and the three-job Hessian form (one, k,
    k^2; window and growth) on 21 columns (the last tile ragged) of the outer lines -1 and 0: the k = 0 mode is among them"""
    rng = np.random.default_rng(7 * n + fb)
    x = rng.standard_normal((2, n, 21)) + 1j * rng.standard_normal((2, n, 21))
    if fb == 4:
        x = x.astype(np.complex64).astype(np.complex128)
    for mul, rs, g in (((0, 3), 0.0, 0.37), ((0, 1, 2), 0.5, -0.111)):   # (a window that leaves every mode visible in fp32 too)
        fused, plain = Z.xfuse(L, fb, n, x, mul, 1, rs, g, outer_offset=n - 1)
        assert np.all(np.isfinite(plain.view(np.float64)))
        for j in range(len(mul)):
            assert np.count_nonzero(plain[j]) >= plain[j].size - 21 * 2, (n, fb, mul, j)    # (all but what the filter clears at k = 0)
            assert Z.same_bits(fused[j].view(np.float64), plain[j].view(np.float64)), (n, fb, mul, j)
        assert not np.array_equal(plain[0], plain[1])
    assert not np.array_equal(fused[0], x)
