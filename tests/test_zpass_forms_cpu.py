"""tests/zpass_forms.py held to definitions of its own, without a device: expected_rows against an O(n^2) longdouble DFT, the float64
restatements of the contraction against the host compilation of csrc/pf_collapse_core.h (tests/cpu_emul/zpass_forms_emul.cpp, also as
a program under -fsanitize=address,undefined), supported() against what DESIGN.md states, the float-row criterion against a second
independent transform, and every comparison against planted errors it has to reject."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.fft

import zpass_forms as Z

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "cpu_emul", "zpass_forms_emul.cpp")
SO = os.path.join(HERE, "cpu_emul", "libzpass_forms_emul.so")
EXE = os.path.join(HERE, "cpu_emul", "zpass_forms_emul_san")
HDRS = [os.path.join(ROOT, "pinocchio_amd", "csrc", "pf_collapse_core.h")]
CELLS = 10 ** 4


def _stale(product):
    return not os.path.exists(product) or any(os.path.getmtime(product) < os.path.getmtime(s) for s in [SRC] + HDRS)


@pytest.fixture(scope="module")
def emul():
    if _stale(SO):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DZF_EMUL_LIB", "-o", SO, SRC])
    L = C.CDLL(SO)
    dp = C.POINTER(C.c_double)
    L.zf_emul_acc.restype = L.zf_emul_start.restype = C.c_int
    L.zf_emul_acc.argtypes = [C.c_int, C.c_long, dp, dp, dp, dp]
    L.zf_emul_start.argtypes = [C.c_int, C.c_long, dp, dp]
    return L


def cells(fb, seed=5):
    """s0, d[6], h[6] of CELLS cells in the field type, magnitudes spread over six decades, some zeros and equal components"""
    rng = np.random.default_rng(seed + fb)
    F = Z.ftype(fb)
    mag = 10.0 ** rng.uniform(-3, 3, size=(13, CELLS))
    v = (rng.standard_normal((13, CELLS)) * mag).astype(F).astype(np.float64)
    v[:, :50] = 0.0
    v[1:7, 50:100] = v[1, 50:100]
    return np.ascontiguousarray(v[0]), np.ascontiguousarray(v[1:7]), np.ascontiguousarray(v[7:13])


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


@pytest.mark.parametrize("n", [16, 24, 40])
def test_expected_rows_against_the_definition(n):
    rng = np.random.default_rng(n)
    x = Z.spectrum_rows(rng, (5,), n, 8)
    x[0, 0] += 0.3j          # junk imaginary parts in the DC and Nyquist columns are ignored by both
    x[0, n // 2] -= 0.7j
    for mul in (0, 1, 2, 3):
        for band, norm, dc in ((1 << 30, 1.0, 0.0), (n // 2, 1.0 / n ** 3, 0.4 / n ** 2.5), (n // 3, 1.0 / n ** 3, -1.1 / n ** 2.5), (1, 2.5, 0.0)):
            got = Z.expected_rows(x, mul, n, norm, dc, band)
            want = Z.dft_rows(x, mul, n, norm, dc, band)
            assert got.shape == (5, n)
            # pocketfft in float64 and three more roundings per value: a quarter of what the kernels are allowed
            assert np.max(np.abs(got - want)) <= 0.25 * Z.tol(8, n) * float(np.max(np.abs(want))), (n, mul, band)
    # the band really cuts: one mode above it changes nothing, one inside it does
    y = x.copy()
    y[:, n // 3 + 1] += 1.0
    assert np.array_equal(Z.expected_rows(y, 1, n, band=n // 3), Z.expected_rows(x, 1, n, band=n // 3))
    y[:, n // 3] += 1.0
    assert not np.array_equal(Z.expected_rows(y, 1, n, band=n // 3), Z.expected_rows(x, 1, n, band=n // 3))


@pytest.mark.parametrize("fb", [8, 4])
def test_restatements_are_the_host_compilation_bit_for_bit(emul, fb):
    s0, d, h = cells(fb)
    out = np.zeros(CELLS)
    assert emul.zf_emul_acc(fb, CELLS, _p(s0), _p(d), _p(h), _p(out)) == 0
    assert Z.same_bits(out, Z.restated_acc(s0, d, h, Z.ftype(fb)).astype(np.float64))
    assert emul.zf_emul_start(fb, CELLS, _p(h), _p(out)) == 0
    assert Z.same_bits(out, Z.restated_start(h, Z.ftype(fb)).astype(np.float64))
    # ... and both are the definitions to rounding: 13 / 12 operations of half an ulp each on terms of size B, and the cast
    eps = np.finfo(Z.ftype(fb)).eps
    acc = Z.restated_acc(s0, d, h, Z.ftype(fb)).astype(np.longdouble)
    assert np.all(np.abs(acc - Z.expected_acc(s0, d, h)) <= (13 * 2.0 ** -53 + 0.5 * eps) * Z.acc_scale(s0, d, h) * 1.0000001)
    st = Z.restated_start(h, Z.ftype(fb)).astype(np.longdouble)
    tr, s2 = np.abs(h[0]) + np.abs(h[1]) + np.abs(h[2]), sum(np.abs(h[a]) * np.abs(h[b]) for a, b in ((0, 1), (0, 2), (1, 2), (3, 3), (4, 4), (5, 5)))
    assert np.all(np.abs(st - Z.expected_start(h)) <= (16 * 2.0 ** -53 + 0.5 * eps) * 2 * tr * s2 * 1.0000001)


@pytest.mark.parametrize("fb", [8, 4])
def test_program_under_sanitizers(emul, fb, tmp_path):
    if _stale(EXE):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-o", EXE, SRC])
    s0, d, h = cells(fb, seed=9)
    with open(tmp_path / "in.bin", "wb") as fh:
        np.array([fb, CELLS], dtype=np.int64).tofile(fh)
        for a in (s0, d, h):
            a.tofile(fh)
    out = subprocess.run([EXE, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and out.stdout.split() == ["cells", str(CELLS)] and "ERROR" not in out.stderr
    got = np.fromfile(tmp_path / "out.bin", dtype=np.float64).reshape(2, CELLS)
    assert Z.same_bits(got[0], Z.restated_acc(s0, d, h, Z.ftype(fb)).astype(np.float64))
    assert Z.same_bits(got[1], Z.restated_start(h, Z.ftype(fb)).astype(np.float64))


def test_supported_is_what_the_design_states():
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        m = re.search(r"built into the kernels for ((?:\d+, )+\d+ and \d+)", fh.read())
    built_in = [int(v) for v in re.findall(r"\d+", m.group(1))]
    assert built_in == [200, 384, 400, 640, 768, 800, 1000, 1280, 1536, 1600, 2000]
    assert all(Z.supported(8, n) for n in built_in)
    # the power-of-two limits, and the two sizes of the line tests whose six lines need more than 1024 threads (first radix 4)
    assert [n for n in Z.POW2 if not Z.supported(8, n)] == [2048] and all(Z.supported(4, n) for n in Z.POW2)
    assert [n for n in Z.MIXED if not Z.supported(8, n)] == [1800, 1944] == [n for n in Z.MIXED if not Z.supported(4, n)]
    assert Z.radices(900, True) == [4, 5, 5, 3, 3] and Z.radices(768, True) == [8, 8, 4, 3] and Z.radices(1000, True) == [8, 5, 5, 5]
    assert Z.radices(12, False) is None and Z.radices(14, True) is None and not Z.supported(8, 20) and not Z.supported(8, 2056)


def test_persistent_tile_rule():
    assert Z.persistent_tiles(64, 37, 3) == (64, 3) and Z.persistent_tiles(1024, 37, 3) == (4, 30) and Z.persistent_tiles(2048, 5, 6) == (2, 18)


def test_two_independent_transforms_round_to_the_same_floats():
    """the float rows are held to float32(numpy's float64 result) on all but EXACT_FRAC of the cells: a second reference -- scipy's
    pocketfft in longdouble -- rounds to other floats on far fewer cells than that, so the cap is not spent on the reference"""
    differ = total = 0
    for n in Z.ALL_SIZES:
        x, norm = Z.disp_inputs(n, 8)
        for j, mul in enumerate(Z.DISP_MUL):
            a = Z.expected_rows(x[j], mul, n, norm)
            b = Z.expected_rows(x[j].astype(np.clongdouble), mul, n, np.longdouble(norm), irfft=scipy.fft.irfft)
            assert b.dtype == np.longdouble
            differ += int(np.sum(a.astype(np.float32) != b.astype(np.float32)))
            total += a.size
            assert np.max(np.abs(a - b)) <= 0.25 * Z.tol(8, n) * float(np.max(np.abs(b)))
    print("cells", total, "rounded differently", differ)
    assert differ <= 1e-2 * Z.EXACT_FRAC * total


# ---- planted errors: each comparison rejects what it is there to catch ----
def _hessian_case(n=40, fb=8, rows=5, seed=3):
    rng = np.random.default_rng(seed)
    x = Z.spectrum_rows(rng, (6, rows), n, fb)
    norm = 1.0 / n ** 3
    dc = float(np.sqrt(n)) * norm
    return x, norm, dc


@pytest.mark.parametrize("fb", [8, 4])
def test_rows_comparison_rejects_planted_errors(fb):
    n = 40
    x, norm, dc = _hessian_case(n, fb)
    want = np.array([Z.expected_rows(x[j], Z.MUL6[j], n, norm, dc) for j in range(6)])
    good = want.astype(Z.ftype(fb)).astype(np.float64)
    for j in range(6):
        Z.check_rel(good[j], want[j], Z.tol(fb, n))
    with pytest.raises(AssertionError):      # the DC constant left out
        Z.check_rel(Z.expected_rows(x[0], 0, n, norm, 0.0), want[0], Z.tol(fb, n))
    with pytest.raises(AssertionError):      # norm left out
        Z.check_rel(Z.expected_rows(x[0], 0, n, 1.0, dc), want[0], Z.tol(fb, n))
    shifted = good[3].copy()
    shifted[2] = np.roll(shifted[2], 1)      # one row shifted by one element
    with pytest.raises(AssertionError):
        Z.check_rel(shifted, want[3], Z.tol(fb, n))
    swapped = good[1].copy()
    swapped[[1, 2]] = swapped[[2, 1]]        # two rows of a job exchanged
    with pytest.raises(AssertionError):
        Z.check_rel(swapped, want[1], Z.tol(fb, n))
    for muls in (Z.MUL6, Z.DISP_MUL):        # job j with job j + 1's factor: some job of the launch is off
        k = len(muls)
        rejected = 0
        for j in range(k):
            w = Z.expected_rows(x[j], muls[j], n, norm, dc)
            try:
                Z.check_rel(Z.expected_rows(x[j], muls[(j + 1) % k], n, norm, dc), w, Z.tol(fb, n))
            except AssertionError:
                rejected += 1
        assert rejected == sum(muls[j] != muls[(j + 1) % k] for j in range(k)) > 0
    # ... and job j with job j + 1's input
    with pytest.raises(AssertionError):
        Z.check_rel(Z.expected_rows(x[1], 0, n, norm, dc), want[0], Z.tol(fb, n))


def test_float_rows_comparison_rejects_planted_errors():
    n = 200
    x, norm = Z.disp_inputs(n, 8)
    want = Z.expected_rows(x[2], 3, n, norm)
    good = want.astype(np.float32)
    assert Z.check_float_rows(good.astype(np.float64), want) == (0.0, 0.0)
    w = good[7].astype(np.float64)
    trunc = good.copy()
    trunc[7] = np.where(np.abs(w) > np.abs(want[7]), np.nextafter(good[7], np.float32(0)), good[7])   # one row of 37 rounded toward zero
    assert 0.3 * n < np.sum(trunc[7] != good[7]) < 0.7 * n
    with pytest.raises(AssertionError):
        Z.check_float_rows(trunc.astype(np.float64), want)
    two = good.copy()
    two[0, 0] = np.nextafter(np.nextafter(good[0, 0], np.float32(np.inf)), np.float32(np.inf))          # one cell two ulps off
    with pytest.raises(AssertionError):
        Z.check_float_rows(two.astype(np.float64), want)
    with pytest.raises(AssertionError):      # fp64 values where floats belong
        Z.check_float_rows(want, want)
    shifted = good.copy()
    shifted[3] = np.roll(shifted[3], 1)
    with pytest.raises(AssertionError):
        Z.check_float_rows(shifted.astype(np.float64), want)


@pytest.mark.parametrize("fb", [8, 4])
def test_contraction_comparison_rejects_planted_errors(fb):
    n, rows = 40, 5
    F = Z.ftype(fb)
    x, norm, dc = _hessian_case(n, fb, rows)
    rng = np.random.default_rng(8)
    d = np.array([Z.expected_rows(x[j], Z.MUL6[j], n, norm, dc) for j in range(6)]).astype(F).astype(np.float64)
    amp = float(np.max(np.abs(d)))
    h = Z.real_rows(rng, (6, rows, n), fb, amp)
    s0 = Z.real_rows(rng, (rows, n), fb, amp * amp)
    good = Z.restated_acc(s0, d, h, F).astype(np.float64)
    assert Z.check_acc(good, s0, d, h, Z.tol(fb, n)) < 0.5
    half = s0.copy()
    for c in range(6):                       # the off-diagonal factor 2 instead of 4
        half = half - 2.0 * d[c] * h[c]
    with pytest.raises(AssertionError):
        Z.check_acc(half.astype(F).astype(np.float64), s0, d, h, Z.tol(fb, n))
    one = s0.copy()
    for c in range(6):                       # ... of one component only
        one = one - (2.0 if c == 4 else Z.FACTOR[c]) * d[c] * h[c]
    with pytest.raises(AssertionError):
        Z.check_acc(one.astype(F).astype(np.float64), s0, d, h, Z.tol(fb, n))
    with pytest.raises(AssertionError):      # the start value not read
        Z.check_acc(Z.restated_acc(0 * s0, d, h, F).astype(np.float64), s0, d, h, Z.tol(fb, n))
    with pytest.raises(AssertionError):      # d without its DC constant
        d0 = np.array([Z.expected_rows(x[j], Z.MUL6[j], n, norm, 0.0) for j in range(6)])
        Z.check_acc(Z.restated_acc(s0, d0, h, F).astype(np.float64), s0, d, h, Z.tol(fb, n))
    shifted = good.copy()
    shifted[1] = np.roll(shifted[1], 1)
    with pytest.raises(AssertionError):
        Z.check_acc(shifted, s0, d, h, Z.tol(fb, n))
    # the tie is stricter still: one ulp of one cell
    bad = good.copy()
    bad[2, 3] = np.nextafter(F(bad[2, 3]), F(np.inf))
    assert Z.same_bits(good, good.copy()) and not Z.same_bits(bad, good)
