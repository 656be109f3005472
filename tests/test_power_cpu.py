"""The power-spectrum pass without a device: the per-mode arithmetic of the device path (pinocchio_amd/csrc/pf_power_core.h,
compiled for the host in tests/cpu_emul/power_emul.cpp) against the numpy restatement of the definitions (tests/np_power.py) on the
planted spectra of tests/power_cases.py and on random half-spectra; the restatement itself against the analytic spectrum of the
restated generator and against Parseval.  The same file as a program reads the cases under -fsanitize=address,undefined."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import np_power as npp
import power_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "cpu_emul", "power_emul.cpp")
SO = os.path.join(HERE, "cpu_emul", "libpower_emul.so")
EXE = os.path.join(HERE, "cpu_emul", "power_emul_san")
HDRS = [os.path.join(ROOT, "pinocchio_amd", "csrc", "pf_power_core.h"), os.path.join(ROOT, "include", "pinfmax.h")]
RADII = (4.0, 1.5, 0.0)
# tests/test_gpu_power.py holds the device to the same two figures; where they come from is said there
TOL_POWER, TOL_VARIANCE = 1e-14, 1e-13


class Info(C.Structure):   # (this test's own statement of pf_power_info; the package's is held against the header in test_abi_power.py)
    _fields_ = [("modes", C.c_ulonglong), ("nonfinite", C.c_ulonglong)]


def _stale(product):
    return not os.path.exists(product) or any(os.path.getmtime(product) < os.path.getmtime(s) for s in [SRC] + HDRS)


@pytest.fixture(scope="module")
def emul():
    if _stale(SO):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DPOWER_EMUL_LIB", "-o", SO, SRC])
    L = C.CDLL(SO)
    vp = C.c_void_p
    L.power_emul_modes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.power_emul_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, C.POINTER(Info)]
    return L


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def emul_modes(L, spec, y0=0, fb=8):
    spec = np.ascontiguousarray(spec, dtype=np.complex128)
    nyl, n = spec.shape[:2]
    sh, w = np.zeros(spec.shape, np.int32), np.zeros(spec.shape, np.int32)
    k2, t = np.zeros(spec.shape, np.uint64), np.zeros(spec.shape)
    assert L.power_emul_modes(fb, n, y0, nyl, _vp(spec), _vp(sh), _vp(w), _vp(k2), _vp(t)) == 0
    return sh, w, k2, t


def emul_run(L, spec, y0=0, fb=8, radii=RADII):
    spec = np.ascontiguousarray(spec, dtype=np.complex128)
    nyl, n = spec.shape[:2]
    nb = L.power_emul_bins(n)
    r = np.ascontiguousarray(radii, dtype=np.float64)
    nm, ks = np.zeros(nb + 1, np.uint64), np.zeros(nb + 1, np.uint64)
    pw, var = np.zeros(nb + 1), np.zeros(len(r) + 1)
    for a in (nm, ks):
        a[-1] = 0xABCDEF    # the element behind every output stays as it is
    pw[-1] = var[-1] = 123.5
    info = Info()
    assert L.power_emul_run(fb, n, y0, nyl, _vp(spec), len(r), _vp(r), _vp(nm), _vp(ks), _vp(pw), _vp(var), C.byref(info)) == 0
    assert nm[-1] == ks[-1] == 0xABCDEF and pw[-1] == var[-1] == 123.5
    return {"nmodes": nm[:-1], "k2sum": ks[:-1], "power": pw[:-1], "variance": var[:-1], "modes": int(info.modes), "nonfinite": int(info.nonfinite)}


def check(got, want, what):
    assert np.array_equal(got["nmodes"], want["nmodes"]) and np.array_equal(got["k2sum"], want["k2sum"]), what
    assert (got["modes"], got["nonfinite"]) == (want["modes"], want["nonfinite"]), what
    rp, rv = npp.rel(got["power"], want["power"]), npp.rel(got["variance"], want["variance"])
    print(what, "power", rp, "variance", rv)
    assert rp <= TOL_POWER and rv <= TOL_VARIANCE, (what, rp, rv)


def test_bins_against_the_integer_definition(emul):
    for n in range(4, 2049):
        b = emul.power_emul_bins(n) - 1
        assert (2 * b - 1) ** 2 <= 3 * n * n < (2 * b + 1) ** 2, n
        assert b + 1 == npp.bins(n)
    assert emul.power_emul_bins(16) == 15


@pytest.mark.parametrize("n,seed", [(16, 1), (20, 2)])
@pytest.mark.parametrize("fb", [8, 4])
def test_every_mode_of_a_random_half_spectrum(emul, n, seed, fb):
    spec = pc.random_box(seed, n)
    for y0, nyl in ((0, n), (n // 2 - 2, 5)):
        sh, w, k2, t = emul_modes(emul, spec[y0:y0 + nyl], y0, fb)
        gk2, gsh, gw = npp.geometry(n, y0, nyl)
        assert np.array_equal(sh, gsh) and np.array_equal(w, gw) and np.array_equal(k2.astype(np.int64), gk2)
        assert np.array_equal(t.view(np.uint64), npp.terms(spec[y0:y0 + nyl], fb).view(np.uint64))   # the bits of re*re + im*im
        assert sh.max() < npp.bins(n)
    out = emul_run(emul, spec, 0, fb)
    assert int(out["nmodes"].sum()) == n ** 3 == out["modes"]
    check(out, npp.power(spec, 0, RADII, fb), (n, fb))
    halves = [emul_run(emul, spec[a:a + n // 2], a, fb) for a in (0, n // 2)]
    both = npp.add(halves)
    assert np.array_equal(both["nmodes"], out["nmodes"]) and np.array_equal(both["k2sum"], out["k2sum"])
    assert npp.rel(both["power"], out["power"]) <= TOL_POWER and npp.rel(both["variance"], out["variance"]) <= TOL_VARIANCE


CASES = [c[0] for c in pc.cases()]


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("fb", [8, 4])
def test_planted_cases(emul, name, fb):
    _, spec, expect = next(c for c in pc.cases() if c[0] == name)
    sh, w, k2, t = emul_modes(emul, spec, 0, fb)
    gk2, gsh, gw = npp.geometry(pc.N)
    assert np.array_equal(sh, gsh) and np.array_equal(w, gw) and np.array_equal(k2.astype(np.int64), gk2)
    assert np.array_equal(t.view(np.uint64), npp.terms(spec, fb).view(np.uint64))
    got, want = emul_run(emul, spec, 0, fb), npp.power(spec, 0, RADII, fb)
    check(got, want, (name, fb))
    assert int(got["nmodes"].sum()) == pc.N ** 3
    if expect is not None:   # what the case was planted for, said without either implementation
        b, wt, kk, term = expect
        iy, ix, iz = (int(v[0]) for v in np.nonzero(spec))
        assert (int(sh[iy, ix, iz]), int(w[iy, ix, iz]), int(k2[iy, ix, iz])) == (b, wt, kk)
        exp = np.zeros(npp.bins(pc.N))
        exp[b] = wt * term / float(pc.N ** 6)
        assert np.array_equal(got["power"], exp) and np.array_equal(want["power"], exp)   # one term: no rounding in any order
    if name == "all_ones":
        assert np.array_equal(got["power"], 2.0 * got["nmodes"].astype(np.float64) / float(pc.N ** 6))
    if name == "nan_and_inf":
        assert got["nonfinite"] == 4 and np.all(np.isfinite(got["power"])) and np.all(np.isfinite(got["variance"]))
    if name == "minus_zero":
        assert np.count_nonzero(got["power"]) == 1 and got["nonfinite"] == 0
    if name == "subnormal_parts":
        assert np.count_nonzero(got["power"]) == 2   # (the subnormal square vanishes under 1 / N^6; with fp32 fields it arrives as zero)


def test_the_restatement_on_the_generators_own_spectrum():
    """FixedIC: every mode the restated generator writes has |delta_k|^2 / N^6 = PkNorm P_EH(k) / Box^3, so the shell sums of the
    restatement are those of the analytic spectrum over the modes the generator leaves non-zero"""
    import ic_oracle
    p = {"Omega0": 0.25, "OmegaBaryon": 0.044, "Hubble100": 0.7, "PrimordialIndex": 0.96}
    n, box, pkn = 16, 16.0 / 0.7, 1.7e7
    dk = ic_oracle.genic(n, box, 7, pkn, p, fixed=True)       # [kx][ky][kz]
    got = npp.power(npp.from_x_slab(dk))
    want = analytic_shell_sums(n, box, pkn, dk != 0, eh_of(p))
    assert np.count_nonzero(want) >= 8 and got["nonfinite"] == 0
    r = npp.rel(got["power"], want)
    print("restatement against the analytic shell sums:", r)
    assert r <= 1e-12


def eh_of(p):
    import ic_oracle
    L = ic_oracle._lib()
    cos = ic_oracle.Cosmo(p["Omega0"], p["OmegaBaryon"], p["Hubble100"], p["PrimordialIndex"])
    return lambda k: L.orc_powerspec_EH(float(k), C.byref(cos))


def analytic_shell_sums(n, box, pknorm, nonzero_xyz, pk):
    """sum over the shell of w PkNorm P(k) / Box^3, k as the generator forms it (src/GenIC.c: the components times 2 pi / Box, then
    the root of the sum of squares), over the modes of the mask [kx][ky][kz]"""
    k2, sh, w = npp.geometry(n)                                # [ky][kx][kz]
    mask = np.transpose(nonzero_xyz, (1, 0, 2))
    sy = npp.signed(np.arange(n), n)[:, None, None] * np.ones_like(k2)
    sx = npp.signed(np.arange(n), n)[None, :, None] * np.ones_like(k2)
    sz = np.arange(n // 2 + 1)[None, None, :] * np.ones_like(k2)
    terms = [[] for _ in range(npp.bins(n))]
    for iy, ix, iz in zip(*np.nonzero(mask)):
        kv = [float(c) * 2 * math.pi / box for c in (sx[iy, ix, iz], sy[iy, ix, iz], sz[iy, ix, iz])]
        kmag = math.sqrt(kv[0] * kv[0] + kv[1] * kv[1] + kv[2] * kv[2])
        terms[sh[iy, ix, iz]].append(float(w[iy, ix, iz]) * pknorm * pk(kmag) / box ** 3)
    return np.array([math.fsum(t) for t in terms])


@pytest.mark.parametrize("R", [0.0, 1.5, 4.0])
def test_parseval_with_the_inverse_transform(R):
    """the windowed k-space sum is the mean square of the smoothed field in real space"""
    n = 16
    spec = pc.random_box(11, n)                 # [ky][kx][kz]; made Hermitian on the two self-conjugate planes by the round trip
    spec = np.fft.rfftn(np.fft.irfftn(spec, s=(n, n, n), axes=(0, 1, 2)))
    spec[0, 0, 0] = 0.0
    k2, _, _ = npp.geometry(n)
    kf = 2.0 * math.pi / n
    smooth = spec * np.exp(-0.5 * (kf * kf) * (R * R) * k2)
    x = np.fft.irfftn(smooth, s=(n, n, n), axes=(0, 1, 2))      # numpy divides by n^3: delta(x)
    want = math.fsum((x * x).ravel().tolist()) / n ** 3
    got = npp.power(spec, 0, (R,))["variance"][0]
    print("Parseval at R =", R, abs(got - want) / want)
    assert abs(got - want) <= 1e-13 * want


def test_program_under_sanitizers(emul, tmp_path):
    """the stand-alone build of the same file on every case, with arrays of exactly the sizes: clean under the sanitizers, and the
    sums those of the library build"""
    if _stale(EXE):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-o", EXE, SRC])
    todo = [(fb, spec, 0, pc.N, RADII) for fb in (8, 4) for _, spec, _ in pc.cases()]
    todo += [(8, pc.random_box(3, 20)[7:12], 7, 5, ()), (4, pc.random_box(3, 20)[19:20], 19, 1, (2.0,))]
    path = tmp_path / "cases.bin"
    with open(path, "wb") as fh:
        for fb, spec, y0, nyl, radii in todo:
            np.array([fb, spec.shape[1], y0, nyl, len(radii)], dtype=np.int64).tofile(fh)
            np.array(radii, dtype=np.float64).tofile(fh)
            np.ascontiguousarray(spec, dtype=np.complex128).tofile(fh)
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True)
    print(out.stdout[-3000:], out.stderr[-3000:])
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and len(lines) == len(todo) and "ERROR" not in out.stderr
    for k, (fb, spec, y0, nyl, radii) in enumerate(todo):
        c = emul_run(emul, spec, y0, fb, radii)
        w = lines[k].split()
        assert w[:2] == ["case", "%d:" % k], lines[k]
        got = dict(zip(w[2::2], w[3::2]))
        assert (int(got["nmodes"]), int(got["k2sum"]), int(got["nonfinite"])) == (int(c["nmodes"].sum()), int(c["k2sum"].sum()), c["nonfinite"]), k
        sp, sv = 0.0, 0.0
        for v in c["power"]:
            sp += v
        for v in c["variance"]:
            sv += v
        assert float.fromhex(got["power"]) == sp and float.fromhex(got["variance"]) == sv, k
