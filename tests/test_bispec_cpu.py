"""The bispectrum estimator without a device: the numpy restatement (tests/np_bispec.py) of the FFT estimator against the direct
enumeration of all ordered pairs of modes on a Gaussian field, for the sums and for the triangle counts; the open triples, which
enumerate to nothing and are absent from the list; a case with 3 kmax > n, where the estimator closes triangles modulo the grid and
does differ from the enumeration -- what the call's refusal is for; and the arithmetic of the device path
(pinocchio_amd/csrc/pf_bispec_core.h, compiled for the host in tests/cpu_emul/bispec_emul.cpp) against the restatement: bin, list of
triples, term, sign and the fixed-point sums bit for bit.  The same file as a program runs under -fsanitize=address,undefined."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import bispec_cases as bc
import np_bispec as npb
import np_power as npp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "cpu_emul", "bispec_emul.cpp")
SO = os.path.join(HERE, "cpu_emul", "libbispec_emul.so")
EXE = os.path.join(HERE, "cpu_emul", "bispec_emul_san")
HDRS = [os.path.join(ROOT, "pinocchio_amd", "csrc", h) for h in ("pf_power_core.h", "pf_bispec_core.h")] + [os.path.join(ROOT, "include", "pinfmax.h")]
TOL_POWER = 1e-14        # the fixed-point sums against math.fsum (tests/test_gpu_power.py)


def transform_error(n):
    """what one fp64 transform may leave, relative to its largest output: the figure the project holds its own transforms to
    (tests/test_gpu_parity.py), which numpy's stay far below.  To first order a product of three reversed fields is off by three
    times that of its absolute value, and the data fields carry the forward transform's too: 3 e and 4 e of the absolute sums"""
    return 1e-13 * math.log2(n)


def _stale(product):
    return not os.path.exists(product) or any(os.path.getmtime(product) < os.path.getmtime(s) for s in [SRC] + HDRS)


def build_emul():
    if _stale(SO):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DBISPEC_EMUL_LIB", "-o", SO, SRC])
    L = C.CDLL(SO)
    vp = C.c_void_p
    L.bispec_emul_bins.argtypes = [C.c_size_t, vp, C.c_int, C.c_int, C.c_int, vp]
    L.bispec_emul_triangles.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.bispec_emul_terms.argtypes = [C.c_size_t, vp, vp, vp, vp, vp]
    L.bispec_emul_sums.argtypes = [C.c_size_t, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    return L


@pytest.fixture(scope="module")
def emul():
    return build_emul()


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def enumerated():
    """per small case: the restated estimator and the enumeration on one Gaussian field, every ordered triple, computed once"""
    out = {}
    for n, kmin, dk, nk in bc.SMALL:
        delta = bc.gaussian_field(n, 7 + n + dk)
        spec = npp.from_x_slab(np.fft.rfftn(delta, axes=(0, 1, 2)))
        data, km = npb.fields_of(spec, kmin, dk, nk)
        count, km2 = npb.fields_of(spec, kmin, dk, nk, kind=1, read=False)
        assert np.array_equal(km, km2)
        tri, sums, counts = npb.enumerate_pairs(delta, kmin, dk, nk, all_triples=True)
        out[(n, kmin, dk, nk)] = {"data": data, "count": count, "kmodes": km, "tri": tri, "sums": sums, "counts": counts}
    return out


@pytest.mark.parametrize("case", bc.SMALL)
def test_the_estimator_is_the_enumeration_of_all_pairs_of_modes(enumerated, case):
    n, kmin, dk, nk = case
    e = enumerated[case]
    closed = npb.triangles(kmin, dk, nk)
    N3 = float(n) ** 3
    for t, (i, j, l) in enumerate(e["tri"]):
        x = npb.term(e["data"][i], e["data"][j], e["data"][l]).ravel()
        c = npb.term(e["count"][i], e["count"][j], e["count"][l]).ravel()
        got, absum = math.fsum(x.tolist()), math.fsum(np.abs(x).tolist())
        ntri = math.fsum(c.tolist()) / N3
        print(case, (i, j, l), "triangles", int(e["counts"][t]), "count error", abs(ntri - e["counts"][t]), "sum error / absolute sum", abs(got - e["sums"][t]) / absum)
        assert abs(ntri - e["counts"][t]) <= 3 * transform_error(n) * math.fsum(np.abs(c).tolist()) / N3
        assert abs(got - e["sums"][t]) <= 4 * transform_error(n) * absum
        # an open triple enumerates to nothing and is absent from the list; a closed one has triangles at these sizes
        assert ((i, j, l) in closed) == (e["counts"][t] > 0), (i, j, l)
    assert all(int(e["count"][i][0, 0, 0].round()) == int(e["kmodes"][i]) and abs(e["count"][i][0, 0, 0] - int(e["kmodes"][i])) < 1e-9 for i in range(nk))   # I_i(0) == kmodes[i]
    # the count by orbits of the cube's symmetries (what the GPU test uses at the larger sizes) is the enumeration's
    assert list(npb.count_triangles(kmin, dk, nk)) == [int(e["counts"][e["tri"].index(t)]) for t in closed]
    if case == (16, 1, 2, 2):
        assert list(e["counts"]) == [3798, 4418, 17508, 39504]
    if case == (16, 1, 1, 4):
        assert len(e["tri"]) == 20 and (0, 0, 3) not in closed and len(closed) < 20
    if case == (24, 1, 2, 3):
        assert len(closed) == 10 == len(e["tri"]) and int(e["counts"].min()) == 156 and int(e["counts"].max()) == 129864


def test_with_3_kmax_above_n_the_estimator_is_not_the_enumeration():
    """what the refusal is for: triangles that close modulo the grid enter the sum over cells and are no triangles"""
    n, kmin, dk, nk = bc.ALIASED
    assert 3 * (kmin + nk * dk) > n
    delta = bc.gaussian_field(n, 5)
    count, _ = npb.fields_of(np.zeros((n, n, n // 2 + 1), np.complex128), kmin, dk, nk, kind=1, read=False)
    tri, _, counts = npb.enumerate_pairs(delta, kmin, dk, nk)
    ntri, _ = npb.estimator(count, kmin, dk, nk)
    ntri = ntri / float(n) ** 3
    extra = np.round(ntri).astype(np.int64) - counts
    print("aliased triangles per triple", dict(zip(tri, extra.tolist())))
    assert np.all(extra >= 0) and extra.max() > 100 and extra[tri.index((0, 0, 0))] == 0            # (the smallest bin alone stays below n / 3)


@pytest.mark.parametrize("case", bc.CASES + [(64, 1, 2, 10), (1024, 1, 10, 32), (96, 5, 1, 27)])
def test_bin_and_list_of_triples_bit_for_bit(emul, case):
    n, kmin, dk, nk = case
    k2 = np.arange(0, (kmin + nk * dk + 2) ** 2, dtype=np.uint64)
    got = np.full(len(k2) + 1, 77, np.int32)
    assert emul.bispec_emul_bins(len(k2), _vp(k2), kmin, dk, nk, _vp(got)) == 0 and got[-1] == 77
    want = npb.bin_of(k2.astype(np.int64), kmin, dk, nk)
    assert np.array_equal(got[:-1], want.astype(np.int32))
    assert want[0] == -1 and want[kmin * kmin] == 0 and want[kmin * kmin - 1] == -1 and want[(kmin + nk * dk) ** 2] == -1 and want[(kmin + nk * dk) ** 2 - 1] == nk - 1
    tri = npb.triangles(kmin, dk, nk)
    assert emul.bispec_emul_triangles(kmin, dk, nk, n, None) == len(tri)
    ijl = np.full(3 * len(tri) + 1, 77, np.int32)
    assert emul.bispec_emul_triangles(kmin, dk, nk, n, _vp(ijl)) == len(tri) and ijl[-1] == 77
    assert [tuple(r) for r in ijl[:-1].reshape(-1, 3)] == tri == sorted(tri)
    assert all(i <= j <= l for i, j, l in tri) and all((i, i, i) in tri for i in range(nk))


def test_the_refusals_of_the_bins(emul):
    assert emul.bispec_emul_triangles(0, 1, 2, 0, None) == -1 and emul.bispec_emul_triangles(1, 0, 2, 0, None) == -2
    assert emul.bispec_emul_triangles(1, 1, 0, 0, None) == -3 and emul.bispec_emul_triangles(1, 1, 33, 0, None) == -3
    n, kmin, dk, nk = bc.ALIASED
    assert emul.bispec_emul_triangles(kmin, dk, nk, n, None) == -4 and emul.bispec_emul_triangles(kmin, dk, nk, 21, None) == len(npb.triangles(kmin, dk, nk))
    assert emul.bispec_emul_triangles(1, 1, 32, 0, None) == len(npb.triangles(1, 1, 32))


def test_term_and_sign_bit_for_bit(emul):
    rng = np.random.default_rng(3)
    a, b, c = (rng.standard_normal(4000) * np.exp2(rng.integers(-40, 41, 4000).astype(np.float64)) for _ in range(3))
    a[:5], b[5:10] = 0.0, -0.0
    a[10:14], b[10:14], c[10:14] = [1e-200, -1e-200, 1e200, 3.0], [1e-200, 1e-200, 1e200, -5.0], [1.0, 1.0, 1e200, 7.0]      # underflow to +-0, overflow, an exact one
    t, s = np.full(4001, 123.5), np.full(4001, 9, np.int32)
    assert emul.bispec_emul_terms(4000, _vp(a), _vp(b), _vp(c), _vp(t), _vp(s)) == 0 and t[-1] == 123.5 and s[-1] == 9
    want = npb.term(a, b, c)
    assert np.array_equal(t[:-1].view(np.uint64), want.view(np.uint64))
    assert np.array_equal(s[:-1], np.where(want > 0, 0, np.where(want < 0, 1, -1)).astype(np.int32))
    assert list(s[:14]) == [-1] * 12 + [0, 1] and t[13] == -105.0 and set(s[:-1]) == {-1, 0, 1}


@pytest.mark.parametrize("case", bc.SMALL)
def test_the_fixed_point_sums_bit_for_bit(emul, case):
    """the emulation's limbs (the library's) against the restatement's Python integers, bit for bit, and within TOL_POWER of math.fsum"""
    n, kmin, dk, nk = case
    f = bc.random_fields(nk, 5, n, 11 + n)
    f[0, 0, 0, :3] = [0.0, -0.0, 2.0 ** -600]             # terms of zero and a term far below the scale
    want = npb.triples(f, kmin, dk, nk)
    nt = len(npb.triangles(kmin, dk, nk))
    parts, pair, mx = np.full(2 * nt + 1, 123.5), np.full(nk + 1, 123.5), np.full(nk + 1, 123.5)
    assert emul.bispec_emul_sums(f[0].size, _vp(np.ascontiguousarray(f)), kmin, dk, nk, _vp(parts), _vp(pair), _vp(mx)) == 0
    assert parts[-1] == pair[-1] == mx[-1] == 123.5
    assert np.array_equal(parts[:-1].view(np.uint64), want["parts"].ravel().view(np.uint64))
    assert np.array_equal(pair[:-1].view(np.uint64), want["pair"].view(np.uint64)) and np.array_equal(mx[:-1], want["maxima"])
    rp, rq = npp.rel(want["parts"], want["parts_fsum"]), npp.rel(want["pair"], want["pair_fsum"])
    print(case, "fixed point against fsum: parts", rp, "pair", rq)
    assert rp <= TOL_POWER and rq <= TOL_POWER and np.all(want["parts"] > 0)


def test_program_under_sanitizers(emul):
    """the stand-alone build of the same file with arrays of exactly the sizes: clean under the sanitizers"""
    if _stale(EXE):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-o", EXE, SRC])
    for ncell, kmin, dk, nk, seed in ((4096, 1, 1, 4, 1), (1, 2, 3, 1, 2), (777, 1, 2, 32, 3)):
        out = subprocess.run([EXE, str(ncell), str(kmin), str(dk), str(nk), str(seed)], capture_output=True, text=True)
        print(out.stdout[-2000:], out.stderr[-2000:])
        assert out.returncode == 0 and "ERROR" not in out.stderr
        got = dict(zip(out.stdout.split()[0::2], out.stdout.split()[1::2]))
        assert int(got["triangles"]) == len(npb.triangles(kmin, dk, nk))
        assert float.fromhex(got["psum"]) > 0.0 and float.fromhex(got["qsum"]) > 0.0
