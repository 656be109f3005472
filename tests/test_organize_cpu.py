"""sort_and_organize without a device: the numpy restatement (tests/np_organize.py) has the post-conditions of the reference's call
(src/fragment.c:484-520) on random and hand-made inputs, and the sort keys of the device path (pinocchio_amd/csrc/pf_organize_core.h,
compiled for the host in tests/cpu_emul/organize_emul.cpp) order floats and doubles the way the restatement does -- signed zeros,
denormals, infinities and NaN included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import np_organize as npo

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emul", "organize_emul.cpp")
SO = os.path.join(HERE, "cpu_emul", "liborganize_emul.so")
HDR = os.path.join(HERE, "..", "pinocchio_amd", "csrc", "pf_organize_core.h")


@pytest.fixture(scope="module")
def emul():
    if (not os.path.exists(SO)) or os.path.getmtime(SO) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    L = C.CDLL(SO)
    L.emul_keys32.argtypes = [C.c_size_t, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    L.emul_keys64.argtypes = [C.c_size_t, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    return L


def _inputs(rng, count, kind, dtype=np.float32, cells=96 ** 3):
    """kind 0: continuous Fmax; 1: seven distinct values (nearly every comparison a tie); 2: zeros of both signs, infinities, NaN"""
    f = (rng.random(count) * 4.0 - 0.5).astype(dtype)
    if kind == 1:
        f = np.asarray([-0.5, 0.0, 0.5, 1.0, 1.5, 2.5, 3.0], dtype=dtype)[rng.integers(0, 7, count)]
    if kind == 2:
        special = np.asarray([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1.0, np.finfo(dtype).tiny / 4, -np.finfo(dtype).tiny / 4], dtype=dtype)
        pick = rng.random(count) < 0.6
        f[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    pos = rng.choice(cells, size=count, replace=False).astype(np.uint32)   # unique, in random input order
    return f, pos


def _check_postconditions(f, pos, rec):
    o, spos, ind = npo.organize(f, pos)
    fs, ps, rs = f[o], pos[o], rec[o]
    # the same (record, position) pairs, reordered
    assert np.array_equal(np.sort(o), np.arange(len(f)))
    assert sorted(zip(rs.tolist(), ps.tolist())) == sorted(zip(rec.tolist(), pos.tolist()))
    # Fmax non-increasing; NaN, which compares with nothing, behind everything
    nan = np.isnan(fs)
    k = int((~nan).sum())
    assert not nan[:k].any() and nan[k:].all()
    assert np.all(fs[:k][:-1] >= fs[:k][1:])
    # ties (-0.0 == +0.0 among them) and NaN in input order
    same = (fs[:-1] == fs[1:]) | (nan[:-1] & nan[1:])
    assert np.all(o[:-1][same] < o[1:][same])
    # the position index
    assert np.all(spos[:-1] < spos[1:]) and np.array_equal(spos, ps[ind])
    # find_location: every stored position gives the index whose frag_pos equals it ...
    loc = npo.find_location(spos, ind, ps)
    assert np.array_equal(loc, np.arange(len(ps)))
    # ... and positions that are not stored give -1
    absent = np.setdiff1d(np.arange(int(ps.max()) + 3 if len(ps) else 3), ps)
    assert np.all(npo.find_location(spos, ind, absent) == -1)


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_restatement_has_the_post_conditions(kind, dtype):
    rng = np.random.default_rng(100 + kind)
    for count in (1, 2, 3, 64, 257, 5000):
        f, pos = _inputs(rng, count, kind, dtype, cells=20000)
        _check_postconditions(f, pos, rng.integers(0, 1 << 30, count))


def test_the_restatement_on_hand_made_inputs():
    f = np.array([1.0, 3.0, 1.0, -0.0, np.nan, 0.0, -np.inf, 3.0, np.inf, np.nan], dtype=np.float32)
    pos = np.array([40, 7, 12, 3, 99, 0, 5, 8, 21, 1], dtype=np.uint32)
    o, spos, ind = npo.organize(f, pos)
    assert o.tolist() == [8, 1, 7, 0, 2, 3, 5, 6, 4, 9]
    assert pos[o].tolist() == [21, 7, 8, 40, 12, 3, 0, 5, 99, 1]
    assert spos.tolist() == [0, 1, 3, 5, 7, 8, 12, 21, 40, 99]
    assert ind.tolist() == [6, 9, 5, 7, 1, 2, 4, 0, 3, 8]
    assert npo.find_location(spos, ind, np.array([21, 0, 99, 2, 100, 41])).tolist() == [0, 6, 8, -1, -1, -1]
    _check_postconditions(f, pos, np.arange(10))
    # nothing stored
    o, spos, ind = npo.organize(np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.uint32))
    assert len(o) == len(spos) == len(ind) == 0 and npo.find_location(spos, ind, np.array([0, 5])).tolist() == [-1, -1]


def test_count_peaks_through_find_location_equals_the_field_form():
    import np_peaks
    rng = np.random.default_rng(7)
    n = 12
    field = (rng.random((n, n, n)) * 3).astype(np.float32)
    field[rng.random((n, n, n)) < 0.2] = 1.5              # equal neighbours: neither is a peak
    for flast in (0.0, 1.0, 2.0):
        cell = np.flatnonzero(field.ravel() >= flast)
        rng.shuffle(cell)
        f, pos = field.ravel()[cell], cell.astype(np.uint32)
        o, spos, ind = npo.organize(f, pos)
        assert npo.count_peaks(f[o], pos[o], spos, ind, (n, n, n)) == np_peaks.count_peaks(field, flast)[0]


def _special(dtype):
    fi = np.finfo(dtype)
    v = [0.0, -0.0, fi.tiny, -fi.tiny, fi.tiny / 8, -fi.tiny / 8, fi.smallest_subnormal, -fi.smallest_subnormal, fi.max, -fi.max, 1.0, -1.0,
         np.nextafter(dtype(1), dtype(2)), np.inf, -np.inf]
    return np.asarray(v, dtype=dtype)


@pytest.mark.parametrize("dtype,utype,fn", [(np.float32, np.uint32, "emul_keys32"), (np.float64, np.uint64, "emul_keys64")])
def test_device_keys_order_as_the_restatement(emul, dtype, utype, fn):
    rng = np.random.default_rng(11)
    bits = rng.integers(0, np.iinfo(utype).max, 20000, dtype=utype, endpoint=True)          # every exponent, denormals and NaN payloads among them
    nans = np.asarray([np.nan, -np.nan], dtype=dtype).view(utype)
    payload = nans[0] | utype(12345)
    f = np.concatenate([_special(dtype), bits.view(dtype), nans.view(dtype), np.asarray([payload], dtype=utype).view(dtype), _special(dtype)])
    u = np.ascontiguousarray(f.view(utype))
    keys = np.zeros_like(u)
    ptr = C.POINTER(C.c_uint if dtype is np.float32 else C.c_ulonglong)
    getattr(emul, fn)(len(u), u.ctypes.data_as(ptr), keys.ctypes.data_as(ptr))
    # a stable ascending sort of the keys is the restatement's order
    assert np.array_equal(np.argsort(keys, kind="stable").astype(np.uint32), npo.order(f))
    # and key order is value order: a < b <=> key(a) > key(b); equal values, equal keys; every NaN the one largest key
    nan = np.isnan(f)
    assert np.all(keys[nan] == np.iinfo(utype).max) and np.all(keys[~nan] < np.iinfo(utype).max)
    a, b = rng.integers(0, len(f), 50000), rng.integers(0, len(f), 50000)
    ok = ~nan[a] & ~nan[b]
    a, b = a[ok], b[ok]
    assert np.array_equal(f[a] < f[b], keys[a] > keys[b]) and np.array_equal(f[a] == f[b], keys[a] == keys[b])
    z = np.asarray([0.0, -0.0], dtype=dtype).view(utype)
    kz = np.zeros_like(z)
    getattr(emul, fn)(2, z.ctypes.data_as(ptr), kz.ctypes.data_as(ptr))
    assert kz[0] == kz[1]
