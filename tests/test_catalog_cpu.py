"""The output step of build_groups() without a device: the arithmetic of the device path (pinocchio_amd/csrc/pf_catalog_core.h,
compiled for the host in tests/cpu_emul/catalog_emul.cpp and run group by group as the reference runs it) against the numpy
restatement (tests/np_catalog.py) on the cases of tests/catalog_cases.py, with the pass criteria the GPU test applies to the kernels.
The inputs' own condition -- no Mass within 1e-9 bins of a bin edge -- is checked here with the oracle alone, for the cases and for
every Mass up to 200 000.  The same file as a program reads the same cases under -fsanitize=address,undefined."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import catalog_cases as cc
import np_catalog as npc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emul", "catalog_emul.cpp")
SO = os.path.join(HERE, "cpu_emul", "libcatalog_emul.so")
EXE = os.path.join(HERE, "cpu_emul", "catalog_emul_san")
HDRS = [os.path.join(HERE, "..", "pinocchio_amd", "csrc", h) for h in ("pf_catalog_core.h", "pf_plc_core.h", "pf_collapse_core.h")]


def _stale(product):
    return not os.path.exists(product) or any(os.path.getmtime(product) < os.path.getmtime(s) for s in [SRC] + HDRS)


@pytest.fixture(scope="module")
def emul():
    if _stale(SO):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DCATALOG_EMUL_LIB", "-o", SO, SRC])
    L = C.CDLL(SO)
    L.catalog_emul_run.restype = C.c_longlong
    L.catalog_emul_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def run_emul(L, c, capacity=None, flat=None):
    hdr, data = c.flat() if flat is None else flat
    n, nbin = int(hdr[8]), int(hdr[9])
    cap = n if capacity is None else capacity
    rec, idx = np.zeros((cap + 1, 10)), np.zeros(cap + 1, np.int32)
    nin, mas = np.zeros(nbin + 1, np.int32), np.zeros(nbin + 1)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    count = L.catalog_emul_run(vp(hdr), vp(data), cap, vp(rec), vp(idx), vp(nin), vp(mas))
    assert count >= 0
    m = min(count, cap)
    od = np.zeros(m, dtype=cc.catalog_dtype(c.T, c.light))
    od["M"], od["x"], od["v"], od["q"] = rec[:m, 0], rec[:m, 1:4], rec[:m, 4:7], rec[:m, 7:10]
    od["name"] = c.groups["name"][idx[:m]]
    if not c.light:
        od["n"] = c.groups["Mass"][idx[:m]]
    return od, idx[:m], int(count), nin[:nbin], mas[:nbin]


def test_layout_of_catalog_data():
    """src/pinocchio.h:515-524: 56 / 96 bytes, 48 / 88 with LIGHT_OUTPUT"""
    for T, light, size in ((np.float32, False, 56), (np.float64, False, 96), (np.float32, True, 48), (np.float64, True, 88)):
        dt = cc.catalog_dtype(T, light)
        pb = np.dtype(T).itemsize
        assert dt.itemsize == size and [dt.fields[k][1] for k in ("name", "M", "x", "v", "q")] == [0, 8, 8 + pb, 8 + 4 * pb, 8 + 7 * pb]
        assert ("n" in dt.names) == (not light) and (light or dt.fields["n"][1] == 8 + 10 * pb)


@pytest.mark.parametrize("name", list(cc.CASES))
def test_the_inputs_keep_their_conditions(name):
    cc.case(name).input_conditions()


def test_no_mass_up_to_200000_lies_on_a_bin_edge():
    """for MinHaloMass 10 the quotient is log10(Mass / 10) / DELTAM + 0.001 whatever ParticleMass is; its nearest approach to an integer
    over Mass <= 200 000 is 3.3e-6 bins"""
    m = np.arange(1, 200001)
    near = []
    for pm in (cc.PMASS, 1.0, 3.3e9):
        q = npc.bin_quotient(m, pm, np.log10(10.0 * pm) - 0.001 * cc.DELTAM, cc.DELTAM)
        near.append(float(np.abs(q - np.rint(q)).min()))
    print("nearest approach to a bin edge, in bins:", near)
    assert min(near) > 3e-6 and max(near) < 3.6e-6


def test_the_thresholds_are_the_log10_binning(emul):
    """every Mass from 1 to 200 000, and a few beyond, through the threshold table: the bins are those of the cast of the quotient"""
    c = cc.Case("thr", n=200008, masses="histogram", min_mass=1, seed=30)
    g = c.groups
    g["Mass"][:200000] = np.arange(1, 200001)
    g["Mass"][200000:] = [0, -5, 2 ** 31 - 1, 10 ** 9, 150000, 1, 10, 9]
    g["good"], g["point"] = 1, 0
    c.min_mass = -10
    _, _, count, nin, mas = run_emul(emul, c, capacity=0)
    want_n, _, want_s = npc.mass_function(g["Mass"], c.pmass, c.nbin, c.mmin, c.deltam)
    assert count == c.n and np.array_equal(nin, want_n)
    assert np.array_equal(mas, np.array([np.float64(s) * np.float64(c.pmass) for s in want_s]))


@pytest.mark.parametrize("name", list(cc.CASES))
def test_core_on_the_host_against_numpy(emul, name):
    c = cc.case(name)
    od, idx, count, nin, mas = run_emul(emul, c)
    c.check(od, idx, count, nin, mas, printer=print)


def test_the_cases_cover_what_they_are_named_after():
    o = cc.case("n63").oracle()
    g = cc.case("n63").groups
    assert g["Mass"][3] == cc.MIN_MASS - 1 and g["Mass"][4] == cc.MIN_MASS and g["good"][5] == 0 and g["point"][6] == -1
    assert 4 in o["index"] and not np.isin([3, 5, 6], o["index"]).any()
    o2 = cc.case("no_flags").oracle()
    assert np.isin([4, 5, 6], o2["index"]).all() and 3 not in o2["index"]
    # both global wraps fire on q and on x
    for name in ("n64_far", "n4097", "f64_far_light"):
        o = cc.case(name).oracle()
        assert o["qneg"].any() and o["qbig"].any() and o["xneg"].any() and o["xbig"].any(), name
    o = cc.case("n63").oracle()
    assert o["qneg"][:, 2].any() and o["xneg"][:, 2].any() and not o["qbig"].any()
    # q2x's own wrap fires both ways on the periodic axes and never on the others
    for name, axes in (("pbc111", (0, 1, 2)), ("pbc101_seg1", (0, 2)), ("f64_seg1_pbc", (0, 1, 2))):
        o = cc.case(name).oracle()
        for j in range(3):
            assert (o["pbc_hi"][:, j].any() and o["pbc_lo"][:, j].any()) == (j in axes), (name, j)
    # the histograms: bins below zero are skipped with min_mass 1, the short one leaves the top out
    a, b, s = cc.case("hist_all").oracle(), cc.case("hist_min1").oracle(), cc.case("hist_short").oracle()
    assert a["ninbin"].sum() == len(a["index"]) and b["ninbin"].sum() < len(b["index"]) and a["ninbin"][83] == 3
    assert 0 < s["ninbin"].sum() < (cc.case("hist_short").groups["Mass"][s["index"]] >= 10).sum()
    # a group of no extent (Mass 0) is among the records of the scale-dependent cases and in none of their bins
    for name in ("n257_nk10", "f64_nk10"):
        c = cc.case(name)
        assert (c.groups["Mass"][c.oracle()["index"]] == 0).any() and c.oracle()["ninbin"].sum() == (c.groups["Mass"] >= 9).sum()


@pytest.mark.parametrize("name", ["wrap", "wrap_f64"])
def test_wrap_case_in_closed_form(emul, name):
    c = cc.case(name)
    od, idx, count, _, _ = run_emul(emul, c)
    assert count == 4 and od["x"].tobytes() == od["q"].tobytes()
    want = (c.expect_q_cells * (c.ipd * c.hfactor)).astype(c.T)
    assert np.array_equal(od["q"], want), (od["q"], want)


def test_line_1588_and_the_v31_switch_differ(emul):
    a, b = run_emul(emul, cc.case("n65_seg1")), run_emul(emul, cc.case("n65_seg1_v31"))
    assert a[2] == b[2] > 0 and not np.array_equal(a[0]["x"], b[0]["x"]) and np.array_equal(a[0]["v"], b[0]["v"])


def test_capacity(emul):
    c = cc.case("n63")
    full = run_emul(emul, c)
    for cap in (0, 5, full[2]):
        od, idx, count, nin, mas = run_emul(emul, c, capacity=cap)
        assert count == full[2] and od.tobytes() == full[0][:cap].tobytes() and np.array_equal(nin, full[3]) and np.array_equal(mas, full[4])
        c.check(od, idx, count, nin, mas, capacity=cap)


def test_reversed_batch_gives_the_same_histograms(emul):
    c = cc.case("hist_min1")
    a = run_emul(emul, c)
    r = cc.Case("hist_min1_reversed", n=c.n, masses="histogram", min_mass=1, seed=16)
    r.groups = np.ascontiguousarray(c.groups[::-1])
    b = run_emul(emul, r)
    assert a[2] == b[2] and np.array_equal(a[3], b[3]) and a[4].tobytes() == b[4].tobytes()


def test_program_under_sanitizers(emul, tmp_path):
    """the stand-alone build of the same file on every case: clean under the sanitizers, and the counts and the sum of x[0] exactly
    those of the library build"""
    if _stale(EXE):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-o", EXE, SRC])
    names = list(cc.CASES)
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for n in names:
            hdr, data = cc.case(n).flat()
            np.array([hdr.size, data.size], dtype=np.int64).tofile(f)
            hdr.tofile(f)
            data.tofile(f)
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and len(lines) == len(names) and "ERROR" not in out.stderr
    for k, n in enumerate(names):
        od, _, count, nin, _ = run_emul(emul, cc.case(n))
        xsum = 0.0
        for x in od["x"][:, 0].astype(np.float64).tolist():
            xsum += x
        w = lines[k].split()
        assert w[:2] == ["case", "%d:" % k] and int(w[3]) == count and int(w[5]) == int(nin.sum()) and float(w[7]) == xsum, (n, lines[k], count, xsum)
