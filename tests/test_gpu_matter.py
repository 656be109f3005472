"""The matter-density call on the device (include/pinfmax.h: pf_matter_power, pf_debug_matter_deposit, pf_debug_matter_shells) against
the numpy restatement (tests/np_matter.py): planted columns and spectra through the taps, the resident call on every transform path,
field width, product type and LPT order, the state it must leave alone, the undisturbed lattice, the sign and amplitude convention
against the CPU oracle's displacements, the refusals, and the two forms of the deposit (PF_MATTER_LDS) in child processes.

Tolerances.  Grids, counters, nmodes and k2sum are integers: equal.  power, cross_pos and cross_neg through the tap: TOL_POWER = 1e-14,
derived in tests/test_matter_cpu.py (sums of positive terms whose bits the library and the restatement share); the two cross parts are
reached by feeding the tap the second spectrum with the modes of the other sign removed (np_matter.cross_masks), and `cross` is held
to TOL_POWER of their sum.  The resident call adds the error of the forward transform: the project asserts |err| < e M per mode, e =
1e-13 log2 n, M the largest |delta_k| (test_transforms_vs_pocketfft), which gives per shell, over N^6,
  power: 2 e M S_b + e^2 M^2 nmodes_b,  S_b = sum of w |delta_k|;     cross: e M L_b,  L_b = sum of w |delta_lin,k|
(only one factor of a cross term comes out of the transform; the other is the resident spectrum, exported exactly).  With fp32
fields e = 3e-5, the figure the project asserts for forward_transform on fp32 fields against numpy
(tests/test_gpu_multirank.py::test_loopback_slab_passes_on_fields_whose_answer_is_known, tol of fb == 4).  A deconvolved call
carries the factor of the mode on every term and so on its error: the bounds are then formed with w c^2 |delta_k| (w c^2 in the
second term) and w c |delta_lin,k| in place of the plain moduli, c = c[|kx|] c[|ky|] c[kz] of the mode."""
import ctypes as C
import math

import numpy as np
import pytest

import matter_cases as mc
import np_matter as npm
import np_power as npp
import power_cases as pc
from pinocchio_amd import synth

pytestmark = pytest.mark.gpu

TOL_POWER = 1e-14
INT_KEYS = ("deposited", "nonfinite", "outside", "empty_cells", "max_cell", "sum_hi32", "sum_lo32")
NAMES = ("Vel", "Vel_2LPT", "Vel_3LPT_1", "Vel_3LPT_2")


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


def raw_deposit(vel12, weight=None, ngp=False):
    """pf_debug_matter_deposit with a guard element behind every output -> (grid, the integer counters)"""
    from pinocchio_amd import _lib
    L = _lib.load()
    vel12 = np.ascontiguousarray(vel12)
    n = vel12.shape[1]
    grid = np.zeros(n ** 3 + 1, np.uint64)
    grid[-1] = 0xABCDEF
    info = (_lib.MatterInfo * 2)()
    info[1].deposited = info[1].nonfinite_modes = 0xABCDEF
    w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
    rc = L.pf_debug_matter_deposit(vel12.dtype.itemsize, n, vel12.ctypes.data_as(C.c_void_p), 1 if ngp else 0, None if w is None else w.ctypes.data_as(C.POINTER(C.c_double)),
                                   grid.ctypes.data_as(C.POINTER(C.c_ulonglong)), info)
    assert rc == 0, L.pf_last_error()
    assert grid[-1] == 0xABCDEF and info[1].deposited == info[1].nonfinite_modes == 0xABCDEF and info[0].modes == 0 == info[0].nonfinite_modes
    return grid[:-1].reshape(n, n, n), {k: int(getattr(info[0], k)) for k in INT_KEYS}


def check_grid(got, want, name, what, n):
    g, gi = got
    w, wi = want
    assert np.array_equal(g, w), name
    assert gi == wi, (name, gi, wi)
    assert gi["sum_hi32"] * (1 << 32) + gi["sum_lo32"] == gi["deposited"] * npm.ONE, name
    if what == "uniform":
        assert np.all(g == np.uint64(npm.ONE)) and gi["max_cell"] == npm.ONE and gi["empty_cells"] == 0, name
    elif what is not None and what[0] == "one_cell":
        assert int(g[what[1]]) == n ** 3 * npm.ONE == gi["max_cell"] and gi["empty_cells"] == n ** 3 - 1, name
    elif what is not None and what[0] == "counts":
        assert (gi["nonfinite"], gi["outside"]) == what[1:], name


@pytest.mark.parametrize("n", [16, 24])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_planted_deposits_through_the_tap(api, n, dt):
    """rows shorter than a wavefront (16) and no multiple of one (24)"""
    for name, v, w, ngp, what in mc.cases(n, dt):
        want = npm.deposit(v, w, ngp)
        got = raw_deposit(v, w, ngp)
        check_grid(got, want, (name, n, dt), what, n)
        if w is not None and set(w) <= {0.0, 1.0}:   # a 0 / 1 weight is the columns cleared by hand
            by_hand = raw_deposit(mc.zeroed_by_hand(v, w), None, ngp)
            assert np.array_equal(by_hand[0], got[0]) and by_hand[1] == got[1], name
    v = mc.smooth_random(n, dt, 13)
    g, info = api.debug_matter_deposit(v)                       # the binding, and the same bits from run to run
    again = raw_deposit(v)
    assert np.array_equal(g, again[0]) and {k: info[k] for k in INT_KEYS} == again[1]


def test_a_row_of_48_cells(api):
    v = mc.smooth_random(48, np.float32, 17)
    for ngp in (False, True):
        check_grid(raw_deposit(v, None, ngp), npm.deposit(v, None, ngp), (48, ngp), None, 48)


LDS_CHILD = """
import sys
import numpy as np
from pinocchio_amd import api
data = np.load(sys.argv[1])
out = {}
for key in data.files:
    g, info = api.debug_matter_deposit(data[key], ngp=key.endswith("_ngp"))
    out[key] = g
    out[key + "_info"] = np.array([info[k] for k in %r], dtype=np.uint64)
    out[key + "_form"] = np.array(api.matter_form()[0])
np.savez(sys.argv[2], **out)
""" % (INT_KEYS,)


def lds_cases():
    """columns around the edges of the LDS tile of csrc/pf_matter.hip: bricks of 4 x 4 x 16 particles, a margin of 3 cells.  On every
    axis and sign one corner particle of a brick whose cells end one cell inside the tile and one whose cells end one cell beyond it
    (the other particles at rest, so the brick's mean displacement rounds to zero); a bulk flow that the placement must follow; a
    smooth random field"""
    B, M = (4, 4, 16), 3
    out = {}
    for n, dt in ((64, np.float32), (32, np.float64), (16, np.float32)):
        v = mc.zeros(n, dt)
        brick = 0
        for j in range(3):
            for sgn in (-1, 1):
                for beyond in (0, 1):
                    o = [(4 * (brick % 3)) % n, (4 * (brick // 3 % 3) + 4) % n, (16 * (brick % 2)) % n]
                    brick += 1
                    q = list(o)
                    q[j] = o[j] + (B[j] - 1 if sgn > 0 else 0)
                    v[(j,) + tuple(q)] = sgn * (M - 1 + beyond) + 0.25 if sgn > 0 else -(M + beyond) + 0.25
        name = "edges_%d_%s" % (n, np.dtype(dt).name)
        out[name] = v
        out[name + "_ngp"] = v
        flow = mc.smooth_random(n, dt, 23, rms=0.7)
        flow[0] += dt(5.3); flow[1] -= dt(n / 2 + 0.4); flow[2] += dt(n - 2.2)
        out["flow_%d_%s" % (n, np.dtype(dt).name)] = flow
        out["random_%d_%s" % (n, np.dtype(dt).name)] = mc.smooth_random(n, dt, 29)
    return out


def test_the_lds_form_and_the_plain_form_give_the_same_grid(api, tmp_path):
    """PF_MATTER_LDS=1 and =0, each in a fresh child process, on the same columns: identical grids and counters, and those of the
    restatement"""
    import os
    import subprocess
    import sys
    cases = lds_cases()
    np.savez(tmp_path / "in.npz", **cases)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    got = {}
    for lds in ("0", "1"):
        env = dict(os.environ, PF_MATTER_LDS=lds, PYTHONPATH=root)
        r = subprocess.run([sys.executable, "-c", LDS_CHILD, str(tmp_path / "in.npz"), str(tmp_path / ("out%s.npz" % lds))], env=env, capture_output=True, text=True, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        got[lds] = np.load(tmp_path / ("out%s.npz" % lds))
    for key, v in cases.items():
        g, info = npm.deposit(v, None, key.endswith("_ngp"))
        for lds in ("0", "1"):
            assert np.array_equal(got[lds][key], g), (key, lds)
            assert int(got[lds][key + "_form"]) == int(lds), (key, lds)        # the form that was asked for is the one that ran
            assert got[lds][key + "_info"].tolist() == [info[k] for k in INT_KEYS], (key, lds)


def raw_shells(m, lin=None, y0=0, fb=8, ngp=False, deconvolve=False):
    """pf_debug_matter_shells with a guard element behind every output array"""
    from pinocchio_amd import _lib
    L = _lib.load()
    m = np.ascontiguousarray(m, dtype=np.complex128)
    lin = None if lin is None else np.ascontiguousarray(lin, dtype=np.complex128)
    nyl, n = m.shape[:2]
    nb = L.pf_power_bins(n)
    nm, ks = np.zeros(nb + 1, np.uint64), np.zeros(nb + 1, np.uint64)
    pw, cr = np.zeros(nb + 1), np.zeros(nb + 1)
    nm[-1] = ks[-1] = 0xABCDEF
    pw[-1] = cr[-1] = 123.5
    info = (_lib.MatterInfo * 2)()
    info[1].deposited = info[1].nonfinite_modes = 0xABCDEF
    up, dp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_ulonglong))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double)))
    rc = L.pf_debug_matter_shells(fb, n, y0, nyl, dp(m.view(np.float64)), dp(lin.view(np.float64)) if lin is not None else None, (1 if ngp else 0) | (2 if deconvolve else 0),
                                  up(nm), up(ks), dp(pw), dp(cr) if lin is not None else None, info)
    assert rc == 0, L.pf_last_error()
    assert nm[-1] == ks[-1] == 0xABCDEF and pw[-1] == cr[-1] == 123.5 and info[1].deposited == info[1].nonfinite_modes == 0xABCDEF
    return {"nmodes": nm[:-1], "k2sum": ks[:-1], "power": pw[:-1], "cross": cr[:-1] if lin is not None else None, "modes": int(info[0].modes),
            "nonfinite_modes": int(info[0].nonfinite_modes)}


def with_parts(m, lin, y0, fb, ngp, dec):
    """the tap's columns and the two parts of cross, each from a run of its own on a masked second spectrum"""
    got = raw_shells(m, lin, y0, fb, ngp, dec)
    mp_, mn_ = npm.cross_masks(m, lin, y0, fb, ngp, dec)
    got["cross_pos"] = raw_shells(m, mp_, y0, fb, ngp, dec)["cross"]
    got["cross_neg"] = -raw_shells(m, mn_, y0, fb, ngp, dec)["cross"]
    return got


def check_shells(got, want, what):
    assert np.array_equal(got["nmodes"], want["nmodes"]) and np.array_equal(got["k2sum"], want["k2sum"]), what
    assert (got["modes"], got["nonfinite_modes"]) == (want["modes"], want["nonfinite_modes"]), what
    r = {k: npp.rel(got[k], want[k]) for k in ("power", "cross_pos", "cross_neg")}
    scale = want["cross_pos"] + want["cross_neg"]
    d = np.abs(got["cross"] - want["cross"])
    print(what, r, "cross", float(np.max(d / np.where(scale > 0, scale, 1.0))))
    assert all(v <= TOL_POWER for v in r.values()), (what, r)       # each part, not only the difference
    assert np.all(d <= TOL_POWER * scale), what


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)) for k in ("nmodes", "k2sum", "power", "cross"))


@pytest.mark.parametrize("fb", [8, 4])
def test_shell_sums_through_the_tap(api, fb):
    n = 16
    for name, m, lin, expect in mc.planted_modes(n):
        got = with_parts(m, lin, 0, fb, False, False)
        check_shells(got, npm.shells(m, lin, 0, fb), (name, fb))
        for b in range(npp.bins(n)):        # exact small numbers: no rounding in any order
            e = expect.get(b, (0.0, 0.0, 0.0))
            assert (got["power"][b], got["cross_pos"][b], got["cross_neg"][b], got["cross"][b]) == tuple(x / float(n ** 6) for x in e + (e[1] - e[2],)), (name, b)
        check_shells(with_parts(m, lin, 0, fb, False, True), npm.shells(m, lin, 0, fb, False, True), (name, fb, "deconvolved"))
    # a random box, whole and in two slabs whose integer columns add up
    m = pc.random_box(31, n)
    lin = 0.7 * m + 0.5 * pc.random_box(32, n)
    for ngp, dec in ((False, False), (False, True), (True, True)):
        want = npm.shells(m, lin, 0, fb, ngp, dec)
        whole = with_parts(m, lin, 0, fb, ngp, dec)
        check_shells(whole, want, ("random", fb, ngp, dec))
        assert np.count_nonzero(want["cross_neg"]) > n // 4 and int(whole["nmodes"].sum()) == n ** 3 == whole["modes"]
        halves = [raw_shells(m[a:a + 8], lin[a:a + 8], a, fb, ngp, dec) for a in (0, 8)]
        for h, a in zip(halves, (0, 8)):
            hw = npm.shells(m[a:a + 8], lin[a:a + 8], a, fb, ngp, dec)
            assert np.array_equal(h["nmodes"], hw["nmodes"]) and np.array_equal(h["k2sum"], hw["k2sum"]) and h["modes"] == 8 * n * n
            assert npp.rel(h["power"], hw["power"]) <= TOL_POWER and np.all(np.abs(h["cross"] - hw["cross"]) <= TOL_POWER * (hw["cross_pos"] + hw["cross_neg"]))
        for k in ("nmodes", "k2sum"):
            assert np.array_equal(halves[0][k] + halves[1][k], whole[k])
        assert same_bits(whole, raw_shells(m, lin, 0, fb, ngp, dec))            # from run to run
        b = api.debug_matter_shells(m, lin, 0, fb, ngp, dec)                      # the binding
        assert same_bits(whole, b) and b["modes"] == n ** 3
    only = raw_shells(m, None, 0, fb)
    assert only["cross"] is None and np.array_equal(only["power"], raw_shells(m, lin, 0, fb)["power"])
    bad = m.copy()
    bad[3, 2, 1] = np.nan
    bad[0, 0, 8] = np.inf
    got, want = raw_shells(bad, lin, 0, fb), npm.shells(bad, lin, 0, fb)
    assert got["nonfinite_modes"] == want["nonfinite_modes"] == 3 and np.all(np.isfinite(got["power"])) and np.all(np.isfinite(got["cross"]))
    assert npp.rel(got["power"], want["power"]) <= TOL_POWER


SCAN_CHILD = """
import sys
import numpy as np
from pinocchio_amd import api
data = np.load(sys.argv[1])
out = {}
for fb in (8, 4):
    for dec in (False, True):
        got = api.debug_matter_shells(data["m"], data["lin"], 0, fb, False, dec)
        for k in ("nmodes", "k2sum", "power", "cross"):
            out["%s_%d_%d" % (k, fb, dec)] = got[k]
        out["scans_%d_%d" % (fb, dec)] = np.array(api.matter_form()[1])
        out["nonfinite_%d_%d" % (fb, dec)] = np.array(got["nonfinite_modes"])
np.savez(sys.argv[2], **out)
"""


def test_one_scan_and_a_scan_per_sum_give_the_same_bits(api, tmp_path):
    """the shell passes take the maxima of the three sums in one scan where its tables fit, and in a scan per sum on the largest grids;
    PF_MATTER_SCAN_EACH=1 takes the second way on a small grid.  Each in a fresh child process: the form that ran, and identical bits"""
    import os
    import subprocess
    import sys
    n = 16
    m = pc.random_box(51, n)
    lin = 0.6 * m + 0.5 * pc.random_box(52, n)
    m[3, 2, 1] = np.nan
    np.savez(tmp_path / "in.npz", m=m, lin=lin)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    got = {}
    for each in ("0", "1"):
        env = dict(os.environ, PF_MATTER_SCAN_EACH=each, PYTHONPATH=root)
        r = subprocess.run([sys.executable, "-c", SCAN_CHILD, str(tmp_path / "in.npz"), str(tmp_path / ("out%s.npz" % each))], env=env, capture_output=True, text=True, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        got[each] = np.load(tmp_path / ("out%s.npz" % each))
    for fb in (8, 4):
        for dec in (0, 1):
            assert (int(got["0"]["scans_%d_%d" % (fb, dec)]), int(got["1"]["scans_%d_%d" % (fb, dec)])) == (1, 3)
            assert int(got["0"]["nonfinite_%d_%d" % (fb, dec)]) == int(got["1"]["nonfinite_%d_%d" % (fb, dec)]) == 2
            for k in ("nmodes", "k2sum", "power", "cross"):
                a, b = got["0"]["%s_%d_%d" % (k, fb, dec)], got["1"]["%s_%d_%d" % (k, fb, dec)]
                assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (k, fb, dec)
            want = npm.shells(m, lin, 0, fb, False, bool(dec))
            assert npp.rel(got["1"]["power_%d_%d" % (fb, dec)], want["power"]) <= TOL_POWER
            assert np.all(np.abs(got["1"]["cross_%d_%d" % (fb, dec)] - want["cross"]) <= TOL_POWER * (want["cross_pos"] + want["cross_neg"]))


def columns_of(prod, dtype):
    """the twelve columns [12][nxl][n][n] as the device holds them, from the records pf_get_products returns"""
    return np.ascontiguousarray(np.stack([prod[name][..., j] for name in NAMES for j in range(3)]).astype(dtype))


def spectra_bound(n, fb, dens, dk_slab, deconvolve):
    """per-shell bounds of power and cross (over N^6) from the forward transform's asserted error, and numpy's own spectrum.  A
    deconvolved term carries its mode's own factor c (c^2 for power): so does its error"""
    spec = npp.from_x_slab(np.fft.rfftn(dens, axes=(0, 1, 2)))
    e, M = (1e-13 * math.log2(n) if fb == 8 else 3e-5), float(np.max(np.abs(spec)))
    _, sh, w = npp.geometry(n)
    nb = npp.bins(n)
    c = np.ones(spec.shape)
    if deconvolve:
        tab = npm.deconv_table(n)
        a = np.abs(npp.signed(np.arange(n), n))
        c = tab[a][:, None, None] * tab[a][None, :, None] * tab[np.arange(n // 2 + 1)][None, None, :]
    S = np.array([(w * c * c * np.abs(spec))[sh == b].sum() for b in range(nb)])
    Lb = np.array([(w * c * np.abs(dk_slab))[sh == b].sum() for b in range(nb)])
    nm = np.array([(w * c * c)[sh == b].sum() for b in range(nb)], dtype=np.float64)
    n6 = float(n ** 6)
    return spec, (2 * e * M * S + e * e * M * M * nm) / n6, e * M * Lb / n6


RESIDENT = [(n, fb, path, order, dp) for n, fb, path in ((16, 8, 0), (64, 4, 0), (48, 8, 1), (36, 8, 2)) for order in (1, 2, 3) for dp in (False, True) if fb == 8 or not dp]


@pytest.mark.parametrize("n,fb,path,order,dp", RESIDENT)
def test_resident_call(api, n, fb, path, order, dp):
    with api.Fmax(n, field_bytes=fb, double_products=dp) as f:
        assert f.L.pf_transform_path(f.h) == path
        f.synth_density(seed=60 + n, sigma0=0.4)
        f.set_invgrow(*synth.invgrow_table("lcdm"))
        f.set_growth(synth.growth_multipliers())
        f.set_lpt_order(order)
        f.compute_fmax(np.array([1.0, 0.0]), do_lpt=True)
        prod = f.products()
        dk = f.density()
        got = f.matter_power(density=True, deconvolve=(order == 2))
        again = f.matter_power(density=True, deconvolve=(order == 2))
        zel = f.matter_power(weight=(1.0, 0.0, 0.0, 0.0), cross=False, density=True)
    T = np.float64 if dp else np.float32
    cols = columns_of(prod, T)
    if order < 3:
        assert not np.any(cols[3 * order:])          # the columns of the orders that are not computed read zero
    grid, info = npm.deposit(cols)
    assert {k: got[k] for k in INT_KEYS} == info and got["modes"] == n ** 3 and got["nonfinite_modes"] == 0
    dens = npm.contrast(grid, fb)
    assert np.array_equal(got["density"], dens)      # bitwise
    assert same_bits(got, again) and np.array_equal(got["density"], again["density"])
    gz, iz = npm.deposit(cols, (1.0, 0.0, 0.0, 0.0))
    assert np.array_equal(zel["density"], npm.contrast(gz, fb)) and zel["cross"] is None and zel["deposited"] == iz["deposited"]
    assert order == 1 or not np.array_equal(zel["density"], got["density"])
    # spectra: numpy's transform of that density through the shell restatement
    dk_slab = npp.from_x_slab(dk)
    spec, bound_p, bound_c = spectra_bound(n, fb, dens, dk_slab, order == 2)
    want = npm.shells(spec, dk_slab, 0, 8, False, order == 2)
    assert np.array_equal(got["nmodes"], want["nmodes"]) and np.array_equal(got["k2sum"], want["k2sum"])
    dp_, dc_ = np.abs(got["power"] - want["power"]), np.abs(got["cross"] - want["cross"])
    nz = bound_p > 0
    print(n, fb, path, order, dp, "power / bound", float(np.max(dp_[nz] / bound_p[nz])), "cross / bound", float(np.max(dc_[nz] / np.maximum(bound_c[nz], 1e-300))),
          "max_cell", got["max_cell"] / npm.ONE)
    assert np.all(got["power"][~nz] == 0)
    assert np.all(dp_ <= bound_p) and np.all(dc_ <= bound_c)
    assert np.count_nonzero(got["power"]) > n // 4 and np.all(got["cross"][1:3] > 0)


def test_the_call_leaves_the_context_as_it_was(api):
    n = 32

    def run(with_call):
        with api.Fmax(n) as f:
            f.synth_density(seed=77, sigma0=0.4)
            f.set_invgrow(*synth.invgrow_table("lcdm"))
            f.set_growth(synth.growth_multipliers())
            f.compute_fmax(np.array([1.0, 0.0]), do_lpt=True)
            state = (f.device_bytes, f.arithmetic, f.L.pf_replicated_spectrum(f.h))
            prod = f.products().tobytes()
            if with_call:
                f.matter_power(density=True, deconvolve=True)
                f.matter_power(ngp=True, cross=False)
                assert state == (f.device_bytes, f.arithmetic, f.L.pf_replicated_spectrum(f.h))
                assert prod == f.products().tobytes()
            f.compute_displacements(0, 0)
            return f.products().tobytes(), f.power_spectrum("density", (1.0,)), [f.kvector(i) for i in range(3)], f.density()

    a, b = run(False), run(True)
    assert a[0] == b[0]
    assert all(np.array_equal(a[1][k], b[1][k]) for k in ("nmodes", "k2sum", "power", "variance"))
    assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2])) and np.array_equal(a[3], b[3])


@pytest.mark.parametrize("fb,dp", [(8, False), (8, True), (4, False)])
def test_the_undisturbed_lattice(api, fb, dp):
    """a context that has swept but never displaced reads zero columns"""
    n = 16
    with api.Fmax(n, field_bytes=fb, double_products=dp) as f:
        f.synth_density(seed=5)
        f.set_invgrow(*synth.invgrow_table("lcdm"))
        f.sweep(np.array([1.0]))
        for ngp in (False, True):
            got = f.matter_power(density=True, ngp=ngp, deconvolve=True)
            assert not np.any(got["density"]) and not np.any(got["power"]) and not np.any(got["cross"])
            assert (got["deposited"], got["max_cell"], got["empty_cells"], got["nonfinite"], got["outside"]) == (n ** 3, npm.ONE, 0, 0, 0)
            assert int(got["nmodes"].sum()) == n ** 3


def test_sign_units_and_amplitude_against_the_oracle(api):
    """A 32^3 density scaled so that the Zel'dovich displacement has rms 0.05 cells.  The thresholds come from the numpy chain
    (restated deposit, numpy rfftn, restated deconvolved shell sums) run on the CPU oracle's displacements of the same density, never
    from the device: on the lowest two shells the device's r = cross / sqrt(P_mm P_lin) and P_mm / P_lin must lie within MARGIN =
    1e-3 of the oracle chain's, the chain's own must be within 0.02 of 1, and cross must be positive.  The margin: the device's fp32
    displacement columns agree with the oracle's to 4e-7 of their amplitude (smoke()), which moves a shell's power by about that
    relative amount; 1e-3 is three orders above it and below the 0.002 - 0.01 by which the chain's own figures differ from 1."""
    import oracle_lib
    n, MARGIN = 32, 1e-3
    x, y = synth.invgrow_table("lcdm")
    g = synth.growth_multipliers()
    radii = np.array([1.0, 0.0])

    def oracle_columns(dk):
        o = oracle_lib.Oracle(n, 0)
        o.set_density(dk); o.set_invgrow(x, y); o.set_growth(g)
        o.compute_fmax(radii, do_lpt=True)
        p = o.products()
        o.close()
        return columns_of(p, np.float32)

    dk = synth.make_density(n, seed=11, sigma0=1.0)
    rms = math.sqrt(float(np.mean(oracle_columns(dk)[0:3].astype(np.float64) ** 2)))
    dk = dk * (0.05 / rms)
    cols = oracle_columns(dk)
    assert abs(math.sqrt(float(np.mean(cols[0:3].astype(np.float64) ** 2))) - 0.05) < 1e-4
    grid, _ = npm.deposit(cols)
    lin = npp.from_x_slab(dk)
    chain = npm.shells(npp.from_x_slab(np.fft.rfftn(npm.contrast(grid), axes=(0, 1, 2))), lin, 0, 8, False, True)
    plin = npp.power(lin)["power"]
    r_ref = chain["cross"][1:3] / np.sqrt(chain["power"][1:3] * plin[1:3])
    q_ref = chain["power"][1:3] / plin[1:3]
    print("oracle chain: r", r_ref, "P_mm / P_lin", q_ref)
    assert np.all(np.abs(r_ref - 1) < 0.02) and np.all(np.abs(q_ref - 1) < 0.02)
    with api.Fmax(n) as f:
        f.set_density(dk); f.set_invgrow(x, y); f.set_growth(g)
        f.compute_fmax(radii, do_lpt=True)
        got = f.matter_power(deconvolve=True)
        pl = f.power_spectrum("density")["power"]
    r = got["cross"][1:3] / np.sqrt(got["power"][1:3] * pl[1:3])
    q = got["power"][1:3] / pl[1:3]
    print("device: r", r, "P_mm / P_lin", q)
    assert np.all(got["cross"][1:3] > 0)
    assert np.all(np.abs(r - r_ref) <= MARGIN) and np.all(np.abs(q - q_ref) <= MARGIN)


def test_refusals_on_a_live_context(api, capfd):
    from pinocchio_amd import _lib
    n = 16
    nb = api.power_bins(n)
    nm, ks = np.full(nb + 1, 0xABCDEF, np.uint64), np.full(nb + 1, 0xABCDEF, np.uint64)
    pw, cr, dens = np.full(nb + 1, 123.5), np.full(nb + 1, 123.5), np.full(n ** 3 + 1, 123.5)
    info = (_lib.MatterInfo * 2)()
    info[0].deposited = info[1].deposited = 0xABCDEF
    up, dp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_ulonglong))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double)))
    w = np.array([1.0, 1.0, 1.0, 1.0])

    def untouched():
        return np.all(nm == 0xABCDEF) and np.all(ks == 0xABCDEF) and np.all(pw == 123.5) and np.all(cr == 123.5) and np.all(dens == 123.5) and \
            info[0].deposited == info[1].deposited == 0xABCDEF

    with api.Fmax(n) as f:
        L = f.L
        call = lambda **k: L.pf_matter_power(k.get("h", f.h), k.get("flags", 0), k.get("w", dp(w)), k.get("nm", up(nm)), k.get("ks", up(ks)), k.get("pw", dp(pw)),
                                             k.get("cr", dp(cr)), k.get("dens", dp(dens)), k.get("info", info))
        assert call() != 0 and b"pf_matter_power: density not set" in L.pf_last_error() and untouched()       # cross without a density
        assert call(cr=None) != 0 and b"pf_matter_power: products not computed" in L.pf_last_error() and untouched()
        f.synth_density(seed=3)
        assert call() != 0 and b"pf_matter_power: products not computed" in L.pf_last_error() and untouched()
        before = f.device_bytes
        for kw, what in (({"h": None}, b"null argument"), ({"nm": None}, b"null argument"), ({"ks": None}, b"null argument"), ({"pw": None}, b"null argument"),
                         ({"info": None}, b"null argument"), ({"flags": 4}, b"unknown flag bits"), ({"flags": -1}, b"unknown flag bits"),
                         ({"w": dp(np.array([1.0, np.nan, 0.0, 0.0]))}, b"is not finite"), ({"w": dp(np.array([1.0, 0.0, 0.0, -np.inf]))}, b"is not finite")):
            assert call(**kw) != 0, kw
            assert what in L.pf_last_error() and b"pf_matter_power" in L.pf_last_error(), (kw, L.pf_last_error())
            assert untouched(), kw
        assert "ERROR on task 0: pf_matter_power" in capfd.readouterr().out
        assert before == f.device_bytes
    with api.Fmax(n) as f:
        f.synth_density(seed=3)
        f.set_invgrow(*synth.invgrow_table("lcdm"))
        f.sweep(np.array([1.0]))
        before = f.device_bytes
        assert f.L.pf_matter_power(f.h, 0, None, up(nm), up(ks), dp(pw), None, None, info) == 0      # weight, cross and density_host may be NULL
        assert before == f.device_bytes and info[1].deposited == 0xABCDEF and nm[-1] == ks[-1] == 0xABCDEF and pw[-1] == 123.5 and np.all(cr == 123.5)
        assert f.L.pf_matter_power(f.h, 3, dp(w), up(nm), up(ks), dp(pw), dp(cr), dp(dens), info) == 0
        assert cr[-1] == dens[-1] == 123.5 and not np.any(dens[:-1])


def test_more_than_one_rank_is_refused(api):
    from test_gpu_multirank import run_ranks

    def body(f, r):
        f.synth_density(seed=9)
        f.set_invgrow(*synth.invgrow_table("lcdm"))
        f.sweep(np.array([1.0]))
        with pytest.raises(api.PinfmaxError, match="pf_matter_power: one rank only"):
            f.matter_power()
        return True

    assert all(run_ranks(api, 16, 2, body))
