"""The collapse pass on equal input: harness of tests/test_gpu_collapse_matrix.py and tests/test_collapse_matrix_cpu.py.

TEST INFRASTRUCTURE.  The collapse pass (pf_collapse_body, pinocchio_amd/csrc/pf_cell_kernels.hip) is one template dispatched as
about forty kernels.  Here a "side" -- the device through the C ABI, or the host compilation of the per-cell header with a numpy
running maximum -- walks a ladder of radii in the reference's own order of calls (compute_second_derivatives, optionally
initialize_collapse_times from a loaded table, compute_collapse_times) and hands back the Hessian it solved on.  The oracle is given
that very Hessian (Oracle.set_second_derivatives) and runs its whole compute_collapse_times on it, so that only the collapse pass is
left between the two: running maximum, Rmax, variance, table interpolation, ELL_SNG, float or double products.

The contract per cell, with d = |F_side - F_oracle| after every radius:
  floor   2 ulp_fp32(max(|F|, 1)) with float products, 1e-10 max(1, |F|) with double products
  spread  S = the largest change of the oracle's own running result over NOISE ladders on H (1 + u), u uniform in +-4.4e-16 per
          component (two ulps of input noise: what the transform's rounding leaves of "equal")
  a cell passes when d <= max(floor, 8 S); at most max(1, 3e-5 cells) cells fail per radius; the largest d <= 2e-3
  the sets F == 0 and F == -10 are the same on both sides, except where the oracle's own value crosses under the noise: those
  cells count as failing
  TrueVariance of every pass: rel <= 1e-12; Rmax after the ladder identical on >= 99.9 % of the cells
  exact arithmetic with double products: more than half of the cells bitwise equal
ELL_SNG per cell: the integrator's accept/reject decisions hang on the last bit of pow(), so its legs take the figures of
test_ell_sng_table_vs_oracle (> 95 % within 2 ulp_fp32, < 1e-3 beyond 1e-4 max(1, F), Rmax differing on < 5e-3).

The noise ladders are one oracle context of (2 n)^3 cells: eight copies of the n^3 Hessian, each with its own noise, one pass.
"""
from __future__ import annotations

import numpy as np

import oracle_lib
from pinocchio_amd import synth

NOISE = 8
NOISE_AMPL = 4.4e-16
FAIL_SHARE = 3e-5
MAX_ABS = 2e-3
FIELD_PRODUCT_TYPES = ((8, False), (4, False), (8, True))      # (field_bytes, double products)
ARITHMETICS = ("fast", "exact")
VARIANTS = ("plain", "tab0", "tab1", "tab2", "sng")
SNG_COSMO = np.array([0.25, 0.75, 0.0, 0.0])                    # (Omega0, OmegaLambda, OmegaRad, OmegaK), as test_ell_sng_table_vs_oracle
SNG_DIN = 1.28e-5
RADII = {32: (2.0, 1.0, 0.0), 16: (2.0, 0.0), 20: (2.0, 1.0, 0.0), 24: (2.0, 1.0, 0.0)}
SEEDS = {32: 7, 16: 3, 20: 5, 24: 9}


def flavour_of(variant: str) -> int:
    return int(variant[3]) if variant.startswith("tab") else 0


def ulp32(F):
    return np.spacing(np.maximum(np.abs(F), 1.0).astype(np.float32)).astype(np.float64)


def floor_of(F, double_products: bool):
    return 1e-10 * np.maximum(1.0, np.abs(F)) if double_products else 2.0 * ulp32(F)


_dk = {}


def density(n: int):
    if n not in _dk:
        _dk[n] = synth.make_density(n, seed=SEEDS[n])
        _dk[n].setflags(write=False)
    return _dk[n]


_invgrow = []


def invgrow():
    """the knots of the inverse growing mode (synth.invgrow_table integrates the growth equation: made once)"""
    if not _invgrow:
        _invgrow.extend(synth.invgrow_table("lcdm"))
    return _invgrow[0], _invgrow[1]


_var = {}


def field_variance(n: int, radii):
    """TrueVariance of the oracle's own sweep over the radii: stands in for Smoothing.Variance of a TABULATED_CT build"""
    key = (n, tuple(radii))
    if key not in _var:
        o = oracle_lib.Oracle(n, 0)
        o.set_density(density(n))
        o.set_invgrow(*invgrow())
        _var[key] = o.compute_fmax(np.array(radii), do_lpt=False)
        _var[key].setflags(write=False)
        o.close()
    return _var[key]


class Pass:
    """what the oracle leaves after one radius: TrueVariance, the running Fmax / Rmax and the running Fmax of the noise ladders"""

    def __init__(self, tv, F, R, Fnoise):
        self.tv, self.F, self.R, self.Fnoise = tv, F, R, Fnoise
        for a in (F, R, Fnoise):
            if a is not None:
                a.setflags(write=False)


_noise = {}


def _noise_oracle(n, double_products):
    """the (2 n)^3 context of the noise ladders, one per size and product type (making one costs more than a ladder on it)"""
    key = (n, double_products)
    if key not in _noise:
        _noise[key] = oracle_lib.Oracle(2 * n, 0, double_products=double_products)
    return _noise[key]


class Reference:
    """The oracle of one (variant, product type) on Hessians handed to it, with its noise ladders.  variance: per radius, of a
    table variant.  noise = False: no spread (ELL_SNG legs, Route C)."""

    def __init__(self, n, variant, double_products, nradii, variance=None, noise=True):
        self.n, self.variant, self.dp = n, variant, double_products
        self.variance = None if variance is None else np.ascontiguousarray(variance, dtype=np.float64)
        self.nradii = nradii
        self.o = oracle_lib.Oracle(n, 0, double_products=double_products)
        self._configure(self.o)
        self.on = _noise_oracle(n, double_products) if noise else None   # (configured by step(0): one context serves every ladder in turn)
        self.rng = np.random.default_rng(1)
        self.passes = []
        self.hessians = []
        self.tables = {}

    def _configure(self, o):
        o.set_invgrow(*invgrow())
        tab = self.variant.startswith("tab")
        assert not tab or (self.variance is not None and len(self.variance) >= self.nradii)
        o.set_tabulated_ct(self.variance if tab else [])
        o.set_ct_interpolation(flavour_of(self.variant))
        if self.variant == "sng":
            o.set_collapse_model(1, SNG_COSMO, np.full(self.nradii, SNG_DIN))
        else:
            o.set_collapse_model(0)

    def table(self, ismooth):
        """the oracle's own table of this radius, for the side to load: identical on both sides"""
        if ismooth not in self.tables:
            self.tables[ismooth], _ = self.o.ct_build(ismooth, float(self.variance[ismooth]))
        return self.tables[ismooth]

    def step(self, ismooth, H):
        n = self.n
        H = [np.ascontiguousarray(h, dtype=np.float64).reshape(n, n, n) for h in H]
        self.o.set_second_derivatives(H)
        tv = self.o.collapse_times(ismooth)
        p = self.o.products()
        Fn = None
        if self.on is not None:
            if ismooth == 0:
                self._configure(self.on)
                self.on.ladder_of = self
            assert self.on.ladder_of is self, "two ladders interleaved on one noise context"
            big = []
            for h in H:
                u = self.rng.uniform(-NOISE_AMPL, NOISE_AMPL, (NOISE, n ** 3))
                big.append((h.reshape(1, -1) * (1.0 + u)).reshape(2 * n, 2 * n, 2 * n))
            self.on.set_second_derivatives(big)
            self.on.collapse_times(ismooth)
            Fn = self.on.products()["Fmax"].astype(np.float64).reshape(NOISE, n ** 3)
        ps = Pass(tv, p["Fmax"].astype(np.float64).ravel(), p["Rmax"].ravel().copy(), Fn)
        self.passes.append(ps)
        self.hessians.append(H)
        return ps

    def close(self):
        self.o.close()


def check_pass(F, tv, ref: Pass, double_products, exact, label, stats=None):
    """the per-cell contract of one radius (module docstring); F: the side's running Fmax after it.  -> the figures"""
    F = np.asarray(F, dtype=np.float64).ravel()
    Fo = ref.F
    cells = Fo.size
    assert F.shape == Fo.shape
    assert np.isfinite(F).all() and np.isfinite(Fo).all(), label      # Gaussian fields reach neither the NaN skip nor anything non-finite
    d = np.abs(F - Fo)
    floor = floor_of(Fo, double_products)
    spread = np.max(np.abs(ref.Fnoise - Fo[None, :]), axis=0)
    explained = np.zeros(cells, dtype=bool)
    for v in (0.0, -10.0):
        mism = (F == v) != (Fo == v)
        crosses = np.any((ref.Fnoise == v) != (Fo == v)[None, :], axis=0)
        assert not np.any(mism & ~crosses), (label, v, int(np.sum(mism & ~crosses)), np.flatnonzero(mism & ~crosses)[:3])
        explained |= mism
    beyond = d > floor
    fail = (d > np.maximum(floor, 8.0 * spread)) | explained
    fig = dict(label=label, cells=cells, beyond_floor=int(beyond.sum()), failing=int(fail.sum()), worst=float(d.max()),
               tv_rel=abs(tv - ref.tv) / ref.tv, bitwise=float(np.mean(F == Fo)))
    print("collapse-matrix %s: cells %d beyond floor %d failing %d worst d %.3e tv rel %.1e bitwise %.4f"
          % (label, cells, fig["beyond_floor"], fig["failing"], fig["worst"], fig["tv_rel"], fig["bitwise"]))
    if stats is not None:
        stats.append(fig)
    assert fig["failing"] <= max(1, int(FAIL_SHARE * cells)), fig
    assert fig["worst"] <= MAX_ABS, fig
    assert fig["tv_rel"] <= 1e-12, fig
    if exact and double_products:
        assert fig["bitwise"] > 0.5, fig
    return fig


def check_pass_sng(F, tv, ref: Pass, label, stats=None):
    """ELL_SNG per cell: the figures of test_ell_sng_table_vs_oracle (set on the whole path; equal input can only do better)"""
    F = np.asarray(F, dtype=np.float64).ravel()
    Fo = ref.F
    d = np.abs(F - Fo)
    within = float(np.mean(d <= 2.0 * ulp32(Fo)))
    far = float(np.mean(d > 1e-4 * np.maximum(1.0, Fo)))
    fig = dict(label=label, cells=Fo.size, beyond_floor=int(np.sum(d > 2.0 * ulp32(Fo))), failing=int(np.sum(d > 1e-4 * np.maximum(1.0, Fo))),
               worst=float(d.max()), tv_rel=abs(tv - ref.tv) / ref.tv, bitwise=float(np.mean(F == Fo)))
    print("collapse-matrix %s: cells %d beyond 2 ulp %d beyond 1e-4 %d worst d %.3e tv rel %.1e"
          % (label, Fo.size, fig["beyond_floor"], fig["failing"], fig["worst"], fig["tv_rel"]))
    if stats is not None:
        stats.append(fig)
    assert within > 0.95 and far < 1e-3, fig
    assert fig["tv_rel"] <= 1e-12, fig
    return fig


def check_rmax(R, ref: Pass, label, sng=False):
    differing = float(np.mean(np.asarray(R).ravel() != ref.R))
    print("collapse-matrix %s: Rmax differing on %d cells" % (label, int(np.sum(np.asarray(R).ravel() != ref.R))))
    assert differing < (5e-3 if sng else 1e-3), (label, differing)     # (identical on >= 99.9 % of the cells)


def run_ladder(side, ref: Reference, radii, double_products, exact, label, stats=None):
    """One leg: `side` walks the radii; the oracle follows on the side's Hessian (a pass `ref` holds already, made by the leg of the
    other arithmetic, is used again: the Hessian depends on the field type alone, which is asserted).  A side has hessian(ismooth, radius) -> six [n][n][n]
    fp64 fields, load_table(ismooth, variance, table), collapse(ismooth) -> TrueVariance, and products() -> (Fmax, Rmax)."""
    sng = ref.variant == "sng"
    R = None
    figs = []
    for i, r in enumerate(radii):
        H = side.hessian(i, r)
        if i < len(ref.passes):
            for a, b in zip(H, ref.hessians[i]):
                assert np.array_equal(np.asarray(a).reshape(b.shape), b), (label, i)
            ps = ref.passes[i]
        else:
            ps = ref.step(i, H)
        if ref.variant.startswith("tab"):
            side.load_table(i, float(ref.variance[i]), ref.table(i))
        tv = side.collapse(i)
        F, R = side.products()
        lab = "%s R%d" % (label, i)
        figs.append(check_pass_sng(F, tv, ps, lab, stats) if sng else check_pass(F, tv, ps, double_products, exact, lab, stats))
    check_rmax(R, ref.passes[len(radii) - 1], label, sng)
    return figs


class Distinct:
    """The legs of one walk must not be one kernel under several names: a setting that did not take (interpolation flavour, table,
    arithmetic) would leave two legs with the same numbers.  note() holds the final Fmax of every leg against those seen before:
    the direct solve and the three interpolations differ from each other on > 30 % of the cells of a (field, product, arithmetic)
    type (the figure of test_trilinear_and_all_spline_table_interpolation_vs_oracle); with double products, where no fp32 rounding
    hides it, the two arithmetics differ somewhere."""

    def __init__(self):
        self.seen = {}

    def note(self, n, variant, fb, double_products, arithmetic, F):
        F = np.array(F, dtype=np.float64).ravel()
        for (n2, v2, fb2, dp2, a2), F2 in self.seen.items():
            if (n2, fb2, dp2) != (n, fb, double_products):
                continue
            if a2 == arithmetic and v2 != variant:
                assert np.mean(F != F2) > 0.3, (variant, v2, fb, double_products, arithmetic, float(np.mean(F != F2)))
            if a2 != arithmetic and v2 == variant == "plain" and double_products:
                assert not np.array_equal(F, F2), (variant, fb, arithmetic)
        self.seen[(n, variant, fb, double_products, arithmetic)] = F


# ---- Route C: the running maximum --------------------------------------------------------------------------------------------
def run_running_maximum(side, ref_factory, double_products, label):
    """The same radius collapsed as ismooth 0, 1 and 2, then the ladder ascending: what the comparison (double)fold < Fnew of the
    stored PRODFLOAT (quirk Q2) leaves in Rmax.  ref_factory(nradii) -> a Reference without noise."""
    # (a) one radius three times: with float products a cell whose Fnew was rounded down on storing is taken again (Rmax moves on),
    #     one rounded up or stored exactly is not; with double products the stored value is Fnew itself and nothing moves
    ref = ref_factory(3)
    first = None
    for i in range(3):
        H = side.hessian(i, 1.0)
        ps = ref.step(i, H)
        side.collapse(i)
        F, R = side.products()
        F, R = np.asarray(F).ravel(), np.asarray(R).ravel()
        if i == 0:
            first = F.copy()
        else:
            assert np.array_equal(F, first), (label, i)      # the value written again is the value that stood there
        check_rmax(R, ps, "%s repeat %d" % (label, i))
        if i == 1:
            shares = [float(np.mean(ps.R == v)) for v in (0, 1)]
            if double_products:
                assert not np.any(ps.R > 0) and not np.any(R > 0), label
            else:
                assert min(shares) > 0.25, (label, shares)                      # the oracle itself ...
                assert min(float(np.mean(R == v)) for v in (0, 1)) > 0.25, label  # ... and the side
        if i == 2 and double_products:
            assert not np.any(R > 0), label
    ref.close()
    # (b) ascending radii: most cells take the no-update branch
    ref = ref_factory(3)
    for i, r in enumerate((0.0, 1.0, 2.0)):
        H = side.hessian(i, r)
        ps = ref.step(i, H)
        side.collapse(i)
        F, R = side.products()
        check_rmax(R, ps, "%s ascending %d" % (label, i))
    counts = [int(np.sum(ps.R == v)) for v in (0, 1, 2)]
    print("collapse-matrix %s: Rmax counts of the ascending ladder %s" % (label, counts))
    assert counts[0] > 0.5 * ps.R.size and counts[1] > 0 and counts[2] > 0, (label, counts)
    ref.close()


# ---- Route D: outside the table ----------------------------------------------------------------------------------------------
def shares_outside_table(H, variance):
    """shares of the cells beyond |delta| > 7 sigma, x > 3.5 sigma, y > 3.5 sigma of a table made for `variance`, from the
    eigenvalues of the Hessian alone (numpy's eigvalsh; delta = l1 + l2 + l3, x = l1 - l2, y = l2 - l3, l1 >= l2 >= l3)"""
    h = [np.asarray(a, dtype=np.float64).ravel() for a in H]
    T = np.empty((h[0].size, 3, 3))
    T[:, 0, 0], T[:, 1, 1], T[:, 2, 2] = h[0], h[1], h[2]
    T[:, 0, 1] = T[:, 1, 0] = h[3]
    T[:, 0, 2] = T[:, 2, 0] = h[4]
    T[:, 1, 2] = T[:, 2, 1] = h[5]
    lam = np.linalg.eigvalsh(T)[:, ::-1]
    s = np.sqrt(variance)
    return (float(np.mean(np.abs(lam.sum(axis=1)) > 7.0 * s)), float(np.mean(lam[:, 0] - lam[:, 1] > 3.5 * s)),
            float(np.mean(lam[:, 1] - lam[:, 2] > 3.5 * s)))
