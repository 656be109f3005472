"""Every dispatched collapse kernel against the oracle on the kernel's own Hessian (harness and contract: tests/collapse_matrix.py).

pf_launch_collapse_as dispatches pf_collapse_body as about forty kernels -- (plain | table x 3 interpolations | ELL_SNG per cell |
from invariants | with LPT sources) x (fp64 | fp32 fields) x (fast | exact arithmetic) x (float | double products).  The device hands
back the Hessian it solved on (pf_get_second_derivative), the oracle is given that Hessian, and the collapse pass alone is compared:

  Route A  the reference's own order of calls per radius, 5 variants x 3 (field, product) types x 2 arithmetics = 30 legs
  Route B  k_collapse_inv and k_collapse_src exist inside the sweep only: compute_fmax on a fresh context equals Route A's calls
           followed by compute_displacements(1, 0) bit for bit, 3 types x 2 arithmetics = 6 legs
  Route C  the running maximum: one radius collapsed three times, and the ladder ascending
  Route D  the table look-ups outside the table (made for 0.1 x the variance)
  Route E  launch forms: a last workgroup that is partly empty (20^3, 24^3 with fp32 fields), the one-group form of k_collapse_inv

Every leg of Routes A and B asserts through kernel_stats() the kernel class that ran."""
import time

import numpy as np
import pytest

import collapse_matrix as cm
import oracle_lib
from pinocchio_amd import synth

pytestmark = pytest.mark.gpu
VEL = ("Vel", "Vel_2LPT", "Vel_3LPT_1", "Vel_3LPT_2")
_distinct = cm.Distinct()


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


def _new_context(api, n, fb, double_products):
    f = api.Fmax(n, field_bytes=fb, timing=True, double_products=double_products)
    f.set_density(cm.density(n))
    f.set_invgrow(*cm.invgrow())
    f.set_growth(synth.growth_multipliers())
    return f


@pytest.fixture(scope="module")
def contexts(api):
    """one context per (size, field type, product type), shared by the legs: every leg sets the whole state it depends on"""
    held = {}

    def get(n, fb, double_products):
        key = (n, fb, double_products)
        if key not in held:
            held[key] = _new_context(api, n, fb, double_products)
        return held[key]

    yield get
    for f in held.values():
        f.close()


@pytest.fixture(scope="module")
def references():
    held = {}

    def get(n, variant, fb, double_products, factor=1.0):
        key = (n, variant, fb, double_products, factor)
        if key not in held:
            radii = cm.RADII[n]
            var = cm.field_variance(n, radii) * factor if variant.startswith("tab") else None
            held[key] = cm.Reference(n, variant, double_products, len(radii), variance=var, noise=variant != "sng")
        return held[key]

    yield get
    for r in held.values():
        r.close()


class GpuSide:
    """the reference's own order of calls on one context: compute_second_derivatives, the six fields tapped as fp64 copies (exact
    for fp32 fields too), a table loaded where the variant has one, compute_collapse_times, products"""

    def __init__(self, f, variant, arithmetic):
        self.f = f
        self.seconds = 0.0
        f.set_arithmetic(arithmetic)
        assert f.arithmetic == arithmetic
        f.set_tabulated_ct([])
        f.set_ct_interpolation(cm.flavour_of(variant))
        if variant == "sng":
            f.set_collapse_model(1, cm.SNG_COSMO, np.full(len(cm.RADII[f.n]), cm.SNG_DIN))
        else:
            f.set_collapse_model(0)
        f.reset_kernel_stats()

    def _timed(self, fn, *a):
        t = time.perf_counter()
        out = fn(*a)
        self.seconds += time.perf_counter() - t
        return out

    def hessian(self, ismooth, radius):
        self._timed(self.f.compute_second_derivatives, radius)
        return [self._timed(self.f.second_derivative, k) for k in range(6)]

    def load_table(self, ismooth, variance, table):
        self._timed(self.f.ct_load, ismooth, variance, table)

    def collapse(self, ismooth):
        return self._timed(self.f.compute_collapse_times, ismooth)

    def products(self):
        p = self._timed(self.f.products)
        return p["Fmax"].ravel(), p["Rmax"].ravel()

    def classes(self):
        return {k["name"]: k for k in self.f.kernel_stats() if k["launches"]}


def _assert_six_component_collapse_ran(side, passes, label):
    cl = side.classes()
    assert "collapse" in cl and cl["collapse"]["launches"] == passes, (label, sorted(cl))
    assert "collapse_inv" not in cl and "collapse_lpt_sources" not in cl and "zpass_collapse_fused" not in cl, (label, sorted(cl))
    return cl["collapse"]["total_ms"]


def _leg(side, ref, n, double_products, arithmetic, label):
    radii = cm.RADII[n]
    figs = cm.run_ladder(side, ref, radii, double_products, arithmetic == "exact", label)
    ms = _assert_six_component_collapse_ran(side, len(radii), label)
    print("collapse-matrix-leg %s: beyond floor %d failing %d worst d %.3e device calls %.3f s collapse kernels %.3f ms"
          % (label, sum(g["beyond_floor"] for g in figs), sum(g["failing"] for g in figs), max(g["worst"] for g in figs), side.seconds, ms))


def _label(variant, n, fb, double_products, arithmetic):
    return "%s %d^3 fb%d %s %s" % (variant, n, fb, "dp" if double_products else "sp", arithmetic)


# ---- Route A -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arithmetic", cm.ARITHMETICS)
@pytest.mark.parametrize("fb,double_products", cm.FIELD_PRODUCT_TYPES)
@pytest.mark.parametrize("variant", cm.VARIANTS)
def test_route_a_collapse_kernel_vs_oracle_on_its_own_hessian(contexts, references, variant, fb, double_products, arithmetic):
    """32^3 (seed 7) with radii (2, 1, 0); the ELL_SNG legs 16^3 with radii (2, 0).  The table legs load the oracle's own table (made
    for the field's own variance: no cell leaves it), which is data and the same on both sides."""
    n = 16 if variant == "sng" else 32
    side = GpuSide(contexts(n, fb, double_products), variant, arithmetic)
    _leg(side, references(n, variant, fb, double_products), n, double_products, arithmetic, _label(variant, n, fb, double_products, arithmetic))
    _distinct.note(n, variant, fb, double_products, arithmetic, side.products()[0])


# ---- Route B -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arithmetic", cm.ARITHMETICS)
@pytest.mark.parametrize("fb,double_products", cm.FIELD_PRODUCT_TYPES)
def test_route_b_sweep_kernels_equal_route_a_bitwise(api, contexts, fb, double_products, arithmetic):
    """k_collapse_inv (every radius but the last) and k_collapse_src (the last) inside compute_fmax against Route A's calls followed by
    compute_displacements(1, 0): TrueVariance, Fmax, Rmax and every Vel* column bit for bit.  Route A is held to the oracle above."""
    n = 32
    radii = np.array(cm.RADII[n])
    label = _label("sweep", n, fb, double_products, arithmetic)
    side = GpuSide(contexts(n, fb, double_products), "plain", arithmetic)
    tv_a = []
    for i, r in enumerate(radii):
        side.f.compute_second_derivatives(r)
        tv_a.append(side.collapse(i))
    _assert_six_component_collapse_ran(side, len(radii), label)
    side.f.compute_displacements(1, 0)
    pa = side.f.products()
    with _new_context(api, n, fb, double_products) as f:
        f.set_arithmetic(arithmetic)
        f.reset_kernel_stats()
        t = time.perf_counter()
        tv = f.compute_fmax(radii, do_lpt=True)
        p = f.products()
        seconds = time.perf_counter() - t
        cl = {k["name"]: k for k in f.kernel_stats() if k["launches"]}
    assert cl.get("collapse_inv", {}).get("launches") == len(radii) - 1 and cl.get("collapse_lpt_sources", {}).get("launches") == 1, (label, sorted(cl))
    assert "collapse" not in cl, (label, sorted(cl))
    assert np.array_equal(tv, np.array(tv_a)), (label, tv, tv_a)
    for name in ("Fmax", "Rmax") + VEL:
        assert np.array_equal(p[name], pa[name]), (label, name)
    assert all(np.abs(p[name]).max() > 0 for name in VEL) and (p["Rmax"] > 0).any() and (p["Rmax"] < len(radii) - 1).any()
    print("collapse-matrix-leg %s: bit for bit, device calls %.3f s collapse_inv %.3f ms collapse_lpt_sources %.3f ms"
          % (label, seconds, cl["collapse_inv"]["total_ms"], cl["collapse_lpt_sources"]["total_ms"]))


# ---- Route C -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arithmetic", cm.ARITHMETICS)
@pytest.mark.parametrize("fb,double_products", cm.FIELD_PRODUCT_TYPES)
def test_route_c_running_maximum_compares_the_promoted_product(contexts, fb, double_products, arithmetic):
    """(double)fold < Fnew (quirk Q2): a kernel that compared in product precision would pass every other test here"""
    side = GpuSide(contexts(32, fb, double_products), "plain", arithmetic)
    cm.run_running_maximum(side, lambda nr: cm.Reference(32, "plain", double_products, nr, noise=False), double_products,
                           _label("running maximum", 32, fb, double_products, arithmetic))


# ---- Route D -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [8, 4])
@pytest.mark.parametrize("flavour", [0, 1, 2])
def test_route_d_table_lookups_outside_the_table(contexts, references, flavour, fb):
    """the table made for 0.1 x the variance: |delta| > 7 sigma is extrapolated linearly, x, y > 3.5 sigma clamp the node index -- the
    device compilation of those branches, which tables made for the field's own variance never reach"""
    n, variant = 32, "tab%d" % flavour
    ref = references(n, variant, fb, False, 0.1)
    side = GpuSide(contexts(n, fb, False), variant, "fast")
    label = "outside " + _label(variant, n, fb, False, "fast")
    if not ref.passes:   # from the oracle's eigenvalues alone: the premise of the leg
        o = oracle_lib.Oracle(n, 0)
        o.set_density(cm.density(n))
        for i, r in enumerate(cm.RADII[n]):
            shares = cm.shares_outside_table(o.second_derivatives(r), ref.variance[i])
            assert min(shares) > 0.01, (r, shares)
        o.close()
    _leg(side, ref, n, False, "fast", label)


# ---- Route E -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,fb", [(20, 8), (24, 4)])
def test_route_e_partly_empty_last_workgroup(contexts, references, n, fb):
    """20^3 = 8000 cells: the 32nd workgroup of 256 threads is a quarter full (fp64 fields, the general path); 24^3 = 13824 cells with
    fp32 fields: 54 workgroups.  No n = 8 m grid of one rank has a whole number of workgroups' worth of cells to spare otherwise"""
    side = GpuSide(contexts(n, fb, False), "plain", "fast")
    _leg(side, references(n, "plain", fb, False), n, False, "fast", _label("plain", n, fb, False, "fast"))


@pytest.mark.parametrize("arithmetic", cm.ARITHMETICS)
def test_route_e_one_group_form_of_the_invariant_solve(api, contexts, references, arithmetic):
    """k_collapse_inv runs workgroups of two groups of 256 threads unless the block count is odd.  The count is
    min(ceil(cells of the rank / 256), CUs x PF_COLLAPSE_WG_PER_CU): the cap is even on any device with an even number of CUs, and a
    whole n = 8 m box has 2 m^3 blocks, so one rank never gets there -- a slab does: 16^3 on 16 ranks leaves each rank one plane of
    256 cells, ONE block, which two does not divide.  The slabs' Fmax / Rmax must be those of Route A's calls on one rank bit for bit
    (the per-line transforms are the same), and those are held to the oracle here."""
    from test_gpu_multirank import run_ranks
    n, P = 16, 16
    radii = np.array(cm.RADII[n])
    label = _label("one-group invariants", n, 8, False, arithmetic)
    side = GpuSide(contexts(n, 8, False), "plain", arithmetic)
    ref = references(n, "plain", 8, False)
    _leg(side, ref, n, False, arithmetic, _label("plain", n, 8, False, arithmetic))
    F1, R1 = side.products()
    F1, R1 = F1.reshape(n, n, n), R1.reshape(n, n, n)
    dk, (x, y) = cm.density(n), cm.invgrow()

    def body(f, r):
        f.set_arithmetic(arithmetic)
        f.set_density(dk[r:r + 1])
        f.set_invgrow(x, y)
        f.reset_kernel_stats()
        tv = f.sweep(radii)
        cl = {k["name"]: k["launches"] for k in f.kernel_stats() if k["launches"]}
        p = f.products()
        return tv, p["Fmax"], p["Rmax"], cl

    for r, (tv, F, R, cl) in enumerate(run_ranks(api, n, P, body, timing=True)):
        assert cl.get("collapse_inv", 0) >= 1 and cl.get("collapse_inv", 0) + cl.get("collapse", 0) == len(radii), (label, r, cl)
        assert np.allclose(tv, [ps.tv for ps in ref.passes], rtol=1e-12), (label, r)
        assert np.array_equal(F[0], F1[r]) and np.array_equal(R[0], R1[r]), (label, r)
