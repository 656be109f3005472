"""PF_LPT_XFUSE: on one rank the forward x-pass of an LPT source spectrum runs inside the inverse x-passes that read it
(k_strided with PF_DIR_XF, csrc/pf_fft_kernels.hip) instead of as a launch of its own.  The fused kernel runs the stages, twiddles
and plan of the stand-alone forward pass on the tile it has loaded, so every result is the same BITS as with PF_LPT_XFUSE=0:
the products, the source spectra pf_get_kvector returns (which finishes a pending field with the plain forward pass first), and
the products of a re-entrant pf_displacements(0, 0) whether it finds the fields pending (fused again) or finished (plain passes).

Shapes: 128 fp64 (the paired radix-16 first stage, the plan of 1024-point lines: the line goes back through LDS into the paired
input order), 64 fp64 (plain plan; 33 columns in tiles of eight: the last tile holds one valid column), 256 fp64 (plain plan, three
stages, two exchanges), 128 with fp32 fields (k_strided<float>, tiles of sixteen columns, plain plan).  96 (mixed radix) and two
ranks are not covered by the change: the switch is a no-op there and the stand-alone forward x-pass still runs."""
import numpy as np
import pytest

from pinocchio_amd import synth

pytestmark = pytest.mark.gpu

COLUMNS = ("Vel", "Vel_2LPT", "Vel_3LPT_1", "Vel_3LPT_2")   # 4 x 3 = the twelve velocity columns
G2 = np.array([0.9, 0.41, -0.12, 0.13])
G3 = np.array([1.1, 0.37, -0.10, 0.11])


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


def fwd_launches(f):
    return sum(s["launches"] for s in f.kernel_stats() if s["name"] == "xpass_fwd")


def run_one(api, n, fb, seed=11):
    """one context, the whole sequence -> everything that must not depend on the switch, and the xpass_fwd launch counts on the way"""
    x, y = synth.invgrow_table("lcdm")
    out = {}
    with api.Fmax(n, field_bytes=fb, timing=True) as f:
        f.synth_density(seed)
        base = fwd_launches(f)                     # the density's own forward transform (not an LPT source: never fused)
        f.set_invgrow(x, y)
        f.set_growth(synth.growth_multipliers())
        out["tv"] = f.compute_fmax(synth.radii_ladder(3), do_lpt=True)
        out["p0"] = f.products()
        out["fwd0"] = fwd_launches(f) - base
        out["k1_before"] = f.kvector(1)            # S[1] finished in place; S[0] and S[2] stay as they are
        out["fwd1"] = fwd_launches(f) - base
        f.set_growth(G2)
        f.compute_displacements(0, 0)              # re-entry: S[0], S[2] as the first call left them, S[1] whole
        out["p1"] = f.products()
        out["fwd2"] = fwd_launches(f) - base
        out["k_after"] = [f.kvector(i) for i in range(3)]
        out["fwd3"] = fwd_launches(f) - base
        f.set_growth(G3)
        f.compute_displacements(0, 0)              # every field whole: the plain x-passes
        out["p2"] = f.products()
        out["fwd4"] = fwd_launches(f) - base
        out["base"] = base
    return out


_cache = {}


def both(api, monkeypatch, n, fb):
    if (n, fb) not in _cache:
        r = []
        for v in ("0", "1"):
            monkeypatch.setenv("PF_LPT_XFUSE", v)
            r.append(run_one(api, n, fb))
        _cache[(n, fb)] = r
    return _cache[(n, fb)]


def assert_same_products(a, b):
    for name in COLUMNS + ("Fmax", "Rmax"):
        assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), name


SHAPES = [(128, 8), (64, 8), (256, 8), (128, 4)]


@pytest.mark.parametrize("n,fb", SHAPES)
def test_products_and_spectra_are_the_same_bits(api, monkeypatch, n, fb):
    off, on = both(api, monkeypatch, n, fb)
    assert np.array_equal(off["tv"], on["tv"])
    for k in ("p0", "p1", "p2"):
        assert_same_products(off[k], on[k])
    assert np.array_equal(off["k1_before"].view(np.uint64), on["k1_before"].view(np.uint64))
    for i in range(3):
        assert np.array_equal(off["k_after"][i].view(np.uint64), on["k_after"][i].view(np.uint64)), i
    # a second pf_displacements does not touch the spectra
    assert np.array_equal(on["k1_before"].view(np.uint64), on["k_after"][1].view(np.uint64))
    # and the runs are not trivially equal: the growth multipliers changed the displacements
    assert not np.array_equal(on["p0"]["Vel_2LPT"], on["p1"]["Vel_2LPT"])
    assert np.any(on["p0"]["Vel_3LPT_2"] != 0)


@pytest.mark.parametrize("n,fb", SHAPES)
def test_the_forward_x_pass_runs_only_where_the_spectrum_is_asked_for(api, monkeypatch, n, fb):
    off, on = both(api, monkeypatch, n, fb)
    assert off["base"] == on["base"] == 1          # delta(k) of synth_density: the counts below are on top of it
    assert [off[k] for k in ("fwd0", "fwd1", "fwd2", "fwd3", "fwd4")] == [3, 3, 3, 3, 3]
    # fused: none in pf_displacements(1, 0); one for kvector(1); none in the re-entry (pending fields stay pending); two more
    # for kvector(0) and kvector(2); none afterwards
    assert [on[k] for k in ("fwd0", "fwd1", "fwd2", "fwd3", "fwd4")] == [0, 1, 1, 3, 3]


def test_mixed_radix_keeps_its_passes(api, monkeypatch):
    off, on = both(api, monkeypatch, 96, 8)
    for k in ("p0", "p1", "p2"):
        assert_same_products(off[k], on[k])
    for i in range(3):
        assert np.array_equal(off["k_after"][i].view(np.uint64), on["k_after"][i].view(np.uint64))
    assert [on[k] for k in ("fwd0", "fwd1", "fwd2", "fwd3", "fwd4")] == [3, 3, 3, 3, 3]


def test_two_ranks_keep_their_passes(api, monkeypatch):
    from test_gpu_multirank import run_ranks
    n, P = 64, 2
    dk = synth.make_density(n, seed=23)
    x, y = synth.invgrow_table("lcdm")
    nxl = n // P

    def body(f, r):
        f.set_density(dk[r * nxl:(r + 1) * nxl])
        f.set_invgrow(x, y)
        f.set_growth(synth.growth_multipliers())
        f.compute_fmax(synth.radii_ladder(3), do_lpt=True)
        return f.products(), f.kvector(2), fwd_launches(f)

    res = []
    for v in ("0", "1"):
        monkeypatch.setenv("PF_LPT_XFUSE", v)
        res.append(run_ranks(api, n, P, body, timing=True))
    for r in range(P):
        assert_same_products(res[0][r][0], res[1][r][0])
        assert np.array_equal(res[0][r][1].view(np.uint64), res[1][r][1].view(np.uint64))
        assert res[0][r][2] == res[1][r][2] > 0        # the stand-alone forward x-pass runs under either setting
