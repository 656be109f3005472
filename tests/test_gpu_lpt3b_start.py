"""PF_LPT3B_START: the start value of the 3LPT(b) source, 2 (h11 + h22 + h33) S2(h), is a function of the six first-order Hessian
components.  By default (0) the solve of the sweep's last radius no longer stores it and the z-pass that contracts the second-order
Hessian into the source (k_c2r_invariants, MODE 2) forms it from the components it loads anyway, by the solve's own
pf_lpt_sources_cell and rounded to the field type as the stored value was; 1 writes and reads the field as before.  Same bits either
way.  Where the start value is not formed in the sweep (pf_displacements(1, 1): k_lpt_sources), where the contraction is a kernel of
its own (PF_LPT_FUSE=0) and on the mixed-radix sizes the field is written and read as before and the switch changes nothing."""
import numpy as np
import pytest

from pinocchio_amd import synth

pytestmark = pytest.mark.gpu

COLUMNS = ("Vel", "Vel_2LPT", "Vel_3LPT_1", "Vel_3LPT_2")


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


def run_one(api, n, fb, recompute=False, seed=11):
    x, y = synth.invgrow_table("lcdm")
    out = {}
    with api.Fmax(n, field_bytes=fb, timing=True) as f:
        f.synth_density(seed)
        f.set_invgrow(x, y)
        f.set_growth(synth.growth_multipliers())
        if recompute:
            # the sweep forms the sources in passing (and may leave the start value out); pf_displacements(1, 1) then computes the
            # Hessian at R = 0 again and runs k_lpt_sources: all three sources written
            f._chk(f.L.pf_set_sources_in_sweep(f.h, 1))
            out["tv"] = f.sweep(synth.radii_ladder(3))
            f._chk(f.L.pf_set_sources_in_sweep(f.h, 0))
            f.compute_displacements(1, 1)
        else:
            out["tv"] = f.compute_fmax(synth.radii_ladder(3), do_lpt=True)
        out["p"] = f.products()
        out["k"] = [f.kvector(i) for i in range(3)]
        st = {s["name"]: s for s in f.kernel_stats()}
        out["lpt3b_bytes"] = st["zpass_c2r_hess_6_lpt3b"]["alg_bytes"] if "zpass_c2r_hess_6_lpt3b" in st else None
        out["real_bytes"] = float(n) ** 3 * fb
    return out


def both(api, monkeypatch, n, fb, **kw):
    r = []
    for v in ("1", "0"):
        monkeypatch.setenv("PF_LPT3B_START", v)
        r.append(run_one(api, n, fb, **kw))
    return r


def assert_same(a, b):
    assert np.array_equal(a["tv"], b["tv"])
    for name in COLUMNS + ("Fmax", "Rmax"):
        assert np.array_equal(a["p"][name].view(np.uint32), b["p"][name].view(np.uint32)), name
    for i in range(3):
        assert np.array_equal(a["k"][i].view(np.uint64), b["k"][i].view(np.uint64)), i


@pytest.mark.parametrize("n,fb", [(128, 8), (64, 8), (256, 8), (128, 4)])
def test_start_value_formed_in_the_zpass_gives_the_same_bits(api, monkeypatch, n, fb):
    stored, formed = both(api, monkeypatch, n, fb)
    assert_same(stored, formed)
    assert np.any(formed["p"]["Vel_3LPT_2"] != 0)
    # the z-pass took the other mode: it no longer reads the source field (one real field less in its algorithmic bytes)
    assert stored["lpt3b_bytes"] - formed["lpt3b_bytes"] == pytest.approx(stored["real_bytes"], rel=1e-12)


def test_sources_from_k_lpt_sources_keep_the_field(api, monkeypatch):
    stored, formed = both(api, monkeypatch, 64, 8, recompute=True)
    assert_same(stored, formed)
    assert stored["lpt3b_bytes"] == formed["lpt3b_bytes"]


def test_unfused_contraction_keeps_the_field(api, monkeypatch):
    monkeypatch.setenv("PF_LPT_FUSE", "0")
    stored, formed = both(api, monkeypatch, 64, 8)
    assert_same(stored, formed)
    assert stored["lpt3b_bytes"] is None and formed["lpt3b_bytes"] is None
    monkeypatch.delenv("PF_LPT_FUSE")
    monkeypatch.setenv("PF_LPT3B_START", "0")
    assert_same(formed, run_one(api, 64, 8))     # ... and equals the fused contraction


def test_mixed_radix_keeps_the_field(api, monkeypatch):
    stored, formed = both(api, monkeypatch, 96, 8)
    assert_same(stored, formed)
    assert stored["lpt3b_bytes"] == formed["lpt3b_bytes"]
