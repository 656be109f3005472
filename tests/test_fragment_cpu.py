"""The whole fragment() walk of tests/np_fragment.py on the numpy restatements alone, no device: what must close over the sub-boxes
does close, the inputs are not vacuous, and a wrong hand-off between two stages -- one at a time, made on purpose in a copy of the
walk -- is seen by the comparison tests/test_gpu_fragment.py applies to the device's walk, or breaks one of the closing invariants.

Inputs: an np_distribute.random_field Fmax, smoothed twice over the six neighbours (white noise has groups of a handful of particles;
the walk needs some of more than 64), and random velocity columns for the two segments.  At 16^3 a sub-box stores about 1250
particles, and 50 groups of ten and more beside one of more than 64 is near the most such a field gives: of 1200 seeds twelve reach
these counts and five of those every input condition; the case uses one of the five."""
import functools

import numpy as np
import pytest

import np_distribute as npd
import np_fragment as nf
import np_neighbours as npn

PRODUCT = np.dtype([("Rmax", "<i4"), ("Fmax", "<f4"), ("Vel", "<f4", 3), ("Vel_2LPT", "<f4", 3), ("Vel_3LPT_1", "<f4", 3), ("Vel_3LPT_2", "<f4", 3)])
# (n, sub-boxes, boundary layer, seed: one of those whose field meets np_fragment.input_conditions)
CASES = {"16, two tiles": (16, (2, 1, 1), 2, 939), "24, two tiles in y": (24, (1, 2, 1), 2, 130)}


def _products(n, seed):
    """the full-grid records of two segments: the same Fmax and Rmax, other velocities"""
    rng = np.random.default_rng(seed)
    f = npd.random_field(rng, (n, n, n), 0).astype(np.float64)
    for _ in range(2):
        f = (2.0 * f + sum(np.roll(f, s, axis=a) for a in range(3) for s in (-1, 1))) / 8.0
    f = 1.0 + 4.0 * (f - f.min()) / (f.max() - f.min())                      # 1 <= Fmax <= 5: the light cone's table starts at z = 0
    A = np.zeros((n, n, n), dtype=PRODUCT)
    A["Fmax"] = f.astype(np.float32)
    A["Rmax"] = rng.integers(0, 4, (n, n, n))
    B = A.copy()
    for p in (A, B):
        for k, name in enumerate(nf.VEL):
            p[name] = rng.normal(0.0, (1.0, 0.1, 0.03, 0.03)[k], (n, n, n, 3))
    return A, B


@functools.lru_cache(maxsize=None)
def _walk(name, wrong=None):
    """computed once per case and hand-off, shared, left alone"""
    n, nbox, layer, seed = CASES[name]
    A, B = _products(n, seed)
    flast = float(np.median(A["Fmax"]))
    par = nf.Params(n, nbox, layer)
    return nf.walk(nf.NumpyStages(A, B, flast, par), par, flast, wrong), A, B, flast, par


@pytest.mark.parametrize("name", list(CASES))
def test_the_chain_closes(name):
    res, A, B, flast, par = _walk(name)
    nf.invariants(res, A, B, flast, par)
    nf.compare(res, res)                                                   # the comparison accepts a walk against itself


@pytest.mark.parametrize("name", list(CASES))
def test_the_inputs_are_not_vacuous(name):
    res, A, B, flast, par = _walk(name)
    for f in nf.input_conditions(res, par):
        print(name, f)


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("wrong", nf.WRONG)
def test_a_wrong_hand_off_is_seen(name, wrong):
    ref, A, B, flast, par = _walk(name)
    res = _walk(name, wrong)[0]
    seen = []
    for check in (lambda: nf.compare(res, ref), lambda: nf.invariants(res, A, B, flast, par)):
        try:
            check()
        except AssertionError as e:
            seen.append(str(e).splitlines()[0][:120] if str(e) else "assert")
    print(wrong, "->", seen)
    assert seen, wrong


# the fp32 shapes of tests/test_gpu_fragment.py at LPT order 3: (n, sub-boxes, boundary layer)
DEVICE_SHAPES = {"whole": (32, (1, 1, 1), 0), "two tiles": (32, (2, 1, 1), 2), "mixed radix": (24, (1, 2, 1), 2)}


@pytest.mark.parametrize("name", list(DEVICE_SHAPES))
def test_the_device_walk_will_not_be_vacuous(oracle, name):
    """the inputs of the GPU test -- synth.make_density, the radii and the two growth sets of tests/test_gpu_refresh.py -- through the
    CPU oracle of the same arithmetic: the chain closes on them and they meet the input conditions (the GPU test asserts the same
    of the device's own products)"""
    from pinocchio_amd import synth
    n, nbox, layer = DEVICE_SHAPES[name]
    g1 = synth.growth_multipliers()
    o = oracle.Oracle(n, 0)
    o.set_density(synth.make_density(n, seed=synth.SEED))
    o.set_invgrow(*synth.invgrow_table("lcdm"))
    o.set_growth(g1)
    o.compute_fmax(np.array([2.0, 1.0, 0.5, 0.0]), do_lpt=True)
    A = o.products().copy()
    o.set_growth(g1 * np.array([0.75, 0.5, 0.625, 0.875]))
    o.displacements(False)
    B = o.products().copy()
    o.close()
    assert A["Fmax"].tobytes() == B["Fmax"].tobytes() and np.any(A["Vel"] != B["Vel"])
    flast = float(np.median(A["Fmax"]))
    par = nf.Params(n, nbox, layer)
    res = nf.walk(nf.NumpyStages(A, B, flast, par), par, flast)
    nf.invariants(res, A, B, flast, par)
    for f in nf.input_conditions(res, par):
        print(name, f)


def test_the_stand_in_reads_the_tables_only():
    """deterministic, IDs count from 2 in the order of the peaks, every member's chain of best neighbours ends in its group's peak"""
    res, A, B, flast, par = _walk("16, two tiles")
    for r in res["boxes"]:
        start, length, safe = r["box"]
        again = nf.stand_in_groups(r["rec0"]["Fmax"], r["pos"], r["neigh"], r["flags"], start, length, r["pbc"], par.n, flast, par.T)
        assert np.array_equal(again[0], r["gid"]) and again[1].tobytes() == r["zacc"].tobytes()
        gid, groups = r["gid"], r["groups"]
        first = nf.FIRST_GROUP
        pk = np.flatnonzero(r["flags"] & npn.PEAK)
        assert np.array_equal(gid[pk], np.arange(first, first + len(pk))) and np.array_equal(groups["point"][first:], pk)
        assert np.array_equal(groups["Mass"][first:], np.bincount(gid, minlength=len(groups))[first:]) and not groups["Mass"][:first].any()
        assert np.all(groups["Pos"][first:] >= 0) and np.all(groups["Pos"][first:] < np.asarray(length))
