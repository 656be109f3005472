"""What the reference logged after distribute() (src/distribute.c:58-175; "... re-distribution of Fmax done, N particles stored by
all tasks" and "Smallest and largest overhead", src/fragment.c:285-301), reproduced on the CPU: the oracle's Fmax of the run + the
numpy restatement of the reference's loops (tests/np_distribute.py) against tests/golden/distribute_kat.json.

Single-task runs are all-periodic: one sub-box = the box, every map bit set, so the stored total is the number of collapsed cells
and the bound is that of the run's collapsed-cell check (5, 8, 100).

The example run: 128^3 on four tasks, sub-boxes 4 x 1 x 1, boundary layer 17, pbc 0 1 1.  In the first turn each task's map
(create_map, src/fragment.c:708-751) covers x from safe - 1 to Lgrid + safe + 1 of its sub-box, so eight planes of the box are
held by two tasks each and the total is the collapsed count plus the collapsed cells of those planes.
Measured here on the CPU oracle: total 730 927 against the logged 730 924; per task 181 831, 183 044, 184 104, 181 948; the logged
smallest and largest overheads 0.346813 and 0.351149 of 524 288 give 181 830 and 184 103; collapsed 687 252.
Bounds: per task 8, the run's collapsed-cell bound; 16 on the total, because a cell that crosses Flast in a shared plane counts twice;
on an overhead a further 0.5e-6 x ParticlesPerTask, because the log prints six decimals.

These tests need no device: they pin the restatement the GPU tests (tests/test_gpu_distribute.py) compare the kernels with.  The
f(R) run (minutes of table integrations on the CPU) is left to the GPU test.
"""
import json
import os

import numpy as np
import pytest

import ic_oracle
import np_distribute as npd
import oracle_lib

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _load(name):
    with open(os.path.join(GOLD, name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def logged():
    kat = _load("distribute_kat.json")
    assert kat["Flast"] == 1.0
    return {r["run"]: r for r in kat["runs"]}


def _box(p):
    return p["BoxSize_h100"] / p["Hubble100"]   # true Mpc


def _oracle_fmax(kat, dk, splines=None):
    p = kat["params"]
    n = p["GridSize"]
    o = oracle_lib.Oracle(n, 0)
    o.set_density(dk)
    if splines is None:
        x, y = ic_oracle.growth_table_lcdm(p["Omega0"])
        o.set_invgrow(x, y)
    else:
        for i in range(len(kat["radii_Mpc"])):
            o.set_invgrow_radius(i, *splines)
    o.compute_fmax(np.array(kat["radii_Mpc"]) / (_box(p) / n), do_lpt=False)
    return np.ascontiguousarray(o.products()["Fmax"]).reshape(n, n, n)


def stored_per_task(fmax, run, flast=1.0):
    """subbox.Nstored of every task after the first distribute() of a run with the logged geometry"""
    n = fmax.shape[0]
    tasks = run["tasks"]
    boxes = npd.subboxes(n, run["nbox"], max(run["safe"]))
    assert len(boxes) == tasks
    out = []
    for t, (stabl, lgwbl, lgrid, safe, pbc) in enumerate(boxes):
        assert lgwbl == run["Lgwbl"] and lgrid == run["Lgrid"] and safe == run["safe"] and [int(v) for v in pbc] == run["pbc"]
        words = npd.create_map(lgwbl, lgrid, safe, pbc)
        cells, pos = npd.distribute(fmax, tasks, stabl, lgwbl, flast, words, target=t)
        assert len(np.unique(pos)) == len(pos)
        out.append(len(cells))
    return out


def _check_single_task(run, fmax, bound):
    assert run["tasks"] == 1 and run["pbc"] == [1, 1, 1] and run["smallest_overhead"] == run["largest_overhead"]
    (stored,) = stored_per_task(fmax, run)
    with np.errstate(invalid="ignore"):
        assert stored == int((fmax.astype(np.float64) >= 1.0).sum())     # all-periodic: the stored total is the collapsed count
    print(run["run"], "stored", stored, "logged", run["stored"], "difference", stored - run["stored"])
    assert abs(stored - run["stored"]) <= bound, (stored, run["stored"])


@pytest.fixture(scope="module")
def hmf_fmax():
    kat = _load("hmf_validation_kat.json")
    p = kat["params"]
    return _oracle_fmax(kat, ic_oracle.genic(p["GridSize"], _box(p), p["RandomSeed"], kat["PkNorm"], p))


def test_fixture_holds_the_log_lines(logged):
    assert len(logged) == 6
    for r in logged.values():
        assert any("re-distribution of Fmax done, %d particles stored by all tasks" % r["stored"] in l for l in r["log_lines"])
        assert any(l.startswith("Smallest and largest overhead: %f, %f" % (r["smallest_overhead"], r["largest_overhead"])) for l in r["log_lines"])
        assert r["turn"] == ("Second" if r["tasks"] == 1 else "First")   # an all-periodic run skips the first turn
        assert r["particles_per_task"] * r["tasks"] == _load(r["setup"])["params"]["GridSize"] ** 3
    assert logged["RECOMPUTE_DISPLACEMENTS_LCDM"]["stored"] == logged["SCALE_DEP_LCDM"]["stored"]


def test_hmf_validation_stored(logged, hmf_fmax):
    _check_single_task(logged["HMF_Validation"], hmf_fmax, 5)


def test_lcdm_256_stored(logged):
    kat = _load("hmf256_kat.json")
    p = kat["params"]
    fmax = _oracle_fmax(kat, ic_oracle.genic(p["GridSize"], _box(p), p["RandomSeed"], kat["PkNorm"], p, fixed=bool(p["FixedIC"])))
    _check_single_task(logged["RECOMPUTE_DISPLACEMENTS_LCDM"], fmax, 8)
    _check_single_task(logged["SCALE_DEP_LCDM"], fmax, 8)


def test_read_pk_table_256_stored(logged):
    kat = _load("readpk256_kat.json")
    p = kat["params"]
    t = np.array(kat["camb_z0_k_hMpc_P"])
    pk_table = (np.log10(t[:, 0] * p["Hubble100"]), np.log10(t[:, 0] ** 3 * t[:, 1]))
    g = np.array(kat["scaledep_a_D1"])
    dk = ic_oracle.genic(p["GridSize"], _box(p), p["RandomSeed"], 1.0, p, fixed=True, pk_table=pk_table)
    fmax = _oracle_fmax(kat, dk, splines=(np.log10(g[:, 1]), np.log10(g[:, 0])))
    _check_single_task(logged["READ_PK_TABLE_and_SCALE_DEP"], fmax, 100)


def check_four_task_run(run, per_task, bound):
    """the first-turn total and both overheads of a four-task run against the log; bound: the run's collapsed-cell bound"""
    ppt = run["particles_per_task"]
    total = sum(per_task)
    rounding = 0.5e-6 * ppt
    print(run["run"], "per task", per_task, "total", total, "logged", run["stored"], "difference", total - run["stored"])
    print("   smallest", min(per_task), "logged overhead x ParticlesPerTask", run["smallest_overhead"] * ppt, "difference",
          min(per_task) - run["smallest_overhead"] * ppt)
    print("   largest ", max(per_task), "logged overhead x ParticlesPerTask", run["largest_overhead"] * ppt, "difference",
          max(per_task) - run["largest_overhead"] * ppt)
    assert abs(total - run["stored"]) <= 2 * bound, (total, run["stored"])
    assert abs(min(per_task) - run["smallest_overhead"] * ppt) <= bound + rounding
    assert abs(max(per_task) - run["largest_overhead"] * ppt) <= bound + rounding


def test_example_first_turn(logged):
    kat = _load("example_kat.json")
    p = kat["params"]
    run = logged["example"]
    assert (run["tasks"], run["nbox"], run["safe"], run["pbc"], run["particles_per_task"]) == (4, [4, 1, 1], [17, 0, 0], [0, 1, 1], 524288)
    fmax = _oracle_fmax(kat, ic_oracle.genic(p["GridSize"], _box(p), p["RandomSeed"], kat["PkNorm"], p))
    per_task = stored_per_task(fmax, run)
    check_four_task_run(run, per_task, 8)
    # eight planes are held by two tasks each: the total is the collapsed count plus the collapsed cells of those planes
    n = fmax.shape[0]
    collapsed = fmax.astype(np.float64) >= 1.0
    shared = [(t * 32 + d) % n for t in range(4) for d in (-1, 32)]
    assert sum(per_task) == int(collapsed.sum()) + int(collapsed[shared].sum())
    print("collapsed", int(collapsed.sum()))


def well_resolved_map(lgwbl, lgrid, safe):
    cube = np.zeros(tuple(lgwbl), dtype=bool)
    cube[tuple(slice(safe[d], safe[d] + lgrid[d]) for d in range(3))] = True
    return npd.pack_map(cube)


@pytest.mark.parametrize("nbox", [(2, 2, 1), (2, 2, 2), (4, 1, 1)])
@pytest.mark.parametrize("boundary", [1, 2, 3])
def test_contributions_of_a_tiling_hold_every_collapsed_cell_once(hmf_fmax, nbox, boundary):
    """with the maps of the well resolved parts alone the sub-boxes tile the box: every collapsed cell is stored exactly once"""
    n = hmf_fmax.shape[0]
    tasks = nbox[0] * nbox[1] * nbox[2]
    times = np.zeros(n ** 3, dtype=np.int32)
    for t, (stabl, lgwbl, lgrid, safe, pbc) in enumerate(npd.subboxes(n, nbox, boundary)):
        cells, pos = npd.distribute(hmf_fmax, tasks, stabl, lgwbl, 1.0, well_resolved_map(lgwbl, lgrid, safe), target=t)
        assert len(np.unique(pos)) == len(pos)                       # frag_pos is unique within a sub-box
        np.add.at(times, cells, 1)
        # ... and names the cell: sub-box coordinates back to the global ones
        px, rest = np.divmod(pos, lgwbl[1] * lgwbl[2])
        py, pz = np.divmod(rest, lgwbl[2])
        back = (((px + stabl[0]) % n) * n + (py + stabl[1]) % n) * n + (pz + stabl[2]) % n
        assert np.array_equal(back, cells)
    assert np.array_equal(times, (hmf_fmax.astype(np.float64) >= 1.0).ravel().astype(np.int32))


def _hand_made():
    f = np.zeros((4, 4, 4), dtype=np.float32)
    f[0, 1, 2] = f[3, 0, 1] = f[2, 0, 3] = f[2, 3, 0] = 2.0
    return f


def _as_lists(got):
    return [int(v) for v in got[0]], [int(v) for v in got[1]]


def test_restatement_on_hand_made_fields():
    f = _hand_made()
    # a wrap in x: the sub-box holds x = 3, 0; the wrapped segment (x = 0) comes first.  Cell (0,1,2) = index 6 sits at sub-box
    # coordinates (1,1,2) = 2 + 4 (1 + 4 * 1) = 22, cell (3,0,1) = 49 at (0,0,1) = 1
    assert _as_lists(npd.distribute(f, 1, (3, 0, 0), (2, 4, 4), 1.0)) == ([6, 49], [22, 1])
    # a negative start names the same sub-box
    assert _as_lists(npd.distribute(f, 1, (-1, 0, 0), (2, 4, 4), 1.0)) == ([6, 49], [22, 1])
    # a wrap in y: y = 3, 0; box y = 0 first, with (2,0,3) = 35 at (2,1,3) = 3 + 4 (1 + 2 * 2) = 23 and (3,0,1) = 49 at (3,1,1) = 29; then
    # y = 3 with (2,3,0) = 44 at (2,0,0) = 16
    assert _as_lists(npd.distribute(f, 1, (0, 3, 0), (4, 2, 4), 1.0)) == ([35, 49, 44], [23, 29, 16])
    # a wrap in z: z = 2, 3, 0; box z = 0 first, with (2,3,0) = 44 at (2,3,2) = 2 + 3 (3 + 4 * 2) = 35; then (0,1,2) = 6 at (0,1,0) = 3
    # and (2,0,3) = 35 at (2,0,1) = 25
    assert _as_lists(npd.distribute(f, 1, (0, 0, 2), (4, 4, 3), 1.0)) == ([44, 6, 35], [35, 3, 25])
    # two slabs: the owner's own cells first, then the partner's
    assert _as_lists(npd.distribute(f, 2, (3, 0, 0), (2, 4, 4), 1.0, target=0)) == ([6, 49], [22, 1])
    assert _as_lists(npd.distribute(f, 2, (3, 0, 0), (2, 4, 4), 1.0, target=1)) == ([49, 6], [1, 22])
    # a map that clears the cell at 22
    bits = np.ones((2, 4, 4), dtype=bool)
    bits.ravel()[22] = False
    assert _as_lists(npd.distribute(f, 1, (3, 0, 0), (2, 4, 4), 1.0, npd.pack_map(bits))) == ([49], [1])
    # NaN is never taken
    g = f.copy()
    g[3, 0, 1] = np.nan
    assert _as_lists(npd.distribute(g, 1, (3, 0, 0), (2, 4, 4), 1.0)) == ([6], [22])
    assert _as_lists(npd.distribute(g, 1, (3, 0, 0), (2, 4, 4), -np.inf)) == (list(range(0, 16)) + list(range(48, 49)) + list(range(50, 64)),
                                                                             list(range(16, 32)) + list(range(0, 1)) + list(range(2, 16)))
    # a cell equal to Flast is taken; not for the next double above it (outputs.Flast is a double)
    g = f.copy()
    g[0, 1, 2] = 1.0
    assert _as_lists(npd.distribute(g, 1, (3, 0, 0), (2, 4, 4), 1.0)) == ([6, 49], [22, 1])
    assert _as_lists(npd.distribute(g, 1, (3, 0, 0), (2, 4, 4), float(np.nextafter(1.0, 2.0)))) == ([49], [1])
    # a sub-box that misses the slab
    c, w = npd.contribution(f[0:2], 4, 0, (2, 0, 0), (2, 4, 4), 1.0)
    assert len(c) == 0 and len(w) == 0


def test_create_map_and_the_hypercube_order():
    # the example's sub-box: 66 x 128 x 128, the map covers x = 16 .. 49 (safe - 1 .. Lgrid + safe) and all of y, z
    words = npd.create_map((66, 128, 128), (32, 128, 128), (17, 0, 0), (False, True, True))
    assert words.dtype == np.uint32 and words.size == 66 * 128 * 128 // 32
    bits = npd.map_bits(words, 66 * 128 * 128).reshape(66, 128, 128)
    assert bits[16:50].all() and not bits[:16].any() and not bits[50:].any()
    assert npd.create_map((4, 4, 4), (4, 4, 4), (0, 0, 0), (True, True, True)).tolist() == [0xFFFFFFFF, 0xFFFFFFFF]
    assert npd.pack_map(np.ones((3, 3, 5), dtype=bool)).tolist() == [0xFFFFFFFF, 0x1FFF]       # 45 bits: the last word is partial
    # distribute()'s loop (src/distribute.c:115-148) written out: who sends to `target`, in the order the rounds come
    for ntasks in (1, 2, 3, 4, 5, 8):
        log_ntask = 0
        while (1 << log_ntask) < ntasks:
            log_ntask += 1
        for target in range(ntasks):
            order = [target]
            for bit in range(1, 1 << log_ntask):
                for sender in range(ntasks):
                    receiver = sender ^ bit
                    if receiver < ntasks and sender < receiver:
                        if receiver == target:
                            order.append(sender)
                        if sender == target:
                            order.append(receiver)
            assert npd.hypercube_order(ntasks, target) == order
    assert npd.hypercube_order(4, 2) == [2, 3, 0, 1] and npd.hypercube_order(3, 0) == [0, 1, 2] and npd.hypercube_order(3, 2) == [2, 0, 1]
