"""distribute() on the device (pf_distribute, pf_debug_distribute; csrc/pf_distribute.hip) against the numpy restatement of the
reference's loops (tests/np_distribute.py, pinned on the CPU by tests/test_distribute_kat.py and tests/test_distribute_boxes.py).
Selections, orders and records are integers and bytes: every comparison with the restatement is exact.  The last part repeats the
reference's logged totals on the device."""
import json
import os

import numpy as np
import pytest

import ic_oracle
import np_distribute as npd
from pinocchio_amd import synth
from test_gpu_multirank import run_ranks

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
RADII = np.array([2.0, 1.0, 0.5, 0.0])


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


def _swept(api, n, seed=5, lpt=True, **kw):
    f = api.Fmax(n, **kw)
    f.set_density(synth.make_density(n, seed=seed))
    f.set_invgrow(*synth.invgrow_table("lcdm"))
    f.sweep(RADII)
    if lpt:
        f.set_growth(synth.growth_multipliers())
        f.compute_displacements(1, 0)
    return f


def _same_records(rec, want):
    """byte for byte: every field of the structured records, and zeros in the bytes no field names"""
    if rec.dtype != want.dtype or rec.shape != want.shape:
        return False
    named = np.zeros(rec.dtype.itemsize, dtype=bool)
    for name in rec.dtype.names:
        dt, off = rec.dtype.fields[name][:2]
        named[off:off + dt.itemsize] = True
        if np.ascontiguousarray(rec[name]).tobytes() != np.ascontiguousarray(want[name]).tobytes():
            return False
    raw = np.ascontiguousarray(rec).view(np.uint8).reshape(len(rec), rec.dtype.itemsize)
    return not raw[:, ~named].any()


# ------------------------------------------------------------------------------------------------------------------------
# selection and order: the test tap on a caller's slab
# 16: small boxes of a few wavefronts, 24 / 96 / 200: rows that are no multiple of 64 cells, 50: odd slabs
@pytest.mark.parametrize("n,count", [(16, 84), (24, 84), (50, 42), (96, 28), (200, 14)])
def test_debug_distribute_equals_the_restatement(api, n, count):
    taken = 0
    for k, (x0, nxl, start, length, words, flast, field) in enumerate(npd.random_cases(n, count, seed=n)):
        wcell, wpos = npd.contribution(field, n, x0, start, length, flast, words)
        pos, cell, cnt = api.debug_distribute(field, x0, flast, start, length, words)
        assert cnt == len(wcell), (k, x0, nxl, start, length, flast)
        assert np.array_equal(pos, wpos) and np.array_equal(cell, wcell), (k, x0, nxl, start, length, flast)
        taken += cnt
        # capacity smaller than, equal to and larger than the count; a count-only call
        for cap in sorted({0, cnt // 2, max(cnt - 1, 0), cnt, cnt + 5}):
            p2, c2, n2 = api.debug_distribute(field, x0, flast, start, length, words, capacity=cap)
            m = min(cap, cnt)
            assert n2 == cnt and len(p2) == m and np.array_equal(p2, wpos[:m]) and np.array_equal(c2, wcell[:m]), (k, cap)
    assert taken > 0


def test_debug_distribute_on_hand_made_fields(api):
    """the 4^3 cases of tests/test_distribute_kat.py on the device"""
    f = np.zeros((4, 4, 4), dtype=np.float32)
    f[0, 1, 2] = f[3, 0, 1] = f[2, 0, 3] = f[2, 3, 0] = 2.0

    def run(field, start, length, flast, words=None, x0=0):
        pos, cell, cnt = api.debug_distribute(field, x0, flast, start, length, words)
        assert cnt == len(pos)
        return cell.tolist(), pos.tolist()

    assert run(f, (3, 0, 0), (2, 4, 4), 1.0) == ([6, 49], [22, 1])
    assert run(f, (-1, 0, 0), (2, 4, 4), 1.0) == ([6, 49], [22, 1])
    assert run(f, (0, 3, 0), (4, 2, 4), 1.0) == ([35, 49, 44], [23, 29, 16])
    assert run(f, (0, 0, 2), (4, 4, 3), 1.0) == ([44, 6, 35], [35, 3, 25])
    bits = np.ones((2, 4, 4), dtype=bool)
    bits.ravel()[22] = False
    assert run(f, (3, 0, 0), (2, 4, 4), 1.0, npd.pack_map(bits)) == ([49], [1])
    g = f.copy()
    g[3, 0, 1] = np.nan
    assert run(g, (3, 0, 0), (2, 4, 4), 1.0) == ([6], [22])
    assert len(run(g, (3, 0, 0), (2, 4, 4), -np.inf)[0]) == 31
    g = f.copy()
    g[0, 1, 2] = 1.0
    assert run(g, (3, 0, 0), (2, 4, 4), 1.0) == ([6, 49], [22, 1])
    assert run(g, (3, 0, 0), (2, 4, 4), float(np.nextafter(1.0, 2.0))) == ([49], [1])
    # slabs: the second half of the box holds x = 3 (local plane 1: cell 17); the first half misses a sub-box of x = 2, 3
    assert run(f[2:4], (3, 0, 0), (2, 4, 4), 1.0, x0=2) == ([17], [1])
    assert run(f[0:2], (2, 0, 0), (2, 4, 4), 1.0) == ([], [])


def test_errors_in_the_house_format(api, capfd):
    n = 16
    with api.Fmax(n) as f:
        with pytest.raises(api.PinfmaxError, match="pf_distribute: products not computed"):
            f.distribute(1.0, (0, 0, 0), (n, n, n))
        f.set_density(synth.make_density(n, seed=5))
        f.set_invgrow(*synth.invgrow_table("lcdm"))
        f.sweep(RADII)
        for length, text in (((n, n + 1, n), r"len\[1\] = 17 outside \[1, 16\]"), ((0, n, n), r"len\[0\] = 0 outside \[1, 16\]")):
            with pytest.raises(api.PinfmaxError, match="pf_distribute: sub-box does not fit the box: " + text):
                f.distribute(1.0, (0, 0, 0), length)
        lay, _ = f.product_layout()
        lay.off_Vel = 6
        with pytest.raises(api.PinfmaxError, match="pf_distribute: bad layout"):
            f.distribute(1.0, (0, 0, 0), (n, n, n), layout=lay)
        lay, _ = f.product_layout()
        lay.off_Vel_2LPT = lay.off_Vel + 8
        with pytest.raises(api.PinfmaxError, match="pf_distribute: fields of the layout overlap"):
            f.distribute(1.0, (0, 0, 0), (n, n, n), layout=lay)
        with pytest.raises(ValueError, match="map of 3 words"):
            f.distribute(1.0, (0, 0, 0), (n, n, n), map=np.zeros(3, dtype=np.uint32))
    assert "ERROR on task 0: pf_distribute: sub-box does not fit the box" in capfd.readouterr().out
    with pytest.raises(api.PinfmaxError, match="pf_debug_distribute: sub-box does not fit the box"):
        api.debug_distribute(np.zeros((4, 4, 4), dtype=np.float32), 0, 1.0, (0, 0, 0), (5, 4, 4))


# ------------------------------------------------------------------------------------------------------------------------
# records
def _subboxes_for_records(n, seed):
    rng = np.random.default_rng(seed)
    out = [((0, 0, 0), (n, n, n)), ((-3, n - 2, 5), (n // 2, 7, n))]
    for kind in (0, 1, 2, 3, 5):
        out.append(npd.random_subbox(rng, n, 0, n, kind))
    return out


def _padded_layout(api_lib, stride, wpe):
    """no Rmax, no Vel_2LPT, gaps between the fields"""
    lay = api_lib.ProductLayout()
    lay.stride, lay.off_Rmax, lay.off_Fmax, lay.off_Vel_2LPT = stride, -1, 8, -1
    lay.off_Vel, lay.off_Vel_3LPT_1, lay.off_Vel_3LPT_2 = 16 + 4 * wpe, 16 + 20 * wpe, 16 + 36 * wpe
    return lay


def _rows_in_layout(prod, lay, pb):
    """the rows of a structured product array as bytes in another layout"""
    out = np.zeros((len(prod), lay.stride), dtype=np.uint8)
    for name, off, width in (("Rmax", lay.off_Rmax, 4), ("Fmax", lay.off_Fmax, pb), ("Vel", lay.off_Vel, 3 * pb), ("Vel_2LPT", lay.off_Vel_2LPT, 3 * pb),
                             ("Vel_3LPT_1", lay.off_Vel_3LPT_1, 3 * pb), ("Vel_3LPT_2", lay.off_Vel_3LPT_2, 3 * pb)):
        if off >= 0:
            out[:, off:off + width] = np.ascontiguousarray(prod[name]).view(np.uint8).reshape(len(prod), width)
    return out


def _check_records(api, f, n, flast=1.0, seed=0):
    from pinocchio_amd import _lib
    pb = 8 if f.double_products else 4
    prod = f.products().reshape(-1)
    fmax = np.ascontiguousarray(prod["Fmax"]).reshape(n, n, n)
    assert np.abs(prod["Vel_3LPT_2"]).max() > 0
    rng = np.random.default_rng(seed + n)
    total = 0
    for k, (start, length) in enumerate(_subboxes_for_records(n, seed + n)):
        words = None if k % 2 == 0 else npd.pack_map(rng.random(tuple(length)) < 0.7)
        wcell, wpos = npd.contribution(fmax, n, 0, start, length, flast, words)
        rec, pos, cnt = f.distribute(flast, start, length, map=words)
        assert cnt == len(wcell) and np.array_equal(pos, wpos), (start, length)
        assert _same_records(rec, prod[wcell]), (start, length)
        total += cnt
        # absent fields and padding; a record too long for the LDS form (the plain pack)
        for stride in (16 + 52 * (pb // 4), 16 + 52 * (pb // 4) + 240):
            lay = _padded_layout(_lib, stride, pb // 4)
            rows, pos, cnt = f.distribute(flast, start, length, map=words, layout=lay)
            assert rows.shape == (len(wcell), stride) and np.array_equal(pos, wpos)
            assert np.array_equal(rows, _rows_in_layout(prod[wcell], lay, pb)), (start, length, stride)
        # capacity below the count: the first entries, and the count of all
        cap = cnt // 3
        rec, pos, cnt2 = f.distribute(flast, start, length, map=words, capacity=cap)
        assert cnt2 == cnt and len(rec) == cap and _same_records(rec, prod[wcell[:cap]]) and np.array_equal(pos, wpos[:cap])
    assert total > 0
    # a sub-box that misses nothing but takes nothing
    rec, pos, cnt = f.distribute(np.inf, (0, 0, 0), (n, n, n))
    assert cnt == 0 and len(rec) == 0 and len(pos) == 0


@pytest.mark.parametrize("n", [24, 64, 128])
def test_records_equal_the_selected_rows_of_get_products(api, n):
    with _swept(api, n) as f:
        _check_records(api, f, n)


@pytest.mark.parametrize("n", [24, 64])
def test_records_with_double_products(api, n):
    with _swept(api, n, double_products=True) as f:
        assert f.products().dtype.itemsize == 112
        _check_records(api, f, n, seed=1)


def test_records_with_fp32_fields_and_before_the_displacements(api):
    n = 32
    with _swept(api, n, lpt=False, field_bytes=4) as f:
        prod = f.products().reshape(-1)
        assert not np.any(prod["Vel"])                         # src/collapse_times.c:472-489: the displacements read as zero
        fmax = np.ascontiguousarray(prod["Fmax"]).reshape(n, n, n)
        wcell, wpos = npd.contribution(fmax, n, 0, (5, -4, 30), (20, n, 9), 1.0)
        rec, pos, cnt = f.distribute(1.0, (5, -4, 30), (20, n, 9))
        assert cnt == len(wcell) > 0 and np.array_equal(pos, wpos) and _same_records(rec, prod[wcell])


def test_the_plain_pack_gives_the_same_records(api, monkeypatch):
    """PF_DISTRIBUTE_LDS=0: one lane per record into a cleared buffer, the form the staged pack is measured against"""
    n = 64
    monkeypatch.setenv("PF_DISTRIBUTE_LDS", "0")
    with _swept(api, n) as f:
        _check_records(api, f, n, seed=2)


# ------------------------------------------------------------------------------------------------------------------------
# pieces
def _halves_equal_the_whole(f, n, flast):
    whole, wpos, cnt = f.distribute(flast, (0, 0, 0), (n, n, n))
    h = n // 2
    a, apos, ca = f.distribute(flast, (0, 0, 0), (h, n, n))
    b, bpos, cb = f.distribute(flast, (h, 0, 0), (h, n, n))
    assert cnt == ca + cb == len(whole)
    assert _same_records(whole, np.concatenate([a, b]))
    assert np.array_equal(wpos, np.concatenate([apos, bpos.astype(np.int64) + h * n * n]))
    return cnt


def test_a_result_of_many_pieces_equals_its_halves(api, monkeypatch):
    """staging pieces of 1 MB: the 64^3 box leaves in sixteen pieces (and the halves in eight)"""
    n = 64
    monkeypatch.setenv("PF_HANDOFF_CHUNK_MB", "1")
    with _swept(api, n) as f:
        assert _halves_equal_the_whole(f, n, -np.inf) == n ** 3
        assert 0 < _halves_equal_the_whole(f, n, 1.0) < n ** 3
        prod = f.products().reshape(-1)
        rec, pos, cnt = f.distribute(-np.inf, (0, 0, 0), (n, n, n))
        assert _same_records(rec, prod) and np.array_equal(pos, np.arange(n ** 3))


def test_a_256_cubed_box_leaves_in_pieces(api):
    """every cell of 256^3 is 940 MB of records: more than one staging piece (a field, at most 256 MB)"""
    n = 256
    with _swept(api, n, lpt=False) as f:
        assert _halves_equal_the_whole(f, n, -np.inf) == n ** 3


# ------------------------------------------------------------------------------------------------------------------------
# slabs
@pytest.mark.parametrize("n,P,nbox", [(64, 2, (2, 1, 1)), (64, 4, (2, 2, 1)), (64, 8, (2, 2, 2)), (96, 3, (3, 1, 1))])
def test_slabs_concatenated_in_the_order_of_distribute(api, n, P, nbox):
    """P ranks on one GPU through the in-process fabric, P sub-boxes of a tiling with a boundary layer of 3: every rank calls
    distribute for every sub-box; concatenated in distribute()'s order (the owner's own cells, then the hypercube loop) the
    contributions are the restatement's frag[] / frag_pos[], and as a set the single-rank context's answer"""
    dk = synth.make_density(n, seed=23 + P)
    x, y = synth.invgrow_table("lcdm")
    nxl = n // P
    boxes = npd.subboxes(n, nbox, 3)
    assert len(boxes) == P
    maps = [npd.create_map(lgwbl, lgrid, safe, pbc) for (_, lgwbl, lgrid, safe, pbc) in boxes]
    with api.Fmax(n) as f1:
        f1.set_density(dk); f1.set_invgrow(x, y); f1.sweep(RADII)
        prod = f1.products().reshape(-1)
        single = [f1.distribute(1.0, b[0], b[1], map=m) for b, m in zip(boxes, maps)]
    fmax = np.ascontiguousarray(prod["Fmax"]).reshape(n, n, n)

    def body(f, r):
        f.set_density(dk[r * nxl:(r + 1) * nxl]); f.set_invgrow(x, y); f.sweep(RADII)
        return [f.distribute(1.0, b[0], b[1], map=m) for b, m in zip(boxes, maps)]

    res = run_ranks(api, n, P, body)
    for t, (stabl, lgwbl, _, _, _) in enumerate(boxes):
        order = npd.hypercube_order(P, t)
        rec = np.concatenate([res[r][t][0] for r in order])
        pos = np.concatenate([res[r][t][1] for r in order])
        wcell, wpos = npd.distribute(fmax, P, stabl, lgwbl, 1.0, maps[t], target=t)
        assert sum(res[r][t][2] for r in range(P)) == len(wcell) > 0
        assert np.array_equal(pos, wpos), t
        assert _same_records(rec, prod[wcell]), t
        # the single-rank context: the same set
        srec, spos, scnt = single[t]
        assert scnt == len(pos)
        a, b = np.argsort(pos, kind="stable"), np.argsort(spos, kind="stable")
        assert np.array_equal(pos[a], spos[b]) and _same_records(rec[a], srec[b]), t


# ------------------------------------------------------------------------------------------------------------------------
# The reference's logs on the device: the committed runs, set up as tests/test_gpu_peaks.py sets them up; the totals of
# tests/golden/distribute_kat.json within the bound of the collapsed-cell check of the same run (5, 8, 8, 100, 40), doubled for the
# totals of the four-task runs, plus the print-rounding term on the overheads (tests/test_distribute_kat.py has the derivation).
def _kat(name):
    with open(os.path.join(GOLD, name)) as fh:
        return json.load(fh)


def _logged(run):
    return [r for r in _kat("distribute_kat.json")["runs"] if r["run"] == run][0]


def _box(p):
    return p["BoxSize_h100"] / p["Hubble100"]


def _report(name, f, n, bound):
    run = _logged(name)
    boxes = npd.subboxes(n, run["nbox"], max(run["safe"]))
    per_task = []
    for stabl, lgwbl, lgrid, safe, pbc in boxes:
        assert lgwbl == run["Lgwbl"] and lgrid == run["Lgrid"] and safe == run["safe"]
        _, _, cnt = f.distribute(1.0, stabl, lgwbl, map=npd.create_map(lgwbl, lgrid, safe, pbc), capacity=0)
        per_task.append(cnt)
    total, ppt = sum(per_task), run["particles_per_task"]
    print(name, "device per task", per_task, "total", total, "logged", run["stored"], "difference", total - run["stored"])
    if run["tasks"] == 1:
        assert abs(total - run["stored"]) <= bound, (total, run["stored"])
        return
    rounding = 0.5e-6 * ppt
    print("   smallest", min(per_task), "-", run["smallest_overhead"] * ppt, "largest", max(per_task), "-", run["largest_overhead"] * ppt)
    assert abs(total - run["stored"]) <= 2 * bound, (total, run["stored"])
    assert abs(min(per_task) - run["smallest_overhead"] * ppt) <= bound + rounding
    assert abs(max(per_task) - run["largest_overhead"] * ppt) <= bound + rounding


def test_device_reproduces_the_logged_total_of_hmf_validation(api):
    kat = _kat("hmf_validation_kat.json")
    p = kat["params"]
    n = p["GridSize"]
    with api.Fmax(n) as f:
        f.set_density(ic_oracle.genic(n, _box(p), p["RandomSeed"], kat["PkNorm"], p))
        f.set_invgrow(*ic_oracle.growth_table_lcdm(p["Omega0"]))
        f.sweep(np.array(kat["radii_Mpc"]) / (_box(p) / n))
        _report("HMF_Validation", f, n, 5)


def test_device_reproduces_the_first_turn_of_the_example(api):
    kat = _kat("example_kat.json")
    p = kat["params"]
    n = p["GridSize"]
    with api.Fmax(n) as f:
        f.genic_density(p["RandomSeed"], _box(p), p["Omega0"], p["OmegaBaryon"], p["Hubble100"], p["PrimordialIndex"], pknorm=kat["PkNorm"])
        f.set_invgrow(*ic_oracle.growth_table_lcdm(p["Omega0"]))
        f.sweep(np.array(kat["radii_Mpc"]) / (_box(p) / n))
        _report("example", f, n, 8)


def test_device_reproduces_the_logged_totals_of_the_lcdm_256_runs(api):
    kat = _kat("hmf256_kat.json")
    p = kat["params"]
    n = p["GridSize"]
    with api.Fmax(n) as f:
        f.genic_density(p["RandomSeed"], _box(p), p["Omega0"], p["OmegaBaryon"], p["Hubble100"], p["PrimordialIndex"], pknorm=kat["PkNorm"], fixed=True)
        f.set_invgrow(*ic_oracle.growth_table_lcdm(p["Omega0"]))
        f.sweep(np.array(kat["radii_Mpc"]) / (_box(p) / n))
        _report("RECOMPUTE_DISPLACEMENTS_LCDM", f, n, 8)
        _report("SCALE_DEP_LCDM", f, n, 8)


def test_device_reproduces_the_logged_total_of_the_read_pk_table_run(api):
    kat = _kat("readpk256_kat.json")
    p = kat["params"]
    n = p["GridSize"]
    t = np.array(kat["camb_z0_k_hMpc_P"])
    g = np.array(kat["scaledep_a_D1"])
    with api.Fmax(n) as f:
        f.genic_density(p["RandomSeed"], _box(p), p["Omega0"], p["OmegaBaryon"], p["Hubble100"], p["PrimordialIndex"], pknorm=1.0, fixed=True,
                        pk_table=(np.log10(t[:, 0] * p["Hubble100"]), np.log10(t[:, 0] ** 3 * t[:, 1])))
        for i in range(len(kat["radii_Mpc"])):
            f.set_invgrow(np.log10(g[:, 1]), np.log10(g[:, 0]), ismooth=i)
        f.sweep(np.array(kat["radii_Mpc"]) / (_box(p) / n))
        _report("READ_PK_TABLE_and_SCALE_DEP", f, n, 100)


def test_device_reproduces_the_first_turn_of_the_f_of_R_run(api):
    mg = _kat("mg256_kat.json")
    p = mg["params"]
    n = p["GridSize"]
    a0, d0 = mg["growth_first_rows_a_D1"][0]
    radii = np.array(mg["radii_Mpc"])
    size = radii.copy()
    size[-1] = size[-2]
    with api.Fmax(n) as f:
        f.genic_density(p["RandomSeed"], _box(p), p["Omega0"], p["OmegaBaryon"], p["Hubble100"], p["PrimordialIndex"], pknorm=mg["PkNorm"], fixed=True)
        f.set_invgrow(*ic_oracle.growth_table_lcdm(p["Omega0"]))
        f.set_collapse_model(1, cosmo=(p["Omega0"], p["OmegaLambda"], 0.0, 0.0), d_in=np.full(len(radii), d0 * (1e-5 / a0) ** mg["dlnD_dlna_first_row"]))
        f.set_modified_gravity(p["FR0"], 100.0 / 299792.458, size=size)
        f.set_tabulated_ct(np.array(mg["variance"]))
        f.sweep(radii / (_box(p) / n))
        _report("MOD_GRAV_and_SCALE_DEP", f, n, 40)
