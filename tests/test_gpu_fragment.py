"""A whole fragment() walk on the device -- the call sequence of INTEGRATION.md, every sub-box of one box through every device stage,
each stage fed what the one before it returned -- against the same walk on the numpy restatements (tests/np_fragment.py, which
tests/test_fragment_cpu.py runs alone and shows to see a wrong hand-off).

sweep, compute_displacements(1, 0), A = products(), shift_displacements, set_growth(G2), compute_displacements(0, 0), B = products(),
flast = the median of Fmax; then per sub-box frag_map -> fill_box -> commit(False), distribute_sorted_neighbours, the stand-in
grouping on what came back, group_velocity_sums and refresh_segment (order = indices), plc_cross, catalog, distribute_back; at the
end the ZACC / GRUP / FMAX blocks and update_back.  np_fragment.walk is the integrator on both sides; here its stages are the
device's.  The comparison is np_fragment.compare: bit for bit, but for the fp64 sums (npart 2^-53 sum|v| of math.fsum, the written
means bit-equal to the means of the reported sums) and the x, v of the light-cone and catalogue records (the bands of
plc_cases.Case.check / catalog_cases.Case.check)."""
import threading

import numpy as np
import pytest

import catalog_cases as cc
import np_distribute as npd
import np_fragment as nf
import np_groupvel as npg
import plc_cases as pc
from pinocchio_amd import synth
from test_gpu_multirank import run_ranks
from test_gpu_refresh import G1, G2, RADII

pytestmark = pytest.mark.gpu

# name -> (n, sub-boxes, boundary layer, LPT order, double products, nk)
CASES = {"whole": (32, (1, 1, 1), 0, 3, False, 1),
         "two tiles": (32, (2, 1, 1), 2, 3, False, 1),
         "mixed radix": (24, (1, 2, 1), 2, 3, False, 1),
         "double": (32, (2, 1, 1), 2, 3, True, 1),
         "nk = 10": (32, (2, 1, 1), 2, 2, False, 10)}


@pytest.fixture(scope="module")
def api():
    from pinocchio_amd import api as _api
    return _api


def _params(name):
    n, nbox, layer, order, dp, nk = CASES[name]
    return nf.Params(n, nbox, layer, T=np.float64 if dp else np.float32, order=order, nk=nk)


def _frag_layout(T):
    from pinocchio_amd import _lib
    ft = nf.frag_dtype(T)
    return _lib.ProductLayout(ft.itemsize, *nf.offsets(ft, ("Rmax", "Fmax") + nf.VEL))


class DeviceStages:
    """the stages of np_fragment.walk answered by one context"""

    def __init__(self, api, f, flast, par):
        self.api, self.f, self.flast, self.par = api, f, float(flast), par
        self.ft, self.gt = nf.frag_dtype(par.T), pc.group_dtype(par.T)
        self.lay = _frag_layout(par.T)

    def table(self, start, length, safe, pbc, neigh_pbc):
        with self.f.frag_map(start, length, safe) as m:
            m.fill_box()
            m.commit(False)
            rec, pos, spos, ind, neigh, flags, peaks, count = self.f.distribute_sorted_neighbours(self.flast, m, layout=self.lay)
        assert count == len(pos) == len(rec)
        return np.ascontiguousarray(rec).view(self.ft).reshape(count), pos, spos, ind, neigh, flags, peaks

    def sums(self, box, pos, gid, first):
        return self.f.group_velocity_sums(box, pos, gid, first)

    def segment(self, box, pos, gid, rec, frag_off, groups, ngroups, group_off, order, first):
        prev = self.api.prev_layout(*frag_off[4:])
        gl = self.api.group_layout(self.gt.itemsize, self.gt.fields["Mass"][1], *group_off)
        return self.f.refresh_segment(box, pos, gid, rec, self.lay, prev, groups, ngroups, gl, order=order, first_group=first)

    def plc(self, name, stabl, groups):
        par = self.par
        return self.f.plc_cross(self.api.PLC_LAST_CHECK, par.myseg, par.z_seg, stabl, groups, z_prev=par.z_prev, min_mass=par.min_mass, out_dtype=pc.out_dtype(par.T))

    def catalog(self, name, stabl, length, pbc, groups):
        case = nf.CatalogCase(name, self.par, stabl, length, pbc, groups)
        return self.f.catalog(groups=groups, out_dtype=cc.catalog_dtype(self.par.T), **case.call_kwargs())

    def back(self, start, length, safe, pos, zacc, gid):
        return self.f.distribute_back(start, length, safe, pos, zacc, gid)

    def columns(self):
        """the two columns through update_back; with fp32 products the ZACC / GRUP blocks must say the same"""
        T = self.par.T
        nc = self.f.nxl * self.f.n * self.f.n
        rt = np.dtype({"names": ["zacc", "group_ID"], "formats": [np.dtype(T).str, "<i4"], "offsets": [8, 16], "itemsize": 24})
        rec = np.full(nc * 24, 0xA5, dtype=np.uint8)
        self.f.update_back(rec, 8, 16)
        raw = rec.reshape(nc, 24)
        assert np.all(raw[:, :8] == 0xA5) and np.all(raw[:, 20:] == 0xA5) and (T is np.float64 or np.all(raw[:, 12:16] == 0xA5))
        z, g = rec.view(rt)["zacc"].copy(), rec.view(rt)["group_ID"].copy()
        if T is np.float32:
            assert self.f.block("ZACC").tobytes() == z.tobytes() and self.f.block("GRUP").tobytes() == g.tobytes()
        return z, g


def _segments(f, dk, order):
    """the two segments -> (A, B): the records before the shift and after the second displacements"""
    f.set_density(dk)
    f.set_invgrow(*synth.invgrow_table("lcdm"))
    f.set_lpt_order(order)
    f.sweep(RADII)
    f.set_growth(G1)
    f.compute_displacements(1, 0)
    A = f.products()
    f.shift_displacements()
    f.set_growth(G2)
    f.compute_displacements(0, 0)
    return A, f.products()


def _cone(f, par):
    f.plc_set_cosmology(**pc.cosmology_tables(par.nk))
    f.plc_set_geometry(**nf.PlcCase("cone", par, (0, 0, 0), np.zeros(0, dtype=pc.group_dtype(par.T))).geometry_kwargs())


def _device_walk(api, f, par, dk):
    A, B = _segments(f, dk, par.order)
    flast = float(np.median(A["Fmax"]))
    res = nf.walk(DeviceStages(api, f, flast, par), par, flast)
    return A, B, flast, res


class Walk:
    pass


@pytest.fixture(scope="module")
def walks(api):
    """one context per case: the device's walk, the numpy walk on the device's A and B, and the context kept for a second walk
    (computed once per case, shared, left alone)"""
    made = {}

    def get(name):
        if name not in made:
            n, nbox, layer, order, dp, nk = CASES[name]
            w = Walk()
            w.par = _params(name)
            w.dk = synth.make_density(n, seed=synth.SEED)
            w.f = api.Fmax(n, double_products=dp)
            made[name] = w
            _cone(w.f, w.par)
            w.A, w.B, w.flast, w.dev = _device_walk(api, w.f, w.par, w.dk)
            w.ref = nf.walk(nf.NumpyStages(w.A, w.B, w.flast, w.par), w.par, w.flast)
        return made[name]
    yield get
    for w in made.values():
        w.f.close()


@pytest.mark.parametrize("name", list(CASES))
def test_the_walk_is_not_vacuous(walks, name):
    """the input conditions, from the numpy side alone"""
    w = walks(name)
    assert w.A["Fmax"].tobytes() == w.B["Fmax"].tobytes() and w.A["Rmax"].tobytes() == w.B["Rmax"].tobytes()
    kmax = w.par.order if w.par.order < 3 else 4
    for k, v in enumerate(nf.VEL):
        assert (np.any(w.A[v] != w.B[v]) and np.any(w.A[v] != 0)) == (k < kmax), v
    for b, f in enumerate(nf.input_conditions(w.ref, w.par)):
        print(name, "box", b, f)


@pytest.mark.parametrize("name", list(CASES))
def test_stage_by_stage_against_the_chain(walks, name):
    w = walks(name)
    nf.compare(w.dev, w.ref, report=print)
    if not CASES[name][4]:
        assert w.f.block("FMAX").tobytes() == np.ascontiguousarray(w.B["Fmax"]).tobytes()


@pytest.mark.parametrize("name", list(CASES))
def test_what_must_close_closes_on_the_device(walks, name):
    w = walks(name)
    nf.invariants(w.dev, w.A, w.B, w.flast, w.par)


def _flat(res):
    """every byte a walk returned, in a fixed order"""
    out = [res["ZACC"].tobytes(), res["GRUP"].tobytes()]
    for r in res["boxes"]:
        for k in ("rec0", "rec", "pos", "spos", "ind", "neigh", "flags", "gid", "zacc", "groups"):
            out.append(np.ascontiguousarray(r[k]).tobytes())
        out.append(repr((r["peaks"], r["loose"], r["grouped"], r["mismatch"], r["stored"], r["sums"][3:], r["plc"][3:5], r["cat"][2])).encode())
        for a in tuple(r["sums"][:3]) + tuple(r["plc"][:3]) + tuple(r["cat"][:2]) + tuple(r["cat"][3:5]):
            out.append(np.ascontiguousarray(a).tobytes())
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_a_second_walk_on_the_same_context_returns_the_same_bytes(api, walks, name):
    w = walks(name)
    w.f.back_reset()
    w.f.drop_prev()
    assert w.f.prev_shifts == 0
    A, B, flast, res = _device_walk(api, w.f, w.par, w.dk)
    assert A.tobytes() == w.A.tobytes() and B.tobytes() == w.B.tobytes() and flast == w.flast
    first, second = _flat(w.dev), _flat(res)
    assert len(first) == len(second) and all(a == b for a, b in zip(first, second))


def test_two_ranks_add_up_to_the_one_rank_walk(api, walks):
    """P = 2 virtual ranks at LPT order 2 (at order 3 the 3LPT(b) columns differ in the last bit between decompositions).  Every rank
    contributes its distribute; the contributions are concatenated in the order of the hypercube loop; every rank runs organize and
    neighbours on the whole and the stand-in on that; group_velocity_sums (partial sums), refresh_segment and distribute_back run
    on its own slab.  Against the one-rank walk of the same box (the case "nk = 10")."""
    one = walks("nk = 10")
    par, flast, P = one.par, one.flast, 2
    n = par.n
    nxl = n // P
    ft, gt = nf.frag_dtype(par.T), pc.group_dtype(par.T)
    lay = _frag_layout(par.T)
    frag_off, group_off = nf.offsets(ft, nf.VEL + nf.PREV), nf.offsets(gt, nf.VEL + nf.PREV)
    shared = [[None] * P for _ in par.boxes]
    meet = threading.Barrier(P, timeout=120)

    def body(f, r):
        A, B = _segments(f, one.dk[r * nxl:(r + 1) * nxl], par.order)
        assert A.tobytes() == one.A[r * nxl:(r + 1) * nxl].tobytes() and B.tobytes() == one.B[r * nxl:(r + 1) * nxl].tobytes()
        out, offset = [], 0
        for b, (stabl, lgwbl, lgrid, safe, pbc) in enumerate(par.boxes):
            box = (tuple(stabl), tuple(lgwbl), tuple(safe))
            with f.frag_map(stabl, lgwbl, safe) as m:
                m.fill_box()
                m.commit(False)
                shared[b][r] = f.distribute(flast, stabl, lgwbl, map=m, layout=lay)
            meet.wait()
            parts = [shared[b][t] for t in npd.hypercube_order(P, b)]
            rec = np.ascontiguousarray(np.concatenate([p[0] for p in parts]))
            pos = np.ascontiguousarray(np.concatenate([p[1] for p in parts]))
            assert sum(p[2] for p in parts) == len(pos)
            spos, ind = f.organize(rec, pos, lay)
            rec = rec.view(ft).reshape(len(pos))
            neigh, flags, peaks = f.neighbours(pos, np.ascontiguousarray(rec["Fmax"]), stabl, lgwbl, safe)
            gid, zacc, groups = nf.stand_in_groups(rec["Fmax"], pos, neigh, flags, stabl, lgwbl, pbc, n, flast, par.T)
            ngroups = len(groups) - 1
            rec0 = nf.raw(rec).copy().view(ft).reshape(len(rec))
            sums = f.group_velocity_sums(box, pos, gid, nf.FIRST_GROUP)
            gl = api.group_layout(gt.itemsize, -1, *group_off)           # a slab sees a part of every group: Mass is not compared
            counts = f.refresh_segment(box, pos, gid, rec, lay, api.prev_layout(*frag_off[4:]), groups.copy(), ngroups, gl, order=ind)
            gback = np.where(gid >= nf.FIRST_GROUP, gid + offset, gid).astype(np.int32)
            stored = f.distribute_back(stabl, lgwbl, safe, pos, zacc, gback)
            offset += ngroups - 1
            out.append(dict(rec0=rec0, rec=rec, pos=pos, spos=spos, ind=ind, neigh=neigh, flags=flags, peaks=tuple(peaks), gid=gid, zacc=zacc, groups=groups,
                            sums=sums, counts=counts, stored=stored))
        return out, f.block("ZACC"), f.block("GRUP")

    res = run_ranks(api, n, P, body)
    chain = nf.NumpyStages(one.A, one.B, flast, par)
    for b, r1 in enumerate(one.dev["boxes"]):
        ranks = [res[r][0][b] for r in range(P)]
        # every rank made the same tables from the contributions: those of the chain for a box held in P slabs.  (Against the
        # one-rank walk only the order among equal Fmax may differ: the contributions arrive in another order.)
        stabl, lgwbl, lgrid, safe, pbc = par.boxes[b]
        want = dict(zip(("rec0", "pos", "spos", "ind", "neigh", "flags", "peaks"), chain.table(stabl, lgwbl, safe, pbc, pbc, P, b)))
        want["gid"], want["zacc"], _ = nf.stand_in_groups(want["rec0"]["Fmax"], want["pos"], want["neigh"], want["flags"], stabl, lgwbl, pbc, n, flast, par.T)
        for q in ranks:
            for k in ("rec0", "pos", "spos", "ind", "neigh", "flags", "gid", "zacc"):
                assert np.ascontiguousarray(q[k]).tobytes() == np.ascontiguousarray(want[k]).tobytes(), (b, k)
            assert q["peaks"] == tuple(want["peaks"]) == r1["peaks"]
        assert np.array_equal(want["spos"], r1["spos"])
        # the partial sums of the ranks, added per ID in ascending rank
        ids, npart, s = r1["sums"][:3]
        rid, rn, rs, rmod = one.ref["boxes"][b]["sums"]
        tot_n, tot = np.zeros(len(ids), dtype=np.int64), np.zeros((len(ids), 24))
        for q in ranks:
            j = np.searchsorted(ids, q["sums"][0])
            assert np.array_equal(ids[j], q["sums"][0])
            tot_n[j] += q["sums"][1]
            tot[j] += q["sums"][2]
        assert np.array_equal(tot_n, npart) and np.array_equal(tot_n, rn)
        assert np.all(np.abs(tot - rs) <= rn[:, None] * nf.U * rmod)
        assert sum(q["counts"][0] for q in ranks) == r1["loose"] and sum(q["counts"][1] for q in ranks) == r1["grouped"]
        assert sum(q["stored"] for q in ranks) == r1["stored"]
        # the loose particles' records: each rank refreshed those of its slab, together all of them -- held against the one-rank
        # walk position by position (sorted_pos order on both sides)
        merged = nf.raw(ranks[0]["rec"]).copy()
        for q in ranks[1:]:
            mine = np.any(nf.raw(q["rec"]) != nf.raw(q["rec0"]), axis=1)
            merged[mine] = nf.raw(q["rec"])[mine]
        loose = (want["gid"] < nf.FIRST_GROUP)[want["ind"]]
        assert np.array_equal(loose, (r1["gid"] < nf.FIRST_GROUP)[r1["ind"]])
        assert merged[want["ind"]][loose].tobytes() == nf.raw(r1["rec"])[r1["ind"]][loose].tobytes()
        assert merged[want["ind"]][~loose].tobytes() == nf.raw(r1["rec0"])[r1["ind"]][~loose].tobytes()
        # the groups assembled by the owner as INTEGRATION.md has it, and their catalogue on a context of one rank
        groups = ranks[0]["groups"].copy()
        raw = groups.view(np.uint8).reshape(len(groups), gt.itemsize)
        raw[:] = npg.scatter_means(raw, ids, tot_n, tot, group_off, par.T)
        cat = DeviceStages(api, one.f, flast, par).catalog("ranks box %d" % b, stabl, lgwbl, pbc, groups[nf.FIRST_GROUP:].copy())
        for a, c in zip(cat[:2] + cat[3:5], r1["cat"][:2] + r1["cat"][3:5]):
            assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(c).tobytes(), b
        assert cat[2] == r1["cat"][2]
    # the slabs' columns, concatenated, are the one-rank columns
    assert np.concatenate([res[r][1] for r in range(P)]).tobytes() == one.dev["ZACC"].tobytes()
    assert np.concatenate([res[r][2] for r in range(P)]).tobytes() == one.dev["GRUP"].tobytes()
