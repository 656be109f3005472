"""A whole fragment() walk over one box, stage after stage, and the numpy side of it.

fragment() (src/fragment.c:193-472) hands every sub-box through distribute / sort_and_organize, the neighbour lookups of
build_groups, the velocity refresh of a redshift segment, the light-cone test, the catalogue and distribute_back.  Every one of these
stages has a numpy restatement of its own (np_maps, np_distribute, np_organize, np_neighbours, np_refresh, np_groupvel, np_plc,
np_catalog, np_back); this module chains them.  It shares no code with pinocchio_amd.

Three parts:
  * walk(): the integrator.  It owns everything that crosses a stage boundary -- which array goes into which call, in which order,
    with which box, layers, offsets and first group -- and calls the stages through an object with seven methods.  NumpyStages
    answers them from the restatements; tests/test_gpu_fragment.py answers them from the device.  walk(wrong=...) applies ONE
    wrong hand-off, which is how tests/test_fragment_cpu.py shows that a wrong hand-off is seen.
  * stand_in_groups(): an INPUT GENERATOR in the place of the sequential loop of build_groups(), see its docstring.
  * compare() (two walks, stage by stage), invariants() (what must close over all sub-boxes) and input_conditions() (what the walk
    must contain not to be vacuous).  compare() tests that the STAGES agree on equal inputs: walk() is the same on both sides, so
    a hand-off that walk() itself made the wrong way would be made the wrong way twice and compare() would not see it.  What
    tests the integrator is invariants(), which knows nothing of walk() -- and tests/test_fragment_cpu.py, which shows for each
    hand-off of WRONG that one of the two notices.  One argument nothing can test: `order` of the segment step is an access hint
    of the device (the result does not depend on it) and the numpy stage ignores it.
"""
import numpy as np

import catalog_cases as cc
import np_back as npb
import np_catalog as npc
import np_distribute as npd
import np_groupvel as npg
import np_maps
import np_neighbours as npn
import np_organize as npo
import np_peaks
import np_refresh as npr
import plc_cases as pc

FIRST_GROUP = 2                       # FILAMENT + 1: IDs 0 (none) and 1 (filament) are loose particles
VEL = ("Vel", "Vel_2LPT", "Vel_3LPT_1", "Vel_3LPT_2")
PREV = tuple(v + "_prev" for v in VEL)
U = 2.0 ** -53
TOUCH = 4                             # a particle that touches so many groups joins none: a filament particle
# the replications of the walk's cone: the fixture's observer and axis (1, 1, 0) / sqrt 2, the box seen from its corner and from one
# box further out along x, y, both, and all three (i, j, k, F1, F2).  From none of them is a group near the z edges of the box
# inside the aperture of 30 degrees: some groups cross in no replication
REPS = ((0, 0, 0, 5.0, 1.0), (1, 1, 0, 5.0, 1.0), (1, 0, 0, 5.0, 1.0), (0, 1, 0, 5.0, 1.0), (1, 1, 1, 5.0, 1.0))
WRONG = ("back in sorted_pos order", "neigh as positions", "first_group 1", "prev and current swapped", "periodic axis open",
         "one layer less in distribute_back", "Pos in global cells", "stabl of the other sub-box")


def frag_dtype(T):
    """product_data of a -DRECOMPUTE_DISPLACEMENTS build (src/pinocchio.h:233-259) as the compiler lays it out: 104 bytes, 208 with
    PRODFLOAT double"""
    t, pb = np.dtype(T).str, np.dtype(T).itemsize
    first = 2 * pb
    names = ["Rmax", "Fmax"] + list(VEL) + list(PREV)
    return np.dtype({"names": names, "formats": ["<i4", t] + [(t, 3)] * 8, "offsets": [0, pb] + [first + 3 * pb * s for s in range(8)],
                     "itemsize": first + 24 * pb})


def offsets(dtype, names):
    return tuple(dtype.fields[k][1] for k in names)


def columns(A, B):
    """the 24 columns of the whole grid [24][n^3]: the current ones (B, after the shift) 0..11, then the prev ones (A) 12..23"""
    out = []
    for p in (B, A):
        p = p.reshape(-1)
        for name in VEL:
            out += [np.ascontiguousarray(p[name][:, e]) for e in range(3)]
    return np.stack(out)


class Params:
    """what the walk needs beside the products: the boxes, the cone, the output"""

    def __init__(self, n, nbox, layer, T=np.float32, order=3, nk=1, reps=REPS, F_out=1.15, hfactor=0.7):
        self.n, self.nbox, self.layer, self.T, self.order, self.nk = int(n), tuple(nbox), int(layer), T, int(order), int(nk)
        self.boxes = npd.subboxes(self.n, self.nbox, self.layer)
        self.reps, self.F_out, self.hfactor = tuple(reps), float(F_out), float(hfactor)
        self.gs = (self.n,) * 3
        self.myseg, self.z_seg, self.z_prev = 1, 0.0, 0.3          # segment B ends at z = 0, segment A ended at z = 0.3
        self.min_mass = pc.MIN_MASS
        self.ipd, self.pmass = pc.fixture()["InterPartDist"], cc.PMASS
        self.bins = (cc.NBIN_ALL, cc.MMIN, cc.DELTAM)


class PlcCase(pc.Case):
    """one plc_cross of the walk with the oracle and the pass criteria of tests/plc_cases.py: the fixture's cone, the walk's groups"""

    def __init__(self, name, par, stabl, groups):
        fx = pc.fixture()
        self.name, self.T, self.ncand, self.nrep, self.crossing, self.events = name, par.T, len(groups), len(par.reps), "walk", False
        self.myseg, self.order, self.nk, self.use_v31, self.seed = par.myseg, par.order, par.nk, False, 0
        self.ipd = par.ipd
        ax = np.array(fx["axis"])
        self.zvers = ax / np.linalg.norm(ax)
        self.xvers, self.yvers = np.array([0.0, 0.0, 1.0]), np.cross(self.zvers, [0.0, 0.0, 1.0])
        self.reps, self.gs, self.stabl = [tuple(r) for r in par.reps], par.gs, tuple(int(s) for s in stabl)
        self.nzbins, self.lastz, self.delta_z = fx["nzbins"], 0.0, 0.05
        self.z_seg, self.z_prev, self.min_mass = par.z_seg, par.z_prev, par.min_mass
        self.groups, self.f_lo = groups, None


class CatalogCase(cc.Case):
    """one catalog call of the walk with the oracle and the pass criteria of tests/catalog_cases.py"""

    def __init__(self, name, par, stabl, lgwbl, pbc, groups):
        self.name, self.T, self.n, self.nk, self.myseg, self.use_v31, self.order, self.F = name, par.T, len(groups), par.nk, par.myseg, False, par.order, par.F_out
        self.pbc, self.stabl, self.lgwbl = tuple(int(p) for p in pbc), tuple(int(s) for s in stabl), tuple(int(v) for v in lgwbl)
        self.gs, self.hfactor, self.min_mass, self.nbin, self.light, self.flags = par.gs, par.hfactor, par.min_mass, par.bins[0], False, True
        self.ipd, self.pmass, self.mmin, self.deltam = par.ipd, par.pmass, par.bins[1], par.bins[2]
        self.z_seg, self.z_prev = par.z_seg, par.z_prev
        self.groups = groups


# ------------------------------------------------------------------------------------------------------------------------
def stand_in_groups(fmax, frag_pos, neigh, flags, start, length, pbc, n, flast, T):
    """An INPUT GENERATOR, not a restatement: it stands where the sequential loop of build_groups() (src/build_groups.c:245-343)
    stands, so that the stages behind it get group IDs and group records that come from the tables the stages before it made.  It
    restates nothing of the reference's accretion and merging and pins no result.  It is deterministic and reads only what the
    device hands a host loop: the records' Fmax in descending order, frag_pos of the same order, neigh[N, 6] and flags[N].

    Walking iz in record order: a skipped particle gets ID 0; a particle with the PEAK flag opens the next group, counting from 2;
    any other particle looks at its found neighbour with the largest Fmax (ties to the smaller nn): if that neighbour has no ID >= 2
    yet (it is loose, or an equal Fmax puts it later in the order) the particle stays at ID 0; otherwise it joins that neighbour's
    group -- unless its found neighbours already belong to TOUCH or more different groups, which makes it a filament particle,
    ID 1.  (With the map of create_map no stored particle is skipped, and without the last clause every particle would reach a
    group: the clause is what gives the walk loose particles of both kinds.)

    -> (group_ID int32[N], zacc T[N], groups): zacc = Fmax - 1 in the product precision where the ID is >= 1, -1 for a particle
    that nothing accreted (ID 0), as src/allocations.c:519-524 leaves it; groups: records 0 .. ngroups of
    plc_cases.group_dtype(T), 0 and 1 empty.  Of group g: Mass the member count; Pos the mean of the members' sub-box coordinates
    -- on a periodic axis unwrapped about the peak and folded back into [0, L) --, formed in float64 and rounded once to T; name
    the peak's global cell + 1; good the peak's GOOD flag; point the peak's iz; Flast = flast; the eight Vel* fields zero until
    the segment step fills them."""
    f = np.asarray(fmax)
    pos = np.asarray(frag_pos)
    neigh = np.asarray(neigh)
    flags = np.asarray(flags)
    N = len(pos)
    found = neigh >= 0
    fn = np.where(found, f[np.where(found, neigh, 0)].astype(np.float64), -np.inf)
    nn = np.argmax(fn, axis=1) if N else np.zeros(0, int)        # the first of equal maxima: the smaller nn
    best = np.where(found.any(axis=1), neigh[np.arange(N), nn], -1) if N else np.zeros(0, int)
    gid = np.zeros(N, dtype=np.int32)
    peaks = []
    skip, peak = (flags & npn.SKIP) != 0, (flags & npn.PEAK) != 0
    for iz in range(N):
        if skip[iz]:
            continue
        if peak[iz]:
            peaks.append(iz)
            gid[iz] = len(peaks) + 1
        else:
            q = best[iz]
            if q >= 0 and gid[q] >= FIRST_GROUP:
                near = gid[neigh[iz][found[iz]]]
                gid[iz] = 1 if np.unique(near[near >= FIRST_GROUP]).size >= TOUCH else gid[q]
    zacc = np.where(gid >= 1, (f.astype(T) - T(1.0)).astype(T), T(-1.0)).astype(T)
    ngroups = len(peaks) + 1
    groups = np.zeros(ngroups + 1, dtype=pc.group_dtype(T))
    if peaks:
        pk = np.array(peaks, dtype=np.int64)
        c = np.stack(npn.coords(pos, length), axis=1)            # [N][3]
        member = np.flatnonzero(gid >= FIRST_GROUP)
        g = gid[member].astype(np.int64)
        groups["Mass"][FIRST_GROUP:] = np.bincount(g, minlength=ngroups + 1)[FIRST_GROUP:]
        cp = c[pk]                                               # the peaks' coordinates, group g at row g - 2
        for d in range(3):
            L = int(length[d])
            delta = c[member, d] - cp[g - FIRST_GROUP, d]
            if pbc[d]:
                delta = (delta + L // 2) % L - L // 2
            tot = np.zeros(ngroups + 1, dtype=np.int64)
            np.add.at(tot, g, delta)                             # integers: exact
            mean = cp[:, d].astype(np.float64) + tot[FIRST_GROUP:].astype(np.float64) / groups["Mass"][FIRST_GROUP:].astype(np.float64)
            if pbc[d]:
                mean = np.where(mean < 0.0, mean + L, mean)
                mean = np.where(mean >= L, mean - L, mean)
            m = mean.astype(T)
            if pbc[d]:
                m = np.where(m >= T(L), T(0.0), m)               # (the rounding may reach L itself)
            groups["Pos"][FIRST_GROUP:, d] = m
        gc = [(cp[:, d] + int(start[d])) % n for d in range(3)]
        groups["name"][FIRST_GROUP:] = (gc[2] + n * (gc[1] + n * gc[0]) + 1).astype(np.uint64)
        groups["good"][FIRST_GROUP:] = (flags[pk] & npn.GOOD) != 0
        groups["point"][FIRST_GROUP:] = pk
        groups["Flast"][FIRST_GROUP:] = T(flast)
    return gid, zacc, groups


# ------------------------------------------------------------------------------------------------------------------------
class NumpyStages:
    """the stages answered by the restatements, from the full-grid records of the two segments: A before the shift, B after it"""

    def __init__(self, A, B, flast, par):
        self.par, self.flast = par, float(flast)
        n = par.n
        self.A, self.B = A.reshape(-1), B.reshape(-1)
        self.fmax = np.ascontiguousarray(self.B["Fmax"]).reshape(n, n, n)
        self.cols = columns(A, B)
        self.zcol, self.gcol = npb.fresh(n, n, par.T)

    def table(self, start, length, safe, pbc, neigh_pbc, ntasks=1, target=0):
        """frag_map -> fill_box -> commit(False) -> distribute_sorted_neighbours (neigh_pbc: what the neighbour table takes for
        periodic -- the device decides that itself, by length == n).  ntasks, target: the box held in ntasks x-slabs, the
        contributions to the sub-box of task `target` concatenated in the order of the hypercube loop"""
        par = self.par
        words = np_maps.words_of(np_maps.create_map(length, safe, pbc))
        cells, fpos = npd.distribute(self.fmax, ntasks, list(start), list(length), self.flast, words, target)
        order, spos, ind = npo.organize(self.fmax.ravel()[cells], fpos)
        cells, pos = cells[order], fpos[order].astype(np.uint32)
        rec = np.zeros(len(pos), dtype=frag_dtype(par.T))
        for k in ("Rmax", "Fmax") + VEL:
            rec[k] = self.B[k][cells]
        neigh, flags, peaks = npn.neighbours(pos, rec["Fmax"], length, safe, neigh_pbc)
        return rec, pos, spos, ind, neigh, flags, peaks

    def sums(self, box, pos, gid, first):
        n = self.par.n
        index, vel = npr.gather(n, 0, n, box[0], box[1], pos, self.cols)
        ids, npart, s, mod = npg.sums_of(vel, np.asarray(gid)[index], first)
        return ids, npart, s, mod

    def segment(self, box, pos, gid, rec, frag_off, groups, ngroups, group_off, order, first):
        """refresh_segment: the loose particles' records and the group means -> (loose, grouped, mismatch)"""
        n, T = self.par.n, self.par.T
        index, vel = npr.gather(n, 0, n, box[0], box[1], pos, self.cols)
        gid = np.asarray(gid)
        loose = gid[index] < first
        raw = rec.view(np.uint8).reshape(len(rec), rec.dtype.itemsize)
        raw[:] = npr.scatter(raw, index[loose], vel[loose], frag_off[:4], frag_off[4:])
        ids, npart, s, _ = npg.sums_of(vel, gid[index], first)
        graw = groups.view(np.uint8).reshape(len(groups), groups.dtype.itemsize)
        graw[:] = npg.scatter_means(graw, ids, npart, s, group_off, T)
        mism = int(np.sum(groups["Mass"][ids] != npart.astype(np.int64)))
        return int(loose.sum()), int((~loose).sum()), mism

    def plc(self, name, stabl, groups):
        case = PlcCase(name, self.par, stabl, groups)
        o = case.oracle()
        rec = np.zeros(0, dtype=pc.out_dtype(self.par.T))
        cand, rep = np.zeros(0, np.uint32), np.zeros(0, np.int32)
        if o["store"] is not None:
            st, ins = o["store"], o["store"]["inside"]
            cand, rep = o["cand"][ins].astype(np.uint32), o["rep"][ins].astype(np.int32)
            rec = np.zeros(len(cand), dtype=pc.out_dtype(self.par.T))
            rec["Mass"], rec["name"] = groups["Mass"][cand], groups["name"][cand]
            rec["z"], rec["x"], rec["v"] = st["z"][ins], st["x"][ins], st["v"][ins]
        return rec, cand, rep, len(cand), 0, case

    def catalog(self, name, stabl, length, pbc, groups):
        case = CatalogCase(name, self.par, stabl, length, pbc, groups)
        o = case.oracle()
        idx = o["index"]
        rec = np.zeros(len(idx), dtype=cc.catalog_dtype(self.par.T))
        rec["name"], rec["n"] = groups["name"][idx], groups["Mass"][idx]
        for k in ("M", "x", "v", "q"):
            rec[k] = o[k]
        mas = np.array([np.float64(s) * np.float64(self.par.pmass) for s in o["sum_mass"]], np.float64)
        return rec, idx.astype(np.uint32), len(idx), o["ninbin"], mas, case

    def back(self, start, length, safe, pos, zacc, gid):
        n = self.par.n
        self.zcol, self.gcol, stored = npb.distribute_back(n, 0, n, start, length, safe, pos, zacc, gid, self.zcol, self.gcol)
        return stored

    def columns(self):
        return self.zcol.copy(), self.gcol.copy()


def walk(stages, par, flast, wrong=None):
    """the sequence of INTEGRATION.md over every sub-box of par.boxes -> dict: boxes (one dict per sub-box), ZACC, GRUP (the columns
    of the whole grid after the last sub-box), offset (what was added to the IDs >= 2 of every sub-box on the way back: the IDs
    of a sub-box count from 2 again).  wrong: one of WRONG, a hand-off made the wrong way on purpose."""
    assert wrong is None or wrong in WRONG
    n, T = par.n, par.T
    ft, gt = frag_dtype(T), pc.group_dtype(T)
    frag_off = offsets(ft, VEL + PREV)
    group_off = offsets(gt, VEL + PREV)
    if wrong == "prev and current swapped":
        group_off = group_off[4:] + group_off[:4]
    out, offset = [], 0
    for b, (stabl, lgwbl, lgrid, safe, pbc) in enumerate(par.boxes):
        box = (tuple(stabl), tuple(lgwbl), tuple(safe))
        r = {"box": box, "pbc": tuple(pbc), "offset": offset}
        rec, pos, spos, ind, neigh, flags, peaks = stages.table(stabl, lgwbl, safe, pbc, [False] * 3 if wrong == "periodic axis open" else pbc)
        r.update(pos=pos, spos=spos, ind=ind, neigh=neigh, flags=flags, peaks=tuple(peaks), rec0=raw(rec).copy().view(rec.dtype).reshape(len(rec)))
        # the host loop: neigh[] indexes the records (descending Fmax), as frag[] and group_ID[] do
        table = np.where(neigh >= 0, ind[np.where(neigh >= 0, neigh, 0)], -1) if wrong == "neigh as positions" else neigh
        gid, zacc, groups = stand_in_groups(rec["Fmax"], pos, table, flags, stabl, lgwbl, pbc, n, flast, T)
        ngroups = len(groups) - 1
        first = 1 if wrong == "first_group 1" else FIRST_GROUP
        # the segment: order = indices[]; the group means land in the records
        r["sums"] = stages.sums(box, pos, gid, first)
        r["loose"], r["grouped"], r["mismatch"] = stages.segment(box, pos, gid, rec, frag_off, groups, ngroups, group_off, ind, first)
        r.update(rec=rec, gid=gid, zacc=zacc, groups=groups)
        # light cone and catalogue: groups FILAMENT + 1 .. ngroups, Pos in sub-box cells, the start of THIS sub-box
        cand = groups[FIRST_GROUP:].copy()
        pstabl = stabl
        if wrong == "Pos in global cells":
            cand["Pos"] = (cand["Pos"].astype(np.float64) + np.asarray(stabl, np.float64)).astype(T)
        if wrong == "stabl of the other sub-box":
            pstabl = par.boxes[(b + 1) % len(par.boxes)][0]
        r["plc"] = stages.plc("walk box %d" % b, pstabl, cand)
        r["cat"] = stages.catalog("walk box %d" % b, pstabl, lgwbl, pbc, cand)
        # the way back: in record order, as frag_pos is; the layers of distribute_back are the sub-box's safe
        bsafe = [max(s - 1, 0) for s in safe] if wrong == "one layer less in distribute_back" else safe
        gback = np.where(gid >= FIRST_GROUP, gid + offset, gid).astype(np.int32)
        if wrong == "back in sorted_pos order":
            gback = gback[ind]
        r["stored"] = stages.back(stabl, lgwbl, bsafe, pos, zacc, gback)
        offset += ngroups - 1
        out.append(r)
    z, g = stages.columns()
    return {"boxes": out, "ZACC": z, "GRUP": g}


# ------------------------------------------------------------------------------------------------------------------------
def raw(a):
    """the bytes of a record array, one row per record (indexing a structured array with holes does not keep the holes' bytes)"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), a.dtype.itemsize)


def _same(what, a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def compare(got, ref, report=None):
    """`got` (the device's walk, or a walk with a wrong hand-off) against `ref` (the numpy walk), stage by stage in the order of
    the walk, so that the first stage that disagrees is the one named.  Bit for bit but for: the fp64 sums, within npart 2^-53
    sum|v| of math.fsum, with the written means bit-equal to what np_groupvel.scatter_means makes of the sums `got` reports (the
    two checks of tests/test_gpu_groupvel.py); the light-cone records' z, x, v by plc_cases.Case.check; the catalogue's x, v by
    catalog_cases.Case.check."""
    assert len(got["boxes"]) == len(ref["boxes"])
    for b, (g, r) in enumerate(zip(got["boxes"], ref["boxes"])):
        w = "box %d: " % b
        T = r["rec"]["Fmax"].dtype.type
        _same(w + "distribute / organize: the records", raw(g["rec0"]), raw(r["rec0"]))
        for k in ("pos", "spos", "ind"):
            _same(w + "distribute / organize: " + k, g[k], r[k])
        for k in ("neigh", "flags"):
            _same(w + "neighbours: " + k, g[k], r[k])
        assert g["peaks"] == r["peaks"], (w, g["peaks"], r["peaks"])
        for k in ("gid", "zacc"):
            _same(w + "the stand-in on equal tables: " + k, g[k], r[k])
        # the segment
        loose = r["gid"] < FIRST_GROUP
        _same(w + "refresh_segment: the loose particles' records", raw(g["rec"])[loose], raw(r["rec"])[loose])
        _same(w + "refresh_segment: the grouped particles' records keep their bytes", raw(g["rec"])[~loose], raw(r["rec0"])[~loose])
        assert (g["loose"], g["grouped"], g["mismatch"]) == (r["loose"], r["grouped"], r["mismatch"]), (w, g["loose"], g["grouped"], g["mismatch"])
        ids, npart, s = g["sums"][:3]
        rid, rn, rs, rmod = r["sums"]
        _same(w + "group_velocity_sums: group", np.asarray(ids, np.int32), np.asarray(rid, np.int32))
        _same(w + "group_velocity_sums: npart", np.asarray(npart, np.uint32), np.asarray(rn, np.uint32))
        err = np.abs(np.asarray(s) - rs)
        bound = rn[:, None] * U * rmod
        if report and len(rid):
            report(w + "sums: largest error / bound %.3g" % float(np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound), w + "group_velocity_sums: the fp64 sums"
        gt = g["groups"].dtype
        want = np.zeros(len(g["groups"]), dtype=gt)
        for k in gt.names:
            if k not in VEL + PREV:
                want[k] = r["groups"][k]
        wraw = npg.scatter_means(want.view(np.uint8).reshape(len(want), gt.itemsize), ids, npart, s, g.get("group_off", offsets(gt, VEL + PREV)), T)
        _same(w + "refresh_segment: the group records", g["groups"].view(np.uint8).reshape(len(want), gt.itemsize), wraw)
        # the light cone: count, order, names bit for bit; z, x, v by the criteria of the stage's own test
        rec, cand, rep, count, unconv = g["plc"][:5]
        rrec, rcand, rrep, rcount = r["plc"][:4]
        assert count == rcount and unconv == 0, (w, "plc_cross: count", count, rcount, unconv)
        _same(w + "plc_cross: candidates", np.asarray(cand, np.uint32), rcand)
        _same(w + "plc_cross: replications", np.asarray(rep, np.int32), rrep)
        _same(w + "plc_cross: name", rec["name"], rrec["name"])
        _same(w + "plc_cross: Mass", rec["Mass"], rrec["Mass"])
        r["plc"][5].check(rec, cand, rep, count, unconv)
        # the catalogue
        rec, gof, count, nin, mas = g["cat"][:5]
        rrec = r["cat"][0]
        assert count == r["cat"][2], (w, "catalog: count", count, r["cat"][2])
        _same(w + "catalog: group_of", np.asarray(gof, np.uint32), r["cat"][1])
        for k in ("name", "n", "M", "q"):
            _same(w + "catalog: " + k, rec[k], rrec[k])
        _same(w + "catalog: ninbin", np.asarray(nin, np.int32), np.asarray(r["cat"][3], np.int32))
        _same(w + "catalog: massinbin", np.asarray(mas, np.float64), r["cat"][4])
        r["cat"][5].check(rec, gof, count, nin, mas, printer=report)
        # the way back
        assert g["stored"] == r["stored"], (w, "distribute_back: stored", g["stored"], r["stored"])
    _same("ZACC", got["ZACC"], ref["ZACC"])
    _same("GRUP", got["GRUP"], ref["GRUP"])


def invariants(res, A, B, flast, par):
    """what must close over all sub-boxes, whoever computed `res`"""
    n, T = par.n, par.T
    fmax = np.ascontiguousarray(B["Fmax"]).reshape(n, n, n)
    boxes = res["boxes"]
    cols = columns(A, B)
    assert sum(r["peaks"][1] for r in boxes) == np_peaks.count_peaks(fmax, flast)[0], "the good peaks of the sub-boxes are the peaks of the box"
    with np.errstate(invalid="ignore"):
        stored = fmax.astype(np.float64).ravel() >= float(flast)
    assert sum(r["stored"] for r in boxes) == int(stored.sum()), "distribute_back stores every cell with Fmax >= flast once"
    z, g = res["ZACC"], res["GRUP"]
    assert z.dtype == np.dtype(T) and g.dtype == np.int32
    per_id = np.bincount(g[g >= FIRST_GROUP]) if (g >= FIRST_GROUP).any() else np.zeros(0, int)
    seen = 0
    for r in boxes:
        gid, flags, groups = r["gid"], r["flags"], r["groups"]
        ng = len(groups) - 1
        good = (flags & npn.GOOD) != 0
        want = np.bincount(gid[good & (gid >= FIRST_GROUP)], minlength=ng + 1)[FIRST_GROUP:]
        have = np.zeros(ng - 1, int)
        lo = FIRST_GROUP + r["offset"]
        m = per_id[lo:lo + ng - 1]
        have[:len(m)] = m
        assert np.array_equal(have, want), "cells of GRUP == g against the good members of g"
        seen += ng - 1
        # a group of one particle: its means are that particle's columns
        ones = np.flatnonzero(groups["Mass"][FIRST_GROUP:] == 1) + FIRST_GROUP
        if len(ones):
            iz = groups["point"][ones]
            assert np.array_equal(gid[iz], ones)
            found, cell = npr.cells(n, 0, n, r["box"][0], r["box"][1], r["pos"][iz])
            assert found.all()
            for s, name in enumerate(VEL + PREV):
                _same("a group of one particle: " + name, groups[name][ones], np.ascontiguousarray(cols[3 * s:3 * s + 3, cell].T).astype(T))
        # the catalogue
        rec, gof, count, nin, mas = r["cat"][:5]
        cand = groups[FIRST_GROUP:]
        assert np.array_equal(rec["n"], cand["Mass"][np.asarray(gof, np.int64)]), "catalogue n is Mass"
        passing = npc.passing(cand["Mass"], cand["good"], cand["point"], par.min_mass)
        assert count == int(passing.sum()) and int(np.sum(nin)) == int((passing & (cand["Mass"] >= 1)).sum()), "ninbin adds up to the passing groups"
    assert len(per_id) <= FIRST_GROUP + seen, "no ID beyond the last group"
    some = g >= 1
    _same("ZACC where GRUP >= 1", z[some], (fmax.ravel().astype(T) - T(1.0)).astype(T)[some])
    assert np.all(z[~some] == T(-1.0)) and not g[~some].any() and np.all(g >= 0), "elsewhere -1 / 0"
    assert not (some & ~stored).any()


def figures(res, par):
    """the numbers behind input_conditions, per sub-box"""
    out = []
    for r in res["boxes"]:
        gid, flags, groups, (start, length, safe) = r["gid"], r["flags"], r["groups"][FIRST_GROUP:], r["box"]
        c = np.stack(npn.coords(r["pos"], length), axis=1)
        member = gid >= FIRST_GROUP
        cp = c[groups["point"]]
        across = np.zeros(len(groups), bool)
        for d in range(3):
            if r["pbc"][d]:
                L = int(length[d])
                delta = c[member, d] - cp[gid[member] - FIRST_GROUP, d]
                moved = ((delta + L // 2) % L - L // 2) != delta
                across[np.unique(gid[member][moved]) - FIRST_GROUP] = True
        good = (flags & npn.GOOD) != 0
        inlayer = np.zeros(len(gid), bool)                          # from the coordinates, not from the flag
        for d in range(3):
            if not r["pbc"][d]:
                inlayer |= (c[:, d] < int(safe[d])) | (c[:, d] >= int(length[d]) - int(safe[d]))
        layer = np.zeros(len(groups), bool)
        layer[np.unique(gid[member & inlayer]) - FIRST_GROUP] = True
        o = r["plc"][5].oracle()
        crossing = np.zeros(len(groups), bool)
        crossing[np.asarray(r["plc"][1], np.int64)] = True
        passing = npc.passing(groups["Mass"], groups["good"], groups["point"], par.min_mass)
        with np.errstate(invalid="ignore"):
            band = r["plc"][5].band()
            inband = int((o["tried"] & ((np.abs(o["bb"]) < band) | (np.abs(o["aa"]) < band))).sum())
        out.append(dict(stored=len(gid), groups=len(groups), massive=int((groups["Mass"] >= par.min_mass).sum()), largest=int(groups["Mass"].max(initial=0)),
                        single=int((groups["Mass"] == 1).sum()), id0=int((gid == 0).sum()), id1=int((gid == 1).sum()), across_a_face=int(across.sum()),
                        in_the_layer=int(layer.sum()), layer_members_good=int((member & inlayer & good).sum()),
                        crossings=int(r["plc"][3]), passing=int(passing.sum()), passing_without_crossing=int((passing & ~crossing).sum()),
                        pairs_in_the_band=inband, catalogue=int(r["cat"][2])))
    return out


def input_conditions(res, par):
    """what the walk must contain so that no hand-off is tested on nothing; from the numpy side alone, the same counts for every
    box size: 50 groups of Mass >= MIN_MASS in every sub-box, a group of one particle and one of more than 64, loose particles of
    both kinds, a group across a periodic face, members in the boundary layer that are not good, 20 crossings and a passing group
    that crosses in no replication, no tried pair in the band, no passing Mass within 1e-9 bins of a bin edge"""
    fig = figures(res, par)
    open_axes = any(not all(r["pbc"]) for r in res["boxes"])
    for r, f in zip(res["boxes"], fig):
        assert f["massive"] >= 50, f
        assert f["pairs_in_the_band"] == 0, f
        r["cat"][5].input_conditions()                              # no passing Mass within 1e-9 bins of a bin edge
        if r["plc"][2].size:
            r["plc"][5].input_conditions()
    assert sum(f["id0"] for f in fig) >= 1 and sum(f["id1"] for f in fig) >= 1, fig
    assert sum(f["single"] for f in fig) >= 1 and max(f["largest"] for f in fig) > 64, fig
    assert sum(f["across_a_face"] for f in fig) >= 1, fig
    if open_axes:
        assert sum(f["in_the_layer"] for f in fig) >= 1 and sum(f["layer_members_good"] for f in fig) == 0, fig
    assert sum(f["crossings"] for f in fig) >= 20 and sum(f["passing_without_crossing"] for f in fig) >= 1, fig
    return fig
