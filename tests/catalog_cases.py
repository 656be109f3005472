"""The cases of the catalogue tests (tests/test_catalog_cpu.py, tests/test_gpu_catalog.py): inputs made from
tests/golden/plc_tables.json through tests/plc_cases.py, the oracle's answer (tests/np_catalog.py) computed once per case, and the
pass criteria both tests apply to whatever computed the records -- pf_catalog_core.h on the host or the kernels.

Geometry: a sub-box of 64 cells a side that starts at `stabl` in a box of GSglobal = 128 cells; on a periodic axis the sub-box is
the whole box (Lgwbl = 128, stabl = 0).  InterPartDist is the fixture's, ParticleMass 7.1e10.  stabl = (60, 60, -32) puts the z
coordinates below zero and (100, -20, 120) puts x and z beyond GSglobal and y below zero, so that both global wraps of
write_halos.c:300-313 fire on q and on x (checked in input_conditions).  The mass function uses DELTAM = 0.05 and mmin as
src/initialization.c:1122 forms it with MinHaloMass 10."""
import functools

import numpy as np

import np_catalog as npc
import np_plc as npp
import plc_cases as pc

MIN_MASS = pc.MIN_MASS
VEL_NAMES = pc.VEL_NAMES
GS = 128
PMASS = 7.1e10
DELTAM = 0.05
MMIN = float(np.log10(np.float64(MIN_MASS) * np.float64(PMASS)) - 0.001 * DELTAM)   # initialization.c:1122
NBIN_ALL = 100   # log10(150000 / 10) / 0.05 = 83.5: every mass of the cases lies below bin 100
NBIN_SHORT = 20  # ... and Mass > 100 lies beyond bin 20
F32, F64 = np.float32, np.float64


def catalog_dtype(T, light=False):
    """catalog_data (src/pinocchio.h:515-524) as the compiler lays it out"""
    t, pb = np.dtype(T).str, np.dtype(T).itemsize
    names, formats, offsets = ["name", "M", "x", "v", "q"], ["<u8", t, (t, 3), (t, 3), (t, 3)], [0, 8, 8 + pb, 8 + 4 * pb, 8 + 7 * pb]
    size = 8 + 10 * pb
    if not light:
        names, formats, offsets = names + ["n", "pad"], formats + ["<i4", "<i4"], offsets + [size, size + 4]
        size += 8
    return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": size})


class Case:
    """one call of pf_catalog and what the oracle says of it"""

    def __init__(self, name, T=F32, n=65, nk=1, myseg=0, use_v31=False, order=3, F=1.15, pbc=(0, 0, 0), stabl=(60, 60, -32), hfactor=0.67, min_mass=MIN_MASS,
                 masses="random", nbin=NBIN_ALL, light=False, flags=True, seed=1):
        self.name, self.T, self.n, self.nk, self.myseg, self.use_v31, self.order, self.F = name, T, n, nk, myseg, use_v31, order, F
        self.pbc = tuple(int(p) for p in pbc)
        self.stabl = tuple(0 if p else s for p, s in zip(self.pbc, stabl))
        self.lgwbl = tuple(GS if p else 64 for p in self.pbc)
        self.gs, self.hfactor, self.min_mass, self.nbin, self.light, self.flags = (GS, GS, GS), hfactor, min_mass, nbin, light, flags
        self.ipd, self.pmass, self.mmin, self.deltam = pc.fixture()["InterPartDist"], PMASS, MMIN, DELTAM
        self.z_seg, self.z_prev = 0.0, 0.3
        rng = np.random.default_rng(seed)
        g = np.zeros(n, dtype=pc.group_dtype(T))
        g["Pos"] = rng.uniform(0.5, np.array(self.lgwbl) - 0.5, (n, 3))
        # (a few next to the faces of a periodic axis: a displacement of order one cell takes them across)
        for i in range(min(n, 48)):
            for j in range(3):
                if self.pbc[j] and i % 3 != 2:
                    g["Pos"][i, j] = (0.05, GS - 0.05)[(i + j) % 2]
        for k, nm in enumerate(VEL_NAMES):
            g[nm] = rng.normal(0.0, (1.0, 0.1, 0.03, 0.03)[k % 4], (n, 3))
        if masses == "histogram":
            # 1 ... 5000 and a few at 150 000
            m = rng.integers(1, 5001, n)
            m[:8] = [1, 9, 10, 11, 5000, 150000, 150000, 150000][:n]
            g["Mass"] = m
        elif nk == 1:
            g["Mass"] = rng.integers(MIN_MASS, 500, n)
        else:
            g["Mass"] = rng.choice([0, 1, 2, 12, 50, 300, 2000, 4000], n)   # plc_cases' list: below, inside and at the top of set_obj's range
        g["name"] = rng.integers(1, 2 ** 62, n, dtype=np.int64).astype(np.uint64)
        g["good"], g["point"] = 1, rng.integers(0, 1000, n)
        g["Flast"] = 1.3
        # the filter rows of plc_cases: Mass just below and at MinHaloMass, good = 0, point = -1
        if masses == "random" and nk == 1:
            for i, (f, val) in enumerate((("Mass", MIN_MASS - 1), ("Mass", MIN_MASS), ("good", 0), ("point", -1))):
                if n > 8 + i:
                    g[f][3 + i] = val
        self.groups = g

    # -- the two sides' inputs ------------------------------------------------------------------------------------------
    def bins(self):
        return (self.nbin, self.mmin, self.deltam)

    def call_kwargs(self):
        """keyword arguments of Fmax.catalog beside groups, group_layout, capacity and out"""
        return dict(F=self.F, myseg=self.myseg, z_seg=self.z_seg, stabl=self.stabl, Lgwbl=self.lgwbl, InterPartDist=self.ipd, ParticleMass=self.pmass, GSglobal=self.gs,
                    hfactor=self.hfactor, pbc=self.pbc, min_mass=self.min_mass, z_prev=self.z_prev, use_v31=self.use_v31, bins=self.bins())

    def np_objects(self, groups=None):
        g = self.groups if groups is None else groups
        seg = npp.Segment(self.myseg, self.z_seg, self.z_prev, self.use_v31, self.order)
        vel = np.stack([g[nm] for nm in VEL_NAMES]) if len(g) else np.zeros((8, 0, 3), self.T)
        box = npc.Box(self.stabl, self.lgwbl, self.pbc, self.gs, self.ipd, self.pmass, self.hfactor)
        return pc.cosmology(self.nk), seg, npp.Groups(g["Mass"], g["Pos"].reshape(-1, 3), vel, self.T), box

    def passes(self, groups=None):
        g = self.groups if groups is None else groups
        return npc.passing(g["Mass"], g["good"] if self.flags else None, g["point"] if self.flags else None, self.min_mass)

    @functools.lru_cache(None)
    def oracle(self):
        """dict: index (the passing groups, ascending), the records of them, ninbin, massinbin (running sum), sum_mass"""
        cos, seg, G, box = self.np_objects()
        idx = np.nonzero(self.passes())[0]
        o = npc.records(cos, seg, npp.subset(G, idx), self.F, box)
        o["index"] = idx
        o["ninbin"], o["massinbin"], o["sum_mass"] = npc.mass_function(self.groups["Mass"][idx], self.pmass, self.nbin, self.mmin, self.deltam)
        return o

    def flat(self):
        """the case as tests/cpu_emul/catalog_emul.cpp reads it: (hdr int64, data float64)"""
        kw, g = pc.cosmology_tables(self.nk), self.groups
        kgm = np.asarray(kw.get("k_gm_displ", []), np.float64)
        hdr = np.array([np.dtype(self.T).itemsize, kw["x"].size, self.nk, kgm.size, self.myseg, int(self.use_v31), self.order, self.min_mass, self.n, self.nbin,
                        *self.stabl, *self.lgwbl, *self.gs, *self.pbc], dtype=np.int64)
        val = np.zeros((27, self.n))
        val[0:3] = g["Pos"].reshape(-1, 3).T
        for k, nm in enumerate(VEL_NAMES):
            val[3 + 3 * k:6 + 3 * k] = g[nm].reshape(-1, 3).T
        ok = ((g["point"] >= 0) & (g["good"] != 0)) if self.flags else np.ones(self.n, bool)
        data = np.concatenate([[kw.get("logkmin", -3.0), kw.get("deltalogk", 0.5), kw["k_for_GM"], kw.get("rad_gm0", 0.0)], [self.z_seg, self.z_prev],
                               [self.F, self.ipd, self.pmass, self.hfactor, self.mmin, self.deltam], kw["x"], kw["comvdist"], kw["hubble"], np.ravel(kw["grow"]),
                               np.ravel(kw["fomega"]), kgm, g["Mass"].astype(np.float64), ok.astype(np.float64), val.ravel()]).astype(np.float64)
        return hdr, data

    # -- the pass criteria ----------------------------------------------------------------------------------------------
    def L(self):
        """the largest coordinate magnitude of the case, in cells: positions in the sub-box, in the global box, and the box itself"""
        if not self.n:
            return float(self.gs[0])
        p = self.groups["Pos"].astype(np.float64)
        return float(max(np.abs(p).max(), np.abs(p + np.asarray(self.stabl)).max(), self.gs[0]) + 8.0)

    def band(self):
        """8 ulp32(L) cells, plc_cases.Case.band: the sum of at most eight PRODFLOAT terms of magnitude <= L that a position is"""
        return 8.0 * float(np.spacing(np.float32(self.L())))

    def input_conditions(self):
        """what the generator owes the tests, from the oracle alone: no Mass present within 1e-9 bins of a bin edge"""
        m = self.groups["Mass"][self.passes()]
        m = m[m >= 1]
        if m.size:
            q = npc.bin_quotient(m, self.pmass, self.mmin, self.deltam)
            assert (np.abs(q - np.rint(q)) > 1e-9).all(), self.name

    def check(self, rec, group_of, count, ninbin, massinbin, capacity=None, printer=None):
        """rec: structured records of catalog_dtype; group_of their batch indices; count, ninbin, massinbin as the call returned them"""
        o = self.oracle()
        T, idx = self.T, o["index"]
        g = self.groups
        assert count == len(idx), (self.name, count, len(idx))
        m = count if capacity is None else min(count, capacity)
        group_of = np.asarray(group_of, np.int64)
        assert len(rec) == len(group_of) == m
        assert np.array_equal(group_of, idx[:m]), self.name                    # the set and the order: ascending batch index
        sel = slice(0, m)
        assert np.array_equal(rec["name"], g["name"][idx[sel]]), self.name
        if "n" in rec.dtype.names:
            assert np.array_equal(rec["n"], g["Mass"][idx[sel]]), self.name
        assert rec["M"].tobytes() == o["M"][sel].tobytes(), self.name
        assert rec["q"].tobytes() == np.ascontiguousarray(o["q"][sel]).tobytes(), self.name
        scale = self.ipd * self.hfactor
        if m:
            top = T(np.float64(self.gs[0]) * scale)
            x = rec["x"].astype(np.float64)
            assert (rec["x"] >= 0).all() and (rec["x"] <= top).all(), (self.name, float(x.min()), float(x.max()))
            Lbox = self.gs[0] * scale
            dx = np.abs(x - o["x"][sel].astype(np.float64))
            dx = np.minimum(dx, np.abs(Lbox - dx)).max()
            assert dx <= scale * self.band(), (self.name, dx, scale * self.band())
            dv = np.abs(rec["v"].astype(np.float64) - o["v"][sel].astype(np.float64)).max(axis=1)
            vb = 8.0 * np.spacing(o["vscale"][sel].astype(np.float32)).astype(np.float64)
            assert (dv <= vb).all(), (self.name, float((dv / vb).max()))
        self.last_bit_equal = bool(rec["x"].tobytes() == np.ascontiguousarray(o["x"][sel]).tobytes() and rec["v"].tobytes() == np.ascontiguousarray(o["v"][sel]).tobytes())
        if printer:
            printer(self.name, "records", m, "of", count, "x and v bit-equal to the oracle's:", self.last_bit_equal)
        # the mass function counts all passing groups, whatever the capacity
        assert np.array_equal(ninbin, o["ninbin"]), (self.name, ninbin, o["ninbin"])
        want = np.array([np.float64(s) * np.float64(self.pmass) for s in o["sum_mass"]], np.float64)
        assert np.asarray(massinbin, np.float64).tobytes() == want.tobytes(), self.name
        tol = (o["ninbin"].astype(np.float64) + 1.0) * 2.0 ** -53 * o["massinbin"]
        assert (np.abs(np.asarray(massinbin) - o["massinbin"]) <= tol).all(), self.name
        if self.nbin == NBIN_ALL and self.min_mass >= MIN_MASS:   # the bins cover every passing group: none below mmin, none beyond the top
            assert int(np.sum(ninbin)) == int((g["Mass"][idx] >= 1).sum()), self.name


def wrap_case(T):
    """all velocities zero, so x must be bit-equal to q; Pos + stabl lands exactly on -0.5 (y of group 0), on 0 (y of group 1), on
    GSglobal (x of group 0) and on GSglobal - 0.5 (x of group 1)"""
    c = Case("wrap", T=T, n=4, stabl=(100, -20, 120), hfactor=1.0, seed=20)
    g = c.groups
    for nm in VEL_NAMES:
        g[nm] = 0.0
    g["Mass"], g["good"], g["point"] = 20, 1, 0
    g["Pos"][0] = (28.0, 19.5, 8.0)      # 128, -0.5, 128
    g["Pos"][1] = (27.5, 20.0, 7.5)      # 127.5, 0, 127.5
    g["Pos"][2] = (28.5, 20.5, 8.5)      # 128.5, 0.5, 128.5
    g["Pos"][3] = (0.0, 0.0, 0.0)        # 100, -20, 120
    c.expect_q_cells = np.array([[0.0, 127.5, 0.0], [127.5, 0.0, 127.5], [0.5, 0.5, 0.5], [100.0, 108.0, 120.0]])
    return c


# name -> how the case is made.  Group counts 0, 1, 63, 64, 65, 257, 1025, 4097 (one lane, a wave less one, a wave, a wave and one, a
# workgroup and one, four and one, sixteen and one); float and double products; segments 0 and 1 with both use_v31; orders 1, 2, 3;
# F 1.0, 1.15, 1.3; the four pbc / stabl settings; hfactor 0.67 and 1; nk = 1 and 10; min_mass 10 and 1; nbin 100 and 20
CASES = {
    "n0": lambda: Case("n0", n=0),
    "n1": lambda: Case("n1", n=1, F=1.0, hfactor=1.0),
    "n63": lambda: Case("n63", n=63, seed=2),
    "n64_far": lambda: Case("n64_far", n=64, stabl=(100, -20, 120), F=1.3, seed=3),
    "n65_seg1": lambda: Case("n65_seg1", n=65, myseg=1, seed=4),
    "n65_seg1_v31": lambda: Case("n65_seg1_v31", n=65, myseg=1, use_v31=True, seed=4),
    "n257_nk10": lambda: Case("n257_nk10", n=257, nk=10, min_mass=0, seed=5),
    "n1025_seg1_nk10_o2": lambda: Case("n1025_seg1_nk10_o2", n=1025, nk=10, myseg=1, order=2, min_mass=0, stabl=(100, -20, 120), seed=6),
    "n4097": lambda: Case("n4097", n=4097, stabl=(100, -20, 120), hfactor=1.0, seed=7),
    "order1": lambda: Case("order1", order=1, F=1.0, seed=8),
    "order2_seg1": lambda: Case("order2_seg1", order=2, myseg=1, F=1.3, seed=9),
    "pbc111": lambda: Case("pbc111", n=257, pbc=(1, 1, 1), seed=10),
    "pbc101_seg1": lambda: Case("pbc101_seg1", n=257, pbc=(1, 0, 1), myseg=1, hfactor=1.0, seed=11),
    "no_flags": lambda: Case("no_flags", n=63, flags=False, seed=2),
    "light": lambda: Case("light", n=65, light=True, seed=12),
    "f64_nk10": lambda: Case("f64_nk10", T=F64, n=257, nk=10, min_mass=0, seed=13),
    "f64_seg1_pbc": lambda: Case("f64_seg1_pbc", T=F64, n=65, myseg=1, pbc=(1, 1, 1), F=1.3, seed=14),
    "f64_far_light": lambda: Case("f64_far_light", T=F64, n=64, stabl=(100, -20, 120), light=True, hfactor=1.0, seed=15),
    "hist_all": lambda: Case("hist_all", n=4097, masses="histogram", seed=16),
    "hist_min1": lambda: Case("hist_min1", n=4097, masses="histogram", min_mass=1, seed=16),
    "hist_short": lambda: Case("hist_short", n=1025, masses="histogram", min_mass=1, nbin=NBIN_SHORT, seed=17),
    "wrap": lambda: wrap_case(F32),
    "wrap_f64": lambda: wrap_case(F64),
}


@functools.lru_cache(None)
def case(name):
    """the case and its oracle, made once per process and left unchanged"""
    return CASES[name]()
