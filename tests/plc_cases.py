"""The cases of the light-cone tests (tests/test_plc_cpu.py, tests/test_gpu_plc.py): inputs made from tests/golden/plc_tables.json, the
oracle's answer (tests/np_plc.py) computed once per case, and the pass criteria both tests apply to whatever computed the records --
pf_plc_core.h on the host or the kernels.

Geometry: the fixture's cone (observer at the origin, axis (1, 1, 0) / sqrt 2, aperture 30 degrees, InterPartDist 5.58 Mpc) and a
sub-box of 64 cells a side that starts at `stabl`.  The 13-replication cases use the fixture's replications and its grid of 128; the
cases with 1 and 65 replications shift the observer by whole boxes of 8 cells, so that every replication sees the sub-box under a
small angle.  Displacements are of order one cell, against a slope of the comoving distance of about 700 cells per unit F, so
condition_PLC is monotonic on every interval (checked by the CPU test)."""
import functools
import json
import os

import numpy as np

import np_plc as npp

HERE = os.path.dirname(os.path.abspath(__file__))
MIN_MASS = 10
VEL_NAMES = ["Vel", "Vel_2LPT", "Vel_3LPT_1", "Vel_3LPT_2", "Vel_prev", "Vel_2LPT_prev", "Vel_3LPT_1_prev", "Vel_3LPT_2_prev"]
NK10 = dict(logkmin=-3.0, deltalogk=0.5, rad_gm0=40.0, k_gm_displ=[5e-4, 0.02, 0.08, 0.3, 1.2, 5.0, 50.0])


@functools.lru_cache(None)
def fixture():
    return json.load(open(os.path.join(HERE, "golden", "plc_tables.json")))


@functools.lru_cache(None)
def cosmology_tables(nk):
    """keyword arguments of Fmax.plc_set_cosmology and of np_plc.Cosmology"""
    fx = fixture()
    r = np.array(fx["rows"], dtype=np.float64)
    a = r[:, 0]
    z = 1.0 / a - 1.0
    hub = 100.0 * fx["Hubble100"] * np.sqrt(fx["Omega0"] * (1.0 + z) ** 3 + fx["OmegaLambda"])
    grow, fom = np.log10(r[:, 2:6].T), r[:, 6:10].T.copy()
    kw = dict(x=np.log10(a), comvdist=r[:, 1].copy(), hubble=hub, k_for_GM=0.1)
    if nk == 1:
        kw.update(grow=grow[:, None, :].copy(), fomega=fom[:, None, :].copy())
    else:
        # ten k-bins: the fixture's columns times a smooth factor in k -- inputs, not a claim about the cosmology
        j = np.arange(nk, dtype=np.float64)
        kw.update(grow=grow[:, None, :] + np.log10(1.0 + 0.01 * j * (1.0 + 0.1 * j))[None, :, None], fomega=fom[:, None, :] * (1.0 + 0.004 * j)[None, :, None], **NK10)
    return kw


@functools.lru_cache(None)
def cosmology(nk):
    return npp.Cosmology(**cosmology_tables(nk))


def group_dtype(T):
    t = np.dtype(T).str
    return np.dtype([("Mass", "<i4"), ("Pos", t, 3)] + [(n, t, 3) for n in VEL_NAMES] + [("name", "<u8"), ("good", "<i4"), ("point", "<i4"), ("Flast", t)], align=True)


def synthetic_reps(nrep, kind):
    shifts = [(i, j, k) for k in (0, -1, 1) for i in (0, -1, 1, -2, 2) for j in (0, 1, -1, 2, -2)][:nrep]
    out = []
    for n, (i, j, k) in enumerate(shifts):
        if kind in ("all", "none"):
            out.append((i, j, k, 1.5, 1.0))
        elif kind == "last":
            out.append((i, j, k, 1.5, 1.0 if n == nrep - 1 else 1.4))
        else:
            out.append((i, j, k, 1.2 if n % 3 == 1 else 1.5, 1.15 if n % 2 else 1.0))
    return out


class Case:
    """one call of pf_plc_cross and what the oracle says of it"""

    def __init__(self, name, T=np.float32, ncand=65, nrep=13, crossing="random", events=False, myseg=0, order=3, nk=1, use_v31=False, seed=1):
        self.name, self.T, self.ncand, self.nrep, self.crossing, self.events = name, T, ncand, nrep, crossing, events
        self.myseg, self.order, self.nk, self.use_v31, self.seed = myseg, order, nk, use_v31, seed
        fx = fixture()
        rng = np.random.default_rng(seed)
        self.ipd = fx["InterPartDist"]
        ax = np.array(fx["axis"])
        self.zvers = ax / np.linalg.norm(ax)
        self.xvers, self.yvers = np.array([0.0, 0.0, 1.0]), np.cross(self.zvers, [0.0, 0.0, 1.0])
        if nrep == 13:
            self.reps, self.gs, self.stabl = [tuple(r) for r in fx["replications"]], fx["GridSize"], (60, 60, -32)
        else:
            self.reps, self.gs, self.stabl = synthetic_reps(nrep, crossing), (8, 8, 8), (60, 60, -32)
        self.nzbins, self.lastz, self.delta_z = fx["nzbins"], 0.0, 0.05
        self.z_seg, self.z_prev = 0.0, 0.3
        n = ncand
        g = np.zeros(n, dtype=group_dtype(T))
        lo, hi = (16.0, 48.0) if crossing == "all" else (0.5, 63.5)
        g["Pos"] = rng.uniform(lo, hi, (n, 3))
        for k, nm in enumerate(VEL_NAMES):
            g[nm] = rng.normal(0.0, (1.0, 0.1, 0.03, 0.03)[k % 4], (n, 3))
        if nk == 1:
            g["Mass"] = rng.integers(MIN_MASS, 500, n)
        else:
            # masses that put set_obj's interp below 0 (2000, 4000: myk = k_GM_displ[0] < kmin), inside its range, in its top interval
            # (1, 2) and AT its top: a group of no extent, Mass 0, has interp == Nsmooth - 1, where the reference reads
            # k_GM_displ[Nsmooth] with weight zero, and its myk = k_GM_displ[Nsmooth - 1] = 50 > kmax takes the last k-bin alone
            g["Mass"] = rng.choice([0, 1, 2, 12, 50, 300, 2000, 4000], n)
        g["name"] = rng.integers(1, 2 ** 62, n, dtype=np.int64).astype(np.uint64)
        g["good"], g["point"] = 1, rng.integers(0, 1000, n)
        if crossing == "none":
            g["Flast"] = 1.001
        elif crossing == "all":
            g["Flast"] = 1.3
        elif crossing == "last":
            g["Flast"] = 1.001
            if n:
                g["Flast"][-1] = 1.3
        else:
            g["Flast"] = rng.uniform(1.05, 1.3, n)
            # the filter: Mass just below and at MinHaloMass, good = 0, point = -1
            for i, (f, val) in enumerate((("Mass", MIN_MASS - 1), ("Mass", MIN_MASS), ("good", 0), ("point", -1))):
                if nk == 1 and n > 8 + i:
                    g[f][3 + i] = val
        self.min_mass = MIN_MASS if nk == 1 else 0
        self.groups = g
        # (the table's spline is monotonic for z > -0.017 only: no interval begins below F = 1)
        self.f_lo = np.maximum(g["Flast"] - rng.uniform(0.01, 0.1, n), 1.0).astype(T) if events else None

    # -- the two sides' inputs ------------------------------------------------------------------------------------------
    def geometry_kwargs(self):
        return dict(center=(0.0, 0.0, 0.0), xvers=self.xvers, yvers=self.yvers, zvers=self.zvers, aperture=fixture()["PLCAperture"], Fstop=fixture()["Fstop"],
                    InterPartDist=self.ipd, GSglobal=self.gs, repls=self.reps, LastzForPLC=self.lastz, delta_z=self.delta_z, nzbins=self.nzbins)

    def np_objects(self, groups=None, use_v31=None):
        g = self.groups if groups is None else groups
        geo = npp.Geometry((0.0, 0.0, 0.0), self.zvers, fixture()["PLCAperture"], fixture()["Fstop"], self.ipd, self.gs, self.reps, self.stabl, self.lastz, self.delta_z, self.nzbins)
        seg = npp.Segment(self.myseg, self.z_seg, self.z_prev, self.use_v31 if use_v31 is None else use_v31, self.order)
        vel = np.stack([g[nm] for nm in VEL_NAMES])
        return cosmology(self.nk), geo, seg, npp.Groups(g["Mass"], g["Pos"], vel, self.T)

    @functools.lru_cache(None)
    def oracle(self, with_flags=True):
        cos, geo, seg, G = self.np_objects()
        g = self.groups
        passes = ((g["point"] >= 0) & (g["good"] != 0)) if with_flags else None
        return npp.cross(cos, geo, seg, G, g["Flast"], self.events, self.f_lo, passes, self.min_mass)

    def flat(self):
        """the case as tests/cpu_emul/plc_emul.cpp reads it: (hdr int64, data float64)"""
        kw, g = cosmology_tables(self.nk), self.groups
        kgm = np.asarray(kw.get("k_gm_displ", []), np.float64)
        hdr = np.array([np.dtype(self.T).itemsize, kw["x"].size, self.nk, kgm.size, self.myseg, int(self.use_v31), self.order, int(self.events), self.min_mass,
                        self.ncand, len(self.reps), self.nzbins, *self.stabl, *self.gs], dtype=np.int64)
        val = np.zeros((29, self.ncand))
        val[0:3] = g["Pos"].T
        for k, nm in enumerate(VEL_NAMES):
            val[3 + 3 * k:6 + 3 * k] = g[nm].T
        val[27] = g["Flast"]
        if self.events:
            val[28] = self.f_lo
        data = np.concatenate([[kw.get("logkmin", -3.0), kw.get("deltalogk", 0.5), kw["k_for_GM"], kw.get("rad_gm0", 0.0)], [self.z_seg, self.z_prev], [0.0, 0.0, 0.0], self.zvers,
                               [fixture()["PLCAperture"], fixture()["Fstop"], self.ipd, self.lastz, self.delta_z], kw["x"], kw["comvdist"], kw["hubble"],
                               np.ravel(kw["grow"]), np.ravel(kw["fomega"]), kgm, np.ravel(np.array(self.reps, np.float64)), g["Mass"].astype(np.float64),
                               ((g["point"] >= 0) & (g["good"] != 0)).astype(np.float64), val.ravel()]).astype(np.float64)
        return hdr, data

    # -- the pass criteria ----------------------------------------------------------------------------------------------
    def L(self):
        """the largest coordinate magnitude of the case: positions relative to the observers, in cells"""
        _, geo, _, G = self.np_objects()
        if not self.ncand:
            return 1.0
        p = G.q.astype(np.float64) + np.asarray(self.stabl)
        return float(max(np.abs(p).max(), np.abs(p[:, None, :] - geo.observer[None]).max()) + 8.0)

    def band(self):
        """8 ulp32(L) cells: the sum of at most eight fp32 terms of magnitude <= L that a position is"""
        return 8.0 * float(np.spacing(np.float32(self.L())))

    def input_conditions(self):
        """what the generator owes the tests, from the oracle alone: at most 1e-3 of the tried pairs in the band, condition_PLC monotonic
        on every crossing interval, no crossing pair within 1e-3 degrees of the aperture's edge, every root found"""
        o = self.oracle()
        tr = o["tried"]
        if tr.sum():
            with np.errstate(invalid="ignore"):
                inband = (np.abs(o["bb"]) < self.band()) | (np.abs(o["aa"]) < self.band())
            assert (inband & tr).sum() <= 1e-3 * tr.sum(), (self.name, int((inband & tr).sum()), int(tr.sum()))
        if len(o["cand"]):
            cos, geo, seg, G = self.np_objects()
            assert (o["resid"] < 1e-2 * self.ipd).all()
            assert (np.abs(o["store"]["angle"] - fixture()["PLCAperture"]) > 1e-3).all(), self.name
            lo, hi = o["Flo"][o["cand"]].astype(np.float64), self.groups["Flast"][o["cand"]].astype(np.float64)
            prev = None
            for t in np.linspace(0.0, 1.0, 17):
                c = npp.condition_at(cos, geo, seg, G, o["cand"], o["rep"], (lo + t * (hi - lo)).astype(self.T))
                assert prev is None or (c < prev).all(), (self.name, t)
                prev = c

    def check(self, rec, cand, rep, count, unconverged, capacity=None):
        """rec: structured records (Mass, name, z, x, v); cand, rep: their pairs; count, unconverged as the call returned them"""
        o = self.oracle()
        cos, geo, seg, G = self.np_objects()
        assert unconverged == 0, self.name
        band, brent_err = self.band(), 1e-2 * self.ipd
        cand, rep = np.asarray(cand, np.int64), np.asarray(rep, np.int64)
        assert len(rec) == len(cand) == len(rep) == (count if capacity is None else min(count, capacity))
        # ascending (candidate, replication) order
        key = cand * (len(self.reps) + 1) + rep
        assert (np.diff(key) > 0).all(), self.name
        # the set of stored pairs equals the oracle's, but for pairs whose |aa| or |bb| lies in the band
        st = o["store"]
        want = set(zip(o["cand"][st["inside"]].tolist(), o["rep"][st["inside"]].tolist())) if st is not None else set()
        got = set(zip(cand.tolist(), rep.tolist()))
        if capacity is None or capacity >= count:
            for (i, r) in want ^ got:
                assert o["tried"][i, r] and (abs(o["bb"][i, r]) < band or abs(o["aa"][i, r]) < band), (self.name, i, r, o["bb"][i, r], o["aa"][i, r])
        else:
            assert got <= want and len(got) == capacity
        if not len(cand):
            return
        F = rec["z"].astype(self.T)  # z = F - 1 is exact for F in [1, 2): recover F
        F = (F.astype(np.float64) + 1.0).astype(self.T)
        assert np.array_equal(((F.astype(np.float64) - 1.0).astype(self.T)), rec["z"]), self.name
        g = self.groups
        Flo, Flast = o["Flo"][cand], g["Flast"][cand]
        assert ((F >= np.minimum(Flo, Flast)) & (F <= np.maximum(Flo, Flast))).all(), self.name
        c = npp.condition_at(cos, geo, seg, G, cand, rep, F)
        assert (np.abs(c) < brent_err).all(), (self.name, float(np.abs(c).max()), brent_err)
        s = npp.store_at(cos, geo, seg, G, cand, rep, F)
        assert s["inside"].all(), self.name
        assert np.array_equal(rec["z"], s["z"]) and np.array_equal(rec["Mass"], g["Mass"][cand]) and np.array_equal(rec["name"], g["name"][cand]), self.name
        dx = np.abs(rec["x"].astype(np.float64) - s["x"].astype(np.float64)).max()
        assert dx <= self.ipd * band, (self.name, dx, self.ipd * band)
        dv = np.abs(rec["v"].astype(np.float64) - s["v"].astype(np.float64)).max(axis=1)
        vb = 8.0 * np.spacing(s["vscale"].astype(np.float32)).astype(np.float64)
        assert (dv <= vb).all(), (self.name, float((dv / vb).max()))
        self.last_bit_equal = bool(np.array_equal(rec["x"], s["x"]) and np.array_equal(rec["v"], s["v"]))

    def nz_expected(self, rec):
        nz = np.zeros(self.nzbins)
        b = ((rec["z"].astype(np.float64) - self.lastz) / self.delta_z).astype(int)
        b = np.where(b == self.nzbins, b - 1, b)
        np.add.at(nz, b[(b >= 0) & (b < self.nzbins)], 1.0)
        return nz


def equality_case(T, events):
    """two groups on the cone's axis and one replication with F1 = 1.18, F2 = 1.12: group 0 has F_lo == F1, group 1 has Flast == F2.  Both
    are tried at an event; in the last check (F_lo = Fstop) group 1 is not (Flast > F2 fails)"""
    c = Case("equality", T=T, ncand=2, nrep=1, crossing="random", events=events, seed=5)
    c.reps = [(0, 0, 0, 1.18, 1.12)]
    c.stabl = (50, 50, 0)
    c.min_mass = 0
    cos = cosmology(1)
    F1, F2 = T(1.18), T(1.12)
    g = c.groups
    for nm in VEL_NAMES:
        g[nm] = 0.0
    g["good"], g["point"], g["Mass"] = 1, 0, 20
    ends = [(F1, T(1.21)), (T(1.09), F2)]
    for i, (lo, hi) in enumerate(ends):
        d = cos.comvdist(0.5 * (float(lo) + float(hi)) - 1.0) / c.ipd
        g["Pos"][i] = d * c.zvers - np.array(c.stabl)
        g["Flast"][i] = hi
    assert (g["Pos"] >= 0).all() and (g["Pos"] < 64).all()
    c.f_lo = np.array([e[0] for e in ends], dtype=T) if events else None
    return c


def aperture_case(T):
    """groups at 25 and at 35 degrees from the cone's axis (aperture 30), all crossing replication (0, 0, 0) in the last check"""
    c = Case("aperture", T=T, ncand=64, nrep=1, crossing="all", seed=6)
    c.reps = [(0, 0, 0, 1.5, 1.0)]
    c.stabl = (8, 8, -32)
    c.min_mass = 0
    g = c.groups
    rng = np.random.default_rng(6)
    for nm in VEL_NAMES:
        g[nm] *= 0.01
    for i in range(c.ncand):
        ang = np.radians(25.0 if i % 2 == 0 else 35.0)
        phi = rng.uniform(-0.5, 0.5) + (0.0 if i % 4 < 2 else np.pi)
        d = rng.uniform(50.0, 55.0)
        # a ring around the axis restricted to directions near +-z, so that the point stays in the sub-box
        u = np.cos(ang) * c.zvers + np.sin(ang) * (np.cos(phi) * c.xvers + np.sin(phi) * c.yvers)
        g["Pos"][i] = d * u - np.array(c.stabl)
    assert (g["Pos"] >= 0).all() and (g["Pos"] < 64).all(), (g["Pos"].min(), g["Pos"].max())
    return c


# name -> how the case is made.  Candidate counts 0, 1, 63, 64, 65, 1025, 4097 (one lane, a wave less one, a wave, a wave and one, four
# workgroups and one, sixteen and one); 1, 13 and 65 replications; both modes; segments 0 and 1; orders 1, 2, 3; float and double
# products; nk = 1 and 10
F32, F64 = np.float32, np.float64
CASES = {
    "n0": lambda: Case("n0", ncand=0),
    "n1_r1_all": lambda: Case("n1_r1_all", ncand=1, nrep=1, crossing="all"),
    "n63_r13": lambda: Case("n63_r13", ncand=63, seed=2),
    "n64_r65_events": lambda: Case("n64_r65_events", ncand=64, nrep=65, events=True, seed=3),
    "n65_r13_seg1": lambda: Case("n65_r13_seg1", ncand=65, myseg=1, seed=4),
    "n65_r13_seg1_v31": lambda: Case("n65_r13_seg1_v31", ncand=65, myseg=1, use_v31=True, seed=4),
    "n1025_r65_events_seg1_nk10_o2": lambda: Case("n1025_r65_events_seg1_nk10_o2", ncand=1025, nrep=65, events=True, myseg=1, nk=10, order=2, seed=5),
    "n4097_r13": lambda: Case("n4097_r13", ncand=4097, seed=6),
    "none": lambda: Case("none", crossing="none"),
    "all_r65": lambda: Case("all_r65", ncand=64, nrep=65, crossing="all", seed=7),
    "last_r65": lambda: Case("last_r65", ncand=65, nrep=65, crossing="last", seed=8),
    "order1": lambda: Case("order1", order=1, seed=9),
    "order2_seg1_events": lambda: Case("order2_seg1_events", order=2, myseg=1, events=True, seed=10),
    "nk10": lambda: Case("nk10", ncand=257, nk=10, seed=11),
    "f64_nk10": lambda: Case("f64_nk10", T=F64, ncand=257, nk=10, seed=12),
    "f64_seg1_events_r65": lambda: Case("f64_seg1_events_r65", T=F64, ncand=65, nrep=65, myseg=1, events=True, seed=13),
    "equality_events": lambda: equality_case(F32, True),
    "equality_last_check": lambda: equality_case(F32, False),
    "equality_events_f64": lambda: equality_case(F64, True),
    "aperture": lambda: aperture_case(F32),
}


@functools.lru_cache(None)
def case(name):
    """the case and its oracle, made once per process and left unchanged"""
    return CASES[name]()


def out_dtype(T):
    t = np.dtype(T).str
    return np.dtype({"names": ["Mass", "name", "z", "x", "v"], "formats": ["<i4", "<u8", t, (t, 3), (t, 3)], "offsets": [0, 8, 16, 16 + np.dtype(T).itemsize, 16 + 4 * np.dtype(T).itemsize],
                     "itemsize": 72 if np.dtype(T).itemsize == 8 else 48})
