"""The cases of the particle-state tests (tests/test_points_cpu.py, tests/test_gpu_points.py): inputs on prescribed columns, the
oracle's answer (tests/np_points.py) computed once per case, and the pass criteria both tests apply to whatever computed the states --
pf_points_core.h on the host or the kernel.  The cosmology tables are those of tests/plc_cases.py (nk = 1 and 10).

Columns: Fmax uniform in [1.05, 4) -- inside the knots, which span F = 0.661 .. 4.786 --, in [1.02, 1.3) with myseg = 1, velocities normal with the spreads 1, 0.1,
0.03, 0.03 cells of the four families, current and prev drawn apart.  Positions are drawn with repetition from the cells of the
sub-box.  The segment ends at z = 0 and begins at z = 0.3.

Pass criteria (the same for the host emulation and the device, against np_points with the host's libm, over every found particle):
  index, found   exact
  x              within Case.band() = 8 ulp32(L) cells, L the largest coordinate magnitude of the case, the distance taken modulo the
                 box on periodic axes; inside [0, Lgwbl[d]] on periodic axes
  w*, sigmaD     float products: within 1 ulp32 of max(|value|, 1) (w*) and of the value (sigmaD) -- both sides compute in double and
                 differ by a few ulp64 before the one rounding to float --; double products: within ULP64_BOUND ulp64 of
                 max(|value|, 1), see there"""
import functools

import numpy as np

import np_points as npo
import plc_cases as pc

F32, F64 = np.float32, np.float64

# double products: the largest distance of w* and sigmaD from the restatement measured on an MI355X over all cases of this file and
# the context cases of tests/test_gpu_points.py, in ulp64 of max(|value|, 1), was MEASURED_ULP64 (profiles/points_notes.md); the bound is twice
# that, rounded up to a power of two.  The margin covers libm differences between ROCm versions.
MEASURED_ULP64 = 6.69
ULP64_BOUND = 16.0

BOX16 = dict(n=16, x0=0, nxl=16, start=(-3, 0, 13), length=(12, 16, 10), safe=(1, 0, 1))      # y periodic; x and z open, their starts wrap
SLAB24 = dict(n=24, x0=12, nxl=12, start=(8, 3, 0), length=(9, 5, 24), safe=(2, 1, 0))        # the upper of two slabs; z periodic
MISS24 = dict(n=24, x0=0, nxl=12, start=(14, 3, 0), length=(9, 5, 24), safe=(2, 1, 0))        # the lower slab: planes 14 .. 22 miss it
Z_SEG, Z_PREV, SIGMA0 = 0.0, 0.3, 1.7


def ulp32(a):
    return np.spacing(np.abs(np.asarray(a, np.float64)).astype(np.float32)).astype(np.float64)


def check_states(T, got, want, length, periodic, band, name="", printer=None):
    """got, want [m][8]; -> the largest distance of w* / sigmaD in ulp64 of max(|value|, 1) (double products; 0.0 for float)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.dtype(T) and got.shape == want.shape, (name, got.dtype, got.shape, want.shape)
    worst = 0.0
    if len(got):
        g, w = got.astype(np.float64), want.astype(np.float64)
        assert np.isfinite(g).all(), name
        for d in range(3):
            dist = np.abs(g[:, 5 + d] - w[:, 5 + d])
            if periodic[d]:
                dist = np.minimum(dist, float(length[d]) - dist)
                assert ((g[:, 5 + d] >= 0.0) & (g[:, 5 + d] <= float(length[d]))).all(), (name, d)
            assert (dist <= band).all(), (name, d, float(dist.max()), band)
        dw, ds = np.abs(g[:, :4] - w[:, :4]), np.abs(g[:, 4] - w[:, 4])
        if np.dtype(T) == np.float32:
            assert (dw <= ulp32(np.maximum(np.abs(w[:, :4]), 1.0))).all(), (name, float((dw / ulp32(np.maximum(np.abs(w[:, :4]), 1.0))).max()))
            assert (ds <= ulp32(w[:, 4])).all(), (name, float((ds / ulp32(w[:, 4])).max()))
        else:
            worst = max(float((dw / np.spacing(np.maximum(np.abs(w[:, :4]), 1.0))).max()), float((ds / np.spacing(np.maximum(np.abs(w[:, 4]), 1.0))).max()))
            if printer:
                printer(f"{name}: largest distance of w*, sigmaD from the restatement: {worst:.2f} ulp64")
            assert ULP64_BOUND is not None and worst <= ULP64_BOUND, (name, worst, ULP64_BOUND)
    if printer:
        printer(f"{name}: {len(got)} states, {'bit-equal to' if got.tobytes() == want.tobytes() else 'within the bounds of'} the restatement")
    return worst


class Case:
    """one call of pf_debug_point_states and what the oracle says of it"""

    def __init__(self, name, T=F32, box=BOX16, count=777, myseg=0, order=2, lpt_order=3, nk=1, k_point=0.1, k_sigma=0.1, use_v31=False, kind="random", seed=1):
        self.name, self.T, self.box, self.count, self.myseg, self.order, self.lpt_order, self.nk = name, T, box, count, myseg, order, lpt_order, nk
        self.k_point, self.k_sigma, self.use_v31, self.kind = k_point, k_sigma, use_v31, kind
        self.n, self.x0, self.nxl, self.start, self.length, self.safe = (box[k] for k in ("n", "x0", "nxl", "start", "length", "safe"))
        self.periodic = [self.length[d] == self.n for d in range(3)]
        rng = np.random.default_rng(seed)
        n, nc = self.n, self.nxl * self.n * self.n
        # a later segment holds the collapse times between its two ends, F in [1, 1.3]: beyond them the weights extrapolate
        self.fmax = (rng.uniform(1.02, 1.3, nc) if myseg else rng.uniform(1.05, 4.0, nc)).astype(T)
        spread = np.repeat(np.tile([1.0, 0.1, 0.03, 0.03], 2), 3)[:, None]
        if myseg and kind == "branches":
            spread = 0.25 * spread      # F = 5.5 in a later segment has w = -4.3: displacements stay below a box length
        self.cols = (rng.normal(0.0, 1.0, (24, nc)) * spread).astype(T)
        ncells = int(np.prod(self.length))
        self.pos = rng.integers(0, ncells, count).astype(np.uint32)
        if kind == "branches":
            # the three branches of my_spline_eval: F = 5.5 lies below the first knot (-log10 F < x[0]), 0.6 above the last, 1.0 on the knot x = 0
            self.fmax[0::5], self.fmax[1::5], self.fmax[2::5] = 5.5, 0.6, 1.0
        if kind in ("wrap_zero", "wrap_both"):
            self.pos = rng.permutation(ncells).astype(np.uint32)[:count]
            self.cols[:] = 0
        if kind == "wrap_both":
            # the periodic axis of BOX16 is y, where sub-box and global coordinates agree: Vel_y = +6 in the upper half, -6 in the lower, so
            # that with w in (0.2, 1) the particles next to either face leave through it
            y = (np.arange(nc) // n) % n
            self.cols[1] = np.where(y >= n // 2, 6.0, -6.0)
            self.cols[13] = self.cols[1]
        for a in (self.fmax, self.cols, self.pos):
            a.setflags(write=False)

    def hint(self):
        """indices[] of sort_and_organize: the particles in ascending position"""
        return np.argsort(self.pos, kind="stable").astype(np.int32)

    @functools.lru_cache(None)
    def oracle(self):
        return npo.states(pc.cosmology(self.nk), self.n, self.x0, self.nxl, self.start, self.length, self.pos, self.fmax, self.cols, self.myseg, Z_SEG, Z_PREV, self.use_v31,
                          self.order, SIGMA0, self.k_sigma, self.k_point, self.lpt_order)

    def flat(self):
        """the case as tests/cpu_emul/points_emul.cpp reads it: (hdr int64, data float64)"""
        kw = pc.cosmology_tables(self.nk)
        hdr = np.array([np.dtype(self.T).itemsize, kw["x"].size, self.nk, self.myseg, int(self.use_v31), self.order, self.lpt_order, self.n, self.x0, self.nxl, self.count,
                        *self.start, *self.length], dtype=np.int64)
        data = np.concatenate([[kw.get("logkmin", -3.0), kw.get("deltalogk", 0.5), kw["k_for_GM"]], [Z_SEG, Z_PREV], [SIGMA0, self.k_sigma, self.k_point], kw["x"],
                               np.ravel(kw["grow"]), self.pos.astype(np.float64), self.fmax.astype(np.float64), np.ravel(self.cols).astype(np.float64)]).astype(np.float64)
        return hdr, data

    def L(self):
        o = self.oracle()
        m = float(max(self.length))
        if len(o["index"]):
            m = max(m, float(np.abs(o["states"][:, 5:].astype(np.float64)).max()), float(np.abs(o["q"].astype(np.float64)).max()))
        return m

    def band(self):
        """8 ulp32(L) cells: the sum of at most eight fp32 terms of magnitude <= L that a position is"""
        return 8.0 * float(np.spacing(np.float32(self.L())))

    def input_conditions(self):
        """what the generator owes the tests, from the oracle alone"""
        o = self.oracle()
        idx, st = o["index"], o["states"].astype(np.float64)
        assert np.isfinite(st).all(), self.name
        if self.box is MISS24:
            assert len(idx) == 0 and self.count > 0
        elif self.box is SLAB24:
            assert 0 < len(idx) < self.count
        else:
            assert len(idx) == self.count
        if self.count >= 777:
            assert len(np.unique(self.pos)) < self.count or self.kind.startswith("wrap")   # duplicates
        for d in range(3):
            if self.periodic[d] and len(idx):      # one wrap suffices: no displacement of a box length
                assert ((st[:, 5 + d] >= 0.0) & (st[:, 5 + d] <= self.length[d])).all(), (self.name, d)
        if not self.kind.startswith("wrap") and len(idx):
            # no x within the band of a face of the sub-box: there a last bit could decide a wrap (periodic axes) or the side
            for d in range(3):
                x = st[:, 5 + d]
                assert (np.abs(x) > self.band()).all() and (np.abs(x - self.length[d]) > self.band()).all(), (self.name, d)
        if self.kind == "branches":
            v = -np.log10(o["F"].astype(np.float64))
            x = pc.cosmology_tables(self.nk)["x"]
            assert (v < x[0]).any() and (v > x[-1]).any() and (v == x[34]).any() and x[34] == 0.0, self.name
        if self.kind == "wrap_zero":
            d = self.periodic.index(True)
            assert o["states"][:, 5:].tobytes() == o["q"].tobytes() and (o["q"][:, d] == self.T(self.length[d] - 0.5)).any() and not o["hi"].any() and not o["lo"].any()
        if self.kind == "wrap_both":
            for d in range(3):
                assert (o["hi"][:, d].any() and o["lo"][:, d].any()) == self.periodic[d], (self.name, d)
        if self.nk > 1:
            cos = pc.cosmology(self.nk)
            kp, ks = npo.k_branch(cos, self.k_point, (1,)), npo.k_branch(cos, self.k_sigma, (1,))
            want = {"below": (False, 0, False, cos.nk - 1), "above": (False, cos.nk - 1, False, 0), "bins": (True, 2, True, 6)}[self.kind]
            assert (bool(kp[3][0]), int(kp[1][0]), bool(ks[3][0]), int(ks[1][0])) == want, (self.name, kp, ks)

    def check(self, index, states, found, capacity=None, printer=None):
        o = self.oracle()
        assert found == len(o["index"]), (self.name, found, len(o["index"]))
        m = found if capacity is None else min(found, capacity)
        index = np.asarray(index)
        assert index.dtype == np.uint32 and np.array_equal(index, o["index"][:m]), self.name
        self.last_ulp64 = check_states(self.T, states, o["states"][:m], self.length, self.periodic, self.band(), self.name, printer)
        return self.last_ulp64


CASES = {
    "c0": lambda: Case("c0", count=0),
    "c1": lambda: Case("c1", count=1, seed=2),
    "c63": lambda: Case("c63", count=63, seed=3),
    "c64": lambda: Case("c64", count=64, seed=4),
    "c65": lambda: Case("c65", count=65, seed=5),
    "c777": lambda: Case("c777", seed=6),
    "slab24": lambda: Case("slab24", box=SLAB24, seed=7),
    "miss24": lambda: Case("miss24", box=MISS24, seed=8),
    "f64": lambda: Case("f64", T=F64, seed=9),
    "f64_slab24_seg1_o3": lambda: Case("f64_slab24_seg1_o3", T=F64, box=SLAB24, myseg=1, order=3, seed=10),
    "seg1": lambda: Case("seg1", myseg=1, seed=11),
    "seg1_o3": lambda: Case("seg1_o3", myseg=1, order=3, seed=12),
    "seg1_o3_v31": lambda: Case("seg1_o3_v31", myseg=1, order=3, use_v31=True, seed=12),
    "o1": lambda: Case("o1", order=1, seed=13),
    "o3": lambda: Case("o3", order=3, seed=14),
    "o3_lpt2": lambda: Case("o3_lpt2", order=3, lpt_order=2, seed=14),
    "o2_lpt1_seg1": lambda: Case("o2_lpt1_seg1", order=2, lpt_order=1, myseg=1, seed=15),
    "branches": lambda: Case("branches", kind="branches", seed=16),
    "branches_f64_seg1": lambda: Case("branches_f64_seg1", T=F64, myseg=1, kind="branches", seed=17),
    "nk10_below": lambda: Case("nk10_below", nk=10, k_point=5e-4, k_sigma=50.0, kind="below", seed=18),
    "nk10_above": lambda: Case("nk10_above", nk=10, k_point=50.0, k_sigma=5e-4, kind="above", order=3, seed=19),
    "nk10_bins": lambda: Case("nk10_bins", nk=10, k_point=0.02, k_sigma=1.2, kind="bins", seed=20),
    "nk10_bins_f64_seg1_o3": lambda: Case("nk10_bins_f64_seg1_o3", T=F64, nk=10, k_point=0.02, k_sigma=1.2, kind="bins", myseg=1, order=3, seed=21),
    "wrap_zero": lambda: Case("wrap_zero", kind="wrap_zero", seed=22),
    "wrap_zero_f64_seg1": lambda: Case("wrap_zero_f64_seg1", T=F64, myseg=1, kind="wrap_zero", seed=23),
    "wrap_both": lambda: Case("wrap_both", kind="wrap_both", seed=24),
    "wrap_both_seg1_f64": lambda: Case("wrap_both_seg1_f64", T=F64, myseg=1, kind="wrap_both", seed=25),
}
# the cases the device runs (the tap's columns count as LPT order 3)
TAP_CASES = [k for k in CASES if "_lpt" not in k]


@functools.lru_cache(None)
def case(name):
    """the case and its oracle, made once per process and left unchanged"""
    return CASES[name]()
