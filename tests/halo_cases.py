"""Planted halo lists for the halo-power call (include/pinfmax.h: pf_halo_power) -- TEST INFRASTRUCTURE shared by the CPU and the
device tests.  cases(n) yields dicts: name, pos [count][3] float64, mass [count] int32, scale, mass_weight, ranges [(lo, hi), ...]
and `what`, which says per range what the case was planted for:
  ("cell", (x, y, z), value)   the CIC grid holds exactly `value` in that cell and nothing elsewhere
  ("counts", selected, nonfinite, outside)
  ("empty",)                   nothing is selected
  ("refused",)                 the weights add up to 2^34 or more
  None                         nothing beyond the restatement"""
import numpy as np

BIG = 1 << 30


def _case(name, pos, mass, ranges, what, scale=1.0, mass_weight=False):
    pos = np.ascontiguousarray(np.asarray(pos, dtype=np.float64).reshape(-1, 3))
    mass = np.ascontiguousarray(mass, dtype=np.int32)
    assert len(mass) == len(pos) and len(what) == len(ranges)
    return {"name": name, "pos": pos, "mass": mass, "scale": scale, "mass_weight": mass_weight, "ranges": list(ranges), "what": list(what)}


def random_list(seed, count, n, mmax=5000):
    """count haloes: half uniform in the box, half clustered around a few centres; masses from 10 up, log-uniform"""
    rng = np.random.default_rng(seed)
    uni = rng.uniform(0.0, n, size=(count // 2, 3))
    centres = rng.uniform(0.0, n, size=(7, 3))
    clu = centres[rng.integers(0, 7, size=count - count // 2)] + rng.normal(0.0, 0.9, size=(count - count // 2, 3))
    pos = np.mod(np.concatenate([uni, clu]), n)
    mass = np.floor(10.0 * np.exp(rng.uniform(0.0, np.log(mmax / 10.0), size=count))).astype(np.int32)
    return np.ascontiguousarray(pos[rng.permutation(count)]), mass


def cases(n):
    one = (1, 2 ** 31 - 1)
    out = []
    # t = 0 on every axis: the whole weight in one cell
    out.append(_case("cell_centre", [[3.5, 7.5, 0.5]], [5], [one], [("cell", (3, 7, 0), 1 << 30)]))
    out.append(_case("cell_centre_weighted", [[3.5, 7.5, 0.5]], [5], [one], [("cell", (3, 7, 0), 5 << 30)], mass_weight=True))
    # the upper edge: n - 1e-13 stays below n; -1e-20 wraps to exactly n (the sum rounds), which is inside [0, n]
    out.append(_case("upper_edge", [[n - 1e-13, 1.25, 2.75], [-1e-20, -1e-20, -1e-20], [4.0, -1e-20, n - 1e-13]], [3, 4, 5], [one], [("counts", 3, 0, 0)]))
    # pos * scale == n exactly: wraps to 0
    out.append(_case("product_is_n", [[2.0, 1.0, 0.5], [2.0, 2.0, 2.0]], [7, 8], [one], [("counts", 2, 0, 0)], scale=n / 2.0))
    # a scale that is no power of two: the product rounds
    out.append(_case("scaled", random_list(3, 40, n)[0] * (1.0 / 0.37), random_list(3, 40, n)[1], [one], [("counts", 40, 0, 0)], scale=0.37))
    # what is not a position
    bad = [[np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [1.0, 1.0, -np.inf], [1e30, 1.0, 1.0], [1.0, -1e30, 1.0], [2.0 * n + 0.5, 1.0, 1.0], [1.0, 1.0, -n - 0.5],
           [np.nan, 1e30, 1.0], [1.5, 2.5, 3.5]]
    out.append(_case("not_positions", bad, [10] * 9, [one, (11, 12)], [("counts", 1, 4, 4), ("empty",)]))
    # both ends of a range are inside it; ranges may overlap; a range may be empty
    pos, _ = random_list(5, 8, n)
    out.append(_case("range_ends", pos, [9, 10, 10, 15, 20, 20, 21, 1000], [(10, 20), (1, 10), (20, 21), (15, 2 ** 31 - 1), (22, 999), (10, 10)],
                     [("counts", 5, 0, 0), ("counts", 3, 0, 0), ("counts", 3, 0, 0), ("counts", 5, 0, 0), ("empty",), ("counts", 2, 0, 0)]))
    out.append(_case("range_ends_weighted", pos, [9, 10, 10, 15, 20, 20, 21, 1000], [(10, 20), (22, 999), (21, 1000)],
                     [("counts", 5, 0, 0), ("empty",), ("counts", 2, 0, 0)], mass_weight=True))
    # every halo in one cell: 300 of them spread inside the cell (3, 4, 5) (CIC spills over its neighbours, NGP does not)
    rng = np.random.default_rng(9)
    out.append(_case("one_cell", np.array([3.0, 4.0, 5.0]) + rng.uniform(0.0, 1.0, size=(300, 3)), rng.integers(1, 50, size=300), [one, (1, 25)], [None, None]))
    out.append(_case("one_cell_centre", np.tile([3.5, 4.5, 5.5], (300, 1)), rng.integers(1, 50, size=300), [one], [("cell", (3, 4, 5), 300 << 30)]))
    # the headroom: 15 haloes of mass 2^30 on one cell centre fill the cell to 15 2^60; 16 are refused
    out.append(_case("headroom_15", np.tile([n - 0.5, 0.5, n - 0.5], (15, 1)), [BIG] * 15, [(BIG, BIG)], [("cell", (n - 1, 0, n - 1), 15 << 60)], mass_weight=True))
    out.append(_case("headroom_16", np.tile([n - 0.5, 0.5, n - 0.5], (16, 1)), [BIG] * 16, [(BIG, BIG)], [("refused",)], mass_weight=True))
    # ... unweighted the same sixteen are sixteen unit weights
    out.append(_case("headroom_16_unweighted", np.tile([n - 0.5, 0.5, n - 0.5], (16, 1)), [BIG] * 16, [(BIG, BIG)], [("cell", (n - 1, 0, n - 1), 16 << 30)]))
    # the largest mass an int holds: W^2 needs both halves
    out.append(_case("largest_int", [[1.5, 1.5, 1.5], [2.25, 3.0, 4.75], [9.0, 9.0, 9.0]], [2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1], [one], [("counts", 3, 0, 0)], mass_weight=True))
    # a list that spans more than one workgroup of 256 and is no multiple of a wavefront
    pos, mass = random_list(11, 777, n)
    out.append(_case("random_777", pos, mass, [one, (100, 2 ** 31 - 1), (1000, 2 ** 31 - 1)], [None, None, None]))
    out.append(_case("random_777_weighted", pos, mass, [one, (100, 2 ** 31 - 1), (1000, 2 ** 31 - 1)], [None, None, None], mass_weight=True))
    out.append(_case("no_haloes", np.zeros((0, 3)), np.zeros(0, np.int32), [one], [("empty",)]))
    return out
