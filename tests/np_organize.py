"""sort_and_organize() restated in numpy, from what it leaves behind rather than from how it gets there.

After the reference's call (src/fragment.c:484-520) over N stored particles of a sub-box:
  * frag[] / frag_pos[] hold the same (record, position) pairs as before, reordered so that frag[i].Fmax is non-increasing;
  * indices[p] is the index, in the new order, of the particle with the p-th smallest frag_pos;
  * sorted_pos[p] == frag_pos[indices[p]], strictly ascending (positions are unique within a sub-box);
  * find_location(pos) (:592-603) binary-searches sorted_pos and returns indices[p] where sorted_pos[p] == pos, -1 otherwise.
qsort leaves the order of equal Fmax open.  The project's rule: ties keep the order of the input (a stable sort), "equal" means equal
as floating-point values (-0.0 ties with +0.0), and NaN goes last, after -inf, in input order."""
import numpy as np


def order(fmax):
    """new -> old: the input index of every record of the sorted order"""
    f = np.asarray(fmax)
    # x + 0 turns -0.0 into +0.0 and leaves every other value alone; numpy sorts NaN (-NaN is NaN) behind +inf = -(-inf)
    with np.errstate(invalid="ignore"):          # (signalling NaN)
        return np.argsort(-(f + f.dtype.type(0)), kind="stable").astype(np.uint32)


def index(frag_pos_sorted):
    """(sorted_pos, indices) of positions that are already in the new order"""
    p = np.asarray(frag_pos_sorted)
    ind = np.argsort(p, kind="stable")
    return p[ind].astype(np.uint32), ind.astype(np.int32)


def organize(fmax, frag_pos):
    """-> (order, sorted_pos, indices)"""
    o = order(fmax)
    spos, ind = index(np.asarray(frag_pos)[o])
    return o, spos, ind


def find_location(sorted_pos, indices, pos):
    """find_location for an array of positions: the index in the new order of the particle at `pos`, -1 where none is stored"""
    pos = np.asarray(pos)
    if len(sorted_pos) == 0:
        return np.full(pos.shape, -1, dtype=np.int64)
    p = np.searchsorted(sorted_pos, pos)
    p = np.minimum(p, len(sorted_pos) - 1)
    return np.where(np.asarray(sorted_pos)[p] == pos, np.asarray(indices, dtype=np.int64)[p], -1)


def count_peaks(fmax_sorted, frag_pos_sorted, sorted_pos, indices, length):
    """the strict six-neighbour peaks among the stored cells of a sub-box that is the whole periodic box (length[3] = n, n, n), found
    the way the reference's count_peaks consumes the arrays: every neighbour is looked up with find_location"""
    lx, ly, lz = (int(v) for v in length)
    pos = np.asarray(frag_pos_sorted).astype(np.int64)
    f = np.asarray(fmax_sorted)
    k = pos % lz
    j = (pos // lz) % ly
    i = pos // (lz * ly)
    peak = np.ones(len(pos), dtype=bool)
    for di, dj, dk in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        npos = ((k + dk) % lz) + lz * (((j + dj) % ly) + ly * ((i + di) % lx))
        loc = find_location(sorted_pos, indices, npos)
        there = loc >= 0
        peak &= ~(there & ~(f > f[np.where(there, loc, 0)]))
    return int(peak.sum())
