"""The maps of fragment() restated in numpy from the reference's loops: create_map() (src/fragment.c:708-751), update_map()
(src/build_groups.c:2246-2318) and count_peaks() (src/fragment.c:605-706) over the stored set a map selects.

A map is a boolean array [Lx][Ly][Lz] over subbox.Lgwbl here; words_of() packs it the way the reference stores it (bit
pos = z + Lz (y + Ly x), COORD_TO_INDEX, in word pos // 32, bit pos % 32, UINTLEN = 32).  Shares nothing with the device kernels
or with pinocchio_amd/csrc/pf_map_core.h: the fill is three slices, a sphere is one np.ogrid expression per group, and the
triple loop of the reference is kept beside it as update_map_loops() (tests/test_maps_cpu.py holds the two against each other).
create_map_words / create_map_count / update_map_sparse are the same answers for sub-boxes of up to 2^32 cells, where no cube fits:
words on request, the closed-form bit count, and the requested positions as a sorted int64 list (tests/test_large_index_cpu.py holds
them against the dense forms).
"""
import math

import numpy as np

import np_peaks


def words_of(bits):
    """bool [Lx][Ly][Lz] -> uint32 words, ceil(cells / 32) of them; the unused bits of the last word are zero"""
    flat = np.asarray(bits, dtype=bool).ravel()
    nw = (flat.size + 31) // 32
    padded = np.zeros(nw * 32, dtype=np.uint8)
    padded[:flat.size] = flat
    return np.packbits(padded.reshape(nw, 32), axis=1, bitorder="little").view("<u4").ravel().copy()


def bits_of(words, length):
    """the inverse of words_of"""
    cells = int(length[0]) * int(length[1]) * int(length[2])
    w = np.ascontiguousarray(words, dtype="<u4")
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:cells].astype(bool).reshape(tuple(int(v) for v in length))


def create_map(length, safe, pbc):
    """frag_map_update after create_map(): per direction [safe - 1, Lgrid + safe + 1) with Lgrid = len - 2 safe, [0, Lgrid) when periodic"""
    out = np.zeros(tuple(int(v) for v in length), dtype=bool)
    sl = []
    for d in range(3):
        lgrid = int(length[d]) - 2 * int(safe[d])
        sl.append(slice(0, lgrid) if pbc[d] else slice(int(safe[d]) - 1, lgrid + int(safe[d]) + 1))
    out[tuple(sl)] = True
    return out


def centre_and_size(pos, mass, blf):
    """(int)(Pos + 0.5) and (int)(BoundaryLayerFactor * pow(Mass / 4.188790205, 0.333333333333333) + 0.5): C's cast truncates"""
    c = [int(float(p) + 0.5) for p in pos]
    size = int(float(blf) * math.pow(float(int(mass)) / 4.188790205, 0.333333333333333) + 0.5)
    return c, size


def update_map(current, pos, mass, blf, pbc):
    """(frag_map_update, (nadd0, nadd1)) of update_map() on the map `current` (bool [Lx][Ly][Lz]) for the groups pos[g][3], mass[g].
    One np.ogrid expression per group; nadd0 counts with multiplicity (the test reads frag_map, not frag_map_update)"""
    current = np.asarray(current, dtype=bool)
    L = current.shape
    upd = np.zeros(L, dtype=bool)
    nadd0 = nadd1 = 0
    for g in range(len(mass)):
        c, size = centre_and_size(pos[g], mass[g], blf)
        if size <= 0:
            continue
        off = np.arange(-size, size)
        idx, ok = [], []
        for d in range(3):
            c1 = c[d] + off
            inside = (c1 >= 0) & (c1 < L[d])
            if pbc[d]:
                w = np.where(c1 < 0, c1 + L[d], np.where(c1 >= L[d], c1 - L[d], c1))   # ONE wrap
                assert np.all((w >= 0) & (w < L[d])), "the reference would index out of bounds"
                idx.append(w)
                ok.append(np.ones(len(off), dtype=bool))
            else:
                idx.append(np.where(inside, c1, 0))
                ok.append(inside)
        oi, oj, ok3 = np.ogrid[:2 * size, :2 * size, :2 * size]
        valid = ok[0][oi] & ok[1][oj] & ok[2][ok3]
        nadd1 += int(valid.size - valid.sum())
        sphere = (off[oi] ** 2 + off[oj] ** 2 + off[ok3] ** 2) <= size * size
        cur = current[idx[0][oi], idx[1][oj], idx[2][ok3]]
        take = valid & sphere & ~cur
        nadd0 += int(take.sum())
        ii, jj, kk = np.broadcast_arrays(idx[0][oi], idx[1][oj], idx[2][ok3])
        upd[ii[take], jj[take], kk[take]] = True
    return upd, (nadd0, nadd1)


def update_map_loops(current, pos, mass, blf, pbc):
    """the reference's triple loop, line by line (slow: tiny boxes only)"""
    current = np.asarray(current, dtype=bool)
    L = current.shape
    upd = np.zeros(L, dtype=bool)
    nadd = [0, 0]

    def coord(c1, d):
        if c1 < 0 or c1 >= L[d]:
            if pbc[d]:
                return c1 + L[d] if c1 < 0 else c1 - L[d]
            return -1
        return c1

    for g in range(len(mass)):
        (ig, jg, kg), size = centre_and_size(pos[g], mass[g], blf)
        size2 = size * size
        for i1 in range(ig - size, ig + size):
            i = coord(i1, 0)
            for j1 in range(jg - size, jg + size):
                j = coord(j1, 1)
                for k1 in range(kg - size, kg + size):
                    k = coord(k1, 2)
                    if i < 0 or j < 0 or k < 0:
                        nadd[1] += 1
                        continue
                    if not current[i, j, k]:
                        rr = (i1 - ig) ** 2 + (j1 - jg) ** 2 + (k1 - kg) ** 2
                        if rr <= size2:
                            upd[i, j, k] = True
                            nadd[0] += 1
    return upd, (nadd[0], nadd[1])


# ------------------------------------------------------------------------------------------------------------------------
# sparse forms for sub-boxes of up to 2^32 cells: nothing here allocates per cell (or per word) of the sub-box
def box_ranges(length, safe, pbc):
    """create_map's range [lo, hi) per direction"""
    lo = [0 if pbc[d] else int(safe[d]) - 1 for d in range(3)]
    hi = [int(length[d]) if pbc[d] else int(length[d]) - int(safe[d]) + 1 for d in range(3)]
    return lo, hi


def in_ranges(pos, length, lo, hi):
    """whether the bits at the positions pos (int64, any shape) lie in the box [lo, hi) of a map over `length`"""
    pos = np.asarray(pos, dtype=np.int64)
    ly, lz = int(length[1]), int(length[2])
    c = (pos // (lz * ly), (pos // lz) % ly, pos % lz)
    out = np.ones(pos.shape, dtype=bool)
    for d in range(3):
        out &= (c[d] >= lo[d]) & (c[d] < hi[d])
    return out


def create_map_words(length, safe, pbc, word_index):
    """the words word_index (any order, int64) of words_of(create_map(length, safe, pbc)), from the per-direction ranges: bit b of word
    w is position 32 w + b; positions beyond the last cell are zero"""
    w = np.asarray(word_index, dtype=np.int64)
    cells = int(length[0]) * int(length[1]) * int(length[2])
    lo, hi = box_ranges(length, safe, pbc)
    out = np.zeros(len(w), dtype=np.uint32)
    for a in range(0, len(w), 1 << 18):                     # in pieces: 32 positions per word
        pos = 32 * w[a:a + (1 << 18), None] + np.arange(32, dtype=np.int64)[None, :]
        bit = in_ranges(np.minimum(pos, cells - 1), length, lo, hi) & (pos < cells)
        out[a:a + (1 << 18)] = (bit.astype(np.uint32) << np.arange(32, dtype=np.uint32)[None, :]).sum(axis=1, dtype=np.uint32)
    return out


def create_map_count(length, safe, pbc):
    """the bits create_map sets: the product of its three ranges"""
    lo, hi = box_ranges(length, safe, pbc)
    return (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2])


def update_map_sparse(current, length, pos, mass, blf, pbc):
    """update_map() without the cube: current is None (an empty frag_map) or a function of an int64 position array that gives its
    bits.  -> (the ascending int64 positions the groups request, (nadd0, nadd1), {word: mask} of the words of frag_map_update that
    are not zero).  One np.ogrid expression per group, as update_map"""
    L = [int(v) for v in length]
    requested = []
    nadd0 = nadd1 = 0
    for g in range(len(mass)):
        c, size = centre_and_size(pos[g], mass[g], blf)
        if size <= 0:
            continue
        off = np.arange(-size, size, dtype=np.int64)
        idx, ok = [], []
        for d in range(3):
            c1 = c[d] + off
            inside = (c1 >= 0) & (c1 < L[d])
            if pbc[d]:
                w = np.where(c1 < 0, c1 + L[d], np.where(c1 >= L[d], c1 - L[d], c1))   # ONE wrap
                assert np.all((w >= 0) & (w < L[d])), "the reference would index out of bounds"
                idx.append(w)
                ok.append(np.ones(len(off), dtype=bool))
            else:
                idx.append(np.where(inside, c1, 0))
                ok.append(inside)
        oi, oj, ok3 = np.ogrid[:2 * size, :2 * size, :2 * size]
        valid = ok[0][oi] & ok[1][oj] & ok[2][ok3]
        nadd1 += int(valid.size - valid.sum())
        sphere = (off[oi] ** 2 + off[oj] ** 2 + off[ok3] ** 2) <= size * size
        p = idx[2][ok3] + L[2] * (idx[1][oj] + L[1] * idx[0][oi])
        cand = p[valid & sphere]
        if current is not None:
            cand = cand[~np.asarray(current(cand), dtype=bool)]
        nadd0 += len(cand)
        requested.append(cand)
    allpos = np.unique(np.concatenate(requested)) if requested else np.zeros(0, dtype=np.int64)
    words = {}
    if len(allpos):
        wi, first = np.unique(allpos >> 5, return_index=True)
        masks = np.bitwise_or.reduceat(np.uint64(1) << (allpos & 31).astype(np.uint64), first)
        words = {int(a): int(b) for a, b in zip(wi, masks)}
    return allpos, (nadd0, nadd1), words


def stored_mask(field, flast, box, mapbits):
    """bool [Lx][Ly][Lz]: what a distribute with this map stores of the box = (start, len, safe): bit set and Fmax >= flast"""
    sub = np_peaks.cut(np.asarray(field), box[0], box[1])
    with np.errstate(invalid="ignore"):
        return np.asarray(mapbits, dtype=bool) & (sub.astype(np.float64) >= float(flast))


def count_peaks_stored(field, flast, box, mapbits):
    """(Npeaks, ngood) of count_peaks() when the stored list is the map's: np_peaks.peak_mask_of_subbox on the sub-box with every
    cell that is not stored made NaN (never stored, vetoes nothing)"""
    field = np.asarray(field)
    n = field.shape[0]
    start, length, safe = box
    pbc = [int(length[d]) == n for d in range(3)]
    sub = np_peaks.cut(field, start, length).copy()
    sub[~stored_mask(field, flast, box, mapbits)] = np.nan
    peak = np_peaks.peak_mask_of_subbox(sub, flast, pbc)
    good = peak
    for axis in range(3):
        s, L = int(safe[axis]), int(length[axis])
        keep = np.zeros(L, dtype=bool)
        keep[s:L - s] = True
        shape = [1, 1, 1]
        shape[axis] = L
        good = good & keep.reshape(shape)
    return int(peak.sum()), int(good.sum())
