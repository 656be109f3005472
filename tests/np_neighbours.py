"""The neighbour lookups of the fragmentation loops restated in numpy, from the reference's loop (src/build_groups.c:245-343; the same
block stands in quick_build_groups, :1916-2004, and in count_peaks, src/fragment.c:605-706).

Over the N stored particles of a sub-box in the order after sort_and_organize(), for particle iz:
  * (i, j, k) = INDEX_TO_COORD(frag_pos[iz], Lgwbl) (src/pinocchio.h:84);
  * skip: in a direction that is not periodic the coordinate is 0 or L - 1 (:251-254);
  * good_particle: safe <= coordinate < L - safe in all three directions (:262-264);
  * for nn = 0..5 (x-, x+, y-, y+, z-, z+) the neighbour's coordinates, wrapped once where the direction is periodic (:274-306), and
    pos = find_location(i1, j1, k1); a neighbour that is found gives indices[pos] and peak_cond &= (Fmax[iz] > Fmax[indices[pos]])
    (:318-323); a skipped particle looks nothing up (:266);
  * Npeaks counts peak_cond among the particles that are not skipped, Ngood those that are good particles too.

Built on np_organize.find_location; shares no code with the device path."""
import numpy as np

import np_organize as npo

SKIP, GOOD, PEAK = 1, 2, 4


def coords(frag_pos, length):
    """INDEX_TO_COORD -> (i, j, k) as int64 arrays"""
    lx, ly, lz = (int(v) for v in length)
    pos = np.asarray(frag_pos).astype(np.int64)
    return pos // (lz * ly), (pos // lz) % ly, pos % lz


def skip_good(frag_pos, length, safe, pbc):
    c = coords(frag_pos, length)
    skip = np.zeros(len(c[0]), dtype=bool)
    good = np.ones(len(c[0]), dtype=bool)
    for d in range(3):
        L, s = int(length[d]), int(safe[d])
        if not pbc[d]:
            skip |= (c[d] == 0) | (c[d] == L - 1)
        good &= (c[d] >= s) & (c[d] < L - s)
    return skip, good


def neighbour_positions(frag_pos, length, pbc):
    """-> (npos[N, 6], wrapped[N, 6]): COORD_TO_INDEX of the six neighbours by the reference's switch (no neighbour leaves the box for
    a particle that is not skipped; the rows of skipped particles are meaningless) and whether the periodic wrap was taken"""
    lx, ly, lz = (int(v) for v in length)
    c = coords(frag_pos, length)
    npos = np.zeros((len(c[0]), 6), dtype=np.int64)
    wrapped = np.zeros((len(c[0]), 6), dtype=bool)
    for nn in range(6):
        d, up = nn // 2, nn % 2
        L = int(length[d])
        c1 = [c[0], c[1], c[2]]
        if up:
            w = (c[d] == L - 1) if pbc[d] else np.zeros(len(c[d]), dtype=bool)
            c1[d] = np.where(w, 0, c[d] + 1)
        else:
            w = (c[d] == 0) if pbc[d] else np.zeros(len(c[d]), dtype=bool)
            c1[d] = np.where(w, L - 1, c[d] - 1)
        npos[:, nn] = c1[2] + lz * (c1[1] + ly * c1[0])
        wrapped[:, nn] = w
    return npos, wrapped


def neighbours(frag_pos, fmax, length, safe, pbc):
    """-> (neigh[N, 6] int32, flags[N] uint8, (Npeaks, Ngood)) of particles already in the order of sort_and_organize"""
    pos = np.asarray(frag_pos)
    f = np.asarray(fmax)
    count = len(pos)
    spos, ind = npo.index(pos)
    skip, good = skip_good(pos, length, safe, pbc)
    npos, _ = neighbour_positions(pos, length, pbc)
    neigh = np.full((count, 6), -1, dtype=np.int64)
    peak = ~skip
    for nn in range(6):
        loc = npo.find_location(spos, ind, npos[:, nn])
        loc = np.where(skip, -1, loc)
        there = loc >= 0
        with np.errstate(invalid="ignore"):
            peak &= ~there | (f > f[np.where(there, loc, 0)])
        neigh[:, nn] = loc
    flags = (skip * SKIP + good * GOOD + peak * PEAK).astype(np.uint8)
    return neigh.astype(np.int32), flags, (int(peak.sum()), int((peak & good).sum()))
