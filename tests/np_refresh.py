"""The velocity refresh of a redshift segment restated in numpy, from the reference's loops.

For every segment after the first, fragment() (src/fragment.c:398-430) copies Vel* to Vel*_prev in products[]
(shift_all_displacements, :832-850), recomputes Vel* and runs distribute() again, which carries both sets from the cell of each stored
particle to its frag[] record.  Which cell that is, is the arithmetic of keep_data_back (src/distribute.c:806-830) for particle iz of
the sub-box (subbox.stabl, subbox.Lgwbl):
  * (i, j, k) = INDEX_TO_COORD(frag_pos[iz], Lgwbl) (:811; src/pinocchio.h:84);
  * the global cell (coordinate + stabl + n) % n per direction (:820-822);
  * it belongs to the fft box -- here an x-slab, planes x0 .. x0 + nxl - 1, whole in y and z -- when x lies in it (:825-827), at
    fftpos = z + n (y + n (x - x0)) (:830).
The good_particle test of :815-817 is NOT part of it: distribute() stores every particle of the map, the boundary layer included, and
each has velocities; only zacc and group_ID go back for the good ones alone.

Vectorised; shares no code with the device path."""
import numpy as np


def coords(frag_pos, length):
    """INDEX_TO_COORD -> (i, j, k) as int64 arrays"""
    lx, ly, lz = (int(v) for v in length)
    pos = np.asarray(frag_pos).astype(np.int64)
    return pos // (lz * ly), (pos // lz) % ly, pos % lz


def cells(n, x0, nxl, start, length, frag_pos):
    """-> (found[N] bool, fftpos[N] int64; meaningful where found)"""
    c = coords(frag_pos, length)
    g = [np.mod(c[d] + int(start[d]), int(n)) for d in range(3)]      # = (c + stabl + n) % n for the reference's stabl in (-n, n)
    found = (g[0] >= x0) & (g[0] < x0 + nxl)
    return found, g[2] + n * (g[1] + n * (g[0] - x0))


def gather(n, x0, nxl, start, length, frag_pos, cols24):
    """cols24 [24][nxl n n]: the current columns 0..11, then the prev columns 0..11 of the slab -> (index uint32[found], vel24[found][24]):
    the particles whose cell lies in the slab, in ascending particle index, and the 24 values of their cells"""
    cols24 = np.asarray(cols24)
    found, fftpos = cells(n, x0, nxl, start, length, frag_pos)
    index = np.flatnonzero(found)
    return index.astype(np.uint32), np.ascontiguousarray(cols24[:, fftpos[index]].T)


def scatter(frag, index, vel24, off_cur, off_prev=(-1, -1, -1, -1)):
    """frag: uint8 [count][stride], the caller's records.  Record index[j] gets values 3 s .. 3 s + 2 of vel24[j] at byte off_cur[s]
    (s = 0..3: Vel, Vel_2LPT, Vel_3LPT_1, Vel_3LPT_2) and values 12 + 3 s .. at byte off_prev[s], for the offsets that are not negative;
    a copy comes back, frag is not modified"""
    out = np.array(frag, copy=True)
    vel24 = np.ascontiguousarray(vel24)
    pb = vel24.dtype.itemsize
    raw = vel24.view(np.uint8).reshape(len(index), 24 * pb)
    for s, off in enumerate(tuple(off_cur) + tuple(off_prev)):
        if off >= 0 and len(index):
            out[np.asarray(index, dtype=np.int64), off:off + 3 * pb] = raw[:, 3 * s * pb:3 * (s + 1) * pb]
    return out
