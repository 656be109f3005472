"""distribute_back() restated in numpy, from the reference's loops (src/distribute.c:703-946).

keep_data_back (:799-837) and the loop of send_data_back (:859-896) walk the Nstored particles of a sub-box (subbox.stabl, subbox.Lgwbl,
subbox.safe); for particle iz:
  * (i, j, k) = INDEX_TO_COORD(frag_pos[iz], Lgwbl) (src/pinocchio.h:84); with CLASSIC_FRAGMENTATION the position is iz itself;
  * good_particle: safe <= coordinate < L - safe in all three directions (:815-817);
  * the global cell (coordinate + stabl + n) % n per direction (:820-822);
  * when it is good and its global cell lies in the receiving fft box -- here an x-slab, planes x0 .. x0 + nxl - 1, whole in y and z --
    products[fftpos].zacc / .group_ID = frag[iz].zacc / .group_ID with fftpos = z + n (y + n (x - x0)) (:830-832); send_data_back
    puts (fftpos, zacc, group_ID) into back_buffer instead (:882-884) and recv_data_back stores them (:935-939).
products[].zacc starts at -1, .group_ID at 0 (src/allocations.c:519-524).

Vectorised; shares no code with the device path."""
import numpy as np


def fresh(n, nxl, dtype=np.float32):
    """the two columns before anything is written"""
    nc = int(nxl) * int(n) * int(n)
    return np.full(nc, -1.0, dtype=dtype), np.zeros(nc, dtype=np.int32)


def coords(frag_pos, length):
    """INDEX_TO_COORD -> (i, j, k) as int64 arrays"""
    lx, ly, lz = (int(v) for v in length)
    pos = np.asarray(frag_pos).astype(np.int64)
    return pos // (lz * ly), (pos // lz) % ly, pos % lz


def selection(n, x0, nxl, start, length, safe, frag_pos):
    """-> (taken[N] bool, fftpos[N] int64; meaningful where taken)"""
    c = coords(frag_pos, length)
    good = np.ones(len(c[0]), dtype=bool)
    g = []
    for d in range(3):
        L, s = int(length[d]), int(safe[d])
        good &= (c[d] >= s) & (c[d] < L - s)
        g.append(np.mod(c[d] + int(start[d]), int(n)))      # = (c + stabl + n) % n for the reference's stabl in (-n, n)
    taken = good & (g[0] >= x0) & (g[0] < x0 + nxl)
    return taken, g[2] + n * (g[1] + n * (g[0] - x0))


def send_data_back(n, x0, nxl, start, length, safe, frag_pos, zacc, group_id):
    """the back_data entries a sender makes for the fft box (x0, nxl): (pos uint32, zacc, group_ID), in the order of the particles"""
    if frag_pos is None:
        frag_pos = np.arange(len(zacc))
    taken, fftpos = selection(n, x0, nxl, start, length, safe, frag_pos)
    return fftpos[taken].astype(np.uint32), np.asarray(zacc)[taken], np.asarray(group_id)[taken].astype(np.int32)


def distribute_back(n, x0, nxl, start, length, safe, frag_pos, zacc, group_id, zcol=None, gcol=None):
    """-> (zacc column, group_ID column, stored) of the slab after the call; zcol / gcol: the columns before it (None: -1 / 0), which
    are not modified.  Positions must be unique (which duplicate the reference keeps is the order of its loop)."""
    zacc = np.asarray(zacc)
    f = fresh(n, nxl, zacc.dtype)
    zcol = f[0] if zcol is None else np.array(zcol, copy=True)
    gcol = f[1] if gcol is None else np.array(gcol, copy=True)
    pos, z, g = send_data_back(n, x0, nxl, start, length, safe, frag_pos, zacc, group_id)
    zcol[pos] = z
    gcol[pos] = g
    return zcol, gcol, len(pos)
