"""count_peaks (src/fragment.c:605-706, the default non-CLASSIC_FRAGMENTATION form) restated in numpy from the reference's loop.

The reference works on a sub-box of Lgwbl[3] cells cut out of the periodic box: it keeps a list of the *stored* cells (Fmax >=
outputs.Flast, update_distmap, src/distribute.c:695), walks that list, skips the border layers of the directions in which the
sub-box is not periodic (:630-635), and compares the cell with the six neighbours it finds in the list (find_location gives -1
for a neighbour that is not stored, which then says nothing, :678-682).  The comparison is a strict `>`.  A peak is "well
resolved" when it lies outside the safety layers (:691-694).

Shares nothing with the device kernel: the sub-box is cut out first (np.take with wrapping indices), then the loop runs on the
sub-box's own coordinates with np.roll for a periodic direction and a shifted slice for the others.
"""
import numpy as np


def cut(field, start, length):
    """the sub-box [len_x][len_y][len_z] that starts at `start` (global coordinates, wrapping around the box)"""
    n = field.shape[0]
    sub = field
    for axis in range(3):
        sub = np.take(sub, (int(start[axis]) + np.arange(int(length[axis]))) % n, axis=axis)
    return sub


def peak_mask_of_subbox(sub, flast, pbc):
    """boolean [len_x][len_y][len_z]: the peaks of the sub-box; pbc[d]: the sub-box spans the box in direction d"""
    f = np.asarray(sub)
    with np.errstate(invalid="ignore"):
        stored = f.astype(np.float64) >= float(flast)          # NaN is never stored
    peak = stored.copy()
    for axis in range(3):
        L = f.shape[axis]
        for step in (-1, +1):
            if pbc[axis]:
                fn = np.roll(f, -step, axis=axis)               # fn[i] = f[i + step], wrapping (:644, :649 ...)
                sn = np.roll(stored, -step, axis=axis)
            else:
                # no wrap: the neighbour of a border cell does not exist -- the border cells are dropped below anyway
                fn = np.full(f.shape, np.nan, dtype=f.dtype)
                sn = np.zeros(f.shape, dtype=bool)
                src = [slice(None)] * 3
                dst = [slice(None)] * 3
                if step > 0:
                    src[axis], dst[axis] = slice(1, L), slice(0, L - 1)
                else:
                    src[axis], dst[axis] = slice(0, L - 1), slice(1, L)
                fn[tuple(dst)] = f[tuple(src)]
                sn[tuple(dst)] = stored[tuple(src)]
            with np.errstate(invalid="ignore"):
                peak &= ~sn | (f > fn)                          # peak_cond &= (F > Fn) only for a neighbour in the list
        if not pbc[axis]:                                       # "avoid borders"
            border = [slice(None)] * 3
            for edge in (0, L - 1):
                border[axis] = edge
                peak[tuple(border)] = False
    return peak


def count_peaks(field, flast, region=None):
    """(npeaks, ngood) of `field` [n][n][n] (index order x, y, z); region = (start[3], len[3], safe[3]) or None = the whole box"""
    field = np.asarray(field)
    n = field.shape[0]
    assert field.shape == (n, n, n)
    start, length, safe = ((0, 0, 0), (n, n, n), (0, 0, 0)) if region is None else region
    pbc = [int(length[d]) == n for d in range(3)]
    peak = peak_mask_of_subbox(cut(field, start, length), flast, pbc)
    good = peak
    for axis in range(3):
        s, L = int(safe[axis]), int(length[axis])
        keep = np.zeros(L, dtype=bool)
        keep[s:L - s] = True
        shape = [1, 1, 1]
        shape[axis] = L
        good = good & keep.reshape(shape)
    return int(peak.sum()), int(good.sum())


def peak_mask(field, flast):
    """the peaks of the whole periodic box, boolean [n][n][n]"""
    return peak_mask_of_subbox(np.asarray(field), flast, [True, True, True])


def sorted_peaks(field, flast):
    """(flat index, Fmax) of the peaks of the whole box by descending Fmax, ties by ascending index (index_compare_F)"""
    field = np.asarray(field)
    idx = np.flatnonzero(peak_mask(field, flast).ravel())
    f = field.ravel()[idx]
    order = np.lexsort((idx, -f.astype(np.float64)))
    return idx[order], f[order]
