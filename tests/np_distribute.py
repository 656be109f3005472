"""distribute() (src/distribute.c:58-175, the default non-CLASSIC_FRAGMENTATION form) restated in numpy from the reference's loops:
create_map (src/fragment.c:708-751), intersection (:178-297), keep_data / send_data / recv_data (:300-600) with build_distmap and
update_distmap (:670-698), and the hypercube order of :109-148.

distribute() moves the product records from the FFT slabs to the fragmentation sub-boxes.  For every (slab, sub-box) pair it
walks the cells of up to eight intersection boxes in index order, keeps a cell when its bit of the sub-box's map is set and
products[].Fmax >= outputs.Flast, and appends the record to frag[] and the cell's sub-box-space index to frag_pos[].  The owner of a
sub-box stores its own slab's cells first (keep_data), then what the other tasks send in the order of the hypercube loop.

Shares nothing with the device code (csrc/pf_distribute.hip), which works on flat indices i of a box table: here the sub-box is cut
out of the periodic box first -- the coordinate axes with wrapping np.take, as np_peaks.cut does with the field -- every cell of
the cut knows its global coordinates and its sub-box index, and an intersection box is a plain slice of the cut.
"""
import itertools

import numpy as np

UINTLEN = 32


def segments(n, f0, flen, s0, slen):
    """one dimension of intersection(): the FFT box [f0, f0 + flen) against the sub-box that starts at s0 (negative: + n, :190)
    -> [wrapped segment or None, segment up to the box edge or None] as (start, stop), the order of ax / ay / az = 0, 1 (:226-262)"""
    if s0 < 0:
        s0 += n
    stop1 = f0 + flen
    stop2 = min(s0 + slen, n)
    first = (max(f0, s0), min(stop1, stop2))
    wrapped = None
    if s0 + slen > n:
        wrapped = (max(f0, 0), min(stop1, (s0 + slen) % n))
    return [seg if seg is not None and seg[0] < seg[1] else None for seg in (wrapped, first)]


def intersection(n, fbox, sbox):
    """intersection(fbox, sbox, ibox): the boxes (start[3], len[3]) in the order the reference stores them"""
    per_dim = [segments(n, fbox[d], fbox[d + 3], sbox[d], sbox[d + 3]) for d in range(3)]
    out = []
    for ax, ay, az in itertools.product((0, 1), repeat=3):
        segs = (per_dim[0][ax], per_dim[1][ay], per_dim[2][az])
        if all(s is not None for s in segs):
            out.append(([s[0] for s in segs], [s[1] - s[0] for s in segs]))
    return out


def create_map(lgwbl, lgrid, safe, pbc):
    """frag_map_update after create_map(): the well resolved region plus one row on each side of a direction that is not periodic,
    as uint32 words -- bit p % 32 of word p // 32 for p = COORD_TO_INDEX(i, j, k, Lgwbl) (set_mapup_bit, :753-759)"""
    cube = np.zeros(tuple(int(v) for v in lgwbl), dtype=bool)
    sl = []
    for d in range(3):
        sl.append(slice(0, int(lgrid[d])) if pbc[d] else slice(int(safe[d]) - 1, int(lgrid[d]) + int(safe[d]) + 1))
    cube[tuple(sl)] = True
    return pack_map(cube)


def pack_map(cube):
    """a boolean sub-box [Lgwbl_x][Lgwbl_y][Lgwbl_z] -> the map words (maplength = ceil(Npart / 32), src/initialization.c:1073)"""
    bits = np.asarray(cube, dtype=bool).ravel()          # C order: z fastest, COORD_TO_INDEX
    words = (bits.size + UINTLEN - 1) // UINTLEN
    padded = np.zeros(words * UINTLEN, dtype=np.uint8)
    padded[:bits.size] = bits
    return np.packbits(padded, bitorder="little").view("<u4").copy()


def map_bits(words, count):
    """get_map_bit for positions 0 .. count - 1 (None: every bit set)"""
    if words is None:
        return np.ones(count, dtype=bool)
    w = np.ascontiguousarray(words, dtype="<u4")
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:count].astype(bool)


def subboxes(n, nbox, safe):
    """set_subboxes (src/initialization.c:1006-1057) for a box that nbox divides: task t -> (stabl[3], Lgwbl[3], Lgrid[3], safe[3],
    pbc[3]); safe is the boundary layer of a direction that is cut (a direction with one sub-box is periodic and has none)"""
    out = []
    nn = nbox[1] * nbox[2]
    for t in range(nbox[0] * nn):
        mybox = (t // nn, (t % nn) // nbox[2], (t % nn) % nbox[2])
        lgrid = [n // nbox[d] for d in range(3)]
        pbc = [nbox[d] == 1 for d in range(3)]
        sf = [0 if pbc[d] else int(safe) for d in range(3)]
        stabl = [mybox[d] * lgrid[d] - sf[d] for d in range(3)]
        lgwbl = [lgrid[d] + 2 * sf[d] for d in range(3)]
        out.append((stabl, lgwbl, lgrid, sf, pbc))
    return out


def contribution(fmax_slab, n, x0, start, length, flast, words=None):
    """what the task that holds planes x0 .. of the box contributes to the sub-box (start, length): keep_data when it owns the
    sub-box, the buffers of send_data otherwise -> (local cell index z + n (y + n x_local), frag_pos), both in the reference's order"""
    slab = np.asarray(fmax_slab)
    nxl = slab.shape[0]
    assert slab.shape == (nxl, n, n)
    length = [int(v) for v in length]
    start = [int(v) for v in start]
    # the cut: global coordinate of every sub-box coordinate, and the sub-box index of every cell of the cut
    axes = [np.take(np.arange(n), (start[d] + np.arange(length[d])) % n) for d in range(3)]
    pos = np.arange(length[0] * length[1] * length[2], dtype=np.int64).reshape(length)
    wanted = map_bits(words, pos.size).reshape(length)
    cells, where = [], []
    for bstart, blen in intersection(n, [x0, 0, 0, nxl, n, n], start + length):
        # the box inside the cut: it lies in one segment of every direction, so it is a slice
        sl = []
        for d in range(3):
            p0 = (bstart[d] - start[d]) % n
            assert np.array_equal(axes[d][p0:p0 + blen[d]], np.arange(bstart[d], bstart[d] + blen[d]))
            sl.append(slice(p0, p0 + blen[d]))
        sl = tuple(sl)
        gx, gy, gz = np.meshgrid(axes[0][sl[0]] - x0, axes[1][sl[1]], axes[2][sl[2]], indexing="ij")
        f = slab[gx, gy, gz].astype(np.float64)
        with np.errstate(invalid="ignore"):
            take = wanted[sl] & (f >= float(flast))          # update_distmap, :695 (NaN is never taken)
        take = take.ravel()                                   # x slowest, z fastest: INDEX_TO_COORD(i, ., ., ., box + 3)
        cells.append(((gx * n + gy) * n + gz).ravel()[take])
        where.append(pos[sl].ravel()[take])
    if not cells:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(cells), np.concatenate(where)


def map_bits_at(words, pos):
    """get_map_bit for the positions pos (int64, any shape) by word lookup: bit pos % 32 of word pos // 32 (None: every bit set)"""
    pos = np.asarray(pos, dtype=np.int64)
    if words is None:
        return np.ones(pos.shape, dtype=bool)
    w = np.asarray(words, dtype=np.uint32)
    return ((w[pos >> 5] >> (pos & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def contribution_sparse(fmax_slab, n, x0, start, length, flast, words=None):
    """contribution() without an array over the cells of the sub-box, for sub-boxes of up to 2^32 cells: every intersection box
    carries its own coordinates -- global g = bstart .. bstart + blen - 1 per direction, sub-box coordinate p = (g - start) mod n,
    position pz + Lz (py + Ly px) in int64 by broadcasting over the box -- and reads its map bits by word lookup.  Memory goes as
    the cells of the slab, never as those of the sub-box.  -> (local cell index, frag_pos), int64, in the reference's order"""
    slab = np.asarray(fmax_slab)
    nxl = slab.shape[0]
    assert slab.shape == (nxl, n, n)
    length = [int(v) for v in length]
    start = [int(v) for v in start]
    cells, where = [], []
    for bstart, blen in intersection(n, [x0, 0, 0, nxl, n, n], start + length):
        g = [np.arange(bstart[d], bstart[d] + blen[d], dtype=np.int64) for d in range(3)]
        p = [np.mod(g[d] - start[d], n) for d in range(3)]
        assert all(p[d].max() < length[d] for d in range(3)), "an intersection box lies inside the sub-box"
        pos = p[2][None, None, :] + length[2] * (p[1][None, :, None] + length[1] * p[0][:, None, None])
        f = slab[bstart[0] - x0:bstart[0] - x0 + blen[0], bstart[1]:bstart[1] + blen[1], bstart[2]:bstart[2] + blen[2]].astype(np.float64)
        with np.errstate(invalid="ignore"):
            take = map_bits_at(words, pos) & (f >= float(flast))
        cell = g[2][None, None, :] + n * (g[1][None, :, None] + n * (g[0][:, None, None] - x0))
        cells.append(np.broadcast_to(cell, take.shape)[take])      # boolean indexing walks in C order: x slowest, z fastest
        where.append(pos[take])
    if not cells:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(cells), np.concatenate(where)


def hypercube_order(ntasks, target):
    """the tasks in the order their cells reach frag[] of `target`: itself (keep_data), then its partner of every round of the
    hypercube loop (:115-148: bit = 1 .. 2^ceil(log2 ntasks) - 1, partner = target ^ bit when that task exists)"""
    log_ntask = 0
    while (1 << log_ntask) < ntasks:
        log_ntask += 1
    order = [target]
    for bit in range(1, 1 << log_ntask):
        partner = target ^ bit
        if partner < ntasks:
            order.append(partner)
    return order


def distribute(fmax, ntasks, start, length, flast, words=None, target=0):
    """frag[] (as global cell index z + n (y + n x)) and frag_pos[] of the sub-box that task `target` owns, of a box [n][n][n] held
    in ntasks x-slabs"""
    fmax = np.asarray(fmax)
    n = fmax.shape[0]
    nxl = n // ntasks
    cells, where = [], []
    for task in hypercube_order(ntasks, target):
        c, w = contribution(fmax[task * nxl:(task + 1) * nxl], n, task * nxl, start, length, flast, words)
        cells.append(c + task * nxl * n * n)
        where.append(w)
    return np.concatenate(cells), np.concatenate(where)


# ------------------------------------------------------------------------------------------------------------------------
# seeded cases shared by the CPU test of the box table (tests/test_distribute_boxes.py) and the GPU test of the kernels
def random_subbox(rng, n, x0, nxl, kind):
    """kind: 0 anything, 1 wraps in every direction, 2 negative start, 3 len == n in one to three directions, 4 misses the slab
    (None when the slab is the whole box), 5 one cell thick, 6 the whole box"""
    length = [int(v) for v in rng.integers(1, n + 1, 3)]
    start = [int(v) for v in rng.integers(0, n, 3)]
    if kind == 1:
        length = [int(v) for v in rng.integers(2, n + 1, 3)]
        start = [int(rng.integers(n - length[d] + 1, n)) for d in range(3)]
    elif kind == 2:
        start = [-int(v) for v in rng.integers(1, n, 3)]
    elif kind == 3:
        for d in rng.permutation(3)[:int(rng.integers(1, 4))]:
            length[int(d)] = n
    elif kind == 4:
        if nxl == n:
            return None
        length[0] = int(rng.integers(1, n - nxl + 1))
        start[0] = (x0 + nxl + int(rng.integers(0, n - nxl - length[0] + 1))) % n
    elif kind == 5:
        length[int(rng.integers(0, 3))] = 1
    elif kind == 6:
        start, length = [0, 0, 0], [n, n, n]
    return start, length


def random_field(rng, shape, kind):
    """fp32 fields: 0 smooth random, 1 ties (a few distinct values around Flast), 2 NaN and infinities sprinkled in"""
    f = (rng.random(shape) * 3.0).astype(np.float32)
    if kind == 1:
        f = rng.choice(np.array([0.0, 0.5, 1.0, np.nextafter(np.float32(1.0), np.float32(2.0)), 1.75, 2.0], dtype=np.float32), size=shape)
    elif kind == 2:
        r = rng.random(shape)
        f[r < 0.05] = np.nan
        f[(r >= 0.05) & (r < 0.08)] = np.inf
        f[(r >= 0.08) & (r < 0.11)] = -np.inf
    return f


def random_map(rng, length, kind):
    """kind 0: None (every bit), 1 random bits, 2 all zero, 3 random with a word count that is odd (not a multiple of 64 bits)"""
    cells = length[0] * length[1] * length[2]
    if kind == 0:
        return None
    if kind == 2:
        return np.zeros((cells + 31) // 32, dtype=np.uint32)
    words = pack_map(rng.random(tuple(length)) < 0.6)
    if kind == 3 and words.size % 2 == 0:
        words = np.concatenate([words, rng.integers(0, 2 ** 32, 1, dtype=np.uint64).astype(np.uint32)])   # bits beyond the sub-box: never read
    return words


FLASTS = (1.0, 0.0, 1.75, float("inf"), float("-inf"), float(np.nextafter(1.0, 2.0)))


def random_cases(n, count, seed):
    """-> (x0, nxl, start, length, map words, flast, field [nxl][n][n]) in turn through every kind of sub-box, map, flast and field"""
    rng = np.random.default_rng(seed)
    divisors = [p for p in (1, 2, 3, 4, 8) if n % p == 0]
    out = []
    k = 0
    while len(out) < count:
        k += 1
        p = divisors[k % len(divisors)]
        nxl = n // p
        x0 = int(rng.integers(0, p)) * nxl
        sub = random_subbox(rng, n, x0, nxl, k % 7)
        if sub is None:
            continue
        start, length = sub
        out.append((x0, nxl, start, length, random_map(rng, length, (k // 7) % 4), FLASTS[(k // 3) % len(FLASTS)],
                    random_field(rng, (nxl, n, n), (k // 5) % 3)))
    return out
