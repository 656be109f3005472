"""The group velocities of a redshift segment restated in numpy, from the reference's loop.

recompute_group_velocities() (src/fragment.c:852-909) walks the linking list of every group i in FILAMENT + 1 .. ngroups and sums the
eight velocity fields of frag[] over its Mass particles, then divides by Mass.  The particles of group i are those with group_ID == i,
so the sums are a segmented sum over group_ID of the 24 numbers pf_gather_velocities returns (tests/np_refresh.py):
  * a particle is FOUND when its cell lies in the slab (np_refresh.cells: no good_particle test);
  * it is COUNTED when it is found and group_ID >= first_group, LOOSE when it is found and group_ID < first_group;
  * sum24[j][k] is the sum of column k over the counted particles of the j-th group present, in ascending group ID.
Here the sums are exact: math.fsum, or int64 for integer-valued columns.  Shares no code with the device path."""
import math

import numpy as np

import np_refresh as npr


def classes(n, x0, nxl, start, length, frag_pos, group_id, first_group):
    """-> (found, loose, counted) bool[N], and the slab cell of every particle (meaningful where found)"""
    found, cell = npr.cells(n, x0, nxl, start, length, frag_pos)
    gid = np.asarray(group_id).astype(np.int64)
    return found, found & (gid < first_group), found & (gid >= first_group), cell


def _segments(gid_counted):
    """the counted particles by group: (group IDs ascending, list of index arrays into the counted set)"""
    if len(gid_counted) == 0:
        return np.zeros(0, dtype=np.int64), []
    order = np.argsort(gid_counted, kind="stable")
    ids, first = np.unique(gid_counted[order], return_index=True)
    return ids, np.split(order, first[1:])


def sums_of(vals, group_id, first_group):
    """vals [N][24] (the 24 numbers of N found particles), their group IDs -> (group int32[G], npart uint32[G], sum24 float64[G][24],
    abs24 float64[G][24]): the correctly rounded sums (math.fsum) of the values and of their moduli over the particles with
    group_ID >= first_group, per group in ascending ID"""
    vals = np.asarray(vals, dtype=np.float64).reshape(-1, 24)
    gid = np.asarray(group_id).astype(np.int64)
    idx = np.flatnonzero(gid >= first_group)
    ids, members = _segments(gid[idx])
    out = np.zeros((len(ids), 24))
    mod = np.zeros((len(ids), 24))
    for j, mem in enumerate(members):
        v = vals[idx[mem]]
        for k in range(24):
            out[j, k] = math.fsum(v[:, k])
            mod[j, k] = math.fsum(np.abs(v[:, k]))
    return ids.astype(np.int32), np.array([len(m) for m in members], dtype=np.uint32), out, mod


def sums(n, x0, nxl, start, length, frag_pos, group_id, first_group, cols24):
    """-> (group int32[G], npart uint32[G], sum24 float64[G][24]): the correctly rounded sums (math.fsum) of the 24 columns over the
    counted particles of every group"""
    cols24 = np.asarray(cols24)
    found, _, _, cell = classes(n, x0, nxl, start, length, frag_pos, group_id, first_group)
    idx = np.flatnonzero(found)
    return sums_of(cols24[:, cell[idx]].T, np.asarray(group_id)[idx], first_group)[:3]


def abs_sums(n, x0, nxl, start, length, frag_pos, group_id, first_group, cols24):
    """sum |v| per group and column (for the error bounds), as float64[G][24]"""
    return sums(n, x0, nxl, start, length, frag_pos, group_id, first_group, np.abs(np.asarray(cols24, dtype=np.float64)))[2]


def int_sums(n, x0, nxl, start, length, frag_pos, group_id, first_group, cols24):
    """as sums() for integer-valued columns, in int64 arithmetic -> sum24 as float64 (exact below 2^53)"""
    cols24 = np.asarray(cols24)
    ic = cols24.astype(np.int64)
    assert np.array_equal(ic, cols24)
    _, _, counted, cell = classes(n, x0, nxl, start, length, frag_pos, group_id, first_group)
    idx = np.flatnonzero(counted)
    gid = np.asarray(group_id).astype(np.int64)[idx]
    ids, inv = np.unique(gid, return_inverse=True)
    out = np.zeros((len(ids), 24), dtype=np.int64)
    np.add.at(out, inv, ic[:, cell[idx]].T)
    assert np.abs(out).max(initial=0) < 2 ** 53
    return ids.astype(np.int32), np.bincount(inv, minlength=len(ids)).astype(np.uint32), out.astype(np.float64)


def scatter_means(groups, group, npart, sum24, offsets, dtype):
    """groups: uint8 [ngroups + 1][stride], the caller's group records.  Record group[j] gets (dtype)(sum24[j][3 s .. 3 s + 2] / npart[j])
    at byte offsets[s] (s = 0..3: Vel, Vel_2LPT, Vel_3LPT_1, Vel_3LPT_2; 4..7 their *_prev) for the offsets that are not negative; a
    copy comes back"""
    out = np.array(groups, copy=True)
    dtype = np.dtype(dtype)
    pb = dtype.itemsize
    for j, g in enumerate(np.asarray(group, dtype=np.int64)):
        for s, off in enumerate(offsets):
            if off >= 0:
                mean = (np.asarray(sum24[j][3 * s:3 * s + 3], dtype=np.float64) / float(npart[j])).astype(dtype)
                out[g, off:off + 3 * pb] = mean.view(np.uint8)
    return out


def reference_means(vel24, group_id, first_group, rng):
    """recompute_group_velocities() for PRODFLOAT = float as the reference runs it: vel24 float32[N][24] are the particles' frag[]
    fields; per group a float32 running sum along a linking list (here: the members in a random order), divided by (double) Mass
    and stored as float -> {group: (mass, mean float32[24])}"""
    gid = np.asarray(group_id).astype(np.int64)
    out = {}
    for g in np.unique(gid[gid >= first_group]):
        mem = rng.permutation(np.flatnonzero(gid == g))
        acc = np.zeros(24, dtype=np.float32)
        for i in mem:
            acc = (acc + vel24[i]).astype(np.float32)
        out[int(g)] = (len(mem), (acc.astype(np.float64) / float(len(mem))).astype(np.float32))
    return out
