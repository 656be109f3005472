// pf_groupvel_core.h -- the arithmetic of the group velocities of a redshift segment (pf_groupvel.hip): what recompute_group_velocities()
// (src/fragment.c:852-909) computes, restated as a segmented sum over sorted keys.  Plain C++ with no device dependence, so that a CPU
// test compiles it on its own (tests/cpu_emul/groupvel_emul.cpp) and walks it unit by unit against the numpy restatement
// (tests/np_groupvel.py).
//
// One key per counted particle: group ID above the cell index of the slab, the cell in the low `cellbits` bits (the bits of the last
// cell of the slab) and the ID directly above them, so that the bits in use are one run and the radix sort visits no others.  After the
// sort the particles of a group are contiguous and in cell order.  Particle j of the sorted array is a HEAD when j = 0 or its group
// differs from that of j - 1, a TAIL when j = m - 1 or its group differs from that of j + 1; the slot of a group in the output is the
// number of heads before its own.
//
// The sum of a group is built in a fixed tree that depends on the sorted array alone.  The array is cut into UNITS of consecutive keys
// (a wavefront's 64 on the device), PF_GV_UNITS units are a TILE (a workgroup's).  Of the segments of one group inside a unit
//   * those that begin (a head) and end (a tail) in the unit are complete and go to the group's slot;
//   * the one that reaches the unit from before (its first key is no head) is the unit's F part; it CLOSES when its tail lies in the unit;
//   * the one that leaves the unit (its last key is no tail) and began in it is the unit's L part.
// pf_gv_combine walks the units of a tile in order and adds an F part to what is open: a segment that closes goes to its slot when it
// was opened in the tile, and is the tile's own F part when it was not; what is open at the end is the tile's L part, or its F part
// that does not close.  pf_gv_fold then starts at every tile with an L part and adds the F parts of the tiles behind it, in tile
// order, up to the one that closes.  A part is PF_GV_NV doubles: the 24 columns and the number of particles (exact below 2^53).
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define PF_GV_HD __host__ __device__ __forceinline__
#else
#define PF_GV_HD static inline
#endif

#define PF_GV_NV 25            // values of a part: columns 0..23 and the count
#define PF_GV_WAVE 64          // keys of a unit on the device
#define PF_GV_WAVES 4          // waves of a workgroup
#define PF_GV_ROUNDS 4         // units a wave takes, one after the other
#define PF_GV_UNITS (PF_GV_WAVES * PF_GV_ROUNDS)
#define PF_GV_TILE (PF_GV_UNITS * PF_GV_WAVE)   // 1024 keys

#define PF_GV_HAS_F 1u         // flags of a unit and of a tile
#define PF_GV_F_CLOSES 2u
#define PF_GV_HAS_L 4u

// bits of x: 0 for 0, 1 for 1, 2 for 2 and 3, ...
PF_GV_HD unsigned int pf_gv_bits(unsigned long long x) {
  unsigned int b = 0;
  while (x) { b++; x >>= 1; }
  return b;
}
PF_GV_HD unsigned long long pf_gv_key(unsigned int gid, unsigned long long cell, unsigned int cellbits) { return ((unsigned long long)gid << cellbits) | cell; }
PF_GV_HD unsigned int pf_gv_group(unsigned long long key, unsigned int cellbits) { return (unsigned int)(key >> cellbits); }
PF_GV_HD unsigned long long pf_gv_cell(unsigned long long key, unsigned int cellbits) { return key & ((1ull << cellbits) - 1ull); }
PF_GV_HD bool pf_gv_head(const unsigned long long *keys, unsigned long long j, unsigned int cellbits) {
  return j == 0 || pf_gv_group(keys[j - 1], cellbits) != pf_gv_group(keys[j], cellbits);
}
PF_GV_HD bool pf_gv_tail(const unsigned long long *keys, unsigned long long m, unsigned long long j, unsigned int cellbits) {
  return j + 1 >= m || pf_gv_group(keys[j + 1], cellbits) != pf_gv_group(keys[j], cellbits);
}

// where the sums go: slot s of the output holds column k at sum[24 s + k] and the count at npart[s]; tile t keeps its F part at
// carryF[PF_GV_NV t ..], its L part at carryL[PF_GV_NV t ..] with the slot it belongs to in slotL[t], and its flags in tflags[t]
struct PfGvOut { double *sum; unsigned int *npart; double *carryF, *carryL; unsigned int *slotL, *tflags; };

PF_GV_HD void pf_gv_emit(const PfGvOut &o, unsigned int slot, int k, double v) {
  if (k < 24) o.sum[(size_t)24 * slot + k] = v;
  else o.npart[slot] = (unsigned int)v;
}

// value k (0 .. PF_GV_NV - 1) of the parts of nu units of tile t, in unit order: F[PF_GV_NV u + k], L[PF_GV_NV u + k], slotL[u], flags[u].
// Every k runs the same walk; the one with k == 0 writes what a tile has once
PF_GV_HD void pf_gv_combine(const PfGvOut &o, unsigned long long t, int nu, const double *F, const double *L, const unsigned int *slotL, const unsigned int *flags, int k) {
  bool open = false, from_before = false;
  double acc = 0.0;
  unsigned int slot = 0, tf = 0;
  for (int u = 0; u < nu; u++) {
    const unsigned int fl = flags[u];
    if (fl & PF_GV_HAS_F) {
      if (!open) { acc = F[PF_GV_NV * u + k]; open = true; from_before = true; }   // the first unit of the tile
      else acc += F[PF_GV_NV * u + k];
      if (fl & PF_GV_F_CLOSES) {
        if (from_before) { o.carryF[PF_GV_NV * t + k] = acc; tf |= PF_GV_HAS_F | PF_GV_F_CLOSES; }
        else pf_gv_emit(o, slot, k, acc);
        open = false;
      }
    }
    if (fl & PF_GV_HAS_L) { acc = L[PF_GV_NV * u + k]; slot = slotL[u]; open = true; from_before = false; }
  }
  if (open) {
    if (from_before) { o.carryF[PF_GV_NV * t + k] = acc; tf |= PF_GV_HAS_F; }
    else { o.carryL[PF_GV_NV * t + k] = acc; tf |= PF_GV_HAS_L; if (k == 0) o.slotL[t] = slot; }
  }
  if (k == 0) o.tflags[t] = tf;
}

// value k of the group that leaves tile t: its L part and the F parts of the tiles behind it up to the one that closes
PF_GV_HD void pf_gv_fold(const PfGvOut &o, unsigned long long t, unsigned long long ntiles, int k) {
  if (!(o.tflags[t] & PF_GV_HAS_L)) return;
  double acc = o.carryL[PF_GV_NV * t + k];
  for (unsigned long long u = t + 1; u < ntiles; u++) {
    acc += o.carryF[PF_GV_NV * u + k];
    if (o.tflags[u] & PF_GV_F_CLOSES) break;
  }
  pf_gv_emit(o, o.slotL[t], k, acc);
}
