// pf_map_core.h -- the cell arithmetic of the fragmentation maps (pf_map.hip): create_map() (src/fragment.c:708-751) and update_map()
// (src/build_groups.c:2246-2318) cut into the pieces the kernels are made of.  Plain C++ with no device dependence, so that a CPU
// test compiles it on its own (tests/cpu_emul/map_emul.cpp) and walks it lane by lane against the numpy restatement of the
// reference's loops (tests/np_maps.py).
//
// The map: one bit per cell of the sub-box with its boundary layer, len[3] = subbox.Lgwbl; bit pos = z + Lz (y + Ly x)
// (COORD_TO_INDEX, src/pinocchio.h:85) lives in word pos >> 5, bit pos & 31 (UINTLEN = 32).  Along z the bits of a row are
// consecutive, which is what both kernels build on.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define PF_MAP_HD __host__ __device__ __forceinline__
#else
#define PF_MAP_HD static inline
#endif

struct PfMapBox { int len[3], pbc[3]; };          // subbox.Lgwbl, subbox.pbc
struct PfMapGroup { int ig, jg, kg, size; };      // update_map's (int)(Pos + 0.5) and size of one group (an int4 on the device)

// ---- the wrap / out-of-range rule of update_map (:2263-2295), one direction: the coordinate of cube cell c1, wrapped ONCE in a
// periodic direction, -1 outside a direction that is not ----
PF_MAP_HD int pf_map_coord(int c1, int len, int pbc) {
  if (c1 >= 0 && c1 < len) return c1;
  if (!pbc) return -1;
  return c1 < 0 ? c1 + len : c1 - len;
}

PF_MAP_HD unsigned int pf_map_pos(const PfMapBox &b, int i, int j, int k) {   // COORD_TO_INDEX; at most 2^32 cells
  return (unsigned int)((unsigned long long)k + (unsigned long long)b.len[2] * ((unsigned long long)j + (unsigned long long)b.len[1] * (unsigned long long)i));
}

// ---- create_map: per direction the range [safe - 1, Lgrid + safe + 1) with Lgrid = len - 2 safe, or [0, len) when periodic ----
PF_MAP_HD void pf_map_box_range(int len, int safe, int pbc, int *lo, int *hi) {
  if (pbc) { *lo = 0; *hi = len; }
  else { *lo = safe - 1; *hi = len - safe + 1; }
}
// row r of the box (x slowest): its first bit and its length
PF_MAP_HD void pf_map_box_row(const PfMapBox &b, const int lo[3], const int hi[3], unsigned long long r, unsigned long long *first, unsigned int *length) {
  const unsigned long long ny = (unsigned long long)(hi[1] - lo[1]);
  const int i = lo[0] + (int)(r / ny), j = lo[1] + (int)(r % ny);
  *first = (unsigned long long)pf_map_pos(b, i, j, lo[2]);
  *length = (unsigned int)(hi[2] - lo[2]);
}
// the bits of word `word` that belong to the run [first, first + length) of consecutive bits
PF_MAP_HD unsigned int pf_map_word_mask(unsigned long long first, unsigned long long length, unsigned long long word) {
  const unsigned long long w0 = word * 32ull, w1 = w0 + 32ull, e = first + length;
  const unsigned long long lo = first > w0 ? first : w0, hi = e < w1 ? e : w1;
  if (hi <= lo) return 0u;
  const unsigned int nb = (unsigned int)(hi - lo);
  return (nb == 32u ? 0xFFFFFFFFu : ((1u << nb) - 1u)) << (unsigned int)(lo - w0);
}

// ---- update_map: the unit of work is a ROW, one (group, i1, j1) pair: 2 size cells consecutive in k1.  A wavefront takes an
// "item": one row when it is 64 cells or longer (in chunks of 64 lanes), otherwise as many whole rows of the same group as fit
// 64 lanes.  A group has 4 size^2 rows. ----
PF_MAP_HD int pf_map_rows_per_item(int size) { return size <= 0 ? 0 : (2 * size >= 64 ? 1 : 64 / (2 * size)); }
PF_MAP_HD unsigned long long pf_map_items(int size) {
  if (size <= 0) return 0;
  const unsigned long long rows = 4ull * (unsigned long long)size * (unsigned long long)size, per = (unsigned long long)pf_map_rows_per_item(size);
  return (rows + per - 1) / per;
}
PF_MAP_HD int pf_map_chunks(int size) { return (2 * size + 63) / 64; }   // rounds of 64 lanes an item takes

struct PfMapCell {
  bool valid;        // the lane holds a cell of the cube
  bool out;          // ... that lies outside the sub-box in a direction that is not periodic: nadd[1]
  bool inside;       // ... whose offset has rr <= size^2
  unsigned int pos;  // its bit (valid && !out)
};
PF_MAP_HD PfMapCell pf_map_cell(const PfMapBox &b, const PfMapGroup &g, unsigned long long item, int chunk, int lane) {
  PfMapCell c;
  c.valid = c.out = c.inside = false; c.pos = 0;
  const int L = 2 * g.size;
  unsigned long long row;
  int kk;
  if (L >= 64) {
    row = item; kk = chunk * 64 + lane;
    if (kk >= L) return c;
  } else {
    const int per = 64 / L, sub = lane / L;
    kk = lane - sub * L;
    row = item * (unsigned long long)per + (unsigned long long)sub;
    if (chunk || sub >= per || row >= (unsigned long long)L * (unsigned long long)L) return c;
  }
  c.valid = true;
  const int di = (int)(row / (unsigned long long)L) - g.size, dj = (int)(row % (unsigned long long)L) - g.size, dk = kk - g.size;
  const int i = pf_map_coord(g.ig + di, b.len[0], b.pbc[0]), j = pf_map_coord(g.jg + dj, b.len[1], b.pbc[1]), k = pf_map_coord(g.kg + dk, b.len[2], b.pbc[2]);
  if (i < 0 || j < 0 || k < 0) { c.out = true; return c; }   // (tested before the sphere, as the reference does: nadd[1] counts cube cells)
  c.pos = pf_map_pos(b, i, j, k);
  c.inside = di * di + dj * dj + dk * dk <= g.size * g.size;
  return c;
}

// ---- one atomic per touched word: the lanes of a wavefront whose bits are consecutive and lie in one word form a run; its first
// lane ORs the set flags of the whole run.  `live`: the lane holds a bit (valid && !out). ----
PF_MAP_HD bool pf_map_run_head(int lane, bool live, bool live_prev, unsigned int pos, unsigned int pos_prev) {
  return lane == 0 || !live || !live_prev || pos != pos_prev + 1u || (pos & 31u) == 0u;
}
// heads / flags: the ballots of pf_map_run_head and of "this lane sets its bit"; the word mask the head `lane` (bit `pos`) ORs in
PF_MAP_HD unsigned int pf_map_run_mask(unsigned long long heads, unsigned long long flags, int lane, unsigned int pos) {
  const unsigned long long above = lane == 63 ? 0ull : (heads >> (lane + 1)) << (lane + 1);
  const int end = above ? __builtin_ctzll(above) : 64;   // the next head, or the end of the wavefront
  const int len = end - lane;                   // (<= 32 - (pos & 31): a head stands at every word boundary)
  const unsigned long long m = (flags >> lane) & (len >= 64 ? ~0ull : ((1ull << len) - 1ull));
  return (unsigned int)m << (pos & 31u);
}
