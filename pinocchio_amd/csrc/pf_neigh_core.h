// pf_neigh_core.h -- the cell arithmetic of the neighbour table (pf_neighbours.hip): what the loops of build_groups()
// (src/build_groups.c:245-343), quick_build_groups() (:1916-2004) and count_peaks() (src/fragment.c:605-706) compute per stored
// particle before they touch the group state -- INDEX_TO_COORD, the border skip (:251-254), good_particle (:262-264), the six
// neighbour coordinates with their single wrap (the switch at :274-306) -- and the searches of find_location() (src/fragment.c:592-603)
// over sorted_pos.  Plain C++ with no device dependence, so that a CPU test compiles it on its own
// (tests/cpu_emul/neighbours_emul.cpp) and walks it cell by cell against the numpy restatement (tests/np_neighbours.py).
//
// Positions: pos = z + Lz (y + Ly x) (COORD_TO_INDEX, src/pinocchio.h:84-85) over len[3] = subbox.Lgwbl.  A z-row is the run of Lz
// consecutive positions of one (x, y): row id r = y + Ly x, positions [r Lz, (r + 1) Lz).
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define PF_NEIGH_HD __host__ __device__ __forceinline__
#else
#define PF_NEIGH_HD static inline
#endif

struct PfNeighBox { int len[3], pbc[3], safe[3]; };   // subbox.Lgwbl, subbox.pbc, subbox.safe

PF_NEIGH_HD void pf_neigh_coord(const PfNeighBox &b, unsigned int pos, int c[3]) {   // INDEX_TO_COORD
  const unsigned int lz = (unsigned int)b.len[2], ly = (unsigned int)b.len[1], r = pos / lz;
  c[2] = (int)(pos - r * lz); c[1] = (int)(r % ly); c[0] = (int)(r / ly);
}
PF_NEIGH_HD unsigned int pf_neigh_pos(const PfNeighBox &b, const int c[3]) {   // COORD_TO_INDEX; at most 2^32 cells
  return (unsigned int)((unsigned long long)c[2] + (unsigned long long)b.len[2] * ((unsigned long long)c[1] + (unsigned long long)b.len[1] * (unsigned long long)c[0]));
}
PF_NEIGH_HD unsigned int pf_neigh_row(const PfNeighBox &b, const int c[3]) { return (unsigned int)c[1] + (unsigned int)b.len[1] * (unsigned int)c[0]; }

// "skips the peak condition if the point is at the border (and PBCs are not active)" (:251-254)
PF_NEIGH_HD bool pf_neigh_skip(const PfNeighBox &b, const int c[3]) {
  bool s = false;
  for (int d = 0; d < 3; d++) s = s || (!b.pbc[d] && (c[d] == 0 || c[d] == b.len[d] - 1));
  return s;
}
// good_particle (:262-264)
PF_NEIGH_HD bool pf_neigh_good(const PfNeighBox &b, const int c[3]) {
  bool g = true;
  for (int d = 0; d < 3; d++) g = g && c[d] >= b.safe[d] && c[d] < b.len[d] - b.safe[d];
  return g;
}
// neighbour nn = 0..5 (x-, x+, y-, y+, z-, z+) of a particle that is not skipped: its coordinates, wrapped once in a periodic
// direction (:274-306).  Returns whether it wrapped.  (Without the wrap the coordinate stays inside: a particle that is not skipped
// lies in 1 .. len - 2 of a direction that is not periodic.)
PF_NEIGH_HD bool pf_neigh_step(const PfNeighBox &b, const int c[3], int nn, int c1[3]) {
  const int d = nn >> 1;
  c1[0] = c[0]; c1[1] = c[1]; c1[2] = c[2];
  if (!(nn & 1)) {
    if (b.pbc[d] && c[d] == 0) { c1[d] = b.len[d] - 1; return true; }
    c1[d] = c[d] - 1;
  } else {
    if (b.pbc[d] && c[d] == b.len[d] - 1) { c1[d] = 0; return true; }
    c1[d] = c[d] + 1;
  }
  return false;
}

// find_location(): the rank of `pos` in the ascending a[lo, hi), -1 when it is not there; at most log2(hi - lo) + 1 steps, every
// index read lies in [lo, hi)
PF_NEIGH_HD long long pf_neigh_find(const unsigned int *a, unsigned int lo, unsigned int hi, unsigned int pos) {
  while (lo < hi) {
    const unsigned int mid = lo + ((hi - lo) >> 1), v = a[mid];
    if (v == pos) return (long long)mid;
    if (v < pos) lo = mid + 1; else hi = mid;
  }
  return -1;
}
// the first rank of a[0, m) whose position is not below `key` (m when there is none): the start of the z-row that begins at `key`
PF_NEIGH_HD unsigned int pf_neigh_lower_bound(const unsigned int *a, unsigned int m, unsigned long long key) {
  unsigned int lo = 0, hi = m;
  while (lo < hi) {
    const unsigned int mid = lo + ((hi - lo) >> 1);
    if ((unsigned long long)a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The lookup of neighbour nn of the particle at rank p of sorted_pos (coordinates c, not skipped): the RANK of the neighbour, -1 when
// none is stored there.  rowstart[r], r = 0 .. Lx Ly: pf_neigh_lower_bound of r Lz, so that the ranks of z-row r are
// [rowstart[r], rowstart[r + 1]); null selects the plain form, one search of the whole array (the reference's way).
//   z-/z+   no search: rank p -/+ 1 exactly when its position is pos -/+ 1; a periodic wrap in z lands on the first (z+) or last
//           (z-) rank of the particle's own row, which holds p and so is not empty
//   others  a search of the neighbour's row alone: at most Lz contiguous entries
PF_NEIGH_HD long long pf_neigh_rank(const PfNeighBox &b, unsigned int m, const unsigned int *spos, const unsigned int *rowstart, unsigned int p, const int c[3],
                                    int nn) {
  int c1[3];
  const bool wrapped = pf_neigh_step(b, c, nn, c1);
  const unsigned int npos = pf_neigh_pos(b, c1);
  if (!rowstart) return pf_neigh_find(spos, 0u, m, npos);
  if (nn < 4) { const unsigned int row = pf_neigh_row(b, c1); return pf_neigh_find(spos, rowstart[row], rowstart[row + 1], npos); }
  const unsigned int own = pf_neigh_row(b, c);
  long long q;
  if (wrapped) q = (nn & 1) ? (long long)rowstart[own] : (long long)rowstart[own + 1] - 1;
  else q = (nn & 1) ? (long long)p + 1 : (long long)p - 1;
  return (q >= 0 && q < (long long)m && spos[q] == npos) ? q : -1;
}
