// pf_back_core.h -- the cell arithmetic of distribute_back() (src/distribute.c:703-946): what keep_data_back() (:799-837) and the loop
// of send_data_back() (:859-896) compute per stored particle of a sub-box before they store its zacc and group_ID into products[] of
// an FFT slab -- INDEX_TO_COORD, the good_particle test (:815-817), the shift into the periodic box (:820-822), membership of the
// receiving fft box (:824-827) and the position in it (:830).  Plain C++ with no device dependence, so that a CPU test compiles it
// on its own (tests/cpu_emul/back_emul.cpp) and walks it particle by particle against the numpy restatement (tests/np_back.py).
//
// Positions: pos = z + Lz (y + Ly x) over len[3] = subbox.Lgwbl, as in pf_neigh_core.h, whose INDEX_TO_COORD and good_particle are
// used as they are.  The receiving fft box is an x-slab: planes x0 .. x0 + nxl - 1 of the n^3 box, whole in y and z, so that only x
// decides membership; a cell of it has the index z + n (y + n (x - x0)) of every product column.
#pragma once
#include <stddef.h>

#include "pf_neigh_core.h"

#define PF_BACK_HD PF_NEIGH_HD

// box: subbox.Lgwbl, subbox.pbc (not used here), subbox.safe; start: subbox.stabl reduced to [0, n) (pf_dist_wrap, as pf_distribute
// reduces it: the reference adds n once, :820-822); the slab
struct PfBackBox { PfNeighBox box; int start[3]; int n, x0, nxl; };

// "global box frame" (:820-822): c[d] < len[d] <= n and 0 <= start[d] < n, so one subtraction is the modulo
PF_BACK_HD void pf_back_global(const PfBackBox &b, const int c[3], int g[3]) {
  for (int d = 0; d < 3; d++) { g[d] = c[d] + b.start[d]; if (g[d] >= b.n) g[d] -= b.n; }
}
// (:824-827) for a slab
PF_BACK_HD bool pf_back_in_slab(const PfBackBox &b, const int g[3]) { return g[0] >= b.x0 && g[0] < b.x0 + b.nxl; }
// COORD_TO_INDEX(ibox - fft_box[0], jbox, kbox, fft_box + 3) (:830) of a cell of the slab
PF_BACK_HD size_t pf_back_index(const PfBackBox &b, const int g[3]) {
  return (size_t)g[2] + (size_t)b.n * ((size_t)g[1] + (size_t)b.n * (size_t)(g[0] - b.x0));
}
// the particle at sub-box position pos (< Lx Ly Lz): whether this slab takes it, and where
PF_BACK_HD bool pf_back_cell(const PfBackBox &b, unsigned int pos, size_t *addr) {
  int c[3], g[3];
  pf_neigh_coord(b.box, pos, c);
  if (!pf_neigh_good(b.box, c)) return false;
  pf_back_global(b, c, g);
  if (!pf_back_in_slab(b, g)) return false;
  *addr = pf_back_index(b, g);
  return true;
}
