// Host compilation of the cell arithmetic of the neighbour table (pinocchio_amd/csrc/pf_neigh_core.h) for tests/test_neighbours_cpu.py:
// the per-cell quantities, and the lookup of the kernel walked rank by rank as its lanes walk it.
#include "../../pinocchio_amd/csrc/pf_neigh_core.h"

static PfNeighBox box_of(const int *len, const int *pbc, const int *safe) {
  PfNeighBox b;
  for (int d = 0; d < 3; d++) { b.len[d] = len[d]; b.pbc[d] = pbc[d]; b.safe[d] = safe[d]; }
  return b;
}

extern "C" {

// per position: coordinates, skip, good, row id; for a cell that is not skipped the six neighbour positions and whether they wrapped
void emul_cells(const int *len, const int *pbc, const int *safe, size_t count, const unsigned int *pos, int *coord /* [3 count] */, unsigned char *skip,
                unsigned char *good, unsigned int *row, unsigned int *npos /* [6 count] */, unsigned char *wrapped /* [6 count] */) {
  const PfNeighBox b = box_of(len, pbc, safe);
  for (size_t i = 0; i < count; i++) {
    int c[3];
    pf_neigh_coord(b, pos[i], c);
    for (int d = 0; d < 3; d++) coord[3 * i + d] = c[d];
    skip[i] = pf_neigh_skip(b, c); good[i] = pf_neigh_good(b, c); row[i] = pf_neigh_row(b, c);
    for (int nn = 0; nn < 6; nn++) {
      npos[6 * i + nn] = 0; wrapped[6 * i + nn] = 0;
      if (skip[i]) continue;
      int c1[3];
      wrapped[6 * i + nn] = pf_neigh_step(b, c, nn, c1);
      npos[6 * i + nn] = pf_neigh_pos(b, c1);
    }
  }
}

// rowstart[0 .. Lx Ly] of m ascending positions
void emul_rowstart(const int *len, unsigned int m, const unsigned int *spos, unsigned int *rowstart) {
  const unsigned long long nrows = (unsigned long long)len[0] * (unsigned long long)len[1];
  for (unsigned long long r = 0; r <= nrows; r++) rowstart[r] = pf_neigh_lower_bound(spos, m, r * (unsigned long long)len[2]);
}

// the rank of every neighbour of every rank p (-1: none, and for a skipped particle); rowstart null: the plain form
void emul_ranks(const int *len, const int *pbc, const int *safe, unsigned int m, const unsigned int *spos, const unsigned int *rowstart, long long *rank /* [6 m] */) {
  const PfNeighBox b = box_of(len, pbc, safe);
  for (unsigned int p = 0; p < m; p++) {
    int c[3];
    pf_neigh_coord(b, spos[p], c);
    for (int nn = 0; nn < 6; nn++) rank[6 * (size_t)p + nn] = pf_neigh_skip(b, c) ? -1 : pf_neigh_rank(b, m, spos, rowstart, p, c, nn);
  }
}
}
