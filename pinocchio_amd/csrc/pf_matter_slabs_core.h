// pf_matter_slabs_core.h -- the plan of the slab form of the mass assignment (include/pinfmax.h: pf_matter_power_slabs): how far the
// particles of a slab reach beyond it, the window of planes a rank deposits into, and which planes of that window travel to which
// rank in which slot of the all-to-all.  Plain C++ for host and device: k_matter_reach of pf_matter.hip calls the reach, the host code
// of pf_matter.hip the plan, and a CPU test compiles both on their own (tests/cpu_emul/matter_slabs_emul.cpp) against the numpy
// restatement (tests/np_matter_slabs.py).  The position arithmetic is pf_matter_core.h's.
//
//   reach     of a particle of plane q0 whose x position is finite and inside [0, n]: the x planes it adds to -- CIC: i0 and, where
//             its weight t is not zero, i0 + 1; NGP: floor(pos) --, each as the signed minimal-image offset
//             s = ((plane - q0 + n/2) mod n) - n/2.  A rank's reach is Hlo = max(0, -min s), Hhi = max(0, max s).  Only the x columns
//             are read: a particle that its y or z position keeps out of the grid still counts, which can widen a window by a plane
//             and never narrows one
//   window    with the maxima Hlo, Hhi over the ranks: nxl + Hlo + Hhi >= n: the whole box, w0 = 0, wn = n; else w0 = x0 - Hlo (mod n),
//             wn = nxl + Hlo + Hhi.  Target plane g lies at window plane (g - w0) mod n iff that is below wn
//   blocks    plane g belongs to rank g / nxl.  L(r, q), q != r: the local planes of rank q inside the window of rank r, ascending;
//             slot j of the block that r sends to q is plane L(r, q)[j].  B = the longest list over all pairs: every rank finds it
//             from (n, P, Hlo, Hhi) alone, by enumeration.  Two ghost regions that belong to one peer (P = 2) and windows that span
//             several owners (reach beyond a slab's thickness) are lists like any other
#pragma once
#include "pf_matter_core.h"

PF_MATTER_HD int pf_matter_slabs_mod(int a, int n) { const int r = a % n; return r < 0 ? r + n : r; }
PF_MATTER_HD int pf_matter_slabs_offset(int plane, int q0, int n) { return pf_matter_slabs_mod(plane - q0 + n / 2, n) - n / 2; }

// the x position `pos` of a particle of plane q0 -> false: not deposited whatever its other axes are; true: the smallest and the
// largest offset of the planes it adds to
template <class T> PF_MATTER_HD bool pf_matter_reach(T pos, int q0, int n, int ngp, int *smin, int *smax) {
  if (!(pos - pos == (T)0) || !(pos >= (T)0 && pos <= (T)n)) return false;
  if (ngp) {
    *smin = *smax = pf_matter_slabs_offset(pf_matter_ngp_axis<T>(pos, n), q0, n);
    return true;
  }
  int cell[2];
  uint32_t w[2];
  pf_matter_cic_axis<T>(pos, n, cell, w);
  const int a = pf_matter_slabs_offset(cell[0], q0, n);
  *smin = *smax = a;
  if (w[1]) {
    const int b = pf_matter_slabs_offset(cell[1], q0, n);
    if (b < a) *smin = b; else *smax = b;
  }
  return true;
}

// the window of the rank whose slab begins at x0 -> 1: it is the whole box
PF_MATTER_HD int pf_matter_window(int n, int nxl, int x0, int hlo, int hhi, int *w0, int *wn) {
  if ((long long)nxl + hlo + hhi >= n) { *w0 = 0; *wn = n; return 1; }
  *w0 = pf_matter_slabs_mod(x0 - hlo, n); *wn = nxl + hlo + hhi;
  return 0;
}
// the window plane of target plane g, -1: outside
PF_MATTER_HD int pf_matter_window_plane(int g, int w0, int wn, int n) {
  const int p = g - w0 + (g < w0 ? n : 0);
  return p < wn ? p : -1;
}
// L(r, q) into list (nxl entries at most; null: the length alone) -> its length
PF_MATTER_HD int pf_matter_block_list(int n, int P, int hlo, int hhi, int r, int q, int *list) {
  const int nxl = n / P;
  int w0, wn, count = 0;
  pf_matter_window(n, nxl, r * nxl, hlo, hhi, &w0, &wn);
  for (int l = 0; l < nxl; l++)
    if (pf_matter_window_plane(q * nxl + l, w0, wn, n) >= 0) {
      if (list) list[count] = l;
      count++;
    }
  return count;
}
// B: planes per peer block
PF_MATTER_HD int pf_matter_block_planes(int n, int P, int hlo, int hhi) {
  int B = 0;
  for (int r = 0; r < P; r++)
    for (int q = 0; q < P; q++) {
      if (q == r) continue;
      const int len = pf_matter_block_list(n, P, hlo, hhi, r, q, (int *)0);
      if (len > B) B = len;
    }
  return B;
}
// what pf_debug_matter_exchange reports as the form: 0 nothing crosses, 1 ghost planes, 2 every rank deposits the whole box
PF_MATTER_HD int pf_matter_exchange_form(int n, int P, int hlo, int hhi) {
  if (P == 1 || (hlo == 0 && hhi == 0)) return 0;
  return (long long)(n / P) + hlo + hhi >= n ? 2 : 1;
}
