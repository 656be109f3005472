// pf_corr_core.h -- one cell of the separation-space shell pass (include/pinfmax.h: pf_halo_correlation): the shell of its
// separation, the Legendre weights of its angle to the line of sight from exact integers, and which of the six positive sums of a
// shell its terms enter.  Plain C++ for host and device: the kernels of pf_power.hip call it, and a CPU test compiles it on its own
// (tests/cpu_emul/corr_emul.cpp) against the numpy restatement (tests/np_corr.py).  The file that includes this is compiled without
// contraction.
//
//   separation  the cell (x, y, z) of a circular correlation lies at s = pf_power_signed(i, n) on every axis (n/2 stays positive);
//               r2 = sx^2 + sy^2 + sz^2, the shell is pf_power_shell(r2), the weight 1: the whole lattice is stored
//   mu^2        a / r2 with a = s_los^2; the weights are pf_multipole_weights(a, r2): at r2 = 0, L2 = L4 = 0
//   terms       v, v L2, v L4 of the cell's value v, one product each
//   sums        2 k + 0 the positive terms of order k (l = 2 k), 2 k + 1 the negated negative ones: l = 0 has both signs here.  A
//               term of zero enters none; a value that is not finite enters the counts of its shell and no sum
#pragma once
#include <math.h>
#include <stdint.h>

#include "pf_multipole_core.h"

#define PF_CORR_HD PF_POWER_HD
#define PF_CORR_NORDERS 3   // PF_CORR_ORDERS of pinfmax.h
#define PF_CORR_NSUMS 6     // positive sums per shell of ONE field; PF_CORR_SUMS of pinfmax.h counts both fields

PF_CORR_HD unsigned int pf_corr_r2(int sx, int sy, int sz) { return (unsigned int)(sx * sx + sy * sy + sz * sz); }
// the signed separation on axis `los`, squared
PF_CORR_HD unsigned int pf_corr_a(int los, int sx, int sy, int sz) { return (unsigned int)(los == 0 ? sx * sx : los == 1 ? sy * sy : sz * sz); }

// the three signed terms of a cell: l = 0, 2, 4
PF_CORR_HD void pf_corr_terms(double v, double L2, double L4, double x[3]) { x[0] = v; x[1] = v * L2; x[2] = v * L4; }
// term k of value x != 0 enters, as |x|, ONE of the six sums
PF_CORR_HD int pf_corr_sum_of(int k, double x) { return x > 0.0 ? 2 * k : 2 * k + 1; }

// the element of the form pass: a mode's term over N^3, one division, rounded once to the field type by the caller; a term that is
// not finite, and the k = 0 mode, give zero (*bad says which of the two it was: the former is counted)
PF_CORR_HD double pf_corr_form(double t, unsigned int k2, double n3, bool *bad) {
  *bad = !pf_power_finite(t);
  if (*bad || !k2) return 0.0;
  return t / n3;
}
