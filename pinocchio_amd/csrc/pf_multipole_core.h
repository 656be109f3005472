// pf_multipole_core.h -- one mode of the multipole shell pass (include/pinfmax.h: pf_halo_multipoles): the Legendre weights of its
// angle to the line of sight from exact integers, and which of the eleven positive sums of a shell its terms enter.  Plain C++ for
// host and device: the kernels of pf_power.hip call it, and a CPU test compiles it on its own (tests/cpu_emul/multipole_emul.cpp)
// against the numpy restatement (tests/np_multipoles.py).  The file that includes this is compiled without contraction.
//
//   mu^2        a / k2 with a = s_los^2, s_los the signed wavenumber on the axis of the line of sight, and k2 as in pf_power_k2
//   weights     L0 = 1;  L2 = (double)(3 a - k2) / (double)(2 k2);  L4 = (double)(35 a^2 - 30 a k2 + 3 k2^2) / (double)(8 k2^2): the
//               integers in 64 bits (below 2^50 for n <= 2048), each converted exactly, one division each.  k2 = 0: L2 = L4 = 0
//   terms       t L_l, one product, of the auto and the cross term of the mode (pf_matter_auto, pf_matter_cross)
//   sums        0 auto l0;  1, 2 auto l2 (the positive terms, the negated negative ones);  3, 4 auto l4;  5, 6 cross l0;  7, 8 cross
//               l2;  9, 10 cross l4.  A term of zero (k2 = 0 for l > 0) enters none: a mode adds to at most six of the eleven
#pragma once
#include <math.h>
#include <stdint.h>

#include "pf_matter_core.h"

#define PF_MULTIPOLE_HD PF_POWER_HD
#define PF_MULTIPOLE_NSUMS 11          // PF_MULTIPOLE_SUMS of pinfmax.h
#define PF_MULTIPOLE_NSUMS_AUTO 5      // ... of which the first five need no second spectrum

// the signed wavenumber on axis `los` of the mode (sx, sy, kz) of a half-spectrum, squared
PF_MULTIPOLE_HD unsigned int pf_multipole_a(int los, int sx, int sy, unsigned int kz) {
  return los == 0 ? (unsigned int)(sx * sx) : los == 1 ? (unsigned int)(sy * sy) : kz * kz;
}

PF_MULTIPOLE_HD void pf_multipole_weights(unsigned int a_, unsigned int k2_, double *L2, double *L4) {
  if (!k2_) { *L2 = 0.0; *L4 = 0.0; return; }
  const long long a = (long long)a_, k2 = (long long)k2_;
  *L2 = (double)(3 * a - k2) / (double)(2 * k2);
  *L4 = (double)(35 * a * a - 30 * a * k2 + 3 * k2 * k2) / (double)(8 * k2 * k2);
}

// the six signed terms of a mode: 0 auto l0, 1 auto l2, 2 auto l4, 3 cross l0, 4 cross l2, 5 cross l4
PF_MULTIPOLE_HD void pf_multipole_terms(double t_auto, double t_cross, double L2, double L4, double x[6]) {
  x[0] = t_auto; x[1] = t_auto * L2; x[2] = t_auto * L4;
  x[3] = t_cross; x[4] = t_cross * L2; x[5] = t_cross * L4;
}
// term k of value x != 0 enters, as |x|, ONE of the eleven sums: 2k - 1 where it is positive, 2k where it is negative (term 0 is
// never negative: sum 0).  A term of zero enters none
PF_MULTIPOLE_HD int pf_multipole_sum_of(int k, double x) { return k == 0 ? 0 : x > 0.0 ? 2 * k - 1 : 2 * k; }
