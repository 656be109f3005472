// pf_bispec_core.h -- the integer side and the one term of the bispectrum estimator (include/pinfmax.h: pf_halo_bispectrum): the k-bin
// of a mode, which ordered triples of bins can close a triangle, the term of a cell and the sum it enters.  Plain C++ for host and
// device: the kernels of pf_bispec.hip call it, and a CPU test compiles it on its own (tests/cpu_emul/bispec_emul.cpp) against the
// numpy restatement (tests/np_bispec.py).  The file that includes this is compiled without contraction.
//
//   k-bins     nk linear bins in integer units of the fundamental: bin i takes (kmin + i dk)^2 <= k2 < (kmin + (i + 1) dk)^2, k2 the
//              exact integer of pf_power_k2; no square root anywhere.  kmax = kmin + nk dk, and 3 kmax <= n keeps every component of
//              k1 + k2 + k3 below n in magnitude: a sum over cells of three band-limited fields then closes true triangles alone
//   triples    i <= j <= l can close when the largest side is below the sum of the other two somewhere in the bins: the smallest
//              |k| of bin l, kmin + l dk, against the supremum of |k1| + |k2|, 2 kmin + (i + j + 2) dk.  For a pair (i, j) the closed
//              l are the run j .. pf_bispec_last(i, j); the list is lexicographic in (i, j, l)
//   term       t = (a b) c of the cell's three values widened to double, each product rounded once; |t| enters the positive sum
//              (0) or the negative one (1) of the triple, a term of zero neither.  With M = (M_i M_j) M_l of the fields' largest
//              |values| formed the same way, |t| <= M, since rounding is monotone: M gives the exponent of the fixed point
//              (pf_power_core.h) without a pass over the terms
#pragma once
#include <math.h>
#include <stdint.h>

#include "pf_power_core.h"

#define PF_BISPEC_HD PF_POWER_HD
#define PF_BISPEC_KBINS 32   // PF_BISPEC_MAX_KBINS of pinfmax.h

// 0: fine; 1 kmin, 2 dk, 3 nk out of range; 4: 3 kmax > n (n <= 0: not checked)
PF_BISPEC_HD int pf_bispec_check(int kmin, int dk, int nk, int n) {
  if (kmin < 1 || kmin > 4096) return 1;
  if (dk < 1 || dk > 4096) return 2;
  if (nk < 1 || nk > PF_BISPEC_KBINS) return 3;
  if (n > 0 && 3ll * ((long long)kmin + (long long)nk * dk) > (long long)n) return 4;
  return 0;
}

// the edges of bin i as squares
PF_BISPEC_HD unsigned long long pf_bispec_edge2(int kmin, int dk, int i) {
  const unsigned long long e = (unsigned long long)kmin + (unsigned long long)i * (unsigned long long)dk;
  return e * e;
}
PF_BISPEC_HD bool pf_bispec_in_bin(unsigned long long k2, unsigned long long lo2, unsigned long long hi2) { return k2 >= lo2 && k2 < hi2; }
// the bin of k2, -1 for none
PF_BISPEC_HD int pf_bispec_bin(unsigned long long k2, int kmin, int dk, int nk) {
  if (k2 < pf_bispec_edge2(kmin, dk, 0)) return -1;
  for (int i = 0; i < nk; i++)
    if (k2 < pf_bispec_edge2(kmin, dk, i + 1)) return i;
  return -1;
}

PF_BISPEC_HD bool pf_bispec_closed(int kmin, int dk, int i, int j, int l) {
  return (long long)kmin + (long long)l * dk < 2ll * kmin + ((long long)i + j + 2) * dk;
}
// the last l >= j of the pair (i, j), i <= j < nk, that closes ((i, j, j) always does)
PF_BISPEC_HD int pf_bispec_last(int kmin, int dk, int nk, int i, int j) {
  int l = j;
  while (l + 1 < nk && pf_bispec_closed(kmin, dk, i, j, l + 1)) l++;
  return l;
}
// the closed triples in lexicographic order -> their number; ijl (may be null): [nt][3]
PF_BISPEC_HD int pf_bispec_triangles(int kmin, int dk, int nk, int *ijl) {
  int nt = 0;
  for (int i = 0; i < nk; i++)
    for (int j = i; j < nk; j++) {
      const int last = pf_bispec_last(kmin, dk, nk, i, j);
      for (int l = j; l <= last; l++, nt++)
        if (ijl) { ijl[3 * nt] = i; ijl[3 * nt + 1] = j; ijl[3 * nt + 2] = l; }
    }
  return nt;
}

PF_BISPEC_HD double pf_bispec_term(double a, double b, double c) {
  const double ab = a * b;
  return ab * c;
}
PF_BISPEC_HD double pf_bispec_pair(double a) { return a * a; }
// the sum a term enters: 0 the positive terms, 1 the negated negative ones, -1 none
PF_BISPEC_HD int pf_bispec_sum_of(double t) { return t > 0.0 ? 0 : t < 0.0 ? 1 : -1; }

// the element of the mask pass for a mode inside the bin: one part of the mode times the window factor (c < 0: none), rounded once
PF_BISPEC_HD double pf_bispec_masked(double part, double c) { return c < 0.0 ? part : part * c; }
