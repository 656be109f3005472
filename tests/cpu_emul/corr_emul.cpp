// corr_emul.cpp -- pinocchio_amd/csrc/pf_corr_core.h compiled for the host and run on one thread: what pf_power.hip forms by lanes,
// LDS tables and integer atomics -- the shell and the Legendre weights of a cell, the sum each of its terms enters, the six
// fixed-point sums of a shell, the element of the form pass -- as plain loops.  As a library (-DCORR_EMUL_LIB) tests/test_corr_cpu.py
// holds it against tests/np_corr.py; as a program it runs the shell pass on a field of its own under -fsanitize=address,undefined.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/pinfmax.h"
#include "../../pinocchio_amd/csrc/pf_corr_core.h"

typedef unsigned long long u64;

static bool bad_window(int n, int los, int x0, int nxl) { return n < 2 || (n & 1) || n > 2048 || los < 0 || los > 2 || x0 < 0 || nxl < 1 || x0 + nxl > n; }

// of every cell of the planes [x0, x0 + nxl): r2, shell, L2, L4
extern "C" int corr_emul_cells(int n, int los, int x0, int nxl, u64 *r2, int *shell, double *L2, double *L4) {
  if (bad_window(n, los, x0, nxl)) return 1;
  for (int x = 0; x < nxl; x++)
    for (int y = 0; y < n; y++)
      for (int z = 0; z < n; z++) {
        const int sx = pf_power_signed(x + x0, n), sy = pf_power_signed(y, n), sz = pf_power_signed(z, n);
        const size_t i = ((size_t)x * n + y) * n + z;
        const unsigned int q = pf_corr_r2(sx, sy, sz);
        r2[i] = q; shell[i] = pf_power_shell(q);
        pf_multipole_weights(pf_corr_a(los, sx, sy, sz), q, &L2[i], &L4[i]);
      }
  return 0;
}

// index [3][cells]: the sum term k of a cell enters, -1 for none
extern "C" int corr_emul_index(int n, int los, int x0, int nxl, const double *real, int *index) {
  if (bad_window(n, los, x0, nxl)) return 1;
  const size_t nc = (size_t)nxl * n * n;
  for (int x = 0; x < nxl; x++)
    for (int y = 0; y < n; y++)
      for (int z = 0; z < n; z++) {
        const int sx = pf_power_signed(x + x0, n), sy = pf_power_signed(y, n), sz = pf_power_signed(z, n);
        const size_t i = ((size_t)x * n + y) * n + z;
        double L2, L4, t[PF_CORR_NORDERS];
        pf_multipole_weights(pf_corr_a(los, sx, sy, sz), pf_corr_r2(sx, sy, sz), &L2, &L4);
        pf_corr_terms(real[i], L2, L4, t);
        for (int k = 0; k < PF_CORR_NORDERS; k++) index[k * nc + i] = (pf_power_finite(real[i]) && fabs(t[k]) > 0.0) ? pf_corr_sum_of(k, t[k]) : -1;
      }
  return 0;
}

// the shell pass on the planes of a real field of doubles [nxl][n][n]: ncells, r2sum, parts [6][nb] through the library's own fixed
// point -- the largest term of a shell and sum first, then the limbs under its exponent
extern "C" int corr_emul_shells(int n, int los, int x0, int nxl, const double *real, u64 *ncells, u64 *r2sum, double *parts, u64 *nonfinite) {
  if (bad_window(n, los, x0, nxl)) return 1;
  const int nb = pf_power_nbins(n);
  std::vector<double> mx((size_t)PF_CORR_NSUMS * nb, 0.0);
  std::vector<u64> limbs((size_t)PF_CORR_NSUMS * nb * 4, 0);
  for (int b = 0; b < nb; b++) ncells[b] = r2sum[b] = 0;
  *nonfinite = 0;
  for (int pass = 0; pass < 2; pass++)
    for (int x = 0; x < nxl; x++)
      for (int y = 0; y < n; y++)
        for (int z = 0; z < n; z++) {
          const int sx = pf_power_signed(x + x0, n), sy = pf_power_signed(y, n), sz = pf_power_signed(z, n);
          const unsigned int q = pf_corr_r2(sx, sy, sz);
          const int b = pf_power_shell(q);
          const double v = real[((size_t)x * n + y) * n + z];
          const bool fin = pf_power_finite(v);
          if (pass == 0) {
            ncells[b]++; r2sum[b] += q;
            if (!fin) ++*nonfinite;
          }
          if (!fin) continue;
          double L2, L4, t[PF_CORR_NORDERS];
          pf_multipole_weights(pf_corr_a(los, sx, sy, sz), q, &L2, &L4);
          pf_corr_terms(v, L2, L4, t);
          for (int k = 0; k < PF_CORR_NORDERS; k++) {
            const double m = fabs(t[k]);
            if (!(m > 0.0)) continue;
            const int s = pf_corr_sum_of(k, t[k]);
            double &top = mx[(size_t)s * nb + b];
            if (pass == 0) { if (m > top) top = m; continue; }
            uint32_t l[3];
            pf_power_limbs(m, pf_power_exponent(top), l);
            for (int i = 0; i < 3; i++) limbs[((size_t)s * nb + b) * 4 + i] += l[i];
          }
        }
  for (int s = 0; s < PF_CORR_NSUMS; s++)
    for (int b = 0; b < nb; b++) {
      const double top = mx[(size_t)s * nb + b];
      parts[(size_t)s * nb + b] = top > 0.0 ? pf_power_from_limbs(&limbs[((size_t)s * nb + b) * 4], 4, pf_power_exponent(top)) : 0.0;
    }
  return 0;
}

// the element of the form pass for `count` terms: out = t / n3 or zero, bad = the term is not finite
extern "C" int corr_emul_form(size_t count, const double *t, const unsigned int *k2, double n3, double *out, int *bad) {
  for (size_t i = 0; i < count; i++) {
    bool b;
    out[i] = pf_corr_form(t[i], k2[i], n3, &b);
    bad[i] = b ? 1 : 0;
  }
  return 0;
}

extern "C" int corr_emul_sizes(size_t *s) {   // what the ABI test holds against ctypes
  s[0] = PF_CORR_ORDERS; s[1] = PF_CORR_SUMS; s[2] = PF_CORR_NORDERS; s[3] = PF_CORR_NSUMS; s[4] = sizeof(pf_corr_info); s[5] = sizeof(pf_halo_info);
  return 6;
}

#ifndef CORR_EMUL_LIB
// corr_emul_san N LOS X0 NXL SEED: the shell pass on a field of the generator below, arrays of exactly the sizes
int main(int argc, char **argv) {
  if (argc < 6) { fprintf(stderr, "usage: %s n los x0 nxl seed\n", argv[0]); return 2; }
  const int n = atoi(argv[1]), los = atoi(argv[2]), x0 = atoi(argv[3]), nxl = atoi(argv[4]);
  u64 state = strtoull(argv[5], nullptr, 10);
  if (bad_window(n, los, x0, nxl) || n > 64) { fprintf(stderr, "bad arguments\n"); return 2; }
  const size_t nc = (size_t)nxl * n * n, nb = (size_t)pf_power_nbins(n);
  std::vector<double> real(nc), parts(PF_CORR_NSUMS * nb), L2(nc), L4(nc);
  std::vector<u64> ncells(nb), r2sum(nb), r2(nc);
  std::vector<int> shell(nc), index(PF_CORR_NORDERS * nc);
  for (size_t i = 0; i < nc; i++) {   // a 64-bit LCG; the top bits as a signed value of a few binades
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    real[i] = ldexp((double)(long long)(state >> 11) - 4503599627370496.0, -40 - (int)((state >> 3) & 7));
  }
  real[nc / 2] = NAN;
  u64 nonfin;
  if (corr_emul_cells(n, los, x0, nxl, r2.data(), shell.data(), L2.data(), L4.data()) || corr_emul_index(n, los, x0, nxl, real.data(), index.data()) ||
      corr_emul_shells(n, los, x0, nxl, real.data(), ncells.data(), r2sum.data(), parts.data(), &nonfin))
    return 2;
  double psum = 0.0, lsum = 0.0;
  u64 cells = 0;
  long long isum = 0;
  for (double x : parts) psum += x;
  for (size_t i = 0; i < nc; i++) lsum += L2[i] + L4[i];
  for (u64 x : ncells) cells += x;
  for (int x : index) isum += x;
  printf("cells %llu nonfinite %llu isum %lld psum %a lsum %a\n", cells, nonfin, isum, psum, lsum);
  return 0;
}
#endif
