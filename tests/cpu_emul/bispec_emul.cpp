// bispec_emul.cpp -- pinocchio_amd/csrc/pf_bispec_core.h compiled for the host and run on one thread: what pf_bispec.hip forms by
// lanes, registers and integer atomics -- the k-bin of a mode, the list of closed triples, the term of a cell and the sum it enters,
// the fixed-point sums of a triple and of a pair -- as plain loops.  As a library (-DBISPEC_EMUL_LIB) tests/test_bispec_cpu.py holds
// it against tests/np_bispec.py; as a program it runs the sums on fields of its own under -fsanitize=address,undefined.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/pinfmax.h"
#include "../../pinocchio_amd/csrc/pf_bispec_core.h"

typedef unsigned long long u64;

extern "C" int bispec_emul_bins(size_t count, const u64 *k2, int kmin, int dk, int nk, int *bin) {
  if (pf_bispec_check(kmin, dk, nk, 0)) return 1;
  for (size_t i = 0; i < count; i++) {
    bin[i] = pf_bispec_bin(k2[i], kmin, dk, nk);
    for (int b = 0; b < nk; b++)   // the form the mask pass uses agrees with it
      if (pf_bispec_in_bin(k2[i], pf_bispec_edge2(kmin, dk, b), pf_bispec_edge2(kmin, dk, b + 1)) != (bin[i] == b)) return 2;
  }
  return 0;
}

// the number of closed triples; ijl (may be null): [nt][3]; -(the refusal of pf_bispec_check with n) where there is one
extern "C" int bispec_emul_triangles(int kmin, int dk, int nk, int n, int *ijl) {
  const int bad = pf_bispec_check(kmin, dk, nk, n);
  return bad ? -bad : pf_bispec_triangles(kmin, dk, nk, ijl);
}

// term and sum index of `count` triples of values
extern "C" int bispec_emul_terms(size_t count, const double *a, const double *b, const double *c, double *t, int *sum) {
  for (size_t i = 0; i < count; i++) { t[i] = pf_bispec_term(a[i], b[i], c[i]); sum[i] = pf_bispec_sum_of(t[i]); }
  return 0;
}

// the sums of nk fields of ncell finite doubles: parts [2][nt], pair [nk], maxima [nk], through the library's fixed point -- the
// exponent from the product of the maxima, three limbs per term, the counters carried by pf_power_from_limbs
extern "C" int bispec_emul_sums(size_t ncell, const double *f, int kmin, int dk, int nk, double *parts, double *pair, double *maxima) {
  if (pf_bispec_check(kmin, dk, nk, 0)) return 1;
  const int nt = pf_bispec_triangles(kmin, dk, nk, nullptr);
  std::vector<int> ijl(3 * (size_t)nt);
  pf_bispec_triangles(kmin, dk, nk, ijl.data());
  for (int i = 0; i < nk; i++) {
    maxima[i] = 0.0;
    for (size_t x = 0; x < ncell; x++) if (fabs(f[i * ncell + x]) > maxima[i]) maxima[i] = fabs(f[i * ncell + x]);
  }
  for (int t = 0; t < nt; t++) {
    const double *a = f + (size_t)ijl[3 * t] * ncell, *b = f + (size_t)ijl[3 * t + 1] * ncell, *c = f + (size_t)ijl[3 * t + 2] * ncell;
    const double m = pf_bispec_term(maxima[ijl[3 * t]], maxima[ijl[3 * t + 1]], maxima[ijl[3 * t + 2]]);
    const int e = m > 0.0 ? pf_power_exponent(m) : 0;
    u64 limbs[2][3] = {{0, 0, 0}, {0, 0, 0}};
    for (size_t x = 0; x < ncell; x++) {
      const double v = pf_bispec_term(a[x], b[x], c[x]);
      const int s = pf_bispec_sum_of(v);
      if (s < 0) continue;
      if (fabs(v) > m) return 2;   // (rounding is monotone: never)
      uint32_t l[3];
      pf_power_limbs(fabs(v), e, l);
      for (int k = 0; k < 3; k++) limbs[s][k] += l[k];
    }
    for (int s = 0; s < 2; s++) parts[(size_t)s * nt + t] = pf_power_from_limbs(limbs[s], 3, e);
  }
  for (int i = 0; i < nk; i++) {
    const double m = pf_bispec_pair(maxima[i]);
    const int e = m > 0.0 ? pf_power_exponent(m) : 0;
    u64 limbs[3] = {0, 0, 0};
    for (size_t x = 0; x < ncell; x++) {
      uint32_t l[3];
      pf_power_limbs(pf_bispec_pair(f[i * ncell + x]), e, l);
      for (int k = 0; k < 3; k++) limbs[k] += l[k];
    }
    pair[i] = pf_power_from_limbs(limbs, 3, e);
  }
  return 0;
}

extern "C" int bispec_emul_sizes(size_t *s) {   // what the ABI test holds against ctypes
  s[0] = PF_BISPEC_MAX_KBINS; s[1] = PF_BISPEC_KBINS; s[2] = sizeof(pf_bispec_info); s[3] = sizeof(pf_halo_info); s[4] = sizeof(pf_corr_info);
  return 5;
}

#ifndef BISPEC_EMUL_LIB
// bispec_emul_san NCELL KMIN DK NK SEED: the sums on fields of the generator below, arrays of exactly the sizes
int main(int argc, char **argv) {
  if (argc < 6) { fprintf(stderr, "usage: %s ncell kmin dk nk seed\n", argv[0]); return 2; }
  const size_t ncell = strtoull(argv[1], nullptr, 10);
  const int kmin = atoi(argv[2]), dk = atoi(argv[3]), nk = atoi(argv[4]);
  u64 state = strtoull(argv[5], nullptr, 10);
  if (pf_bispec_check(kmin, dk, nk, 0) || ncell < 1 || ncell > (1u << 20)) { fprintf(stderr, "bad arguments\n"); return 2; }
  const int nt = pf_bispec_triangles(kmin, dk, nk, nullptr);
  std::vector<int> ijl(3 * (size_t)nt), bin(ncell), sum(ncell);
  std::vector<double> f((size_t)nk * ncell), parts(2 * (size_t)nt), pair(nk), maxima(nk), t(ncell);
  std::vector<u64> k2(ncell);
  for (size_t i = 0; i < f.size(); i++) {   // a 64-bit LCG; the top bits as a signed value of a few binades
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    f[i] = ldexp((double)(long long)(state >> 11) - 4503599627370496.0, -40 - (int)((state >> 3) & 7));
  }
  for (size_t i = 0; i < ncell; i++) k2[i] = i;
  if (bispec_emul_triangles(kmin, dk, nk, 0, ijl.data()) != nt || bispec_emul_bins(ncell, k2.data(), kmin, dk, nk, bin.data()) ||
      bispec_emul_terms(ncell, f.data(), f.data() + (nk > 1 ? ncell : 0), f.data() + (size_t)(nk - 1) * ncell, t.data(), sum.data()) ||
      bispec_emul_sums(ncell, f.data(), kmin, dk, nk, parts.data(), pair.data(), maxima.data()))
    return 2;
  double psum = 0.0, qsum = 0.0;
  long long isum = 0, bsum = 0;
  for (double x : parts) psum += x;
  for (double x : pair) qsum += x;
  for (int x : ijl) isum += x;
  for (int x : bin) bsum += x;
  printf("triangles %d isum %lld bsum %lld psum %a qsum %a\n", nt, isum, bsum, psum, qsum);
  return 0;
}
#endif
