// power_emul.cpp -- pinocchio_amd/csrc/pf_power_core.h compiled for the host and run mode by mode on one thread: what pf_power.hip
// forms by workgroups and integer atomics -- the scan for the maxima, the fixed-point sums, the conversion -- as plain loops.  As a
// library (-DPOWER_EMUL_LIB) tests/test_power_cpu.py holds it against tests/np_power.py; as a program it reads the cases that test
// wrote and runs them under -fsanitize=address,undefined.
//
// A spectrum is a ky-slab [nyl][n (kx)][n/2+1][2] of doubles, rows y0 .. y0 + nyl - 1 (the layout of pf_debug_power_spectrum).
// A case in the file: int64 fb, n, y0, nyl, ns; then ns doubles (radii) and the slab.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/pinfmax.h"
#include "../../pinocchio_amd/csrc/pf_power_core.h"

typedef unsigned long long u64;

static double term_of(int fb, const double *e) {
  if (fb == 4) return pf_power_term<float>((float)e[0], (float)e[1]);
  return pf_power_term<double>(e[0], e[1]);
}

extern "C" int power_emul_bins(int n) { return pf_power_nbins(n); }

// shell, weight, k2 and term of every mode of the slab, in its own order
extern "C" int power_emul_modes(int fb, int n, int y0, int nyl, const double *spec, int *shell, int *weight, u64 *k2, double *term) {
  const int nzh = n / 2 + 1;
  size_t i = 0;
  unsigned int root = 0;
  for (int yl = 0; yl < nyl; yl++)
    for (int x = 0; x < n; x++)
      for (int z = 0; z < nzh; z++, i++) {
        k2[i] = pf_power_k2(x, y0 + yl, z, n);
        // the root as the device finds it: bit by bit for the first mode, from the root of the mode before for the others
        root = i ? pf_power_isqrt_near((unsigned int)k2[i], root) : pf_power_isqrt((unsigned int)k2[i]);
        if (root != pf_power_isqrt((unsigned int)k2[i])) return 3;
        shell[i] = pf_power_shell_of_root((unsigned int)k2[i], root);
        if (shell[i] != pf_power_shell(k2[i])) return 3;
        weight[i] = pf_power_weight(z, n);
        term[i] = term_of(fb, spec + 2 * i);
      }
  return 0;
}

static u64 bits_of(double x) { u64 b; memcpy(&b, &x, 8); return b; }
static double from_bits(u64 b) { double x; memcpy(&x, &b, 8); return x; }

// the whole call as the device runs it: maxima as integer maxima of the bit patterns, sums as limb counters
extern "C" int power_emul_run(int fb, int n, int y0, int nyl, const double *spec, int ns, const double *radius_cells, u64 *nmodes, u64 *k2sum, double *power,
                              double *variance, pf_power_info *info) {
  if ((fb != 4 && fb != 8) || n < 2 || (n & 1) || y0 < 0 || nyl < 1 || y0 + nyl > n || ns < 0 || ns > PF_MAX_SMOOTH) return 1;
  const int nzh = n / 2 + 1, nb = pf_power_nbins(n);
  const size_t count = (size_t)nyl * n * nzh;
  std::vector<int> shell(count), weight(count);
  std::vector<u64> k2(count);
  std::vector<double> term(count);
  power_emul_modes(fb, n, y0, nyl, spec, shell.data(), weight.data(), k2.data(), term.data());
  const double kf = 2.0 * 3.14159265358979323846 / (double)n;
  std::vector<double> a(ns);
  for (int r = 0; r < ns; r++) a[r] = (kf * kf) * (radius_cells[r] * radius_cells[r]);
  // the window tables of the device path: one per radius, entry j = exp(-(a j^2))
  std::vector<double> E((size_t)ns * nzh);
  for (int r = 0; r < ns; r++)
    for (int j = 0; j < nzh; j++) E[(size_t)r * nzh + j] = pf_power_window_entry(a[r], j);
  std::vector<int> ax(count), ay(count), az(count);
  {
    size_t i = 0;
    for (int yl = 0; yl < nyl; yl++)
      for (int x = 0; x < n; x++)
        for (int z = 0; z < nzh; z++, i++) { ax[i] = abs(pf_power_signed(x, n)); ay[i] = abs(pf_power_signed(y0 + yl, n)); az[i] = z; }
  }
  auto window = [&](double wt, int r, size_t i) { return pf_power_windowed(wt, E[(size_t)r * nzh + ax[i]], E[(size_t)r * nzh + ay[i]], E[(size_t)r * nzh + az[i]]); };
  std::vector<u64> smax(nb, 0), vmax(ns, 0), pl(4 * (size_t)nb, 0), vl(4 * (size_t)ns, 0);
  for (int b = 0; b < nb; b++) nmodes[b] = k2sum[b] = 0;
  info->modes = (u64)nyl * n * n; info->nonfinite = 0;
  for (size_t i = 0; i < count; i++) {
    const int b = shell[i];
    if (b < 0 || b >= nb) return 2;
    nmodes[b] += (u64)weight[i]; k2sum[b] += (u64)weight[i] * k2[i];
    if (!pf_power_finite(term[i])) { info->nonfinite += (u64)weight[i]; continue; }
    if (term[i] > 0.0 && bits_of(term[i]) > smax[b]) smax[b] = bits_of(term[i]);
    if (k2[i])
      for (int r = 0; r < ns; r++) {
        const double x = window(term[i], r, i);
        if (x > 0.0 && bits_of(x) > vmax[r]) vmax[r] = bits_of(x);
      }
  }
  for (size_t i = 0; i < count; i++) {
    if (!pf_power_finite(term[i]) || !(term[i] > 0.0)) continue;
    const int b = shell[i];
    const double wt = (double)weight[i] * term[i];
    uint32_t l[3];
    pf_power_limbs(wt, pf_power_exponent(from_bits(smax[b])), l);
    for (int k = 0; k < 3; k++) pl[4 * (size_t)b + k] += l[k];
    if (k2[i])
      for (int r = 0; r < ns; r++) {
        const double x = window(wt, r, i);
        if (x > 0.0) {
          pf_power_limbs(x, pf_power_exponent(from_bits(vmax[r])), l);
          for (int k = 0; k < 3; k++) vl[4 * (size_t)r + k] += l[k];
        }
      }
  }
  const double n3 = (double)n * (double)n * (double)n, n6 = n3 * n3;
  for (int b = 0; b < nb; b++) power[b] = smax[b] ? pf_power_from_limbs(&pl[4 * (size_t)b], 4, pf_power_exponent(from_bits(smax[b]))) / n6 : 0.0;
  for (int r = 0; r < ns; r++) variance[r] = vmax[r] ? pf_power_from_limbs(&vl[4 * (size_t)r], 4, pf_power_exponent(from_bits(vmax[r]))) / n6 : 0.0;
  return 0;
}

extern "C" int power_emul_sizes(size_t *s) {   // what the ABI test holds against ctypes
  s[0] = sizeof(pf_power_info); s[1] = offsetof(pf_power_info, modes); s[2] = offsetof(pf_power_info, nonfinite); s[3] = PF_MAX_SMOOTH;
  return 4;
}

#ifndef POWER_EMUL_LIB
// power_emul_san FILE
int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  long long head[5];
  int ncase = 0;
  while (fread(head, 8, 5, f) == 5) {
    const int fb = (int)head[0], n = (int)head[1], y0 = (int)head[2], nyl = (int)head[3], ns = (int)head[4];
    if (head[1] < 2 || head[1] > 256 || head[3] < 1 || head[3] > head[1] || head[4] < 0 || head[4] > PF_MAX_SMOOTH) { fprintf(stderr, "bad case header\n"); return 2; }
    const size_t count = (size_t)nyl * n * (n / 2 + 1);
    std::vector<double> radii(ns), spec(2 * count);   // exactly the sizes: a read beyond them is the sanitizer's to find
    if ((ns && fread(radii.data(), 8, ns, f) != (size_t)ns) || fread(spec.data(), 8, 2 * count, f) != 2 * count) { fprintf(stderr, "short case\n"); return 2; }
    const int nb = power_emul_bins(n);
    std::vector<u64> nm(nb), ks(nb);
    std::vector<double> pw(nb), var(ns);
    pf_power_info info;
    if (power_emul_run(fb, n, y0, nyl, spec.data(), ns, radii.data(), nm.data(), ks.data(), pw.data(), var.data(), &info)) return 2;
    u64 snm = 0, sks = 0;
    double sp = 0.0, sv = 0.0;
    for (int b = 0; b < nb; b++) { snm += nm[b]; sks += ks[b]; sp += pw[b]; }
    for (int r = 0; r < ns; r++) sv += var[r];
    printf("case %d: nmodes %llu k2sum %llu nonfinite %llu power %a variance %a\n", ncase++, snm, sks, info.nonfinite, sp, sv);
  }
  fclose(f);
  return 0;
}
#endif
