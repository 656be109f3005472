// matter_emul.cpp -- pinocchio_amd/csrc/pf_matter_core.h compiled for the host and run particle by particle and mode by mode on one
// thread: what pf_matter.hip forms by lanes and integer atomics -- the deposit, the counters of the contrast pass, the scan for the
// maxima, the fixed-point sums, the conversion -- as plain loops.  As a library (-DMATTER_EMUL_LIB) tests/test_matter_cpu.py holds it
// against tests/np_matter.py; as a program it reads the cases that test wrote and runs them under -fsanitize=address,undefined.
//
// Columns are [12][n^3] PRODFLOATs of pb bytes; a spectrum is a ky-slab [nyl][n (kx)][n/2+1][2] of doubles.
// A case in the file: int64 kind (0 deposit, 1 shells).  Deposit: int64 pb, n, flags, has_weight; 4 doubles; the columns.
// Shells: int64 fb, n, y0, nyl, flags, has_lin; the slab(s).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/pinfmax.h"
#include "../../pinocchio_amd/csrc/pf_matter_core.h"

typedef unsigned long long u64;

template <class T> static void deposit_t(int n, const T *col, int flags, const double *w, u64 *grid, pf_matter_info *info) {
  const size_t nc = (size_t)n * n * n;
  for (size_t i = 0; i < nc; i++) {
    const int q[3] = {(int)(i / ((size_t)n * n)), (int)(i / n % n), (int)(i % n)};
    T pos[3];
    for (int j = 0; j < 3; j++) {
      T v[4];
      for (int o = 0; o < 4; o++) v[o] = pf_matter_column<T>(col[(size_t)(3 * o + j) * nc + i], w, o);
      pos[j] = pf_matter_pos<T>(q[j], n, v[0], v[1], v[2], v[3]);
    }
    const int cls = pf_matter_class<T>(pos, n);
    if (cls == 1) { info->nonfinite++; continue; }
    if (cls == 2) { info->outside++; continue; }
    info->deposited++;
    if (flags & PF_MATTER_NGP) {
      grid[((size_t)pf_matter_ngp_axis<T>(pos[0], n) * n + pf_matter_ngp_axis<T>(pos[1], n)) * n + pf_matter_ngp_axis<T>(pos[2], n)] += PF_MATTER_ONE;
      continue;
    }
    int cell[3][2];
    uint32_t wt[3][2];
    for (int j = 0; j < 3; j++) pf_matter_cic_axis<T>(pos[j], n, cell[j], wt[j]);
    for (int a = 0; a < 2; a++)
      for (int b = 0; b < 2; b++)
        for (int c = 0; c < 2; c++) grid[((size_t)cell[0][a] * n + cell[1][b]) * n + cell[2][c]] += (u64)wt[0][a] * wt[1][b] * wt[2][c];
  }
}

extern "C" int matter_emul_deposit(int pb, int n, const void *vel12, int flags, const double *weight, u64 *grid, pf_matter_info *info) {
  if ((pb != 4 && pb != 8) || n < 2) return 1;
  const size_t nc = (size_t)n * n * n;
  memset(info, 0, sizeof(*info));
  for (size_t i = 0; i < nc; i++) grid[i] = 0;
  if (pb == 8) deposit_t<double>(n, (const double *)vel12, flags, weight, grid, info);
  else deposit_t<float>(n, (const float *)vel12, flags, weight, grid, info);
  for (size_t i = 0; i < nc; i++) {
    info->empty_cells += grid[i] == 0;
    if (grid[i] > info->max_cell) info->max_cell = grid[i];
    info->sum_hi32 += grid[i] >> 32; info->sum_lo32 += grid[i] & 0xffffffffull;
  }
  return 0;
}

extern "C" int matter_emul_deconv(int n, int p, double *table) {
  for (int j = 0; j <= n / 2; j++) table[j] = pf_matter_deconv_entry(j, n, p);
  return 0;
}

static u64 bits_of(double x) { u64 b; memcpy(&b, &x, 8); return b; }
static double from_bits(u64 b) { double x; memcpy(&x, &b, 8); return x; }
static double widen(int fb, double x) { return fb == 4 ? (double)(float)x : x; }

// parts: [2 nb], the positive and the negated negative cross sums over N^6 (may be null)
extern "C" int matter_emul_shells(int fb, int n, int y0, int nyl, const double *spec_m, const double *spec_lin, int flags, u64 *nmodes, u64 *k2sum, double *power,
                                  double *cross, double *parts, pf_matter_info *info) {
  if ((fb != 4 && fb != 8) || n < 2 || (n & 1) || y0 < 0 || nyl < 1 || y0 + nyl > n) return 1;
  const int nzh = n / 2 + 1, nb = pf_power_nbins(n);
  const size_t count = (size_t)nyl * n * nzh;
  std::vector<double> C(nzh);
  const bool dec = (flags & PF_MATTER_DECONVOLVE) != 0;
  for (int j = 0; j < nzh; j++) C[j] = pf_matter_deconv_entry(j, n, (flags & PF_MATTER_NGP) ? 1 : 2);
  std::vector<double> ta(count), tc(count, 0.0);
  std::vector<int> shell(count), weight(count);
  memset(info, 0, sizeof(*info));
  info->modes = (u64)nyl * n * n;
  for (int b = 0; b < nb; b++) nmodes[b] = k2sum[b] = 0;
  size_t i = 0;
  for (int yl = 0; yl < nyl; yl++)
    for (int x = 0; x < n; x++)
      for (int z = 0; z < nzh; z++, i++) {
        const u64 k2 = pf_power_k2(x, y0 + yl, z, n);
        shell[i] = pf_power_shell(k2); weight[i] = pf_power_weight(z, n);
        if (shell[i] < 0 || shell[i] >= nb) return 2;
        const double c = dec ? pf_matter_deconv(C[abs(pf_power_signed(x, n))] * C[abs(pf_power_signed(y0 + yl, n))], 1.0, C[z]) : -1.0;
        const double a = widen(fb, spec_m[2 * i]), b = widen(fb, spec_m[2 * i + 1]);
        ta[i] = pf_matter_auto(a, b, c);
        if (spec_lin) tc[i] = pf_matter_cross(a, b, widen(fb, spec_lin[2 * i]), widen(fb, spec_lin[2 * i + 1]), c);
        nmodes[shell[i]] += (u64)weight[i]; k2sum[shell[i]] += (u64)weight[i] * k2;
        if (!(pf_power_finite(ta[i]) && pf_power_finite(tc[i]))) { info->nonfinite_modes += (u64)weight[i]; shell[i] = -1; }
      }
  std::vector<double> sum(3 * (size_t)nb, 0.0);
  for (int which = 0; which < (spec_lin ? 3 : 1); which++) {
    std::vector<u64> smax(nb, 0), pl(4 * (size_t)nb, 0);
    for (i = 0; i < count; i++) {
      if (shell[i] < 0) continue;
      const double t = pf_matter_part(which, ta[i], tc[i]);
      if (t > 0.0 && bits_of(t) > smax[shell[i]]) smax[shell[i]] = bits_of(t);
    }
    for (i = 0; i < count; i++) {
      if (shell[i] < 0) continue;
      const double t = pf_matter_part(which, ta[i], tc[i]);
      if (!(t > 0.0)) continue;
      uint32_t l[3];
      pf_power_limbs((double)weight[i] * t, pf_power_exponent(from_bits(smax[shell[i]])), l);
      for (int k = 0; k < 3; k++) pl[4 * (size_t)shell[i] + k] += l[k];
    }
    for (int b = 0; b < nb; b++) sum[(size_t)which * nb + b] = smax[b] ? pf_power_from_limbs(&pl[4 * (size_t)b], 4, pf_power_exponent(from_bits(smax[b]))) : 0.0;
  }
  const double n3 = (double)n * (double)n * (double)n, n6 = n3 * n3;
  for (int b = 0; b < nb; b++) {
    power[b] = sum[b] / n6;
    if (cross) cross[b] = (sum[nb + b] - sum[2 * (size_t)nb + b]) / n6;
    if (parts) { parts[b] = sum[nb + b] / n6; parts[nb + b] = sum[2 * (size_t)nb + b] / n6; }
  }
  return 0;
}

extern "C" int matter_emul_sizes(size_t *s) {   // what the ABI test holds against ctypes
  s[0] = sizeof(pf_matter_info);
  s[1] = offsetof(pf_matter_info, deposited); s[2] = offsetof(pf_matter_info, nonfinite); s[3] = offsetof(pf_matter_info, outside);
  s[4] = offsetof(pf_matter_info, empty_cells); s[5] = offsetof(pf_matter_info, max_cell); s[6] = offsetof(pf_matter_info, sum_hi32);
  s[7] = offsetof(pf_matter_info, sum_lo32); s[8] = offsetof(pf_matter_info, modes); s[9] = offsetof(pf_matter_info, nonfinite_modes);
  s[10] = PF_MATTER_NGP; s[11] = PF_MATTER_DECONVOLVE;
  return 12;
}

#ifndef MATTER_EMUL_LIB
// matter_emul_san FILE
int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  long long kind;
  int ncase = 0;
  while (fread(&kind, 8, 1, f) == 1) {
    if (kind == 0) {
      long long head[4];
      double w[4];
      if (fread(head, 8, 4, f) != 4 || fread(w, 8, 4, f) != 4) { fprintf(stderr, "short case\n"); return 2; }
      const int pb = (int)head[0], n = (int)head[1], flags = (int)head[2];
      if ((pb != 4 && pb != 8) || head[1] < 2 || head[1] > 64) { fprintf(stderr, "bad case header\n"); return 2; }
      const size_t nc = (size_t)n * n * n;
      std::vector<char> col(12 * nc * pb);   // exactly the sizes: a read or write beyond them is the sanitizer's to find
      std::vector<u64> grid(nc);
      if (fread(col.data(), 1, col.size(), f) != col.size()) { fprintf(stderr, "short case\n"); return 2; }
      pf_matter_info info;
      if (matter_emul_deposit(pb, n, col.data(), flags, head[3] ? w : nullptr, grid.data(), &info)) return 2;
      u64 h = 1469598103934665603ull;   // FNV-1a of the grid's words
      for (size_t i = 0; i < nc; i++) { h ^= grid[i]; h *= 1099511628211ull; }
      printf("case %d: deposited %llu nonfinite %llu outside %llu empty %llu max %llu hi %llu lo %llu hash %llu\n", ncase++, info.deposited, info.nonfinite, info.outside,
             info.empty_cells, info.max_cell, info.sum_hi32, info.sum_lo32, h);
    } else if (kind == 1) {
      long long head[6];
      if (fread(head, 8, 6, f) != 6) { fprintf(stderr, "short case\n"); return 2; }
      const int fb = (int)head[0], n = (int)head[1], y0 = (int)head[2], nyl = (int)head[3], flags = (int)head[4];
      if (head[1] < 2 || head[1] > 256 || head[3] < 1 || head[3] > head[1]) { fprintf(stderr, "bad case header\n"); return 2; }
      const size_t count = (size_t)nyl * n * (n / 2 + 1);
      std::vector<double> m(2 * count), l(head[5] ? 2 * count : 0);
      if (fread(m.data(), 8, m.size(), f) != m.size() || (l.size() && fread(l.data(), 8, l.size(), f) != l.size())) { fprintf(stderr, "short case\n"); return 2; }
      const int nb = pf_power_nbins(n);
      std::vector<u64> nm(nb), ks(nb);
      std::vector<double> pw(nb), cr(nb, 0.0);
      pf_matter_info info;
      if (matter_emul_shells(fb, n, y0, nyl, m.data(), l.size() ? l.data() : nullptr, flags, nm.data(), ks.data(), pw.data(), l.size() ? cr.data() : nullptr, nullptr, &info))
        return 2;
      u64 snm = 0, sks = 0;
      double sp = 0.0, sc = 0.0;
      for (int b = 0; b < nb; b++) { snm += nm[b]; sks += ks[b]; sp += pw[b]; sc += cr[b]; }
      printf("case %d: nmodes %llu k2sum %llu nonfinite %llu power %a cross %a\n", ncase++, snm, sks, info.nonfinite_modes, sp, sc);
    } else { fprintf(stderr, "bad case kind\n"); return 2; }
  }
  fclose(f);
  return 0;
}
#endif
