// halo_emul.cpp -- pinocchio_amd/csrc/pf_halo_core.h compiled for the host and run halo by halo on one thread: what pf_halo.hip forms
// by lanes, ballots and integer atomics -- the selection with its sums, the deposit, the counters of the contrast pass, the contrast
// -- as plain loops.  As a library (-DHALO_EMUL_LIB) tests/test_halo_cpu.py holds it against tests/np_halo.py; as a program it reads
// the cases that test wrote and runs them under -fsanitize=address,undefined.
//
// A case in the file: int64 n, x0, nxl, flags, count, lo, hi; double scale; count x 3 doubles; count ints.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/pinfmax.h"
#include "../../pinocchio_amd/csrc/pf_halo_core.h"

typedef unsigned long long u64;

// 0 done; 3: the weights of the range add up to 2^34 or more (the list-derived counters are filled, the grid is untouched)
extern "C" int halo_emul_deposit(int n, int x0, int nxl, int flags, size_t count, const double *pos, double scale, const int *mass, int lo, int hi, u64 *grid,
                                 pf_halo_info *info) {
  if (n < 2 || x0 < 0 || nxl < 1 || x0 + nxl > n || lo < 1 || hi < lo) return 1;
  const bool mw = (flags & PF_HALO_MASS_WEIGHT) != 0;
  memset(info, 0, sizeof(*info));
  u64 w2hi = 0, w2lo = 0;
  for (size_t i = 0; i < count; i++) {
    if (!pf_halo_in_range(mass[i], lo, hi)) continue;
    double p[3];
    for (int j = 0; j < 3; j++) p[j] = pf_halo_pos(pos[3 * i + j], scale, n);
    const int cls = pf_halo_class(p, n);
    if (cls == 1) { info->nonfinite++; continue; }
    if (cls == 2) { info->outside++; continue; }
    const u64 W = pf_halo_weight(mass[i], mw), W2 = W * W;
    info->selected++; info->weight_sum += W;
    w2hi += W2 >> 32; w2lo += W2 & 0xffffffffull;
  }
  const u64 low = w2lo + (w2hi << 32);
  info->weight2_lo = low; info->weight2_hi = (w2hi >> 32) + (low < w2lo ? 1 : 0);
  if (info->weight_sum >= PF_HALO_WEIGHT_LIMIT) return 3;
  const size_t nc = (size_t)nxl * n * n;
  for (size_t i = 0; i < nc; i++) grid[i] = 0;
  for (size_t i = 0; i < count; i++) {
    if (!pf_halo_in_range(mass[i], lo, hi)) continue;
    double p[3];
    for (int j = 0; j < 3; j++) p[j] = pf_halo_pos(pos[3 * i + j], scale, n);
    if (pf_halo_class(p, n) != 0) continue;
    const u64 W = pf_halo_weight(mass[i], mw);
    if (flags & PF_HALO_NGP) {
      const int lx = pf_halo_plane(pf_halo_ngp_axis(p[0], n), x0, nxl);
      if (lx >= 0) grid[((size_t)lx * n + pf_halo_ngp_axis(p[1], n)) * n + pf_halo_ngp_axis(p[2], n)] += W << PF_HALO_SHIFT;
      continue;
    }
    int cell[3][2];
    uint32_t wt[3][2];
    for (int j = 0; j < 3; j++) pf_halo_cic_axis(p[j], n, cell[j], wt[j]);
    for (int a = 0; a < 2; a++) {
      const int lx = pf_halo_plane(cell[0][a], x0, nxl);
      if (lx < 0) continue;
      for (int b = 0; b < 2; b++)
        for (int c = 0; c < 2; c++) grid[((size_t)lx * n + cell[1][b]) * n + cell[2][c]] += W * ((u64)wt[0][a] * wt[1][b]) * wt[2][c];
    }
  }
  for (size_t i = 0; i < nc; i++) {
    info->empty_cells += grid[i] == 0;
    if (grid[i] > info->max_cell) info->max_cell = grid[i];
  }
  return 0;
}

// delta of ncell cells as the field holds it (fb 4: rounded to float), widened to double
extern "C" int halo_emul_contrast(int n, size_t ncell, const u64 *grid, u64 weight_sum, int fb, double *out) {
  if ((fb != 4 && fb != 8) || !weight_sum) return 1;
  const double mean = pf_halo_mean(weight_sum, n);
  for (size_t i = 0; i < ncell; i++) {
    const double d = pf_halo_contrast(grid[i], mean);
    out[i] = fb == 4 ? (double)(float)d : d;
  }
  return 0;
}

extern "C" int halo_emul_sizes(size_t *s) {   // what the ABI test holds against ctypes
  s[0] = sizeof(pf_halo_info);
  s[1] = offsetof(pf_halo_info, selected); s[2] = offsetof(pf_halo_info, weight_sum); s[3] = offsetof(pf_halo_info, weight2_hi);
  s[4] = offsetof(pf_halo_info, weight2_lo); s[5] = offsetof(pf_halo_info, nonfinite); s[6] = offsetof(pf_halo_info, outside);
  s[7] = offsetof(pf_halo_info, empty_cells); s[8] = offsetof(pf_halo_info, max_cell); s[9] = offsetof(pf_halo_info, modes);
  s[10] = offsetof(pf_halo_info, nonfinite_modes);
  s[11] = PF_HALO_NGP; s[12] = PF_HALO_DECONVOLVE; s[13] = PF_HALO_MASS_WEIGHT; s[14] = PF_HALO_MAX_BINS;
  return 15;
}

#ifndef HALO_EMUL_LIB
// halo_emul_san FILE
int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  long long head[7];
  int ncase = 0;
  while (fread(head, 8, 7, f) == 7) {
    double scale;
    if (fread(&scale, 8, 1, f) != 1) { fprintf(stderr, "short case\n"); return 2; }
    const int n = (int)head[0], x0 = (int)head[1], nxl = (int)head[2], flags = (int)head[3], lo = (int)head[5], hi = (int)head[6];
    const size_t count = (size_t)head[4];
    if (head[0] < 2 || head[0] > 64 || head[4] < 0 || head[4] > 100000 || x0 < 0 || nxl < 1 || x0 + nxl > n) { fprintf(stderr, "bad case header\n"); return 2; }
    std::vector<double> pos(3 * count);   // exactly the sizes: a read or write beyond them is the sanitizer's to find
    std::vector<int> mass(count);
    std::vector<u64> grid((size_t)nxl * n * n);
    if (fread(pos.data(), 8, pos.size(), f) != pos.size() || fread(mass.data(), 4, count, f) != count) { fprintf(stderr, "short case\n"); return 2; }
    pf_halo_info info;
    const int rc = halo_emul_deposit(n, x0, nxl, flags, count, pos.data(), scale, mass.data(), lo, hi, grid.data(), &info);
    if (rc != 0 && rc != 3) return 2;
    u64 h = 1469598103934665603ull;   // FNV-1a of the grid's words
    for (size_t i = 0; rc == 0 && i < grid.size(); i++) { h ^= grid[i]; h *= 1099511628211ull; }
    std::vector<double> d(grid.size());
    double dsum = 0.0;
    if (rc == 0 && info.weight_sum) {
      if (halo_emul_contrast(n, grid.size(), grid.data(), info.weight_sum, 4, d.data())) return 2;
      for (double x : d) dsum += x;
    }
    printf("case %d: rc %d selected %llu weight_sum %llu weight2_hi %llu weight2_lo %llu nonfinite %llu outside %llu empty %llu max %llu hash %llu dsum %a\n", ncase++, rc,
           info.selected, info.weight_sum, info.weight2_hi, info.weight2_lo, info.nonfinite, info.outside, info.empty_cells, info.max_cell, h, dsum);
  }
  fclose(f);
  return 0;
}
#endif
