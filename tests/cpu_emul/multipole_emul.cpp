// multipole_emul.cpp -- pinocchio_amd/csrc/pf_multipole_core.h and the redshift-space position of pf_halo_core.h compiled for the
// host and run on one thread: what pf_halo.hip and pf_power.hip form by lanes, LDS tables and integer atomics -- the moved position,
// the deposit, the Legendre weights of a mode, the eleven fixed-point sums of a shell -- as plain loops.  As a library
// (-DMULTIPOLE_EMUL_LIB) tests/test_multipoles_cpu.py holds it against tests/np_multipoles.py; as a program it reads the cases that
// test wrote and runs them under -fsanitize=address,undefined.
//
// A case in the file: int64 n, x0, nxl, flags, count, lo, hi, los, has_vel; double scale, vfac; count x 3 doubles (pos); count x 3
// doubles (vel, only with has_vel); count ints.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/pinfmax.h"
#include "../../pinocchio_amd/csrc/pf_halo_core.h"
#include "../../pinocchio_amd/csrc/pf_multipole_core.h"

typedef unsigned long long u64;

static void position_of(size_t i, const double *pos, const double *vel, double scale, double vfac, int los, int n, double p[3]) {
  for (int j = 0; j < 3; j++) p[j] = pf_halo_pos_rsd(pos[3 * i + j], (vel && j == los) ? vel + 3 * i + j : nullptr, vfac, scale, n);
}

extern "C" int multipole_emul_positions(int n, size_t count, const double *pos, const double *vel, double scale, double vfac, int los, double *out, int *cls) {
  if (los < 0 || los > 2) return 1;
  for (size_t i = 0; i < count; i++) {
    position_of(i, pos, vel, scale, vfac, los, n, out + 3 * i);
    cls[i] = pf_halo_class(out + 3 * i, n);
  }
  return 0;
}

// 0 done; 3: the weights of the range add up to 2^34 or more
extern "C" int multipole_emul_deposit(int n, int x0, int nxl, int flags, size_t count, const double *pos, const double *vel, double scale, double vfac, int los,
                                      const int *mass, int lo, int hi, u64 *grid, pf_halo_info *info) {
  if (n < 2 || x0 < 0 || nxl < 1 || x0 + nxl > n || lo < 1 || hi < lo || los < 0 || los > 2) return 1;
  const bool mw = (flags & PF_HALO_MASS_WEIGHT) != 0;
  memset(info, 0, sizeof(*info));
  u64 w2hi = 0, w2lo = 0;
  for (size_t i = 0; i < count; i++) {
    if (!pf_halo_in_range(mass[i], lo, hi)) continue;
    double p[3];
    position_of(i, pos, vel, scale, vfac, los, n, p);
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
    position_of(i, pos, vel, scale, vfac, los, n, p);
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

// L2 and L4 of every mode of the ky-slab [nyl][n (kx)][n/2 + 1]
extern "C" int multipole_emul_weights(int n, int los, int y0, int nyl, double *L2, double *L4) {
  if (n < 2 || (n & 1) || los < 0 || los > 2 || y0 < 0 || nyl < 1 || y0 + nyl > n) return 1;
  const int nzh = n / 2 + 1;
  for (int y = 0; y < nyl; y++)
    for (int x = 0; x < n; x++)
      for (int z = 0; z < nzh; z++) {
        const int sx = pf_power_signed(x, n), sy = pf_power_signed(y + y0, n);
        const size_t i = ((size_t)y * n + x) * nzh + z;
        pf_multipole_weights(pf_multipole_a(los, sx, sy, (unsigned int)z), (unsigned int)pf_power_k2(x, y + y0, z, n), &L2[i], &L4[i]);
      }
  return 0;
}

// the shell pass on two ky-slabs of doubles [nyl][n][n/2 + 1][2] (lin may be null: five sums), no deconvolution: nmodes, k2sum and
// parts [11][nb] = every positive sum / N^6, through the library's own fixed point -- the largest term of a shell and sum first, then
// the limbs under its exponent
extern "C" int multipole_emul_shells(int n, int los, int y0, int nyl, const double *m, const double *lin, u64 *nmodes, u64 *k2sum, double *parts, u64 *nonfinite) {
  if (n < 2 || (n & 1) || los < 0 || los > 2 || y0 < 0 || nyl < 1 || y0 + nyl > n) return 1;
  const int nzh = n / 2 + 1, nb = pf_power_nbins(n), total = lin ? PF_MULTIPOLE_NSUMS : PF_MULTIPOLE_NSUMS_AUTO;
  std::vector<double> mx((size_t)PF_MULTIPOLE_NSUMS * nb, 0.0);
  std::vector<u64> limbs((size_t)PF_MULTIPOLE_NSUMS * nb * 4, 0);
  for (int b = 0; b < nb; b++) nmodes[b] = k2sum[b] = 0;
  *nonfinite = 0;
  for (int pass = 0; pass < 2; pass++)
    for (int y = 0; y < nyl; y++)
      for (int x = 0; x < n; x++)
        for (int z = 0; z < nzh; z++) {
          const size_t i = ((size_t)y * n + x) * nzh + z;
          const int sx = pf_power_signed(x, n), sy = pf_power_signed(y + y0, n);
          const unsigned int k2 = (unsigned int)pf_power_k2(x, y + y0, z, n), w = (unsigned int)pf_power_weight(z, n);
          const int b = pf_power_shell(k2);
          const double ta = pf_matter_auto(m[2 * i], m[2 * i + 1], -1.0), tc = lin ? pf_matter_cross(m[2 * i], m[2 * i + 1], lin[2 * i], lin[2 * i + 1], -1.0) : 0.0;
          const bool fin = pf_power_finite(ta) && pf_power_finite(tc);
          if (pass == 0) {
            nmodes[b] += w; k2sum[b] += (u64)w * k2;
            if (!fin) *nonfinite += w;
          }
          if (!fin) continue;
          double L2, L4;
          pf_multipole_weights(pf_multipole_a(los, sx, sy, (unsigned int)z), k2, &L2, &L4);
          double x[6];
          pf_multipole_terms(ta, tc, L2, L4, x);
          for (int k = 0; k < 6; k++) {
            const double t = fabs(x[k]);
            const int s = pf_multipole_sum_of(k, x[k]);
            if (!(t > 0.0) || s >= total) continue;
            double &top = mx[(size_t)s * nb + b];
            if (pass == 0) { if (t > top) top = t; continue; }
            uint32_t l[3];
            pf_power_limbs((double)w * t, pf_power_exponent(top), l);
            for (int i = 0; i < 3; i++) limbs[((size_t)s * nb + b) * 4 + i] += l[i];
          }
        }
  const double n3 = (double)n * (double)n * (double)n;
  for (int s = 0; s < PF_MULTIPOLE_NSUMS; s++)
    for (int b = 0; b < nb; b++) {
      const double top = mx[(size_t)s * nb + b];
      parts[(size_t)s * nb + b] = top > 0.0 ? pf_power_from_limbs(&limbs[((size_t)s * nb + b) * 4], 4, pf_power_exponent(top)) / (n3 * n3) : 0.0;
    }
  return 0;
}

extern "C" int multipole_emul_sizes(size_t *s) {   // what the ABI test holds against ctypes
  s[0] = PF_MULTIPOLE_ORDERS; s[1] = PF_MULTIPOLE_SUMS; s[2] = PF_MULTIPOLE_NSUMS; s[3] = PF_MULTIPOLE_NSUMS_AUTO; s[4] = sizeof(pf_halo_info); s[5] = sizeof(pf_matter_info);
  return 6;
}

#ifndef MULTIPOLE_EMUL_LIB
// multipole_emul_san FILE
int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  long long head[9];
  int ncase = 0;
  while (fread(head, 8, 9, f) == 9) {
    double sv[2];
    if (fread(sv, 8, 2, f) != 2) { fprintf(stderr, "short case\n"); return 2; }
    const int n = (int)head[0], x0 = (int)head[1], nxl = (int)head[2], flags = (int)head[3], lo = (int)head[5], hi = (int)head[6], los = (int)head[7];
    const size_t count = (size_t)head[4];
    const bool has_vel = head[8] != 0;
    if (head[0] < 2 || head[0] > 64 || (n & 1) || head[4] < 0 || head[4] > 100000 || x0 < 0 || nxl < 1 || x0 + nxl > n || los < 0 || los > 2) { fprintf(stderr, "bad case header\n"); return 2; }
    std::vector<double> pos(3 * count), vel(has_vel ? 3 * count : 0);   // exactly the sizes: a read or write beyond them is the sanitizer's to find
    std::vector<int> mass(count);
    std::vector<u64> grid((size_t)nxl * n * n);
    if (fread(pos.data(), 8, pos.size(), f) != pos.size() || fread(vel.data(), 8, vel.size(), f) != vel.size() || fread(mass.data(), 4, count, f) != count) {
      fprintf(stderr, "short case\n");
      return 2;
    }
    pf_halo_info info;
    const int rc = multipole_emul_deposit(n, x0, nxl, flags, count, pos.data(), has_vel ? vel.data() : nullptr, sv[0], sv[1], los, mass.data(), lo, hi, grid.data(), &info);
    if (rc != 0 && rc != 3) return 2;
    u64 h = 1469598103934665603ull;   // FNV-1a of the grid's words
    for (size_t i = 0; rc == 0 && i < grid.size(); i++) { h ^= grid[i]; h *= 1099511628211ull; }
    // the weights of every mode of the grid, and the shell pass on the grid's own words as a spectrum of small numbers
    const size_t nmode = (size_t)n * n * (n / 2 + 1);
    std::vector<double> L2(nmode), L4(nmode), spec(2 * nmode), parts((size_t)PF_MULTIPOLE_SUMS * pf_power_nbins(n));
    std::vector<u64> nm(pf_power_nbins(n)), ks(pf_power_nbins(n));
    if (multipole_emul_weights(n, los, 0, n, L2.data(), L4.data())) return 2;
    double lsum = 0.0;
    for (size_t i = 0; i < nmode; i++) lsum += L2[i] + L4[i];
    for (size_t i = 0; i < 2 * nmode; i++) spec[i] = (double)(grid[i % grid.size()] % 1000) - 300.0;
    u64 nonfin;
    if (multipole_emul_shells(n, los, 0, n, spec.data(), spec.data(), nm.data(), ks.data(), parts.data(), &nonfin)) return 2;
    double psum = 0.0;
    for (double x : parts) psum += x;
    printf("case %d: rc %d selected %llu weight_sum %llu nonfinite %llu outside %llu empty %llu max %llu hash %llu lsum %a psum %a\n", ncase++, rc, info.selected,
           info.weight_sum, info.nonfinite, info.outside, info.empty_cells, info.max_cell, h, lsum, psum);
  }
  fclose(f);
  return 0;
}
#endif
