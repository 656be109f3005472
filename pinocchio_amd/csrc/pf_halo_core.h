// pf_halo_core.h -- one halo of the halo-power call (include/pinfmax.h: pf_halo_power): its position in cells, its class, its
// weight and the integer cloud-in-cell / nearest-grid-point factors, and the contrast of one cell.  Plain C++ for host and device:
// the kernels of pf_halo.hip call it, and a CPU test compiles it on its own (tests/cpu_emul/halo_emul.cpp) against the numpy
// restatement (tests/np_halo.py).  The file that includes this is compiled without contraction: p = pos * scale is rounded before
// the wrap subtracts n.
//
//   position   p = pos * scale (one double product); if (p >= n) p -= n; if (p < 0) p += n   (once)
//              in redshift space (pf_halo_multipoles) pos + vel * vfac takes the place of pos on the axis of the line of sight
//   classes    not finite on any axis: `nonfinite`; outside [0, n] on any axis after the wrap: `outside`.  Neither is deposited
//   CIC        u = p - 0.5, i0 = floor(u), d = u - i0 (in [0, 1]: the difference may round up to 1), t = (uint32)(d 1024) truncated
//              (the scaling is exact); factor 1024 - t to the cell i0 mod n and t to (i0 + 1) mod n.  i0 lies in [-1, n - 1] (p == n
//              comes out of the wrap of a tiny negative position).  The eight contributions are W times the product of three
//              factors as uint64: a halo adds exactly W 2^30, below 2^61 for any int W
//   NGP        W << 30 to the cell floor(p) mod n
//   contrast   delta = (double)cell / mean - 1.0, mean = (double)(weight_sum << 30) / (double)n^3
#pragma once
#include <math.h>
#include <stdint.h>

#include "pf_power_core.h"

#define PF_HALO_HD PF_POWER_HD
#define PF_HALO_SHIFT 30                       // a unit weight in the units of the grid is 1 << 30
#define PF_HALO_UNIT 1024u                     // ... the product of three factors that add up to this on every axis
#define PF_HALO_WEIGHT_LIMIT (1ull << 34)      // a bin whose weights add up to this much could overflow a cell

PF_HALO_HD double pf_halo_pos(double pos, double scale, int n) {
  double p = pos * scale;
  const double box = (double)n;
  if (p >= box) p -= box;
  if (p < 0.0) p += box;
  return p;
}

// the same in redshift space (pf_halo_multipoles): on the axis of the line of sight the position is first moved by the velocity,
// s = pos + v * vfac -- the product, then the sum, each rounded once -- and s takes the place of pos.  v null: the axis is not the
// line of sight, or the list has no velocities: pf_halo_pos itself.  A velocity that is not finite makes p not finite whatever vfac
PF_HALO_HD double pf_halo_pos_rsd(double pos, const double *v, double vfac, double scale, int n) {
  if (!v) return pf_halo_pos(pos, scale, n);
  const double shift = *v * vfac;
  const double s = pos + shift;
  return pf_halo_pos(s, scale, n);
}

// 0 deposited, 1 not finite, 2 outside [0, n]
PF_HALO_HD int pf_halo_class(const double p[3], int n) {
  for (int j = 0; j < 3; j++)
    if (!(p[j] - p[j] == 0.0)) return 1;
  for (int j = 0; j < 3; j++)
    if (!(p[j] >= 0.0 && p[j] <= (double)n)) return 2;
  return 0;
}

PF_HALO_HD bool pf_halo_in_range(int mass, int lo, int hi) { return mass >= lo && mass <= hi; }
// (a selected mass is at least lo >= 1)
PF_HALO_HD uint64_t pf_halo_weight(int mass, bool mass_weight) { return mass_weight ? (uint64_t)mass : 1ull; }

// one axis of a position in [0, n]: the two cells and their factors (w[0] + w[1] = 1024)
PF_HALO_HD void pf_halo_cic_axis(double p, int n, int cell[2], uint32_t w[2]) {
  const double u = p - 0.5;
  const double f = floor(u);
  const double d = u - f;
  const uint32_t t = (uint32_t)(d * 1024.0);
  const int i0 = (int)f;
  cell[0] = i0 < 0 ? i0 + n : i0;
  cell[1] = i0 + 1 >= n ? i0 + 1 - n : i0 + 1;
  w[0] = PF_HALO_UNIT - t; w[1] = t;
}
PF_HALO_HD int pf_halo_ngp_axis(double p, int n) {
  const int i = (int)floor(p);
  return i >= n ? i - n : i;
}

// the local index of the global plane cx in the planes [x0, x0 + nxl) (x0 + nxl <= n), -1: not one of them
PF_HALO_HD int pf_halo_plane(int cx, int x0, int nxl) {
  const int l = cx - x0;
  return l >= 0 && l < nxl ? l : -1;
}

PF_HALO_HD double pf_halo_mean(uint64_t weight_sum, int n) {
  const uint64_t n3 = (uint64_t)n * (uint64_t)n * (uint64_t)n;
  return (double)(weight_sum << PF_HALO_SHIFT) / (double)n3;
}
PF_HALO_HD double pf_halo_contrast(uint64_t cell, double mean) { return (double)cell / mean - 1.0; }
