// pf_matter_core.h -- one particle of the mass assignment and one mode of the matter spectra (include/pinfmax.h: pf_matter_power).
// Plain C++ for host and device: the kernels of pf_matter.hip call it, and a CPU test compiles it on its own
// (tests/cpu_emul/matter_emul.cpp) against the numpy restatement (tests/np_matter.py).  T is the context's PRODFLOAT.  The file that
// includes this is compiled without contraction: every product and sum below is rounded once, where it stands.
//
//   position      the reference's initialize_POS (src/write_snapshot.c:907-954) for axis j of the particle of global cell q:
//                   pos = (T)((double)q_j + 0.5 + (double)V1)    (SHIFT is a double literal: the first statement is a double sum)
//                   pos = pos + V2;  pos = pos + (V31 + V32)     (T arithmetic, the inner sum first)
//                   if (pos >= n) pos -= n;  if (pos < 0) pos += n     (T arithmetic, once)
//                 with weights w[4] (double) each column value v is first replaced by (T)(w_k (double)v)
//   classes       a position that is not finite on any axis: `nonfinite`; one outside [0, n] after the single wrap: `outside`.
//                 Neither is deposited
//   CIC           a particle at rest sits on the centre of its cell: u = pos - 0.5, i0 = floor(u), d = u - i0 (in [0, 1]: the
//                 difference may round up to 1), t = (uint32)(d 65536) truncated (the scaling is exact); weight 65536 - t to the
//                 cell i0 mod n and t to (i0 + 1) mod n.  i0 lies in [-1, n - 1] (pos == n can come out of the wrap in float).
//                 The eight contributions are the products of three such factors as uint64: a particle adds exactly 2^48, so a
//                 grid of uint64 is exact whatever the order of the additions -- while fewer than 2^16 whole particles meet in one cell
//   NGP           the whole 2^48 to the cell floor(pos) mod n
//   deconvolution c[j] = sinc(pi j / n)^(-p), p = 1 (NGP) or 2 (CIC), j = 0 .. n/2: one table, built on the host; a mode carries
//                 (c[|kx|] c[|ky|]) c[kz]
//   mode terms    auto = re_m^2 + im_m^2 (pf_power_term), cross = re_m re + im_m im: two products and one sum, each rounded once.
//                 Deconvolved: auto (c c), cross c.  The cross term goes to the sum of the positive terms or, negated, to that of the
//                 negative ones
#pragma once
#include <math.h>
#include <stdint.h>

#include "pf_power_core.h"

#define PF_MATTER_HD PF_POWER_HD
#define PF_MATTER_ONE (1ull << 48)   // one particle in the units of the grid

template <class T> PF_MATTER_HD T pf_matter_column(T v, const double *w, int k) { return w ? (T)(w[k] * (double)v) : v; }

// v1, v2, v31, v32: the (weighted) column values of this axis
template <class T> PF_MATTER_HD T pf_matter_pos(int q, int n, T v1, T v2, T v31, T v32) {
  T pos = (T)((double)q + 0.5 + (double)v1);
  pos = pos + v2;
  const T v3 = v31 + v32;
  pos = pos + v3;
  const T box = (T)n;
  if (pos >= box) pos -= box;
  if (pos < (T)0) pos += box;
  return pos;
}

// 0 deposited, 1 not finite, 2 outside [0, n]
template <class T> PF_MATTER_HD int pf_matter_class(const T pos[3], int n) {
  for (int j = 0; j < 3; j++)
    if (!(pos[j] - pos[j] == (T)0)) return 1;
  for (int j = 0; j < 3; j++)
    if (!(pos[j] >= (T)0 && pos[j] <= (T)n)) return 2;
  return 0;
}

// one axis of a position in [0, n]: the two cells and their weights (w[0] + w[1] = 65536)
template <class T> PF_MATTER_HD void pf_matter_cic_axis(T pos, int n, int cell[2], uint32_t w[2]) {
  const T u = pos - (T)0.5;
  const T f = floor(u);
  const T d = u - f;
  const uint32_t t = (uint32_t)(d * (T)65536);
  const int i0 = (int)f;
  cell[0] = i0 < 0 ? i0 + n : i0;
  cell[1] = i0 + 1 >= n ? i0 + 1 - n : i0 + 1;
  w[0] = 65536u - t; w[1] = t;
}
template <class T> PF_MATTER_HD int pf_matter_ngp_axis(T pos, int n) {
  const int i = (int)floor(pos);
  return i >= n ? i - n : i;
}

PF_MATTER_HD double pf_matter_deconv_entry(int j, int n, int p) {   // (host: the table is built there)
  if (j == 0) return 1.0;
  const double x = 3.14159265358979323846 * (double)j / (double)n;
  const double s = sin(x) / x;
  return p == 1 ? 1.0 / s : 1.0 / (s * s);
}
PF_MATTER_HD double pf_matter_deconv(double cx, double cy, double cz) { return (cx * cy) * cz; }

// the two terms of a mode; c < 0: no deconvolution
PF_MATTER_HD double pf_matter_auto(double re_m, double im_m, double c) {
  const double t = pf_power_term<double>(re_m, im_m);
  return c < 0.0 ? t : t * (c * c);
}
PF_MATTER_HD double pf_matter_cross(double re_m, double im_m, double re, double im, double c) {
  const double a = re_m * re, b = im_m * im;
  const double t = a + b;
  return c < 0.0 ? t : t * c;
}
// which: 0 the auto term, 1 the cross term where it is positive, 2 its negative where it is negative; 0 for a mode that has no part in the sum
PF_MATTER_HD double pf_matter_part(int which, double t_auto, double t_cross) {
  if (which == 0) return t_auto;
  if (which == 1) return t_cross > 0.0 ? t_cross : 0.0;
  return t_cross < 0.0 ? -t_cross : 0.0;
}
