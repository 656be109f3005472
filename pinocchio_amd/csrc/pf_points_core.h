// pf_points_core.h -- the state of one stored particle at its own collapse time: what condition_for_accretion()
// (src/build_groups.c:1286-1317) evaluates through virial() (:1023-1051), set_point() (:1464-1520) with set_weight() (:1411-1444)
// and q2x() (:1554-1603) for the particle the loop of build_groups() works on, as far as it depends on F = frag[iz].Fmax, the
// particle's cell and velocities, the segment and the cosmology tables alone.  Plain C++ for host and device on top of
// pf_plc_core.h (the spline evaluation, the k-bin branch of InterpolateGrowth, set_weight, q2x without its wraps) and
// pf_refresh_core.h (the cell of a stored particle): the kernel of pf_points.hip calls it, and a CPU test compiles it on its own
// (tests/cpu_emul/points_emul.cpp) against the numpy restatement (tests/np_points.py).  T is PRODFLOAT.  The unit is built with
// -ffp-contract=off and every expression rounds where the reference's C does.
//
// The tables of a call.  A call reads the growth families at two k values only: GROW1 .. GROW32 at k_point (set_weight) and GROW1
// at k_sigma (virial).  pf_point_plan picks, from the tables of pf_plc_set_cosmology, the ones those two read -- one per family
// with nk == 1 or with a k outside [kmin, kmax], the two bins around the k otherwise -- and lays them out as a small array of the
// SAME form as the full one (pf_plc_core.h), so that every helper of pf_plc_core.h works on it unchanged:
//   knots | table 0, 1: GROW1 of the bins around k_sigma (the places of COMVDIST and Hubble, which a point does not read)
//         | table 2 + nb f + b: family f = 0..3, bin b < nb around k_point, nb = 1 or 2
// src[j] names the table of the full array that table j of the small one is a copy of (-1: not read, left zero).  In the small array
// a PfPlcK has kk = 0.
#pragma once
#include "pf_plc_core.h"
#include "pf_refresh_core.h"

#define PF_POINT_NREC 8       // PRODFLOATs of a state: w, w2, w31, w32, sigmaD, x[3]
#define PF_POINT_SHIFT 0.5    // SHIFT (src/pinocchio.h:73)
#define PF_POINT_MAX_TABLES 10

// InterpolateGrowth's branch (cosmo.c:1737-1749) for a k value, as pf_plc_group_k finds it for a group's own k
PF_PLC_HD PfPlcK pf_plc_k_of(const PfPlcTab &t, double myk) {
  PfPlcK k;
  k.myk = myk; k.dk = 0.0; k.kk = 0; k.both = 0;
  if (t.nk == 1) return k;
  if (k.myk < t.kmin) return k;
  if (k.myk > t.kmax) { k.kk = t.nk - 1; return k; }
  double dk = (log10(k.myk) - t.logkmin) / t.dlogk;
  int kk = (int)dk;
  if (kk > t.nk - 2) kk = t.nk - 2;
  if (kk < 0) kk = 0;
  dk -= kk;
  k.kk = kk; k.dk = dk; k.both = 1;
  return k;
}

struct PfPointPlan {
  int nb, ntab, doubles;              // bins per family around k_point; tables and doubles of the small array
  int src[PF_POINT_MAX_TABLES];       // table of the full array behind table j, -1: none
  PfPlcK kp, ks;                      // the two k values in the small array (kk = 0)
};
// full: the tables of pf_plc_set_cosmology (n, nk and the k-bin constants are read; no array is)
static inline PfPointPlan pf_point_plan(const PfPlcTab &full, double k_point, double k_sigma) {
  PfPointPlan p;
  const PfPlcK kp = pf_plc_k_of(full, k_point), ks = pf_plc_k_of(full, k_sigma);
  p.nb = kp.both ? 2 : 1;
  p.ntab = 2 + 4 * p.nb;
  p.doubles = pf_plc_tab_doubles(full.n, p.nb, 0);
  p.src[0] = 2 + ks.kk;
  p.src[1] = ks.both ? 2 + ks.kk + 1 : -1;
  for (int f = 0; f < 4; f++)
    for (int b = 0; b < p.nb; b++) p.src[2 + p.nb * f + b] = 2 + full.nk * f + kp.kk + b;
  p.kp = kp; p.kp.kk = 0;
  p.ks = ks; p.ks.kk = 0;
  return p;
}
// the view of the small array at `g` (s / ns: its copy in faster memory, set by whoever stages it)
static inline PfPlcTab pf_point_tab(const PfPlcTab &full, const PfPointPlan &p, const double *g) {
  PfPlcTab t = full;
  t.g = g; t.s = nullptr; t.ns = 0; t.nk = p.nb; t.nsmooth = 0; t.kgm_at = p.doubles;
  return t;
}

// GrowingMode(z, k_sigma) (virial, :1040-1045) from tables 0 and 1 of the small array
PF_PLC_HD double pf_point_sigma_mode(const PfPlcTab &t, const PfPlcK &ks, const PfPlcX &p) {
  const double lg = ks.both ? ks.dk * pf_plc_spline(t, 1, p) + (1 - ks.dk) * pf_plc_spline(t, 0, p) : pf_plc_spline(t, 0, p);
  return pow(10., lg);
}

// box: subbox.Lgwbl as doubles and subbox.pbc; nw: the weights the context's LPT order has (1, 2 or 4)
struct PfPointGeom { double box[3], sigma0; int pbc[3], nw; };

// o: q = the sub-box coordinate + SHIFT and the 24 velocities (those the order does not read may hold anything); sg.order = the
// order q2x uses; s = pf_plc_segment_modes at k_point.  rec = w, w2, w31, w32, sigmaD, x[3]
template <class T> PF_PLC_HD void pf_point_state(const PfPlcTab &t, const PfPointGeom &g, const PfPlcSegIn &sg, const PfPlcK &kp, const PfPlcK &ks, const PfPlcSeg &s,
                                                const PfPlcObj<T> &o, T F, T rec[PF_POINT_NREC]) {
  const double z = (double)F - 1.0;
  const PfPlcX p = pf_plc_locate(t, z);
  PfPlcW<T> w;
  for (int f = 0; f < 4; f++) {   // set_weight (:1411-1444), as pf_plc_weights forms it
    w.w[f] = (T)0;
    if (f >= g.nw) continue;
    const double gm = pf_plc_mode(t, f, kp, p);
    w.w[f] = sg.myseg ? (T)((gm - s.gp[f]) / (s.gs[f] - s.gp[f])) : (T)(gm / s.gs[f]);
  }
  for (int f = 0; f < 4; f++) rec[f] = w.w[f];
  rec[4] = (T)(g.sigma0 * pf_point_sigma_mode(t, ks, p));
  for (int d = 0; d < 3; d++) {
    T pos = pf_plc_q2x<T>(d, o, w, sg);
    if (g.pbc[d]) {   // :1595-1600
      if (pos >= g.box[d]) pos = (T)(pos - g.box[d]);
      if (pos < 0.0) pos = (T)(pos + g.box[d]);
    }
    rec[5 + d] = pos;
  }
}

// the segment's growing modes at k_point for the families the context's order has (the others are not read: 1 keeps a division defined)
static inline PfPlcSeg pf_point_segment_modes(const PfPlcTab &t, const PfPlcSegIn &sg, const PfPlcK &kp, int nw) {
  PfPlcSeg s = pf_plc_segment_modes(t, sg, kp);
  for (int f = nw; f < 4; f++) { s.gs[f] = 1.0; s.gp[f] = 0.0; }
  return s;
}
