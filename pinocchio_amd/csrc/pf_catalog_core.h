// pf_catalog_core.h -- the arithmetic of the output step of build_groups() (src/build_groups.c:888-920): one record of
// write_catalog() (src/write_halos.c:285-317) and the mass-function bin of compute_mf() (:56-65).  Per group it is the arithmetic
// of the light-cone test evaluated at one F -- set_obj, set_weight, set_obj_vel, q2x and vel of pf_plc_core.h -- plus what the
// catalogue adds: q2x's periodic wrap (build_groups.c:1595-1600), the shift to the global box with its two wraps and the
// conversion to Mpc (write_halos.c:300-313).  Plain C++ for host and device: the kernels of pf_catalog.hip call it, and a CPU test
// compiles it on its own (tests/cpu_emul/catalog_emul.cpp) against the numpy restatement (tests/np_catalog.py).  T is PRODFLOAT.
// The unit is built with -ffp-contract=off and every expression rounds where the reference's C does: a product of two PRODFLOATs is
// a PRODFLOAT, anything with a double operand (SGrid, GGrid, Box, InterPartDist * hfactor) is a double, an assignment to a
// PRODFLOAT rounds.
//
// The mass function.  compute_mf bins a group by (int)((log10(Mass * ParticleMass) - mmin) / DELTAM).  The device evaluates no
// log10 for this: pf_cat_thresholds turns (mmin, deltam, nbin, ParticleMass) into nbin + 1 integer thresholds on the host -- thr[b]
// is the smallest Mass >= 1 whose bin, by that very expression and the host libm's log10, is >= b -- by bisection over Mass, and
// pf_cat_bin finds the bin of a Mass by binary search in them.  That is the reference's own binning to the last bit wherever its
// log10(Mass * ParticleMass) does not decrease as Mass grows; a libm whose log10 is not monotonic over the integers times
// ParticleMass could bin a Mass next to an edge differently.  (The cast truncates toward zero, so a Mass whose quotient lies in
// (-1, 0) counts in bin 0, as in the reference.)  Groups with Mass < 1 never enter the histogram.
//
// The histogram itself is two integer arrays: a count and a 64-bit sum of Mass per bin.  The host forms massinbin[b] =
// (double)sumMass[b] * ParticleMass.  The reference adds the doubles Mass * ParticleMass one by one: n_b roundings of at most 2^-53
// relative each against one rounding of the product here (and none of the sum: it is exact below 2^53), so the two differ by at
// most (n_b + 1) 2^-53 relative -- and the integer form does not depend on the order of groups[].
#pragma once
#include "pf_plc_core.h"

#define PF_CAT_NVAL 27        // values of a group: Pos[3] and the eight velocities of 3
#define PF_CAT_NREC 10        // PRODFLOATs of a record: M, x[3], v[3], q[3] (the order of catalog_data, src/pinocchio.h:515-524)
#define PF_CAT_BLOCK 256      // groups of a workgroup
#define PF_CAT_LDS_BINS 2048  // bins of a histogram a workgroup keeps in LDS (24 KB)
#define PF_CAT_NOMASS 0x80000000u   // a threshold no Mass reaches

struct PfCatGeom {
  double ggrid[3], box[3];     // GSglobal and subbox.Lgwbl as doubles
  double stabl[3];             // SGrid
  double scale;                // InterPartDist * hfactor
  double ipd, pmass, hfactor;
  int pbc[3];
};

// sub-box cells -> the global box in Mpc (write_halos.c:300-305 for q, :308-313 for x)
template <class T> PF_PLC_HD T pf_cat_global(T a, int j, const PfCatGeom &g) {
  T q = (T)(a + g.stabl[j]);
  if (q < 0) q = (T)(q + g.ggrid[j]);
  if (q >= g.ggrid[j]) q = (T)(q - g.ggrid[j]);
  q = (T)(q * g.scale);
  return q;
}

// one record of the catalogue at F = outputs.F[iout]: rec = M, x[3], v[3], q[3]
template <class T> PF_PLC_HD void pf_cat_record(const PfPlcTab &t, const PfCatGeom &g, const PfPlcSegIn &sg, const PfPlcK &k, const PfPlcSeg &s,
                                               const PfPlcObj<T> &o, T F, T rec[PF_CAT_NREC]) {
  const double z = F - 1.0;
  const PfPlcX p = pf_plc_locate(t, z);
  const PfPlcW<T> w = pf_plc_weights<T>(t, sg, k, s, p);
  T v[3];
  pf_plc_vel3<T>(t, g.ipd, sg, k, o, w, F, v);
  rec[0] = (T)((double)o.M * g.pmass * g.hfactor);
  for (int j = 0; j < 3; j++) {
    rec[7 + j] = pf_cat_global<T>(o.q[j], j, g);
    T pos = pf_plc_q2x<T>(j, o, w, sg);
    if (g.pbc[j]) {   // build_groups.c:1595-1600
      if (pos >= g.box[j]) pos = (T)(pos - g.box[j]);
      if (pos < 0.0) pos = (T)(pos + g.box[j]);
    }
    rec[1 + j] = pf_cat_global<T>(pos, j, g);
    rec[4 + j] = v[j];
  }
}

// the bin of a Mass: the largest b with thr[b] <= Mass; -1 outside [0, nbin) (and for Mass < 1)
PF_PLC_HD int pf_cat_bin(const unsigned int *thr, int nbin, int Mass) {
  if (Mass < 1 || nbin < 1) return -1;
  const unsigned int m = (unsigned int)Mass;
  if (m < thr[0] || m >= thr[nbin]) return -1;
  int lo = 0, hi = nbin;   // thr[lo] <= m < thr[hi]
  while (hi > lo + 1) {
    const int mid = (lo + hi) >> 1;
    if (thr[mid] <= m) lo = mid; else hi = mid;
  }
  return lo;
}

// host only (the libm's log10):
// compute_mf's bin of a Mass (write_halos.c:59-62), the quotient held to [-1, nbin] before the cast
static inline int pf_cat_bin_log10(double Mass, double pmass, double mmin, double deltam, int nbin) {
  const double amass = Mass * pmass;
  const double q = (log10(amass) - mmin) / deltam;
  if (!(q > -1.0)) return -1;
  if (q >= (double)nbin) return nbin;
  return (int)q;
}
// thr[nbin + 1]: thr[b] = the smallest Mass in [1, 2^31 - 1] whose bin is >= b, PF_CAT_NOMASS where there is none
static inline void pf_cat_thresholds(double mmin, double deltam, int nbin, double pmass, unsigned int *thr) {
  for (int b = 0; b <= nbin; b++) {
    if (pf_cat_bin_log10(1.0, pmass, mmin, deltam, nbin) >= b) { thr[b] = 1u; continue; }
    if (pf_cat_bin_log10(2147483647.0, pmass, mmin, deltam, nbin) < b) { thr[b] = PF_CAT_NOMASS; continue; }
    unsigned int lo = 1u, hi = 2147483647u;   // bin(lo) < b <= bin(hi)
    while (hi > lo + 1u) {
      const unsigned int mid = lo + ((hi - lo) >> 1);
      if (pf_cat_bin_log10((double)mid, pmass, mmin, deltam, nbin) >= b) hi = mid; else lo = mid;
    }
    thr[b] = hi;
  }
}
