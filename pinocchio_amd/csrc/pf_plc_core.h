// pf_plc_core.h -- the arithmetic of the past-light-cone test of build_groups() (src/build_groups.c:356-448, :783-868): set_obj,
// set_weight, set_obj_vel (:1354-1460), q2x and vel (:1554-1643), condition_PLC, store_PLC and the polar transformation
// (:1738-1841), the growth interpolation (src/cosmo.c:1728-1755) and my_spline_eval (:2016-2027).  Plain C++ for host and device: the
// kernels of pf_plc.hip call it, and a CPU test compiles it on its own (tests/cpu_emul/plc_emul.cpp) against the numpy restatement
// (tests/np_plc.py).  T is PRODFLOAT.  Every expression rounds where the reference's does -- the unit is built with
// -ffp-contract=off --: a product of two PRODFLOATs is a PRODFLOAT, `1. - w` is a double, an assignment to a PRODFLOAT rounds.
//
// What the reference recomputes per (group, replication) pair is split here by what it depends on:
//   PfPlcK      the group's own k and its place between two k-bins                          per group
//   PfPlcSeg    the growing modes at the segment's redshifts                                per group
//   PfPlcEnd    position (sub-box cells, stabl added) and comoving distance / InterPartDist per (group, F)
//   pf_plc_condition   the distance to the shifted observer minus the comoving distance     per (group, F, replication)
// A replication moves the observer by whole boxes and touches nothing else.
//
// The tables are one array of doubles: the n knots x = -log10(1 + z), then per table y, c, b, d of n doubles each (GSL's cspline: c
// from pf_spline_coeffs, b and d from pf_spline_bd); table 0 COMVDIST, 1 Hubble, 2 + nk f + kbin the families f = 0..3 GROW1, GROW2,
// GROW31, GROW32 (log10) and 4..7 FOMEGA1, FOMEGA2, FOMEGA31, FOMEGA32; then the nsmooth values of k_GM_displ.  The first `ns` doubles
// may lie in a second, faster copy (LDS on the device).
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define PF_PLC_HD __host__ __device__ __forceinline__
#define PF_PLC_MEMBER __host__ __device__ __forceinline__
#else
#define PF_PLC_HD static inline
#define PF_PLC_MEMBER inline
#endif

#define PF_PLC_PI 3.14159265358979323846   // src/pinocchio.h:56
#define PF_PLC_MAX_ITER 100                // src/build_groups.c:1731
#define PF_PLC_MAX_NK 32
#define PF_PLC_NVAL 29                     // values of a candidate: Pos[3], eight velocities of 3, Flast, F_lo
#define PF_PLC_V_FLAST 27
#define PF_PLC_V_FLO 28
#define PF_PLC_BLOCK 256                   // candidates (pairs) of a workgroup
#define PF_PLC_LDS_DOUBLES 7680            // doubles of the tables a workgroup stages: 60 KB

struct PfPlcTab {
  const double *g, *s;   // the whole array; its first ns doubles once more (null with ns = 0)
  int ns, n, nk;
  double logkmin, dlogk, kmin, kmax, k_for_GM, rad_gm0;
  int nsmooth, kgm_at;   // k_GM_displ[j] = at(kgm_at + j)
  PF_PLC_MEMBER double at(int i) const { return i < ns ? s[i] : g[i]; }
};
PF_PLC_HD int pf_plc_tab_doubles(int n, int nk, int nsmooth) { return n + 4 * n * (2 + 8 * nk) + nsmooth; }

struct PfPlcRep { int i, j, k; double F1, F2; };   // F1, F2 hold PRODFLOAT values
struct PfPlcGeom {
  double center[3], xvers[3], yvers[3], zvers[3], aperture, Fstop, ipd, lastz, delta_z;
  long long gs[3];
  int stabl[3], nzbins, nrep;
  const PfPlcRep *rep;
};
struct PfPlcSegIn { int myseg, use_v31, order; double z_seg, z_prev; };

// where x = -log10(1 + z) lies among the knots: my_spline_eval's three branches, found once for all tables
struct PfPlcX { int where, i; double v, dx; };
PF_PLC_HD PfPlcX pf_plc_locate(const PfPlcTab &t, double z) {
  PfPlcX p;
  p.v = -log10(1. + z);
  const int last = t.n - 1;
  p.i = 0; p.dx = 0.0;
  if (p.v < t.at(0)) { p.where = -1; return p; }
  if (p.v > t.at(last)) { p.where = 1; return p; }
  p.where = 0;
  int ilo = 0, ihi = last;   // gsl_interp_bsearch: the largest i <= n - 2 with x[i] <= v
  while (ihi > ilo + 1) {
    const int i = (ihi + ilo) >> 1;
    if (t.at(i) > p.v) ihi = i; else ilo = i;
  }
  p.i = ilo;
  p.dx = p.v - t.at(ilo);
  return p;
}
PF_PLC_HD double pf_plc_spline(const PfPlcTab &t, int table, const PfPlcX &p) {
  const int y = t.n + 4 * t.n * table, last = t.n - 1;
  if (p.where < 0) return t.at(y) + (p.v - t.at(0)) * (t.at(y + 1) - t.at(y)) / (t.at(1) - t.at(0));
  if (p.where > 0) return t.at(y + last) + (p.v - t.at(last)) * (t.at(y + last) - t.at(y + last - 1)) / (t.at(last) - t.at(last - 1));
  const int i = p.i;
  return t.at(y + i) + p.dx * (t.at(y + 2 * t.n + i) + p.dx * (t.at(y + t.n + i) + p.dx * t.at(y + 3 * t.n + i)));
}

// set_obj's own k of a group (:1361-1378) and InterpolateGrowth's branch for it (cosmo.c:1737-1749).  indx + 1 and kk + 1 are kept
// inside their arrays: at the very top of either range the reference reads one element beyond it with weight zero or one.
struct PfPlcK { double myk, dk; int kk, both; };
template <class T> PF_PLC_HD PfPlcK pf_plc_group_k(const PfPlcTab &t, int M, double ipd) {
  PfPlcK k;
  k.dk = 0.0; k.kk = 0; k.both = 0;
  if (t.nk == 1) { k.myk = t.k_for_GM; return k; }
  const T R = (T)(pow((double)M * 3. / 4. / PF_PLC_PI, 1. / 3.) * ipd);
  double interp = (1. - R / t.rad_gm0) * (double)(t.nsmooth - 1);
  interp = (interp < 0. ? 0. : interp);
  int indx = (int)interp;
  if (indx > t.nsmooth - 2) indx = t.nsmooth - 2;
  if (indx < 0) indx = 0;   // (a Mass below zero: interp is no number)
  const double w = interp - (double)indx;
  k.myk = pow(10., log10(t.at(t.kgm_at + indx)) * (1. - w) + log10(t.at(t.kgm_at + indx + 1)) * w);
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
PF_PLC_HD double pf_plc_growth(const PfPlcTab &t, int family, const PfPlcK &k, const PfPlcX &p) {
  const int tab = 2 + t.nk * family + k.kk;
  if (!k.both) return pf_plc_spline(t, tab, p);
  return k.dk * pf_plc_spline(t, tab + 1, p) + (1 - k.dk) * pf_plc_spline(t, tab, p);
}
// GrowingMode, _2LPT, _3LPT_1 (with its minus sign, cosmo.c:1810), _3LPT_2
PF_PLC_HD double pf_plc_mode(const PfPlcTab &t, int o, const PfPlcK &k, const PfPlcX &p) {
  const double g = pow(10., pf_plc_growth(t, o, k, p));
  return o == 2 ? -g : g;
}

struct PfPlcSeg { double gs[4], gp[4]; };
PF_PLC_HD PfPlcSeg pf_plc_segment_modes(const PfPlcTab &t, const PfPlcSegIn &sg, const PfPlcK &k) {
  PfPlcSeg s;
  const PfPlcX ps = pf_plc_locate(t, sg.z_seg);
  for (int o = 0; o < 4; o++) { s.gs[o] = pf_plc_mode(t, o, k, ps); s.gp[o] = 0.0; }
  if (sg.myseg) {
    const PfPlcX pp = pf_plc_locate(t, sg.z_prev);
    for (int o = 0; o < 4; o++) s.gp[o] = pf_plc_mode(t, o, k, pp);
  }
  return s;
}

// the group as set_obj copies it: q, then v, v2, v31, v32 and their _prev twins
template <class T> struct PfPlcObj { int M; T q[3], v[8][3]; };
template <class T> struct PfPlcW { T w[4]; };

// set_weight (:1411-1444) at z = F - 1
template <class T> PF_PLC_HD PfPlcW<T> pf_plc_weights(const PfPlcTab &t, const PfPlcSegIn &sg, const PfPlcK &k, const PfPlcSeg &s, const PfPlcX &p) {
  PfPlcW<T> w;
  for (int o = 0; o < 4; o++) {
    const double g = pf_plc_mode(t, o, k, p);
    w.w[o] = sg.myseg ? (T)((g - s.gp[o]) / (s.gs[o] - s.gp[o])) : (T)(g / s.gs[o]);
  }
  return w;
}

// q2x (:1554-1603) without periodic wrapping: the test switches subbox.pbc off
template <class T> PF_PLC_HD T pf_plc_q2x(int i, const PfPlcObj<T> &o, const PfPlcW<T> &w, const PfPlcSegIn &sg) {
  T pos;
  if (!sg.myseg) {
    pos = o.q[i] + w.w[0] * o.v[0][i];
    if (sg.order > 1) pos += w.w[1] * o.v[1][i];
    if (sg.order > 2) pos += w.w[2] * o.v[2][i] + w.w[3] * o.v[3][i];
  } else {
    pos = (T)(o.q[i] + (1. - w.w[0]) * o.v[4][i] + w.w[0] * o.v[0][i]);
    if (sg.order > 1) pos = (T)(pos + ((1. - w.w[1]) * o.v[5][i] + w.w[1] * o.v[1][i]));
    // :1588 multiplies w31 with v32 where v31 is meant; use_v31 selects the intended line
    if (sg.order > 2)
      pos = (T)(pos + ((1. - w.w[2]) * o.v[6][i] + w.w[2] * (sg.use_v31 ? o.v[2][i] : o.v[3][i]) + (1. - w.w[3]) * o.v[7][i] + w.w[3] * o.v[3][i]));
  }
  return pos;
}

// what condition_PLC and store_PLC need of a group at F and share between the replications
template <class T> struct PfPlcEnd { T P[3]; double D; };
template <class T> PF_PLC_HD PfPlcEnd<T> pf_plc_end(const PfPlcTab &t, const PfPlcGeom &g, const PfPlcSegIn &sg, const PfPlcK &k, const PfPlcSeg &s,
                                                   const PfPlcObj<T> &o, T F, PfPlcW<T> *wout) {
  const double z = F - 1.0;
  const PfPlcX p = pf_plc_locate(t, z);
  const PfPlcW<T> w = pf_plc_weights<T>(t, sg, k, s, p);
  PfPlcEnd<T> e;
  for (int i = 0; i < 3; i++) e.P[i] = pf_plc_q2x<T>(i, o, w, sg) + g.stabl[i];
  e.D = pf_plc_spline(t, 0, p) / g.ipd;
  if (wout) *wout = w;
  return e;
}
PF_PLC_HD double pf_plc_observer(const PfPlcGeom &g, const PfPlcRep &r, int i) {
  const long long rep = i == 0 ? r.i : i == 1 ? r.j : r.k;
  return g.center[i] - (double)(g.gs[i] * rep);
}
template <class T> PF_PLC_HD double pf_plc_condition(const PfPlcGeom &g, const PfPlcEnd<T> &e, const PfPlcRep &r) {
  double condition = 0.0;
  for (int i = 0; i < 3; i++) {
    const double diff1 = e.P[i] - pf_plc_observer(g, r, i);
    condition += diff1 * diff1;
  }
  return sqrt(condition) - e.D;
}

// the range test of a replication: :819 in the last check, :394-395 at an event
template <class T> PF_PLC_HD bool pf_plc_tried(int events, T Flo, T Flast, const PfPlcRep &r) {
  if (events) return !(Flo > (T)r.F1 || Flast < (T)r.F2);
  return Flast > (T)r.F2;
}
// 0 no crossing, 1 caught on the cone at F_lo, 2 a root in between
PF_PLC_HD int pf_plc_decide(double bb, double aa) { return bb == 0.0 ? 1 : (bb > 0. && aa < 0.0) ? 2 : 0; }

// the crossing F between F_lo (condition bb > 0) and Flast (aa < 0): false position with the Illinois rule on PRODFLOAT arguments,
// bisection where the step leaves the open interval.  Stops as find_brent does (:1865): |condition| < brent_err within MAX_ITER
template <class T> PF_PLC_HD bool pf_plc_root(const PfPlcTab &t, const PfPlcGeom &g, const PfPlcSegIn &sg, const PfPlcK &k, const PfPlcSeg &s,
                                             const PfPlcObj<T> &o, const PfPlcRep &r, T Flo, T Flast, double bb, double aa, T *Fout) {
  const double brent_err = 1.e-2 * g.ipd;
  T a = Flo, b = Flast;
  double fa = bb, fb = aa;
  int side = 0;
  for (int it = 0; it < PF_PLC_MAX_ITER; it++) {
    const T lo = a < b ? a : b, hi = a < b ? b : a;
    T x = (T)(((double)a * fb - (double)b * fa) / (fb - fa));
    if (!(x > lo && x < hi)) x = (T)(0.5 * ((double)a + (double)b));
    if (!(x > lo && x < hi)) return false;   // adjacent PRODFLOATs
    const PfPlcEnd<T> e = pf_plc_end<T>(t, g, sg, k, s, o, x, nullptr);
    const double f = pf_plc_condition<T>(g, e, r);
    if (fabs(f) < brent_err) { *Fout = x; return true; }
    if (f > 0.) { a = x; fa = f; if (side == 1) fb *= 0.5; side = 1; }
    else { b = x; fb = f; if (side == 2) fa *= 0.5; side = 2; }
  }
  return false;
}

// set_obj_vel (:1446-1460) at z = F - 1 with Hubble(z) from its table, and vel (:1607-1643) of the three axes: what store_PLC and the
// catalogue (pf_catalog_core.h) write as a group's velocity
template <class T> PF_PLC_HD void pf_plc_vel3(const PfPlcTab &t, double ipd, const PfPlcSegIn &sg, const PfPlcK &k, const PfPlcObj<T> &o, const PfPlcW<T> &w, T F, T vel[3]) {
  const double z = F - 1.0;
  const PfPlcX p = pf_plc_locate(t, z);
  const T fac = (T)(pf_plc_spline(t, 1, p) / (1. + z) * ipd);
  T Dv[4];
  for (int f = 0; f < 4; f++) Dv[f] = (T)(fac * pf_plc_growth(t, 4 + f, k, p));
  for (int i = 0; i < 3; i++) {
    T vv;
    if (!sg.myseg) {
      vv = o.v[0][i] * Dv[0] * w.w[0];
      if (sg.order > 1) vv += o.v[1][i] * Dv[1] * w.w[1];
      if (sg.order > 2) vv += o.v[2][i] * Dv[2] * w.w[2] + o.v[3][i] * Dv[3] * w.w[3];
    } else {
      vv = (T)((o.v[4][i] * (1. - w.w[0]) + o.v[0][i] * w.w[0]) * Dv[0]);
      if (sg.order > 1) vv = (T)(vv + (o.v[5][i] * (1. - w.w[1]) + o.v[1][i] * w.w[1]) * Dv[1]);
      if (sg.order > 2)
        vv = (T)(vv + ((o.v[6][i] * (1. - w.w[2]) + o.v[2][i] * w.w[2]) * Dv[2] + (o.v[7][i] * (1. - w.w[3]) + o.v[3][i] * w.w[3]) * Dv[3]));
    }
    vel[i] = vv;
  }
}

// store_PLC (:1764-1822) at F: false when the group lies outside the aperture.  rec = z, x[3], v[3]; *iz the bin of the n(z)
// histogram, -1 where the reference would write outside nz[]
template <class T> PF_PLC_HD bool pf_plc_store(const PfPlcTab &t, const PfPlcGeom &g, const PfPlcSegIn &sg, const PfPlcK &k, const PfPlcSeg &s,
                                              const PfPlcObj<T> &o, const PfPlcRep &r, T F, T rec[7], int *iz) {
  PfPlcW<T> w;
  const PfPlcEnd<T> e = pf_plc_end<T>(t, g, sg, k, s, o, F, &w);
  T x[3];
  for (int i = 0; i < 3; i++) x[i] = (T)(g.ipd * (e.P[i] - pf_plc_observer(g, r, i)));
  // coord_transformation_cartesian_polar (:1824-1841): theta alone is read
  const double rho = sqrt((double)(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]));   // the sum in PRODFLOAT, its root in double
  double theta = 90.0;
  if (rho > 0) theta = -acos((x[0] * g.zvers[0] + x[1] * g.zvers[1] + x[2] * g.zvers[2]) / rho) * 180. / PF_PLC_PI + 90.;
  if (!(90. - theta < g.aperture)) return false;
  T vv[3];
  pf_plc_vel3<T>(t, g.ipd, sg, k, o, w, F, vv);
  rec[0] = (T)(F - 1.0);
  for (int i = 0; i < 3; i++) {
    rec[1 + i] = x[i];
    rec[4 + i] = vv[i];
  }
  int b = (int)((rec[0] - g.lastz) / g.delta_z);
  if (b == g.nzbins) b--;
  *iz = (b >= 0 && b < g.nzbins) ? b : -1;
  return true;
}
