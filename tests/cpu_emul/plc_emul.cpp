// plc_emul.cpp -- pinocchio_amd/csrc/pf_plc_core.h compiled for the host and run in the reference's form: one thread, every
// (group, replication) pair on its own, set_obj and the splines evaluated again for each (src/build_groups.c:805-854, :379-436).
// As a library (-DPLC_EMUL_LIB) tests/test_plc_cpu.py holds it against tests/np_plc.py and profiles/tools/plc_time.py times it; as
// a program it reads the cases that test wrote and runs them under -fsanitize=address,undefined.
//
// A case is two flat arrays.  hdr (int64): pb, n, nk, nsmooth, myseg, use_v31, order, events, min_mass, ncand, nrep, nzbins,
// stabl[3], GSglobal[3].  data (double): logkmin, deltalogk, k_for_GM, rad_gm0; z_seg, z_prev; center[3], zvers[3], aperture, Fstop,
// InterPartDist, LastzForPLC, delta_z; x[n], comvdist[n], hubble[n], grow[4][nk][n], fomega[4][nk][n], k_GM_displ[nsmooth];
// replications [nrep][5]; Mass[ncand], pass[ncand], val[29][ncand] (Pos, the eight velocities, Flast, F_lo).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../pinocchio_amd/csrc/pf_collapse_core.h"
#include "../../pinocchio_amd/csrc/pf_plc_core.h"

enum { H_PB, H_N, H_NK, H_NSMOOTH, H_MYSEG, H_USEV31, H_ORDER, H_EVENTS, H_MINMASS, H_NCAND, H_NREP, H_NZBINS, H_STABL, H_GS = H_STABL + 3, H_COUNT = H_GS + 3 };

template <class T>
static long long run(const long long *hdr, const PfPlcTab &t, const PfPlcGeom &g, const PfPlcSegIn &sg, const double *mass, const double *pass, const double *val,
                     size_t cap, double *rec, int *oc, int *orr, double *nz, long long *unconv) {
  const long long nc = hdr[H_NCAND];
  const int events = (int)hdr[H_EVENTS], min_mass = (int)hdr[H_MINMASS];
  long long found = 0;
  *unconv = 0;
  for (long long i = 0; i < nc; i++) {
    if (!(pass[i] != 0.0 && (int)mass[i] >= min_mass)) continue;
    PfPlcObj<T> o;
    o.M = (int)mass[i];
    for (int e = 0; e < 3; e++) o.q[e] = (T)val[(size_t)e * nc + i];
    for (int s = 0; s < 8; s++)
      for (int e = 0; e < 3; e++) o.v[s][e] = (T)val[(size_t)(3 + 3 * s + e) * nc + i];
    const T Flast = (T)val[(size_t)PF_PLC_V_FLAST * nc + i], Flo = events ? (T)val[(size_t)PF_PLC_V_FLO * nc + i] : (T)g.Fstop;
    for (int r = 0; r < g.nrep; r++) {
      const PfPlcRep rep = g.rep[r];
      if (!pf_plc_tried<T>(events, Flo, Flast, rep)) continue;
      // the reference's form: everything again for this pair
      const PfPlcK k = pf_plc_group_k<T>(t, o.M, g.ipd);
      const PfPlcSeg s = pf_plc_segment_modes(t, sg, k);
      const double bb = pf_plc_condition<T>(g, pf_plc_end<T>(t, g, sg, k, s, o, Flo, nullptr), rep);
      const double aa = bb > 0. ? pf_plc_condition<T>(g, pf_plc_end<T>(t, g, sg, k, s, o, Flast, nullptr), rep) : 0.0;
      const int kind = pf_plc_decide(bb, aa);
      if (!kind) continue;
      T F = Flo;
      if (kind == 2 && !pf_plc_root<T>(t, g, sg, k, s, o, rep, Flo, Flast, bb, aa, &F)) { (*unconv)++; continue; }
      T out[7];
      int iz = -1;
      if (!pf_plc_store<T>(t, g, sg, k, s, o, rep, F, out, &iz)) continue;
      if ((size_t)found < cap) {
        for (int q = 0; q < 7; q++) rec[7 * found + q] = (double)out[q];
        oc[found] = (int)i; orr[found] = r;
        if (nz && iz >= 0) nz[iz] += 1.0;
      }
      found++;
    }
  }
  return found;
}

extern "C" long long plc_emul_run(const long long *hdr, const double *d, size_t cap, double *rec, int *oc, int *orr, double *nz, long long *unconv) {
  const int n = (int)hdr[H_N], nk = (int)hdr[H_NK], nsmooth = (int)hdr[H_NSMOOTH], nrep = (int)hdr[H_NREP];
  const long long nc = hdr[H_NCAND];
  if (n < 3 || nk < 1 || nk > PF_PLC_MAX_NK || nrep < 1 || nc < 0 || (nk > 1 && nsmooth < 2)) return -1;
  const double *tp = d, *sd = d + 4, *gd = d + 6, *x = d + 17, *comv = x + n, *hub = comv + n, *grow = hub + n, *fom = grow + (size_t)4 * nk * n, *kgm = fom + (size_t)4 * nk * n;
  const double *reps = kgm + nsmooth, *mass = reps + (size_t)5 * nrep, *pass = mass + nc, *val = pass + nc;
  const int total = pf_plc_tab_doubles(n, nk, nsmooth);
  std::vector<double> blob((size_t)total);
  memcpy(blob.data(), x, (size_t)n * 8);
  auto put = [&](int table, const double *y) {
    double *dst = blob.data() + n + (size_t)4 * n * table;
    memcpy(dst, y, (size_t)n * 8);
    pf_spline_coeffs(x, y, n, dst + n);
    pf_spline_bd(x, y, dst + n, n, dst + 2 * n, dst + 3 * n);
  };
  put(0, comv); put(1, hub);
  for (int f = 0; f < 4; f++)
    for (int j = 0; j < nk; j++) { put(2 + nk * f + j, grow + ((size_t)f * nk + j) * n); put(2 + nk * (4 + f) + j, fom + ((size_t)f * nk + j) * n); }
  for (int j = 0; j < nsmooth; j++) blob[(size_t)total - nsmooth + j] = kgm[j];
  PfPlcTab t;
  t.g = blob.data(); t.s = nullptr; t.ns = 0; t.n = n; t.nk = nk;
  t.logkmin = tp[0]; t.dlogk = tp[1]; t.k_for_GM = tp[2]; t.rad_gm0 = tp[3]; t.kmin = pow(10., tp[0]); t.kmax = pow(10., tp[0] + (nk - 1) * tp[1]);
  t.nsmooth = nsmooth; t.kgm_at = total - nsmooth;
  const bool dbl = hdr[H_PB] == 8;
  std::vector<PfPlcRep> rp((size_t)nrep);
  for (int r = 0; r < nrep; r++) {
    rp[r].i = (int)reps[5 * r]; rp[r].j = (int)reps[5 * r + 1]; rp[r].k = (int)reps[5 * r + 2];
    rp[r].F1 = dbl ? reps[5 * r + 3] : (double)(float)reps[5 * r + 3]; rp[r].F2 = dbl ? reps[5 * r + 4] : (double)(float)reps[5 * r + 4];
  }
  PfPlcGeom g;
  memset(&g, 0, sizeof(g));
  for (int i = 0; i < 3; i++) { g.center[i] = gd[i]; g.zvers[i] = gd[3 + i]; g.stabl[i] = (int)hdr[H_STABL + i]; g.gs[i] = hdr[H_GS + i]; }
  g.aperture = gd[6]; g.Fstop = gd[7]; g.ipd = gd[8]; g.lastz = gd[9]; g.delta_z = gd[10]; g.nzbins = (int)hdr[H_NZBINS]; g.nrep = nrep; g.rep = rp.data();
  PfPlcSegIn sg;
  sg.myseg = (int)hdr[H_MYSEG]; sg.use_v31 = (int)hdr[H_USEV31]; sg.order = (int)hdr[H_ORDER]; sg.z_seg = sd[0]; sg.z_prev = sd[1];
  return dbl ? run<double>(hdr, t, g, sg, mass, pass, val, cap, rec, oc, orr, nz, unconv) : run<float>(hdr, t, g, sg, mass, pass, val, cap, rec, oc, orr, nz, unconv);
}

#ifndef PLC_EMUL_LIB
// plc_emul_san FILE: cases written one after the other as int64 nhdr (= H_COUNT), int64 ndata, hdr, data
int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  long long head[2];
  int ncase = 0;
  while (fread(head, 8, 2, f) == 2) {
    if (head[0] != H_COUNT || head[1] < 17) { fprintf(stderr, "bad case header\n"); return 2; }
    std::vector<long long> hdr((size_t)head[0]);
    std::vector<double> data((size_t)head[1]);
    if (fread(hdr.data(), 8, hdr.size(), f) != hdr.size() || fread(data.data(), 8, data.size(), f) != data.size()) { fprintf(stderr, "short case\n"); return 2; }
    const size_t cap = (size_t)(hdr[H_NCAND] * hdr[H_NREP]);
    std::vector<double> rec(7 * cap + 1), nz((size_t)hdr[H_NZBINS] + 1);
    std::vector<int> oc(cap + 1), orr(cap + 1);
    long long unconv = 0;
    const long long found = plc_emul_run(hdr.data(), data.data(), cap, rec.data(), oc.data(), orr.data(), nz.data(), &unconv);
    double sum = 0.0;
    for (long long j = 0; j < found; j++) sum += rec[7 * j];
    printf("case %d: crossings %lld unconverged %lld zsum %.17g\n", ncase++, found, unconv, sum);
  }
  fclose(f);
  return 0;
}
#endif
