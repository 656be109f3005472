// catalog_emul.cpp -- pinocchio_amd/csrc/pf_catalog_core.h compiled for the host and run in the reference's form: one thread, group by
// group, set_obj and the splines evaluated again for each (src/write_halos.c:285-317, :56-65).  As a library (-DCATALOG_EMUL_LIB)
// tests/test_catalog_cpu.py holds it against tests/np_catalog.py and profiles/tools/catalog_time.py times it; as a program it reads
// the cases that test wrote and runs them under -fsanitize=address,undefined.
//
// A case is two flat arrays.  hdr (int64): pb, n, nk, nsmooth, myseg, use_v31, order, min_mass, ngroups, nbin, stabl[3], Lgwbl[3],
// GSglobal[3], pbc[3].  data (double): logkmin, deltalogk, k_for_GM, rad_gm0; z_seg, z_prev; F, InterPartDist, ParticleMass, hfactor,
// mmin, deltam; x[n], comvdist[n], hubble[n], grow[4][nk][n], fomega[4][nk][n], k_GM_displ[nsmooth]; Mass[ngroups], pass[ngroups],
// val[27][ngroups] (Pos, the eight velocities).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../pinocchio_amd/csrc/pf_collapse_core.h"
#include "../../pinocchio_amd/csrc/pf_catalog_core.h"

enum { H_PB, H_N, H_NK, H_NSMOOTH, H_MYSEG, H_USEV31, H_ORDER, H_MINMASS, H_NGROUPS, H_NBIN, H_STABL, H_LEN = H_STABL + 3, H_GS = H_LEN + 3, H_PBC = H_GS + 3, H_COUNT = H_PBC + 3 };
enum { D_TAB = 0, D_SEG = 4, D_F = 6, D_IPD, D_PMASS, D_HFAC, D_MMIN, D_DELTAM, D_X };

template <class T>
static long long run(const PfPlcTab &t, const PfCatGeom &g, const PfPlcSegIn &sg, double Fd, int min_mass, long long ng, const double *mass, const double *pass, const double *val,
                     int nbin, const unsigned int *thr, size_t cap, double *rec, int *index, int *ninbin, unsigned long long *sum) {
  const T F = (T)Fd;   // outputs.F[iout] as set_obj takes it
  long long found = 0;
  for (long long i = 0; i < ng; i++) {
    const int M = (int)mass[i];
    if (!(pass[i] != 0.0 && M >= min_mass)) continue;
    const int b = nbin > 0 ? pf_cat_bin(thr, nbin, M) : -1;
    if (b >= 0) { ninbin[b]++; sum[b] += (unsigned long long)M; }
    if ((size_t)found < cap) {
      PfPlcObj<T> o;
      o.M = M;
      for (int e = 0; e < 3; e++) o.q[e] = (T)val[(size_t)e * ng + i];
      for (int s = 0; s < 8; s++)
        for (int e = 0; e < 3; e++) o.v[s][e] = (T)val[(size_t)(3 + 3 * s + e) * ng + i];
      // the reference's form: everything again for this group
      const PfPlcK k = pf_plc_group_k<T>(t, o.M, g.ipd);
      const PfPlcSeg s = pf_plc_segment_modes(t, sg, k);
      T out[PF_CAT_NREC];
      pf_cat_record<T>(t, g, sg, k, s, o, F, out);
      for (int q = 0; q < PF_CAT_NREC; q++) rec[PF_CAT_NREC * found + q] = (double)out[q];
      index[found] = (int)i;
    }
    found++;
  }
  return found;
}

// -> the number of passing groups (-1: a bad case); the first min(count, cap) records as rec[10 j + (M, x[3], v[3], q[3])] and their
// groups in index; ninbin[nbin] and massinbin[nbin] = (double)(sum of Mass) * ParticleMass are set
extern "C" long long catalog_emul_run(const long long *hdr, const double *d, size_t cap, double *rec, int *index, int *ninbin, double *massinbin) {
  const int n = (int)hdr[H_N], nk = (int)hdr[H_NK], nsmooth = (int)hdr[H_NSMOOTH], nbin = (int)hdr[H_NBIN];
  const long long ng = hdr[H_NGROUPS];
  if (n < 3 || nk < 1 || nk > PF_PLC_MAX_NK || ng < 0 || nbin < 0 || (nk > 1 && nsmooth < 2)) return -1;
  const double *tp = d + D_TAB, *sd = d + D_SEG, *x = d + D_X, *comv = x + n, *hub = comv + n, *grow = hub + n, *fom = grow + (size_t)4 * nk * n, *kgm = fom + (size_t)4 * nk * n;
  const double *mass = kgm + nsmooth, *pass = mass + ng, *val = pass + ng;
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
  PfCatGeom g;
  for (int i = 0; i < 3; i++) { g.stabl[i] = (double)hdr[H_STABL + i]; g.box[i] = (double)hdr[H_LEN + i]; g.ggrid[i] = (double)hdr[H_GS + i]; g.pbc[i] = hdr[H_PBC + i] != 0; }
  g.ipd = d[D_IPD]; g.pmass = d[D_PMASS]; g.hfactor = d[D_HFAC]; g.scale = d[D_IPD] * d[D_HFAC];
  PfPlcSegIn sg;
  sg.myseg = (int)hdr[H_MYSEG]; sg.use_v31 = (int)hdr[H_USEV31]; sg.order = (int)hdr[H_ORDER]; sg.z_seg = sd[0]; sg.z_prev = sd[1];
  std::vector<unsigned int> thr((size_t)nbin + 1);
  std::vector<unsigned long long> sum((size_t)nbin + 1, 0ull);
  if (nbin > 0) pf_cat_thresholds(d[D_MMIN], d[D_DELTAM], nbin, d[D_PMASS], thr.data());
  for (int b = 0; b < nbin; b++) ninbin[b] = 0;
  const long long found = hdr[H_PB] == 8 ? run<double>(t, g, sg, d[D_F], (int)hdr[H_MINMASS], ng, mass, pass, val, nbin, thr.data(), cap, rec, index, ninbin, sum.data())
                                         : run<float>(t, g, sg, d[D_F], (int)hdr[H_MINMASS], ng, mass, pass, val, nbin, thr.data(), cap, rec, index, ninbin, sum.data());
  for (int b = 0; b < nbin; b++) massinbin[b] = (double)sum[b] * d[D_PMASS];
  return found;
}

#ifndef CATALOG_EMUL_LIB
// catalog_emul_san FILE: cases written one after the other as int64 nhdr (= H_COUNT), int64 ndata, hdr, data
int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  long long head[2];
  int ncase = 0;
  while (fread(head, 8, 2, f) == 2) {
    if (head[0] != H_COUNT || head[1] < D_X) { fprintf(stderr, "bad case header\n"); return 2; }
    std::vector<long long> hdr((size_t)head[0]);
    std::vector<double> data((size_t)head[1]);
    if (fread(hdr.data(), 8, hdr.size(), f) != hdr.size() || fread(data.data(), 8, data.size(), f) != data.size()) { fprintf(stderr, "short case\n"); return 2; }
    const size_t cap = (size_t)hdr[H_NGROUPS], nbin = (size_t)hdr[H_NBIN];
    std::vector<double> rec(PF_CAT_NREC * cap + 1), mass(nbin + 1);
    std::vector<int> index(cap + 1), nin(nbin + 1);
    const long long found = catalog_emul_run(hdr.data(), data.data(), cap, rec.data(), index.data(), nin.data(), mass.data());
    double sum = 0.0;
    long long binned = 0;
    for (long long j = 0; j < found; j++) sum += rec[PF_CAT_NREC * j + 1];
    for (size_t b = 0; b < nbin; b++) binned += nin[b];
    printf("case %d: records %lld binned %lld xsum %.17g\n", ncase++, found, binned, sum);
  }
  fclose(f);
  return 0;
}
#endif
