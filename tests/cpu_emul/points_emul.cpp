// points_emul.cpp -- pinocchio_amd/csrc/pf_points_core.h compiled for the host and run particle by particle on one thread: the cell of
// a stored particle (pf_refresh_core.h), the tables of the call (pf_point_plan, copied into the small array as pf_points.hip copies
// them), the segment's growing modes once, then pf_point_state for every found particle.  As a library (-DPOINTS_EMUL_LIB)
// tests/test_points_cpu.py holds it against tests/np_points.py and profiles/tools/points_time.py times it; as a program it reads the
// cases that test wrote and runs them under -fsanitize=address,undefined.
//
// A case is two flat arrays.  hdr (int64): pb, n (knots), nk, myseg, use_v31, order, lpt_order, ngrid, x0, nxl, count, start[3],
// len[3].  data (double): logkmin, deltalogk, k_for_GM; z_seg, z_prev; sigma0, k_sigma, k_point; x[n], grow[4][nk][n];
// frag_pos[count]; fmax[nxl ngrid^2]; cols24[24][nxl ngrid^2].
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../pinocchio_amd/csrc/pf_collapse_core.h"
#include "../../pinocchio_amd/csrc/pf_points_core.h"

enum { H_PB, H_N, H_NK, H_MYSEG, H_USEV31, H_ORDER, H_LPT, H_NGRID, H_X0, H_NXL, H_COUNT_P, H_START, H_LEN = H_START + 3, H_COUNT = H_LEN + 3 };
enum { D_TAB = 0, D_SEG = 3, D_PAR = 5, D_X = 8 };

template <class T>
static long long run(const PfPlcTab &t, const PfPointGeom &g, const PfPlcSegIn &sg, const PfPointPlan &plan, const PfBackBox &b, long long count, const double *pos,
                     const double *fmax, const double *cols, size_t ncell, size_t cap, double *rec, unsigned int *index) {
  const PfPlcSeg seg = pf_point_segment_modes(t, sg, plan.kp, g.nw);   // once per call
  long long found = 0;
  for (long long i = 0; i < count; i++) {
    const unsigned int p = (unsigned int)pos[i];
    size_t addr = 0;
    if (!pf_refresh_cell(b, p, &addr)) continue;
    if ((size_t)found < cap) {
      int c[3];
      pf_neigh_coord(b.box, p, c);
      PfPlcObj<T> o;
      o.M = 1;
      for (int d = 0; d < 3; d++) o.q[d] = (T)((double)c[d] + PF_POINT_SHIFT);
      for (int s = 0; s < 8; s++)
        for (int e = 0; e < 3; e++) o.v[s][e] = (T)cols[(size_t)(3 * s + e) * ncell + addr];
      T out[PF_POINT_NREC];
      pf_point_state<T>(t, g, sg, plan.kp, plan.ks, seg, o, (T)fmax[addr], out);
      for (int q = 0; q < PF_POINT_NREC; q++) rec[PF_POINT_NREC * found + q] = (double)out[q];
      index[found] = (unsigned int)i;
    }
    found++;
  }
  return found;
}

// -> the number of found particles (-1: a bad case); the first min(found, cap) states as rec[8 j + ...] and their particles in index
extern "C" long long points_emul_run(const long long *hdr, const double *d, size_t cap, double *rec, unsigned int *index) {
  const int n = (int)hdr[H_N], nk = (int)hdr[H_NK], ngrid = (int)hdr[H_NGRID], x0 = (int)hdr[H_X0], nxl = (int)hdr[H_NXL];
  const long long count = hdr[H_COUNT_P];
  if (n < 3 || nk < 1 || nk > PF_PLC_MAX_NK || count < 0 || ngrid < 1 || x0 < 0 || nxl < 1 || x0 + nxl > ngrid) return -1;
  const size_t ncell = (size_t)nxl * ngrid * ngrid;
  const double *tp = d + D_TAB, *sd = d + D_SEG, *par = d + D_PAR, *x = d + D_X, *grow = x + n, *pos = grow + (size_t)4 * nk * n, *fmax = pos + count, *cols = fmax + ncell;
  // the full array as pf_plc_set_cosmology lays it out; a point reads neither COMVDIST, Hubble nor the fomega families: left zero
  const int total = pf_plc_tab_doubles(n, nk, 0);
  std::vector<double> blob((size_t)total, 0.0);
  memcpy(blob.data(), x, (size_t)n * 8);
  for (int f = 0; f < 4; f++)
    for (int j = 0; j < nk; j++) {
      const double *y = grow + ((size_t)f * nk + j) * n;
      double *dst = blob.data() + n + (size_t)4 * n * (2 + nk * f + j);
      memcpy(dst, y, (size_t)n * 8);
      pf_spline_coeffs(x, y, n, dst + n);
      pf_spline_bd(x, y, dst + n, n, dst + 2 * n, dst + 3 * n);
    }
  PfPlcTab full;
  full.g = blob.data(); full.s = nullptr; full.ns = 0; full.n = n; full.nk = nk;
  full.logkmin = tp[0]; full.dlogk = tp[1]; full.k_for_GM = tp[2]; full.rad_gm0 = 0.0; full.kmin = pow(10., tp[0]); full.kmax = pow(10., tp[0] + (nk - 1) * tp[1]);
  full.nsmooth = 0; full.kgm_at = total;
  const PfPointPlan plan = pf_point_plan(full, par[2], par[1]);
  std::vector<double> small((size_t)plan.doubles, 0.0);
  memcpy(small.data(), blob.data(), (size_t)n * 8);
  for (int j = 0; j < plan.ntab; j++)
    if (plan.src[j] >= 0) memcpy(small.data() + n + (size_t)4 * n * j, blob.data() + n + (size_t)4 * n * plan.src[j], (size_t)4 * n * 8);
  const PfPlcTab t = pf_point_tab(full, plan, small.data());
  const int lpt = (int)hdr[H_LPT];
  PfPlcSegIn sg;
  sg.myseg = (int)hdr[H_MYSEG]; sg.use_v31 = (int)hdr[H_USEV31]; sg.order = (int)hdr[H_ORDER] < lpt ? (int)hdr[H_ORDER] : lpt; sg.z_seg = sd[0]; sg.z_prev = sd[1];
  PfBackBox b;
  for (int i = 0; i < 3; i++) {
    b.box.len[i] = (int)hdr[H_LEN + i]; b.box.pbc[i] = hdr[H_LEN + i] == ngrid; b.box.safe[i] = 0;
    b.start[i] = (int)(((hdr[H_START + i] % ngrid) + ngrid) % ngrid);
  }
  b.n = ngrid; b.x0 = x0; b.nxl = nxl;
  PfPointGeom g;
  for (int i = 0; i < 3; i++) { g.box[i] = (double)b.box.len[i]; g.pbc[i] = b.box.pbc[i]; }
  g.sigma0 = par[0]; g.nw = lpt >= 3 ? 4 : lpt == 2 ? 2 : 1;
  return hdr[H_PB] == 8 ? run<double>(t, g, sg, plan, b, count, pos, fmax, cols, ncell, cap, rec, index)
                        : run<float>(t, g, sg, plan, b, count, pos, fmax, cols, ncell, cap, rec, index);
}

#ifndef POINTS_EMUL_LIB
// points_emul_san FILE: cases written one after the other as int64 nhdr (= H_COUNT), int64 ndata, hdr, data
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
    const size_t cap = (size_t)hdr[H_COUNT_P];
    std::vector<double> rec(PF_POINT_NREC * cap + 1);
    std::vector<unsigned int> index(cap + 1);
    const long long found = points_emul_run(hdr.data(), data.data(), cap, rec.data(), index.data());
    double sum = 0.0;
    for (long long j = 0; j < found; j++) sum += rec[PF_POINT_NREC * j + 5];
    printf("case %d: found %lld xsum %.17g\n", ncase++, found, sum);
  }
  fclose(f);
  return 0;
}
#endif
