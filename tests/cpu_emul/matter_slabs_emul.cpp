// matter_slabs_emul.cpp -- pinocchio_amd/csrc/pf_matter_slabs_core.h compiled for the host: the plan of pf_matter_power_slabs as plain
// calls, and P emulated ranks on one thread -- reach, windowed deposit, pack, the all-to-all as a copy, fold -- the way pf_matter.hip
// does it by lanes, integer atomics and device copies.  As a library (-DMATTER_SLABS_EMUL_LIB) tests/test_matter_slabs_cpu.py holds
// it against tests/np_matter_slabs.py and tests/np_matter.py; as a program it reads the cases that test wrote and runs them under
// -fsanitize=address,undefined.
//
// Columns of a box are [12][n^3] PRODFLOATs of pb bytes; the slab of rank r is the cells r nxl n^2 .. of every column.
// A case in the file: int64 pb, n, P, flags, has_weight; 4 doubles; the columns.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/pinfmax.h"
#include "../../pinocchio_amd/csrc/pf_matter_slabs_core.h"

typedef unsigned long long u64;

// out: form, B, then (w0, wn) of every rank, then for every (r, q) the length of L(r, q) and its nxl entries (-1 beyond the list)
extern "C" int slabs_emul_plan(int n, int P, int hlo, int hhi, int *out) {
  if (n < 2 || P < 1 || n % P) return 1;
  const int nxl = n / P;
  out[0] = pf_matter_exchange_form(n, P, hlo, hhi);
  out[1] = pf_matter_block_planes(n, P, hlo, hhi);
  for (int r = 0; r < P; r++) pf_matter_window(n, nxl, r * nxl, hlo, hhi, &out[2 + 2 * r], &out[3 + 2 * r]);
  int *p = out + 2 + 2 * P;
  std::vector<int> list(nxl);
  for (int r = 0; r < P; r++)
    for (int q = 0; q < P; q++, p += 1 + nxl) {
      const int len = q == r ? 0 : pf_matter_block_list(n, P, hlo, hhi, r, q, list.data());
      p[0] = len;
      for (int l = 0; l < nxl; l++) p[1 + l] = l < len ? list[l] : -1;
    }
  return 0;
}

// cell i of the slab [x0, x0 + nxl) lies at col[k * stride + i]
template <class T> static void reach_t(int n, int nxl, int x0, const T *col, size_t stride, int flags, const double *w, int *hlo, int *hhi) {
  const size_t nc = (size_t)nxl * n * n;
  *hlo = *hhi = 0;
  for (size_t i = 0; i < nc; i++) {
    const int q0 = x0 + (int)(i / ((size_t)n * n));
    T v[4];
    for (int o = 0; o < 4; o++) v[o] = pf_matter_column<T>(col[(size_t)(3 * o) * stride + i], w, o);
    int smin, smax;
    if (!pf_matter_reach<T>(pf_matter_pos<T>(q0, n, v[0], v[1], v[2], v[3]), q0, n, (flags & PF_MATTER_NGP) ? 1 : 0, &smin, &smax)) continue;
    if (-smin > *hlo) *hlo = -smin;
    if (smax > *hhi) *hhi = smax;
  }
}

// the columns [12][nxl n^2] of one slab -> out[0] = Hlo, out[1] = Hhi
extern "C" int slabs_emul_reach(int pb, int n, int nxl, int x0, const void *vel12_slab, int flags, const double *weight, int *out) {
  if ((pb != 4 && pb != 8) || n < 2 || nxl < 1 || x0 < 0 || x0 + nxl > n) return 1;
  const size_t nc = (size_t)nxl * n * n;
  if (pb == 8) reach_t<double>(n, nxl, x0, (const double *)vel12_slab, nc, flags, weight, &out[0], &out[1]);
  else reach_t<float>(n, nxl, x0, (const float *)vel12_slab, nc, flags, weight, &out[0], &out[1]);
  return 0;
}

struct Window { int w0, wn; std::vector<u64> g; u64 missed; };

template <class T> static void deposit_t(int n, int nxl, int x0, const T *col, size_t stride, int flags, const double *w, Window *win, pf_matter_info *info) {
  const size_t nc = (size_t)nxl * n * n;
  auto add = [&](int cx, int cy, int cz, u64 v) {
    if (!v) return;
    const int lx = pf_matter_window_plane(cx, win->w0, win->wn, n);
    if (lx < 0) { win->missed++; return; }
    win->g[((size_t)lx * n + cy) * n + cz] += v;
  };
  for (size_t i = 0; i < nc; i++) {
    const int q[3] = {x0 + (int)(i / ((size_t)n * n)), (int)(i / n % n), (int)(i % n)};
    T pos[3];
    for (int j = 0; j < 3; j++) {
      T v[4];
      for (int o = 0; o < 4; o++) v[o] = pf_matter_column<T>(col[(size_t)(3 * o + j) * stride + i], w, o);
      pos[j] = pf_matter_pos<T>(q[j], n, v[0], v[1], v[2], v[3]);
    }
    const int cls = pf_matter_class<T>(pos, n);
    if (cls == 1) { info->nonfinite++; continue; }
    if (cls == 2) { info->outside++; continue; }
    info->deposited++;
    if (flags & PF_MATTER_NGP) {
      add(pf_matter_ngp_axis<T>(pos[0], n), pf_matter_ngp_axis<T>(pos[1], n), pf_matter_ngp_axis<T>(pos[2], n), PF_MATTER_ONE);
      continue;
    }
    int cell[3][2];
    uint32_t wt[3][2];
    for (int j = 0; j < 3; j++) pf_matter_cic_axis<T>(pos[j], n, cell[j], wt[j]);
    for (int a = 0; a < 2; a++)
      for (int b = 0; b < 2; b++)
        for (int c = 0; c < 2; c++) add(cell[0][a], cell[1][b], cell[2][c], (u64)wt[0][a] * wt[1][b] * wt[2][c]);
  }
}

// P ranks on the columns of a whole box -> the grid of the box [n^3], the box's counters (modes = 0) and the six numbers of
// pf_debug_matter_exchange.  2: a contribution missed a window (the plan is wrong)
extern "C" int slabs_emul_box(int pb, int n, int P, const void *vel12, int flags, const double *weight, u64 *grid, pf_matter_info *info, u64 *exch) {
  if ((pb != 4 && pb != 8) || n < 2 || P < 1 || n % P) return 1;
  const int nxl = n / P;
  const size_t box = (size_t)n * n * n, plane = (size_t)n * n, slab = (size_t)nxl * plane;
  memset(info, 0, sizeof(*info));
  int hlo = 0, hhi = 0;
  for (int r = 0; r < P; r++) {
    int a, b;
    if (pb == 8) reach_t<double>(n, nxl, r * nxl, (const double *)vel12 + r * slab, box, flags, weight, &a, &b);
    else reach_t<float>(n, nxl, r * nxl, (const float *)vel12 + r * slab, box, flags, weight, &a, &b);
    if (a > hlo) hlo = a;
    if (b > hhi) hhi = b;
  }
  const int form = pf_matter_exchange_form(n, P, hlo, hhi), B = form ? pf_matter_block_planes(n, P, hlo, hhi) : 0;
  std::vector<Window> win(P);
  for (int r = 0; r < P; r++) {
    pf_matter_window(n, nxl, r * nxl, hlo, hhi, &win[r].w0, &win[r].wn);
    win[r].g.assign((size_t)win[r].wn * plane, 0);
    win[r].missed = 0;
    if (pb == 8) deposit_t<double>(n, nxl, r * nxl, (const double *)vel12 + r * slab, box, flags, weight, &win[r], info);
    else deposit_t<float>(n, nxl, r * nxl, (const float *)vel12 + r * slab, box, flags, weight, &win[r], info);
    if (win[r].missed) return 2;
  }
  exch[0] = (u64)form; exch[1] = (u64)hlo; exch[2] = (u64)hhi; exch[3] = (u64)win[0].wn; exch[4] = (u64)B; exch[5] = (u64)B * plane * 8;
  // pack: send[r] = P blocks of B planes; slots beyond a list keep a pattern that must never be added
  std::vector<std::vector<u64>> send(P), recv(P);
  std::vector<int> list(nxl);
  for (int r = 0; form && r < P; r++) {
    send[r].assign((size_t)P * B * plane, 0xDEADBEEFDEADBEEFull);
    recv[r].assign((size_t)P * B * plane, 0);
    for (int q = 0; q < P; q++) {
      if (q == r) continue;
      const int len = pf_matter_block_list(n, P, hlo, hhi, r, q, list.data());
      for (int j = 0; j < len; j++) {
        const int wp = pf_matter_window_plane(q * nxl + list[j], win[r].w0, win[r].wn, n);
        if (wp < 0) return 2;
        memcpy(&send[r][((size_t)q * B + j) * plane], &win[r].g[(size_t)wp * plane], plane * 8);
      }
    }
  }
  // the all-to-all: block q of rank r's send buffer is block r of rank q's receive buffer
  for (int r = 0; form && r < P; r++)
    for (int q = 0; q < P; q++)
      if (B) memcpy(&recv[q][(size_t)r * B * plane], &send[r][(size_t)q * B * plane], (size_t)B * plane * 8);
  // fold and hand out the rank's own planes
  for (int r = 0; r < P; r++) {
    const int own = pf_matter_window_plane(r * nxl, win[r].w0, win[r].wn, n);
    if (own < 0 || own + nxl > win[r].wn) return 2;
    u64 *mine = &win[r].g[(size_t)own * plane];
    for (int p = 0; form && p < P; p++) {
      if (p == r) continue;
      const int len = pf_matter_block_list(n, P, hlo, hhi, p, r, list.data());
      for (int j = 0; j < len; j++)
        for (size_t i = 0; i < plane; i++) mine[(size_t)list[j] * plane + i] += recv[r][((size_t)p * B + j) * plane + i];
    }
    memcpy(grid + (size_t)r * slab, mine, slab * 8);
  }
  for (size_t i = 0; i < box; i++) {
    info->empty_cells += grid[i] == 0;
    if (grid[i] > info->max_cell) info->max_cell = grid[i];
    info->sum_hi32 += grid[i] >> 32; info->sum_lo32 += grid[i] & 0xffffffffull;
  }
  return 0;
}

#ifndef MATTER_SLABS_EMUL_LIB
// matter_slabs_emul_san FILE
int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  long long head[5];
  int ncase = 0;
  while (fread(head, 8, 5, f) == 5) {
    double w[4];
    if (fread(w, 8, 4, f) != 4) { fprintf(stderr, "short case\n"); return 2; }
    const int pb = (int)head[0], n = (int)head[1], P = (int)head[2], flags = (int)head[3];
    if ((pb != 4 && pb != 8) || head[1] < 2 || head[1] > 64 || head[2] < 1 || head[1] % head[2]) { fprintf(stderr, "bad case header\n"); return 2; }
    const size_t nc = (size_t)n * n * n;
    std::vector<char> col(12 * nc * pb);   // exactly the sizes: a read or write beyond them is the sanitizer's to find
    std::vector<u64> grid(nc);
    if (fread(col.data(), 1, col.size(), f) != col.size()) { fprintf(stderr, "short case\n"); return 2; }
    pf_matter_info info;
    u64 exch[6];
    const int rc = slabs_emul_box(pb, n, P, col.data(), flags, head[4] ? w : nullptr, grid.data(), &info, exch);
    if (rc) { fprintf(stderr, "ERROR: case %d returned %d\n", ncase, rc); return 2; }
    const int nxl = n / P;
    std::vector<int> plan(2 + 2 * (size_t)P + (size_t)P * P * (1 + nxl));   // the plan with arrays of exactly its size, too
    if (slabs_emul_plan(n, P, (int)exch[1], (int)exch[2], plan.data())) return 2;
    u64 h = 1469598103934665603ull;   // FNV-1a of the grid's words
    for (size_t i = 0; i < nc; i++) { h ^= grid[i]; h *= 1099511628211ull; }
    printf("case %d: deposited %llu nonfinite %llu outside %llu empty %llu max %llu hi %llu lo %llu hash %llu form %llu below %llu above %llu window %llu block %llu bytes %llu\n",
           ncase++, info.deposited, info.nonfinite, info.outside, info.empty_cells, info.max_cell, info.sum_hi32, info.sum_lo32, h, exch[0], exch[1], exch[2], exch[3],
           exch[4], exch[5]);
  }
  fclose(f);
  return 0;
}
#endif
