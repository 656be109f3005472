// map_emul.cpp -- pinocchio_amd/csrc/pf_map_core.h compiled for the host: the kernels of pf_map.hip walked lane by lane on the CPU.
//   emul_fill_box   k_map_box: one (row, word) pair per lane; full words stored, shared words ORed
//   emul_update     k_map_spheres: items found by bisection in the prefix, 64 lanes per round, ballots formed by a loop over the
//                   lanes, one OR per run (words != 0) or per bit (words == 0); returns the number of ORs ("atomics")
// tests/test_maps_cpu.py holds both against the numpy restatement (tests/np_maps.py).  With -DMAP_EMUL_MAIN the file is a program
// that runs seeded cases against a literal port of update_map()'s loops, for a build with -fsanitize=address,undefined.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../pinocchio_amd/csrc/pf_map_core.h"

static PfMapBox box_of(const int *len, const int *pbc) {
  PfMapBox b;
  for (int d = 0; d < 3; d++) { b.len[d] = len[d]; b.pbc[d] = pbc[d]; }
  return b;
}

extern "C" long long emul_fill_box(const int *len, const int *safe, const int *pbc, unsigned int *upd) {
  const PfMapBox b = box_of(len, pbc);
  const unsigned long long cells = (unsigned long long)len[0] * len[1] * len[2], nwords = (cells + 31) / 32;
  memset(upd, 0, nwords * sizeof(unsigned int));
  int lo[3], hi[3];
  for (int d = 0; d < 3; d++) pf_map_box_range(len[d], safe[d], pbc[d], &lo[d], &hi[d]);
  const unsigned long long nrows = (unsigned long long)(hi[0] - lo[0]) * (unsigned long long)(hi[1] - lo[1]);
  const unsigned int wpr = (unsigned int)(hi[2] - lo[2] + 30) / 32 + 1;
  long long ors = 0;
  for (unsigned long long t = 0; t < nrows * wpr; t++) {
    const unsigned long long r = t / wpr, q = t - r * wpr;
    unsigned long long first; unsigned int length;
    pf_map_box_row(b, lo, hi, r, &first, &length);
    const unsigned long long word = (first >> 5) + q;
    if (word > ((first + length - 1) >> 5)) continue;
    if (word >= nwords) return -1;
    const unsigned int mask = pf_map_word_mask(first, length, word);
    if (mask == 0xFFFFFFFFu) { if (upd[word]) return -2; upd[word] = mask; }   // a plain store must own its word
    else { upd[word] |= mask; ors++; }
  }
  return ors;
}

static PfMapGroup group_of(const double *pos, int mass, double blf) {
  PfMapGroup g;
  g.ig = (int)(pos[0] + 0.5); g.jg = (int)(pos[1] + 0.5); g.kg = (int)(pos[2] + 0.5);
  g.size = (int)(blf * pow((double)mass / 4.188790205, 0.333333333333333) + 0.5);
  return g;
}

extern "C" long long emul_update(const int *len, const int *pbc, int ngroups, const double *pos, const int *mass, double blf,
                                 const unsigned int *cur, unsigned int *upd, unsigned long long *nadd, int words) {
  const PfMapBox b = box_of(len, pbc);
  const unsigned long long cells = (unsigned long long)len[0] * len[1] * len[2], nwords = (cells + 31) / 32;
  memset(upd, 0, nwords * sizeof(unsigned int));
  nadd[0] = nadd[1] = 0;
  std::vector<PfMapGroup> groups(ngroups);
  std::vector<unsigned long long> prefix(ngroups + 1);
  unsigned long long items = 0;
  for (int g = 0; g < ngroups; g++) { groups[g] = group_of(pos + 3 * g, mass[g], blf); prefix[g] = items; items += pf_map_items(groups[g].size); }
  prefix[ngroups] = items;
  long long ors = 0;
  for (unsigned long long item = 0; item < items; item++) {
    unsigned int lo = 0, hi = (unsigned int)ngroups;
    while (hi - lo > 1) { const unsigned int mid = lo + ((hi - lo) >> 1); if (prefix[mid] <= item) lo = mid; else hi = mid; }
    const PfMapGroup g = groups[lo];
    const unsigned long long local = item - prefix[lo];
    for (int ch = 0; ch < pf_map_chunks(g.size); ch++) {
      PfMapCell cell[64];
      bool live[64], set[64];
      unsigned long long flags = 0, heads = 0;
      for (int lane = 0; lane < 64; lane++) {
        cell[lane] = pf_map_cell(b, g, local, ch, lane);
        live[lane] = cell[lane].valid && !cell[lane].out;
        set[lane] = false;
        if (live[lane]) {
          if (cell[lane].pos >= cells) return -1;
          if (cell[lane].inside) set[lane] = !((cur[cell[lane].pos >> 5] >> (cell[lane].pos & 31u)) & 1u);
        }
        if (set[lane]) { nadd[0]++; flags |= 1ull << lane; }
        if (cell[lane].valid && cell[lane].out) nadd[1]++;
      }
      if (!words) {
        for (int lane = 0; lane < 64; lane++) if (set[lane]) { upd[cell[lane].pos >> 5] |= 1u << (cell[lane].pos & 31u); ors++; }
        continue;
      }
      if (!flags) continue;
      for (int lane = 0; lane < 64; lane++) {
        const int prev = lane ? lane - 1 : 0;   // __shfl_up(., 1): lane 0 reads itself
        if (pf_map_run_head(lane, live[lane], live[prev], cell[lane].pos, cell[prev].pos)) heads |= 1ull << lane;
      }
      for (int lane = 0; lane < 64; lane++)
        if (((heads >> lane) & 1ull) && live[lane]) {
          const unsigned int mask = pf_map_run_mask(heads, flags, lane, cell[lane].pos);
          // every bit of the mask must be the bit of a lane of the run that sets it
          unsigned int want = 0;
          for (int l2 = lane; l2 < 64 && (l2 == lane || !((heads >> l2) & 1ull)); l2++) {
            if ((cell[l2].pos >> 5) != (cell[lane].pos >> 5)) return -3;
            if (set[l2]) want |= 1u << (cell[l2].pos & 31u);
          }
          if (mask != want) return -4;
          if (mask) { upd[cell[lane].pos >> 5] |= mask; ors++; }
        }
    }
  }
  return ors;
}

#ifdef MAP_EMUL_MAIN
// update_map(), src/build_groups.c:2246-2318, on a bit array
static void literal(const int *len, const int *pbc, int ngroups, const double *pos, const int *mass, double blf, const unsigned int *cur,
                    unsigned int *upd, unsigned long long *nadd) {
  const unsigned long long cells = (unsigned long long)len[0] * len[1] * len[2];
  memset(upd, 0, ((cells + 31) / 32) * sizeof(unsigned int));
  nadd[0] = nadd[1] = 0;
  for (int g = 0; g < ngroups; g++) {
    const PfMapGroup q = group_of(pos + 3 * g, mass[g], blf);
    for (int i1 = q.ig - q.size; i1 < q.ig + q.size; i1++)
      for (int j1 = q.jg - q.size; j1 < q.jg + q.size; j1++)
        for (int k1 = q.kg - q.size; k1 < q.kg + q.size; k1++) {
          const int c1[3] = {i1, j1, k1};
          int c[3];
          for (int d = 0; d < 3; d++) {
            if (c1[d] < 0 || c1[d] >= len[d]) c[d] = pbc[d] ? (c1[d] < 0 ? c1[d] + len[d] : c1[d] - len[d]) : -1;
            else c[d] = c1[d];
          }
          if (c[0] < 0 || c[1] < 0 || c[2] < 0) { nadd[1]++; continue; }
          const unsigned long long p = (unsigned long long)c[2] + (unsigned long long)len[2] * ((unsigned long long)c[1] + (unsigned long long)len[1] * c[0]);
          if (!((cur[p >> 5] >> (p & 31)) & 1u)) {
            const int rr = (i1 - q.ig) * (i1 - q.ig) + (j1 - q.jg) * (j1 - q.jg) + (k1 - q.kg) * (k1 - q.kg);
            if (rr <= q.size * q.size) { upd[p >> 5] |= 1u << (p & 31); nadd[0]++; }
          }
        }
  }
}

int main() {
  const int cases[4][9] = {   // len[3], safe[3], pbc[3]
      {20, 23, 37, 4, 4, 4, 0, 0, 0}, {32, 22, 32, 0, 5, 0, 1, 0, 1}, {16, 16, 16, 0, 0, 0, 1, 1, 1}, {40, 9, 70, 1, 1, 1, 0, 0, 0}};
  unsigned int seed = 12345;
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (seed >> 8) / 16777216.0; };
  for (int c = 0; c < 4; c++) {
    const int *len = cases[c], *safe = cases[c] + 3, *pbc = cases[c] + 6;
    const size_t nwords = ((size_t)len[0] * len[1] * len[2] + 31) / 32;
    std::vector<unsigned int> cur(nwords), a(nwords), bw(nwords), bb(nwords);
    if (emul_fill_box(len, safe, pbc, cur.data()) < 0) { printf("case %d: fill failed\n", c); return 1; }
    if (c == 3) for (auto &w : cur) w &= 0x0F0F3C5Au;   // a ragged current map
    const int ng = 60;
    std::vector<double> pos(3 * ng);
    std::vector<int> mass(ng);
    int minlen = len[0] < len[1] ? len[0] : len[1];
    if (len[2] < minlen) minlen = len[2];
    for (int g = 0; g < ng; g++) {
      for (int d = 0; d < 3; d++) pos[3 * g + d] = pbc[d] ? rnd() * (len[d] - 0.6) : -3.0 + rnd() * (len[d] + 6.0);
      mass[g] = 1 + (int)(rnd() * rnd() * 3000.0);
      while ((int)(2.0 * pow(mass[g] / 4.188790205, 0.333333333333333) + 0.5) > minlen) mass[g] /= 2;
    }
    unsigned long long n0[2], n1[2], n2[2];
    literal(len, pbc, ng, pos.data(), mass.data(), 2.0, cur.data(), a.data(), n0);
    const long long ow = emul_update(len, pbc, ng, pos.data(), mass.data(), 2.0, cur.data(), bw.data(), n1, 1);
    const long long ob = emul_update(len, pbc, ng, pos.data(), mass.data(), 2.0, cur.data(), bb.data(), n2, 0);
    if (ow < 0 || ob < 0 || a != bw || a != bb || n0[0] != n1[0] || n0[1] != n1[1] || n0[0] != n2[0] || n0[1] != n2[1]) {
      printf("case %d: mismatch (%lld %lld) nadd %llu %llu / %llu %llu\n", c, ow, ob, n0[0], n0[1], n1[0], n1[1]);
      return 1;
    }
    printf("case %d: nadd %llu %llu, %lld word ORs against %lld bit ORs\n", c, n0[0], n0[1], ow, ob);
  }
  return 0;
}
#endif
