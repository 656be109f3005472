// map_emul.cpp -- pinocchio_amd/csrc/pf_map_core.h compiled for the host: the kernels of pf_map.hip walked lane by lane on the CPU.
//   emul_fill_box   k_map_box: one (row, word) pair per lane; full words stored, shared words ORed
//   emul_update     k_map_spheres: items found by bisection in the prefix, 64 lanes per round, ballots formed by a loop over the
//                   lanes, one OR per run (words != 0) or per bit (words == 0); returns the number of ORs ("atomics")
//   emul_fill_words / emul_update_sparse   the same two for sub-boxes of up to 2^32 cells: the words a caller asks for, and the
//                   words the spheres touch, with no array over the cells or the words of the map
// tests/test_maps_cpu.py holds the first two against the numpy restatement (tests/np_maps.py), tests/test_large_index_cpu.py the
// sparse ones against its sparse forms.  With -DMAP_EMUL_MAIN the file is a program that runs seeded cases, and the production-size
// boxes of large_boxes.h, against a literal port of update_map()'s loops, for a build with -fsanitize=address,undefined.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <vector>

#include "../../pinocchio_amd/csrc/pf_map_core.h"
#include "large_boxes.h"

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

// k_map_spheres walked item by item: curbit(pos) reads CURRENT, orword(word, mask) is the atomicOr into UPDATE
template <typename Cur, typename Or>
static long long update_core(const PfMapBox &b, unsigned long long cells, int ngroups, const double *pos, const int *mass, double blf, Cur curbit, Or orword,
                             unsigned long long *nadd, int words) {
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
          if (cell[lane].inside) set[lane] = !curbit(cell[lane].pos);
        }
        if (set[lane]) { nadd[0]++; flags |= 1ull << lane; }
        if (cell[lane].valid && cell[lane].out) nadd[1]++;
      }
      if (!words) {
        for (int lane = 0; lane < 64; lane++) if (set[lane]) { orword(cell[lane].pos >> 5, 1u << (cell[lane].pos & 31u)); ors++; }
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
          if (mask) { orword(cell[lane].pos >> 5, mask); ors++; }
        }
    }
  }
  return ors;
}

extern "C" long long emul_update(const int *len, const int *pbc, int ngroups, const double *pos, const int *mass, double blf,
                                 const unsigned int *cur, unsigned int *upd, unsigned long long *nadd, int words) {
  const PfMapBox b = box_of(len, pbc);
  const unsigned long long cells = (unsigned long long)len[0] * len[1] * len[2], nwords = (cells + 31) / 32;
  memset(upd, 0, nwords * sizeof(unsigned int));
  return update_core(b, cells, ngroups, pos, mass, blf, [&](unsigned long long p) { return (bool)((cur[p >> 5] >> (p & 31ull)) & 1u); },
                     [&](unsigned long long w, unsigned int mask) { upd[w] |= mask; }, nadd, words);
}

// ---- the sparse forms, for sub-boxes of up to 2^32 cells: no array over the cells or the words of the map ----
// whether bit p lies in the box [lo, hi) of create_map; the coordinates by plain division, not by the header
static bool in_ranges(const int *len, const int *lo, const int *hi, unsigned long long p) {
  const long long k = (long long)(p % (unsigned long long)len[2]), r = (long long)(p / (unsigned long long)len[2]), j = r % len[1], i = r / len[1];
  return i >= lo[0] && i < hi[0] && j >= lo[1] && j < hi[1] && k >= lo[2] && k < hi[2];
}

// k_map_box for the words word[0 .. count - 1] alone: every row of the box that shares bits with a word is looked up as the lane of
// that (row, word) pair looks it up.  -1: the kernel would write beyond the map; -5: the pair lies beyond the words a row is given
extern "C" long long emul_fill_words(const int *len, const int *safe, const int *pbc, size_t count, const unsigned long long *word, unsigned int *mask) {
  const PfMapBox b = box_of(len, pbc);
  const unsigned long long cells = (unsigned long long)len[0] * len[1] * len[2], nwords = (cells + 31) / 32;
  int lo[3], hi[3];
  for (int d = 0; d < 3; d++) pf_map_box_range(len[d], safe[d], pbc[d], &lo[d], &hi[d]);
  const unsigned long long ny = (unsigned long long)(hi[1] - lo[1]);
  const unsigned int wpr = (unsigned int)(hi[2] - lo[2] + 30) / 32 + 1;
  long long pairs = 0;
  for (size_t q = 0; q < count; q++) {
    mask[q] = 0;
    if (word[q] >= nwords) return -1;
    const unsigned long long p0 = word[q] * 32ull, p1 = p0 + 31ull < cells - 1 ? p0 + 31ull : cells - 1;
    for (unsigned long long g = p0 / (unsigned long long)len[2]; g <= p1 / (unsigned long long)len[2]; g++) {   // z-rows j + Ly i that hold bits of the word
      const long long i = (long long)(g / (unsigned long long)len[1]), j = (long long)(g % (unsigned long long)len[1]);
      if (i < lo[0] || i >= hi[0] || j < lo[1] || j >= hi[1]) continue;
      unsigned long long first; unsigned int length;
      pf_map_box_row(b, lo, hi, (unsigned long long)(i - lo[0]) * ny + (unsigned long long)(j - lo[1]), &first, &length);
      if (first + length > cells) return -1;
      const unsigned int m = pf_map_word_mask(first, length, word[q]);
      if (!m) continue;
      if (word[q] < (first >> 5) || word[q] - (first >> 5) >= wpr) return -5;
      mask[q] |= m; pairs++;
    }
  }
  return pairs;
}

// k_map_spheres with CURRENT = the box [cur_lo, cur_hi) of create_map (null: empty) and UPDATE kept as the words that were ORed: the
// first min(*nout, cap) of them, ascending, in out_word / out_mask
extern "C" long long emul_update_sparse(const int *len, const int *pbc, int ngroups, const double *pos, const int *mass, double blf, const int *cur_lo,
                                        const int *cur_hi, size_t cap, unsigned long long *out_word, unsigned int *out_mask, size_t *nout,
                                        unsigned long long *nadd, int words) {
  const PfMapBox b = box_of(len, pbc);
  const unsigned long long cells = (unsigned long long)len[0] * len[1] * len[2];
  std::map<unsigned long long, unsigned int> upd;
  const long long ors = update_core(b, cells, ngroups, pos, mass, blf, [&](unsigned long long p) { return cur_lo && in_ranges(len, cur_lo, cur_hi, p); },
                                    [&](unsigned long long w, unsigned int mask) { upd[w] |= mask; }, nadd, words);
  *nout = upd.size();
  size_t q = 0;
  for (const auto &e : upd) { if (q >= cap) break; out_word[q] = e.first; out_mask[q] = e.second; q++; }
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
  // the production-size boxes: spheres of sizes 1 .. 40 at the far corner, across position 2^31, at the origin and on the faces of the
  // periodic directions, on the map create_map leaves and on an empty one; the loops of update_map() keep the bits they set in a
  // std::map.  Then create_map itself at the words around the ends of the map, of position 2^31 and of random z-rows
  unsigned long long s64 = 4242;
  auto rnd31 = [&]() { s64 = s64 * 6364136223846793005ull + 1442695040888963407ull; return (unsigned int)(s64 >> 33); };
  for (const LargeBox &lb : LARGE_BOXES) {
    const int *len = lb.len;
    int pbc[3], lo[3], hi[3];
    for (int d = 0; d < 3; d++) { pbc[d] = lb.safe[d] == 0; pf_map_box_range(len[d], lb.safe[d], pbc[d], &lo[d], &hi[d]); }
    const unsigned long long cells = large_cells(len), mid = 1ull << 31;
    const double at31[3] = {(double)(mid / ((unsigned long long)len[1] * len[2])), (double)((mid / len[2]) % len[1]), (double)(mid % len[2])};
    std::vector<double> pos = {len[0] - 1.0, len[1] - 1.0, len[2] - 1.0, len[0] - 9.0, len[1] - 3.0, len[2] - 20.0, at31[0], at31[1], at31[2], 0.0, 0.0, 0.0, 3.0, 1.0, 30.0};
    for (int d = 0; d < 3; d++)
      if (pbc[d])
        for (const double face : {0.0, 2.0, len[d] - 1.0, len[d] - 7.0}) {
          double c[3] = {len[0] / 2 + (double)(rnd31() % 40), len[1] / 2 + (double)(rnd31() % 40), len[2] / 2 + (double)(rnd31() % 40)};
          c[d] = face;
          pos.insert(pos.end(), c, c + 3);
        }
    const int ng = (int)(pos.size() / 3);
    std::vector<int> mass(ng);
    for (int g = 0; g < ng; g++) {
      const int size = g < 4 ? (g == 0 ? 1 : g == 1 ? 2 : g == 2 ? 40 : 33) : 1 + (int)(rnd31() % 40);
      mass[g] = (int)(4.188790205 * (pow((size - 0.5) / 2.0, 3) + pow((size + 0.5) / 2.0, 3)) / 2.0);
      if (mass[g] < 1) mass[g] = 1;
      if (group_of(&pos[3 * g], mass[g], 2.0).size != size) { printf("case %s: a mass of %d does not give size %d\n", lb.name, mass[g], size); return 1; }
    }
    unsigned long long runs = 0, bits = 0, nadd_box[2] = {0, 0};
    for (int filled = 1; filled >= 0; filled--) {
      std::map<unsigned long long, unsigned int> want;
      unsigned long long n0[2] = {0, 0};
      for (int g = 0; g < ng; g++) {   // update_map(), :2246-2318
        const PfMapGroup q = group_of(&pos[3 * g], mass[g], 2.0);
        for (int i1 = q.ig - q.size; i1 < q.ig + q.size; i1++)
          for (int j1 = q.jg - q.size; j1 < q.jg + q.size; j1++)
            for (int k1 = q.kg - q.size; k1 < q.kg + q.size; k1++) {
              const int c1[3] = {i1, j1, k1};
              int c[3];
              for (int d = 0; d < 3; d++) {
                if (c1[d] < 0 || c1[d] >= len[d]) c[d] = pbc[d] ? (c1[d] < 0 ? c1[d] + len[d] : c1[d] - len[d]) : -1;
                else c[d] = c1[d];
              }
              if (c[0] < 0 || c[1] < 0 || c[2] < 0) { n0[1]++; continue; }
              const unsigned long long p = (unsigned long long)c[2] + (unsigned long long)len[2] * ((unsigned long long)c[1] + (unsigned long long)len[1] * c[0]);
              const bool cur = filled && c[0] >= lo[0] && c[0] < hi[0] && c[1] >= lo[1] && c[1] < hi[1] && c[2] >= lo[2] && c[2] < hi[2];
              if (!cur) {
                const int rr = (i1 - q.ig) * (i1 - q.ig) + (j1 - q.jg) * (j1 - q.jg) + (k1 - q.kg) * (k1 - q.kg);
                if (rr <= q.size * q.size) { want[p >> 5] |= 1u << (p & 31); n0[0]++; }
              }
            }
      }
      if (!filled && (want.empty() || want.rbegin()->first != (cells - 1) >> 5 || !want.count(mid >> 5))) { printf("case %s: the spheres miss the far corner or 2^31\n", lb.name); return 1; }
      for (int words = 1; words >= 0; words--) {
        std::vector<unsigned long long> ow(want.size() + 1);
        std::vector<unsigned int> om(want.size() + 1);
        size_t nout = 0;
        unsigned long long n1[2];
        const long long ors = emul_update_sparse(len, pbc, ng, pos.data(), mass.data(), 2.0, filled ? lo : nullptr, filled ? hi : nullptr, ow.size(), ow.data(), om.data(), &nout, n1, words);
        bool same = ors >= 0 && nout == want.size() && n1[0] == n0[0] && n1[1] == n0[1];
        size_t q = 0;
        for (auto e = want.begin(); same && e != want.end(); ++e, ++q) same = ow[q] == e->first && om[q] == e->second;
        if (!same) { printf("case %s: mismatch (%lld) nadd %llu %llu / %llu %llu, %zu / %zu touched\n", lb.name, ors, n0[0], n0[1], n1[0], n1[1], want.size(), nout); return 1; }
        if (!filled) (words ? runs : bits) = (unsigned long long)ors;
      }
      if (filled) { nadd_box[0] = n0[0]; nadd_box[1] = n0[1]; }
    }
    // create_map
    const unsigned long long nwords = (cells + 31) / 32, nrows = (unsigned long long)len[0] * len[1];
    std::vector<unsigned long long> word = {0ull, nwords - 1, (mid >> 5) - 1, mid >> 5};
    for (int q = 0; q < 20000; q++) {
      const unsigned long long r = ((((unsigned long long)rnd31() << 31) | rnd31()) % nrows) * (unsigned long long)len[2];
      word.push_back(r >> 5); word.push_back((r + len[2] - 1) >> 5);
      word.push_back((((unsigned long long)rnd31() << 31) | rnd31()) % nwords);
    }
    std::vector<unsigned int> mask(word.size());
    if (emul_fill_words(len, lb.safe, pbc, word.size(), word.data(), mask.data()) < 0) { printf("case %s: fill failed\n", lb.name); return 1; }
    for (size_t q = 0; q < word.size(); q++) {
      unsigned int m = 0;
      for (unsigned long long p = word[q] * 32; p < word[q] * 32 + 32 && p < cells; p++) m |= (unsigned int)in_ranges(len, lo, hi, p) << (p & 31);
      if (m != mask[q]) { printf("case %s: mismatch at word %llu of create_map\n", lb.name, word[q]); return 1; }
    }
    printf("large box %s (%d %d %d): nadd %llu %llu beside the box, %llu runs against %llu bits on an empty map, %zu words of create_map\n", lb.name, len[0], len[1], len[2],
           nadd_box[0], nadd_box[1], runs, bits, word.size());
  }
  return 0;
}
#endif
