// Host build of pinocchio_amd/csrc/pf_distribute_boxes.h for tests/test_distribute_boxes.py: intersection() as the device code
// restates it, and the three passes of csrc/pf_distribute.hip (flag, scan, pack) walked lane by lane on the CPU with the header's box
// table and cell arithmetic -- the decomposition into wavefront slots, masks, workgroup counts and ranks, without the GPU.
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../pinocchio_amd/csrc/pf_distribute_boxes.h"

extern "C" int emul_intersection(int n, const int *fbox, const int *sbox, int *out48) {
  PfDistBox b[8];
  const int nb = pf_dist_intersection(n, fbox, sbox, b);
  for (int i = 0; i < nb; i++)
    for (int d = 0; d < 3; d++) { out48[6 * i + d] = b[i].start[d]; out48[6 * i + 3 + d] = b[i].len[d]; }
  return nb;
}

// returns the number taken, -1 / -2 for the refusals of pf_dist_table_fill; the first min(count, capacity) entries are written
extern "C" long long emul_distribute(int n, int x0, int nxl, const float *fmax, double flast, const int *start, const int *len,
                                     const unsigned int *map, unsigned long long capacity, unsigned int *frag_pos, unsigned int *cell_index) {
  PfDistTable t;
  int bad = 0;
  const int why = pf_dist_table_fill(n, x0, nxl, start, len, &t, &bad);
  if (why) return -why;
  float thr = (float)flast;
  if ((double)thr < flast) thr = nextafterf(thr, INFINITY);
  const unsigned long long nslots = t.ngroups * PF_DIST_GROUP_WAVES;
  std::vector<unsigned long long> masks(nslots, 0), offs(t.ngroups + 1, 0);
  for (unsigned long long slot = 0; slot < nslots; slot++) {         // flag
    unsigned long long m = 0;
    for (int lane = 0; lane < 64; lane++) {
      size_t addr; unsigned int pos;
      bool take = pf_dist_cell(t, slot, lane, &addr, &pos);
      if (take && map) take = (map[pos >> 5] >> (pos & 31u)) & 1u;
      if (take) take = fmax[addr] >= thr;
      if (take) m |= 1ull << lane;
    }
    masks[slot] = m;
  }
  for (unsigned long long g = 0; g < t.ngroups; g++) {               // scan
    unsigned long long c = 0;
    for (int w = 0; w < PF_DIST_GROUP_WAVES; w++) c += (unsigned long long)__builtin_popcountll(masks[g * PF_DIST_GROUP_WAVES + w]);
    offs[g + 1] = offs[g] + c;
  }
  for (unsigned long long g = 0; g < t.ngroups; g++) {               // pack
    unsigned long long woff = 0;
    for (int w = 0; w < PF_DIST_GROUP_WAVES; w++) {
      const unsigned long long slot = g * PF_DIST_GROUP_WAVES + w, m = masks[slot];
      for (int lane = 0; lane < 64; lane++)
        if ((m >> lane) & 1ull) {
          const unsigned long long rec = offs[g] + woff + (unsigned long long)__builtin_popcountll(m & ((1ull << lane) - 1ull));
          size_t addr; unsigned int pos;
          pf_dist_cell(t, slot, lane, &addr, &pos);
          if (rec < capacity) { frag_pos[rec] = pos; cell_index[rec] = (unsigned int)addr; }
        }
      woff += (unsigned long long)__builtin_popcountll(m);
    }
  }
  return (long long)offs[t.ngroups];
}
