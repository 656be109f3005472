// pf_refresh_core.h -- the cell arithmetic of the velocity refresh (pf_refresh.hip): where the velocities of a stored particle of a
// sub-box lie in the product columns of an FFT slab.  It is the position -> cell -> slab arithmetic of keep_data_back()
// (src/distribute.c:806-830) read the other way round -- the reference's second distribute() of a segment (src/fragment.c:398-430)
// carries Vel* from exactly these cells to exactly these particles -- and WITHOUT the good_particle test (:815-817): every stored
// particle has velocities, the boundary layer included; only zacc and group_ID are restricted to the good ones.  Plain C++ with no
// device dependence, so that a CPU test compiles it on its own (tests/cpu_emul/refresh_emul.cpp) and walks it particle by particle
// against the numpy restatement (tests/np_refresh.py).
//
// Positions, the box and the slab: pf_back_core.h, whose pieces are used as they are.
#pragma once
#include <stddef.h>

#include "pf_back_core.h"

#define PF_REFRESH_HD PF_BACK_HD

// the particle at sub-box position pos (< Lx Ly Lz): whether its cell lies in this slab, and its index z + n (y + n (x - x0)) there
PF_REFRESH_HD bool pf_refresh_cell(const PfBackBox &b, unsigned int pos, size_t *addr) {
  int c[3], g[3];
  pf_neigh_coord(b.box, pos, c);
  pf_back_global(b, c, g);
  if (!pf_back_in_slab(b, g)) return false;
  *addr = pf_back_index(b, g);
  return true;
}

// The compaction in ascending particle index.  The particles are cut into blocks of PF_REFRESH_BLOCK, a block into waves of 64; mask[w]
// has bit l set when particle 64 w + l is found, offs[g] is the number found in the blocks before block g.  The output slot of a
// found particle i: offs of its block + the found particles of the block's waves before its own + those before it in its wave.
#define PF_REFRESH_BLOCK 256
#define PF_REFRESH_WAVES (PF_REFRESH_BLOCK / 64)
PF_REFRESH_HD int pf_refresh_popc(unsigned long long m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(m);
#else
  return __builtin_popcountll(m);
#endif
}
PF_REFRESH_HD unsigned int pf_refresh_rank_in_block(const unsigned long long *masks, unsigned long long i) {
  const unsigned long long w = i >> 6, w0 = w & ~(unsigned long long)(PF_REFRESH_WAVES - 1);
  unsigned int r = 0;
  for (unsigned long long q = w0; q < w; q++) r += (unsigned int)pf_refresh_popc(masks[q]);
  return r + (unsigned int)pf_refresh_popc(masks[w] & ((1ull << (i & 63)) - 1ull));
}
PF_REFRESH_HD bool pf_refresh_found(const unsigned long long *masks, unsigned long long i) { return (masks[i >> 6] >> (i & 63)) & 1ull; }
