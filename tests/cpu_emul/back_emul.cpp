// Host compilation of the cell arithmetic of distribute_back on the device (pinocchio_amd/csrc/pf_back_core.h) for
// tests/test_back_cpu.py: the per-particle quantities, and the scatter of the kernel walked particle by particle as its lanes walk it.
// port_back is the loop of keep_data_back (src/distribute.c:806-834) in plain C, the form the device path is measured against
// (profiles/tools/back_time.py).  With -DBACK_EMUL_MAIN the file is a program that holds the two against each other on the boxes of
// the tests; it is built under -fsanitize=address,undefined.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../pinocchio_amd/csrc/pf_distribute_boxes.h"
#include "../../pinocchio_amd/csrc/pf_back_core.h"
#include "large_boxes.h"

static PfBackBox box_of(int n, int x0, int nxl, const int *start, const int *len, const int *safe) {
  PfBackBox b;
  for (int d = 0; d < 3; d++) { b.box.len[d] = len[d]; b.box.pbc[d] = len[d] == n; b.box.safe[d] = safe[d]; b.start[d] = pf_dist_wrap(start[d], n); }
  b.n = n; b.x0 = x0; b.nxl = nxl;
  return b;
}

extern "C" {

// per position: coordinates, good, global cell, whether the slab takes it and where (0 when it does not)
void emul_cells(int n, int x0, int nxl, const int *start, const int *len, const int *safe, size_t count, const unsigned int *pos, int *coord /* [3 count] */,
                unsigned char *good, int *global /* [3 count] */, unsigned char *taken, unsigned long long *addr) {
  const PfBackBox b = box_of(n, x0, nxl, start, len, safe);
  for (size_t i = 0; i < count; i++) {
    int c[3], g[3];
    pf_neigh_coord(b.box, pos[i], c);
    pf_back_global(b, c, g);
    for (int d = 0; d < 3; d++) { coord[3 * i + d] = c[d]; global[3 * i + d] = g[d]; }
    good[i] = pf_neigh_good(b.box, c);
    size_t a = 0;
    taken[i] = pf_back_cell(b, pos[i], &a);
    addr[i] = taken[i] ? a : 0;
  }
}

// the scatter as the kernel does it, one particle after the other; pos null: particle iz at position iz.  Returns the number stored
unsigned long long emul_back(int n, int x0, int nxl, const int *start, const int *len, const int *safe, size_t count, const unsigned int *pos, const float *zacc,
                             const int *gid, float *zcol, int *gcol) {
  const PfBackBox b = box_of(n, x0, nxl, start, len, safe);
  unsigned long long stored = 0;
  for (size_t iz = 0; iz < count; iz++) {
    size_t a;
    if (!pf_back_cell(b, pos ? pos[iz] : (unsigned int)iz, &a)) continue;
    zcol[a] = zacc[iz]; gcol[a] = gid[iz];
    stored++;
  }
  return stored;
}

// keep_data_back, :806-834: unsigned coordinates, one n added before the modulo (stabl lies in (-n, n)), the fft box an x-slab
unsigned long long port_back(int n, int x0, int nxl, const int *stabl, const int *Lgwbl, const int *safe, size_t Nstored, const unsigned int *frag_pos,
                             const float *zacc, const int *gid, float *pzacc, int *pgroup) {
  const int fft_box[6] = {x0, 0, 0, nxl, n, n};
  unsigned long long stored = 0;
  for (size_t iz = 0; iz < Nstored; iz++) {
    const unsigned int I = frag_pos ? frag_pos[iz] : (unsigned int)iz;
    unsigned int kbox = I % Lgwbl[2];
    const int kk = (int)(I / Lgwbl[2]);
    unsigned int jbox = kk % Lgwbl[1], ibox = kk / Lgwbl[1];
    const int good_particle = (ibox >= (unsigned int)safe[0] && ibox < (unsigned int)(Lgwbl[0] - safe[0]) && jbox >= (unsigned int)safe[1] &&
                               jbox < (unsigned int)(Lgwbl[1] - safe[1]) && kbox >= (unsigned int)safe[2] && kbox < (unsigned int)(Lgwbl[2] - safe[2]));
    ibox = (ibox + stabl[0] + n) % n;
    jbox = (jbox + stabl[1] + n) % n;
    kbox = (kbox + stabl[2] + n) % n;
    if (good_particle && ibox >= (unsigned int)fft_box[0] && ibox < (unsigned int)(fft_box[0] + fft_box[3]) && jbox >= (unsigned int)fft_box[1] &&
        jbox < (unsigned int)(fft_box[1] + fft_box[4]) && kbox >= (unsigned int)fft_box[2] && kbox < (unsigned int)(fft_box[2] + fft_box[5])) {
      const size_t fftpos = (size_t)(kbox - fft_box[2]) + (size_t)fft_box[5] * ((size_t)(jbox - fft_box[1]) + (size_t)fft_box[4] * (size_t)(ibox - fft_box[0]));
      pzacc[fftpos] = zacc[iz];
      pgroup[fftpos] = gid[iz];
      stored++;
    }
  }
  return stored;
}
}

#ifdef BACK_EMUL_MAIN
struct Case { int n, x0, nxl, start[3], len[3], safe[3]; };

int main() {
  // the boxes of tests/test_gpu_back.py, on the whole box and on slabs of it
  const Case cases[] = {{16, 0, 16, {0, 0, 0}, {16, 16, 16}, {0, 0, 0}},   {16, 4, 4, {0, 0, 0}, {16, 16, 16}, {0, 0, 0}},
                        {16, 0, 16, {-3, 10, 13}, {11, 9, 8}, {2, 1, 3}},  {16, 12, 4, {-3, 10, 13}, {11, 9, 8}, {2, 1, 3}},
                        {16, 8, 8, {5, 0, -2}, {7, 16, 12}, {1, 0, 2}},    {24, 0, 24, {20, 3, 0}, {9, 5, 24}, {2, 1, 0}},
                        {40, 24, 8, {19, 0, 33}, {17, 9, 40}, {2, 1, 0}},  {3, 0, 3, {0, 0, 0}, {3, 3, 3}, {0, 0, 0}}};
  unsigned long long seed = 12345;
  auto rnd = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (unsigned int)(seed >> 33); };
  for (const Case &cs : cases) {
    const size_t cells = (size_t)cs.len[0] * cs.len[1] * cs.len[2], ncell = (size_t)cs.nxl * cs.n * cs.n;
    std::vector<unsigned int> pos(cells);
    for (size_t i = 0; i < cells; i++) pos[i] = (unsigned int)i;
    for (size_t i = cells; i > 1; i--) { const size_t j = rnd() % i; const unsigned int t = pos[i - 1]; pos[i - 1] = pos[j]; pos[j] = t; }
    const size_t count = (cells * 6 + 9) / 10;
    std::vector<float> zacc(count);
    std::vector<int> gid(count);
    for (size_t i = 0; i < count; i++) { zacc[i] = (rnd() % 7) ? (float)(rnd() % 100000) * 1e-3f : -1.0f; gid[i] = (rnd() % 5) ? (int)(rnd() & 0x7FFFFFFF) : 0; }
    for (int form = 0; form < 2; form++) {   // frag_pos, and the CLASSIC form on the first `count` positions
      std::vector<float> z0(ncell, -1.0f), z1(ncell, -1.0f);
      std::vector<int> g0(ncell, 0), g1(ncell, 0);
      const unsigned int *p = form ? nullptr : pos.data();
      const unsigned long long s0 = emul_back(cs.n, cs.x0, cs.nxl, cs.start, cs.len, cs.safe, count, p, zacc.data(), gid.data(), z0.data(), g0.data());
      const unsigned long long s1 = port_back(cs.n, cs.x0, cs.nxl, cs.start, cs.len, cs.safe, count, p, zacc.data(), gid.data(), z1.data(), g1.data());
      if (s0 != s1) { printf("MISMATCH: %llu stored, the port %llu\n", s0, s1); return 1; }
      for (size_t i = 0; i < ncell; i++)
        if (!(z0[i] == z1[i]) || g0[i] != g1[i]) { printf("MISMATCH at cell %zu\n", i); return 1; }
      printf("n %d slab %d+%d box (%d %d %d)+(%d %d %d) form %d: stored %llu of %zu\n", cs.n, cs.x0, cs.nxl, cs.start[0], cs.start[1], cs.start[2], cs.len[0],
             cs.len[1], cs.len[2], form, s0, count);
    }
  }
  // the production-size boxes: positions up to 2^32 - 1 from a sparse set; two planes on the last x-planes of the sub-box from a start
  // that wraps in all three directions, and the two planes that begin with position 2^31 from a straight start
  for (const LargeBox &lb : LARGE_BOXES) {
    const std::vector<unsigned int> pos = large_positions(lb.len, 200000, rnd);
    const size_t count = pos.size(), ncell = (size_t)2 * lb.n * lb.n;
    std::vector<float> zacc(count);
    std::vector<int> gid(count);
    for (size_t i = 0; i < count; i++) { zacc[i] = (float)(rnd() % 16777216); gid[i] = (rnd() % 5) ? (int)(rnd() & 0x7FFFFFFF) : 0; }
    gid[0] = 0x7FFFFFFF;
    const int zero[3] = {0, 0, 0};
    unsigned long long kept[2];
    for (int geo = 0; geo < 2; geo++) {
      const int *start = geo ? zero : lb.wrapped;
      const int x0 = geo ? large_mid_plane(lb.len) : (lb.wrapped[0] + lb.len[0] - 2) % lb.n;
      std::vector<float> z0(ncell, -1.0f), z1(ncell, -1.0f);
      std::vector<int> g0(ncell, 0), g1(ncell, 0);
      const unsigned long long s0 = emul_back(lb.n, x0, 2, start, lb.len, lb.safe, count, pos.data(), zacc.data(), gid.data(), z0.data(), g0.data());
      const unsigned long long s1 = port_back(lb.n, x0, 2, start, lb.len, lb.safe, count, pos.data(), zacc.data(), gid.data(), z1.data(), g1.data());
      if (s0 != s1 || !s0) { printf("MISMATCH: large box %s: %llu kept, the port %llu\n", lb.name, s0, s1); return 1; }
      for (size_t i = 0; i < ncell; i++)
        if (!(z0[i] == z1[i]) || g0[i] != g1[i]) { printf("MISMATCH: large box %s at cell %zu\n", lb.name, i); return 1; }
      kept[geo] = s0;
    }
    printf("large box %s n %d (%d %d %d): kept %llu on the last planes, %llu at 2^31, of %zu particles\n", lb.name, lb.n, lb.len[0], lb.len[1], lb.len[2], kept[0], kept[1], count);
  }
  return 0;
}
#endif
