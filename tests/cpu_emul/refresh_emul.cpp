// Host compilation of the cell arithmetic and the compaction of the velocity refresh on the device
// (pinocchio_amd/csrc/pf_refresh_core.h) for tests/test_refresh_cpu.py: the per-particle quantities, and the gather walked thread by
// thread as the kernels of pf_refresh.hip walk it -- flags per wave, counts per block, the scan, the slot of each found particle, in
// the particles' own order or in a caller's order.  port_gather is the loop of keep_data_back (src/distribute.c:806-830) in plain C
// without its good_particle test, reading instead of writing.  The file is a program: its main holds the two against each other on
// the boxes of the tests; it is also built under -fsanitize=address,undefined.  -DREFRESH_EMUL_LIB leaves the main out (the shared
// object the test loads).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../pinocchio_amd/csrc/pf_distribute_boxes.h"
#include "../../pinocchio_amd/csrc/pf_refresh_core.h"
#include "large_boxes.h"

static PfBackBox box_of(int n, int x0, int nxl, const int *start, const int *len, const int *safe) {
  PfBackBox b;
  for (int d = 0; d < 3; d++) { b.box.len[d] = len[d]; b.box.pbc[d] = len[d] == n; b.box.safe[d] = safe[d]; b.start[d] = pf_dist_wrap(start[d], n); }
  b.n = n; b.x0 = x0; b.nxl = nxl;
  return b;
}

extern "C" {

// per position: coordinates, global cell, whether the slab holds it and where (0 when it does not)
void emul_cells(int n, int x0, int nxl, const int *start, const int *len, const int *safe, size_t count, const unsigned int *pos, int *coord /* [3 count] */,
                int *global /* [3 count] */, unsigned char *found, unsigned long long *addr) {
  const PfBackBox b = box_of(n, x0, nxl, start, len, safe);
  for (size_t i = 0; i < count; i++) {
    int c[3], g[3];
    pf_neigh_coord(b.box, pos[i], c);
    pf_back_global(b, c, g);
    for (int d = 0; d < 3; d++) { coord[3 * i + d] = c[d]; global[3 * i + d] = g[d]; }
    size_t a = 0;
    found[i] = pf_refresh_cell(b, pos[i], &a);
    addr[i] = found[i] ? a : 0;
  }
}

// the gather as the kernels do it: cols24 = 24 columns of ncell floats; order null or a permutation of 0 .. count - 1; at most `cap`
// entries are written.  Returns the number found
unsigned long long emul_gather(int n, int x0, int nxl, const int *start, const int *len, const int *safe, size_t count, const unsigned int *pos, const int *order,
                               const float *cols24, size_t cap, unsigned int *index, float *vel24) {
  const PfBackBox b = box_of(n, x0, nxl, start, len, safe);
  const size_t ncell = (size_t)nxl * n * n, nb = (count + PF_REFRESH_BLOCK - 1) / PF_REFRESH_BLOCK;
  std::vector<unsigned long long> masks(nb * PF_REFRESH_WAVES, 0ull), offs(nb + 1, 0ull);
  for (size_t i = 0; i < count; i++) {   // k_refresh_flag
    size_t a;
    if (pf_refresh_cell(b, pos[i], &a)) masks[i >> 6] |= 1ull << (i & 63);
  }
  for (size_t g = 0; g < nb; g++) {      // the block counts and k_refresh_scan
    unsigned int s = 0;
    for (int w = 0; w < PF_REFRESH_WAVES; w++) s += (unsigned int)pf_refresh_popc(masks[g * PF_REFRESH_WAVES + w]);
    offs[g + 1] = offs[g] + s;
  }
  for (size_t t = 0; t < count; t++) {   // k_refresh_gather
    const size_t i = order ? (size_t)order[t] : t;
    if (!pf_refresh_found(masks.data(), i)) continue;
    const unsigned long long j = offs[i / PF_REFRESH_BLOCK] + pf_refresh_rank_in_block(masks.data(), i);
    if (j >= cap) continue;
    size_t a = 0;
    pf_refresh_cell(b, pos[i], &a);
    index[j] = (unsigned int)i;
    for (int k = 0; k < 24; k++) vel24[24 * j + k] = cols24[(size_t)k * ncell + a];
  }
  return offs[nb];
}

// keep_data_back, :806-830, without good_particle: unsigned coordinates, one n added before the modulo (stabl lies in (-n, n)), the
// fft box an x-slab; what it finds is appended
unsigned long long port_gather(int n, int x0, int nxl, const int *stabl, const int *Lgwbl, size_t Nstored, const unsigned int *frag_pos, const float *cols24,
                               unsigned int *index, float *vel24) {
  const int fft_box[6] = {x0, 0, 0, nxl, n, n};
  const size_t ncell = (size_t)nxl * n * n;
  unsigned long long found = 0;
  for (size_t iz = 0; iz < Nstored; iz++) {
    const unsigned int I = frag_pos[iz];
    unsigned int kbox = I % Lgwbl[2];
    const int kk = (int)(I / Lgwbl[2]);
    unsigned int jbox = kk % Lgwbl[1], ibox = kk / Lgwbl[1];
    ibox = (ibox + stabl[0] + n) % n;
    jbox = (jbox + stabl[1] + n) % n;
    kbox = (kbox + stabl[2] + n) % n;
    if (ibox >= (unsigned int)fft_box[0] && ibox < (unsigned int)(fft_box[0] + fft_box[3]) && jbox >= (unsigned int)fft_box[1] &&
        jbox < (unsigned int)(fft_box[1] + fft_box[4]) && kbox >= (unsigned int)fft_box[2] && kbox < (unsigned int)(fft_box[2] + fft_box[5])) {
      const size_t fftpos = (size_t)(kbox - fft_box[2]) + (size_t)fft_box[5] * ((size_t)(jbox - fft_box[1]) + (size_t)fft_box[4] * (size_t)(ibox - fft_box[0]));
      index[found] = (unsigned int)iz;
      for (int k = 0; k < 24; k++) vel24[24 * found + k] = cols24[(size_t)k * ncell + fftpos];
      found++;
    }
  }
  return found;
}
}

#ifndef REFRESH_EMUL_LIB
struct Case { int n, x0, nxl, start[3], len[3], safe[3]; };

int main() {
  // the boxes of tests/test_gpu_refresh.py and tests/test_gpu_back.py, on the whole box and on slabs of it
  const Case cases[] = {{16, 0, 16, {0, 0, 0}, {16, 16, 16}, {0, 0, 0}},   {16, 4, 4, {0, 0, 0}, {16, 16, 16}, {0, 0, 0}},
                        {16, 0, 16, {-3, 0, 13}, {7, 16, 5}, {1, 0, 1}},   {16, 4, 4, {14, 0, 2}, {9, 16, 5}, {2, 0, 2}},
                        {16, 8, 4, {14, 0, 2}, {9, 16, 5}, {2, 0, 2}},     {24, 0, 24, {20, 3, 0}, {9, 5, 24}, {2, 1, 0}},
                        {40, 24, 8, {19, 0, 33}, {17, 9, 40}, {2, 1, 0}},  {3, 0, 3, {0, 0, 0}, {3, 3, 3}, {0, 0, 0}}};
  unsigned long long seed = 12345;
  auto rnd = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (unsigned int)(seed >> 33); };
  for (const Case &cs : cases) {
    const size_t cells = (size_t)cs.len[0] * cs.len[1] * cs.len[2], ncell = (size_t)cs.nxl * cs.n * cs.n;
    std::vector<float> cols(24 * ncell);
    for (size_t k = 0; k < 24; k++)
      for (size_t a = 0; a < ncell; a++) cols[k * ncell + a] = (float)(k * 1048576 + a);
    // 60 % of the positions in random order, then a tenth of them once more (duplicates are legal)
    std::vector<unsigned int> pos(cells);
    for (size_t i = 0; i < cells; i++) pos[i] = (unsigned int)i;
    for (size_t i = cells; i > 1; i--) { const size_t j = rnd() % i; const unsigned int t = pos[i - 1]; pos[i - 1] = pos[j]; pos[j] = t; }
    size_t count = (cells * 6 + 9) / 10;
    pos.resize(count);
    for (size_t i = 0; i < count / 10; i++) pos.push_back(pos[rnd() % count]);
    count = pos.size();
    std::vector<int> order(count);
    for (size_t i = 0; i < count; i++) order[i] = (int)i;
    for (size_t i = count; i > 1; i--) { const size_t j = rnd() % i; const int t = order[i - 1]; order[i - 1] = order[j]; order[j] = t; }
    for (int form = 0; form < 2; form++) {   // the particles' own order, and a random one
      std::vector<unsigned int> i0(count + 1, 0xDEADBEEFu), i1(count + 1, 0xDEADBEEFu);
      std::vector<float> v0(24 * count + 1, -7.0f), v1(24 * count + 1, -7.0f);
      const unsigned long long f0 = emul_gather(cs.n, cs.x0, cs.nxl, cs.start, cs.len, cs.safe, count, pos.data(), form ? order.data() : nullptr, cols.data(), count,
                                                i0.data(), v0.data());
      const unsigned long long f1 = port_gather(cs.n, cs.x0, cs.nxl, cs.start, cs.len, count, pos.data(), cols.data(), i1.data(), v1.data());
      if (f0 != f1) { printf("MISMATCH: %llu found, the port %llu\n", f0, f1); return 1; }
      for (size_t j = 0; j < count + 1; j++)
        if (i0[j] != i1[j]) { printf("MISMATCH at entry %zu\n", j); return 1; }
      for (size_t j = 0; j < 24 * count + 1; j++)
        if (!(v0[j] == v1[j])) { printf("MISMATCH at value %zu\n", j); return 1; }
      // a capacity below the count: the first entries alone, nothing behind them
      const size_t cap = (size_t)(f0 / 2);
      std::vector<unsigned int> i2(cap + 1, 0xDEADBEEFu);
      std::vector<float> v2(24 * cap + 1, -7.0f);
      const unsigned long long f2 = emul_gather(cs.n, cs.x0, cs.nxl, cs.start, cs.len, cs.safe, count, pos.data(), form ? order.data() : nullptr, cols.data(), cap,
                                                i2.data(), v2.data());
      if (f2 != f0 || i2[cap] != 0xDEADBEEFu || v2[24 * cap] != -7.0f) { printf("MISMATCH with a capacity of %zu\n", cap); return 1; }
      for (size_t j = 0; j < cap; j++)
        if (i2[j] != i1[j]) { printf("MISMATCH at entry %zu of %zu\n", j, cap); return 1; }
      printf("n %d slab %d+%d box (%d %d %d)+(%d %d %d) form %d: found %llu of %zu\n", cs.n, cs.x0, cs.nxl, cs.start[0], cs.start[1], cs.start[2], cs.len[0],
             cs.len[1], cs.len[2], form, f0, count);
    }
  }
  // the production-size boxes: positions up to 2^32 - 1 from a sparse set; the last x-plane of the sub-box from a start that wraps in
  // all three directions, and the plane of position 2^31 from a straight start; the particles' own order and a random one
  for (const LargeBox &lb : LARGE_BOXES) {
    const std::vector<unsigned int> pos = large_positions(lb.len, 200000, rnd);
    const size_t count = pos.size(), ncell = (size_t)lb.n * lb.n;
    std::vector<float> cols(24 * ncell);
    for (size_t q = 0; q < 24 * ncell; q++) cols[q] = (float)(((unsigned int)q * 2654435761u) >> 8);
    std::vector<int> order(count);
    for (size_t i = 0; i < count; i++) order[i] = (int)i;
    for (size_t i = count; i > 1; i--) { const size_t j = rnd() % i; const int t = order[i - 1]; order[i - 1] = order[j]; order[j] = t; }
    const int zero[3] = {0, 0, 0};
    unsigned long long hits[2];
    for (int geo = 0; geo < 2; geo++) {
      const int *start = geo ? zero : lb.wrapped;
      const int x0 = geo ? large_mid_plane(lb.len) : (lb.wrapped[0] + lb.len[0] - 1) % lb.n;
      std::vector<unsigned int> i0(count + 1, 0xDEADBEEFu), i1(count + 1, 0xDEADBEEFu);
      std::vector<float> v0(24 * count + 1, -7.0f), v1(24 * count + 1, -7.0f);
      const unsigned long long f0 = emul_gather(lb.n, x0, 1, start, lb.len, lb.safe, count, pos.data(), geo ? order.data() : nullptr, cols.data(), count, i0.data(), v0.data());
      const unsigned long long f1 = port_gather(lb.n, x0, 1, start, lb.len, count, pos.data(), cols.data(), i1.data(), v1.data());
      if (f0 != f1 || !f0) { printf("MISMATCH: large box %s: %llu hits, the port %llu\n", lb.name, f0, f1); return 1; }
      if (i0 != i1 || v0 != v1) { printf("MISMATCH: large box %s: the entries differ\n", lb.name); return 1; }
      hits[geo] = f0;
    }
    printf("large box %s n %d (%d %d %d): %llu hits on the last plane, %llu at 2^31, of %zu particles\n", lb.name, lb.n, lb.len[0], lb.len[1], lb.len[2], hits[0], hits[1], count);
  }
  return 0;
}
#endif
