// large_boxes.h -- the production-size sub-boxes of tests/test_large_index_cpu.py for the mains of the *_emul_san programs: A just
// past 2^31 cells, B exactly 2^32 (x and y periodic at n = 2048), C just below 2^32 with no periodic direction; and a sparse particle
// set of such a box -- the edge positions, a block of 6 x 6 x 70 cells at the origin, at the far corner and across the z-row of
// position 2^31, random positions over the whole range -- made without any array over the cells.
#pragma once
#include <algorithm>
#include <vector>

struct LargeBox { const char *name; int n, wrapped[3], len[3], safe[3]; };   // wrapped: a start from which the sub-box wraps in x, y and z
static const LargeBox LARGE_BOXES[3] = {{"A", 1296, {700, 800, 900}, {1291, 1291, 1291}, {1, 3, 3}},
                                        {"B", 2048, {5, 7, 1500}, {2048, 2048, 1024}, {0, 0, 3}},
                                        {"C", 2048, {1000, 900, 1100}, {1625, 1626, 1625}, {1, 2, 3}}};

static inline unsigned long long large_cells(const int *len) { return (unsigned long long)len[0] * (unsigned long long)len[1] * (unsigned long long)len[2]; }
// x of the plane that holds position 2^31
static inline int large_mid_plane(const int *len) { return (int)((1ull << 31) / ((unsigned long long)len[1] * (unsigned long long)len[2])); }

// at least `count` distinct positions in random order; rnd(): 31 random bits per call
template <typename Rnd>
static std::vector<unsigned int> large_positions(const int *len, size_t count, Rnd rnd) {
  const unsigned long long cells = large_cells(len), mid = 1ull << 31;
  std::vector<unsigned long long> p = {0ull, mid - 1, mid, cells - 1};
  const long long c31[3] = {(long long)(mid / ((unsigned long long)len[1] * len[2])), (long long)((mid / len[2]) % len[1]), (long long)(mid % len[2])};
  const int shape[3] = {6, 6, 70};
  long long corner[3][3];
  for (int d = 0; d < 3; d++) {
    corner[0][d] = 0; corner[1][d] = len[d] - shape[d];
    corner[2][d] = std::min<long long>(std::max<long long>(c31[d] - shape[d] / 2, 0), len[d] - shape[d]);
  }
  for (int b = 0; b < 3; b++)
    for (long long i = corner[b][0]; i < corner[b][0] + shape[0]; i++)
      for (long long j = corner[b][1]; j < corner[b][1] + shape[1]; j++)
        for (long long k = corner[b][2]; k < corner[b][2] + shape[2]; k++)
          p.push_back((unsigned long long)k + (unsigned long long)len[2] * ((unsigned long long)j + (unsigned long long)len[1] * (unsigned long long)i));
  while (true) {
    std::sort(p.begin(), p.end());
    p.erase(std::unique(p.begin(), p.end()), p.end());
    if (p.size() >= count) break;
    for (size_t q = p.size(); q < count; q++) p.push_back((((unsigned long long)rnd() << 31) | rnd()) % cells);
  }
  for (size_t i = p.size(); i > 1; i--) std::swap(p[i - 1], p[rnd() % i]);
  std::vector<unsigned int> out(p.size());   // (all of them: the edge positions stay in)
  for (size_t i = 0; i < p.size(); i++) out[i] = (unsigned int)p[i];
  return out;
}
