// pf_distribute_boxes.h -- intersection() of src/distribute.c:178-297 restated: the boxes that an FFT-space box (a rank's x-slab)
// and a fragmentation sub-box have in common; the box table the kernels of pf_distribute.hip are driven by; and the index
// arithmetic of one cell of that table (fft_space_index :603-624, subbox_space_index :627-645).  Plain C++ with no device
// dependence, so that a CPU test compiles it on its own (tests/cpu_emul/distribute_emul.cpp) and holds it against the numpy
// restatement of the same loops (tests/np_distribute.py).
//
// The reference treats every dimension alone.  The sub-box [s, s + len) is cut at the edge of the periodic box into the segment up
// to the edge and, when it goes beyond, the wrapped segment [0, (s + len) % n); each is intersected with the FFT box, so a
// dimension gives 0, 1 or 2 segments and the two boxes up to eight intersections.  They are emitted with x slowest, z fastest and in
// every dimension the WRAPPED segment first (:226-262, ax / ay / az = 0 is istart2 / istop2): distribute() stores the cells in that
// order and the order is part of the result.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define PF_DIST_HD __host__ __device__ __forceinline__
#else
#define PF_DIST_HD static inline
#endif

struct PfDistBox { int start[3], len[3]; };

// a start coordinate as intersection() sees it after "fix negative starting point" (:190-191).  The reference adds n once
// (subbox.stabl lies in (-n, n)); any other start is reduced to the same cell of the periodic box.
static inline int pf_dist_wrap(int s, int n) { s %= n; return s < 0 ? s + n : s; }

// fbox / sbox: start[3] then len[3] (my_fft_box / my_subbox of :62-80); 1 <= sbox len <= n.  Returns the number of boxes written to out[8].
static inline int pf_dist_intersection(int n, const int fbox[6], const int sbox[6], PfDistBox out[8]) {
  int lo[3][2], hi[3][2];   // [dim][0]: the wrapped segment (istart2 / istop2), [dim][1]: the segment up to the box edge (istart / istop)
  for (int d = 0; d < 3; d++) {
    const int s = pf_dist_wrap(sbox[d], n), e = s + sbox[d + 3];
    const int stop1 = fbox[d] + fbox[d + 3];
    const int stop2 = e > n ? n : e;
    lo[d][1] = fbox[d] > s ? fbox[d] : s;
    hi[d][1] = stop1 < stop2 ? stop1 : stop2;
    if (e > n) {
      const int w = e % n;
      lo[d][0] = fbox[d] > 0 ? fbox[d] : 0;
      hi[d][0] = stop1 < w ? stop1 : w;
    } else {
      lo[d][0] = 1; hi[d][0] = 0;
    }
  }
  int nb = 0;
  for (int ax = 0; ax < 2; ax++)
    for (int ay = 0; ay < 2; ay++)
      for (int az = 0; az < 2; az++)
        if (lo[0][ax] < hi[0][ax] && lo[1][ay] < hi[1][ay] && lo[2][az] < hi[2][az]) {
          PfDistBox &b = out[nb++];
          b.start[0] = lo[0][ax]; b.start[1] = lo[1][ay]; b.start[2] = lo[2][az];
          b.len[0] = hi[0][ax] - lo[0][ax]; b.len[1] = hi[1][ay] - lo[1][ay]; b.len[2] = hi[2][az] - lo[2][az];
        }
  return nb;
}

// ---- the box table: one launch covers all boxes ----
// A wavefront takes 64 consecutive i of a box ("slot"); a box starts a new slot, so a slot never straddles two boxes and the
// order of the slots is the order of the cells.  PF_DIST_GROUP_WAVES slots (4096 cells) share one workgroup count.
#define PF_DIST_GROUP_WAVES 64
struct PfDistTable {
  int nbox;
  int bstart[8][3], blen[8][3];         // intersection() boxes in its order, global coordinates
  unsigned long long wave0[9];           // first slot of each box; wave0[nbox ..] = all slots
  int n, x0, nxl;                        // the slab: global x of its first plane, planes
  int sstart[3], slen[3];                // the sub-box: start reduced to [0, n), Lgwbl
  unsigned long long ngroups;            // workgroup counts: ceil(slots / PF_DIST_GROUP_WAVES)
};

// 0 ok; 1: len[*bad] outside [1, n]; 2: more than 2^32 cells (frag_pos is 32-bit like the reference's)
static inline int pf_dist_table_fill(int n, int x0, int nxl, const int start[3], const int len[3], PfDistTable *t, int *bad) {
  *t = PfDistTable();
  unsigned long long cells = 1;
  for (int d = 0; d < 3; d++) {
    *bad = d;
    if (len[d] < 1 || len[d] > n) return 1;
    cells *= (unsigned long long)len[d];
    t->sstart[d] = pf_dist_wrap(start[d], n);
    t->slen[d] = len[d];
  }
  if (cells > (1ull << 32)) return 2;
  t->n = n; t->x0 = x0; t->nxl = nxl;
  const int fbox[6] = {x0, 0, 0, nxl, n, n};
  const int sbox[6] = {start[0], start[1], start[2], len[0], len[1], len[2]};
  PfDistBox boxes[8];
  t->nbox = pf_dist_intersection(n, fbox, sbox, boxes);
  unsigned long long w = 0;
  for (int b = 0; b < t->nbox; b++) {
    for (int d = 0; d < 3; d++) { t->bstart[b][d] = boxes[b].start[d]; t->blen[b][d] = boxes[b].len[d]; }
    t->wave0[b] = w;
    w += ((unsigned long long)boxes[b].len[0] * boxes[b].len[1] * boxes[b].len[2] + 63) / 64;
  }
  for (int b = t->nbox; b <= 8; b++) t->wave0[b] = w;
  t->ngroups = (w + PF_DIST_GROUP_WAVES - 1) / PF_DIST_GROUP_WAVES;
  return 0;
}

// the cell of lane `lane` of slot `slot`: false beyond the end of its box.  *addr = z + n (y + n x_local) in the slab, *pos = its
// sub-box-space index
PF_DIST_HD bool pf_dist_cell(const PfDistTable &t, unsigned long long slot, int lane, size_t *addr, unsigned int *pos) {
  if (slot >= t.wave0[t.nbox]) return false;
  int b = 0;
  while (b + 1 < t.nbox && slot >= t.wave0[b + 1]) b++;
  const unsigned int l0 = t.blen[b][0], l1 = t.blen[b][1], l2 = t.blen[b][2];
  const unsigned long long i64 = (slot - t.wave0[b]) * 64ull + (unsigned int)lane;
  if (i64 >= (unsigned long long)l0 * l1 * l2) return false;
  const unsigned int i = (unsigned int)i64;  // (a sub-box has at most 2^32 cells)
  // INDEX_TO_COORD (src/pinocchio.h:84)
  const unsigned int kk = i / l2, kp = i - kk * l2, ip = kk / l1, jp = kk - ip * l1;
  const int n = t.n;
  const int gx = t.bstart[b][0] + (int)ip, gy = t.bstart[b][1] + (int)jp, gz = t.bstart[b][2] + (int)kp;  // inside the box: no wrap
  *addr = ((size_t)(gx - t.x0) * n + gy) * n + gz;
  int px = gx - t.sstart[0], py = gy - t.sstart[1], pz = gz - t.sstart[2];
  if (px < 0) px += n;
  if (py < 0) py += n;
  if (pz < 0) pz += n;
  *pos = (unsigned int)((unsigned long long)pz + (unsigned long long)t.slen[2] * ((unsigned long long)py + (unsigned long long)t.slen[1] * px));
  return true;
}
