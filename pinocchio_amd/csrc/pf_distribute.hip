// pf_distribute.hip -- distribute() (src/distribute.c:58-175) on the device, for one target sub-box: the step of fragmentation between
// the Fmax >= Flast selection (pf_select_sort.hip) and count_peaks (pf_peaks.hip).  The reference walks every cell of every
// intersection of the rank's FFT box with the sub-box (keep_data :547-600, send_data :300-416), tests a map bit and
// products[].Fmax >= outputs.Flast (update_distmap :685-698) and memcpy's the survivors, in order, into frag[] with their sub-box
// index in frag_pos[].  Here that is an ORDER-PRESERVING stream compaction followed by a gather into records, three kernels and no
// library call:
//
//  k_dist_flag   a wavefront takes 64 consecutive i of a box (the boxes of pf_distribute_boxes.h, one launch over all of them; a box
//                starts a new wavefront slot), forms the slab address z + n (y + n x_local) and the sub-box index of its cell,
//                reads Fmax and the map word, ballots and stores the 64-bit mask; a workgroup -- PF_DIST_GROUP_WAVES slots, 4096
//                cells, in rounds of 256 consecutive cells -- adds the popcounts into its count.  i runs along z: the reads are
//                coalesced in runs of the box's z length.
//  k_dist_scan   exclusive scan of the workgroup counts by one workgroup, 64-bit totals; the last entry is the number taken.
//  k_dist_pack   a workgroup re-reads its masks and its offset, gathers the words of the record from the columns and writes
//                records and frag_pos at offset + rank.  The records of a round are contiguous in the output: they are staged in LDS
//                and written out as consecutive words (one lane per 56-byte record would scatter 4-byte stores 56 bytes apart).  The
//                plain form -- one lane per record straight into a cleared buffer, as k_pack_products -- is kept for the A/B
//                (PF_DISTRIBUTE_LDS=0) and serves records longer than PF_DIST_MAX_WORDS words.  A call packs the records
//                [first, first + cnt) of the selection, so that a result larger than a staging piece leaves in pieces.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include "pf_distribute_boxes.h"
#include "pf_internal.h"

#define PF_DIST_BLOCK 256
#define PF_DIST_ROUNDS (PF_DIST_GROUP_WAVES / (PF_DIST_BLOCK / 64))

template <typename PR>
__global__ void __launch_bounds__(PF_DIST_BLOCK) k_dist_flag(PfDistTable t, const PR *fmax, PR thr, const unsigned int *map,
                                                             unsigned long long *masks, unsigned int *counts) {
  __shared__ unsigned int total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned long long g = blockIdx.x;
  unsigned int cnt = 0;
  for (int r = 0; r < PF_DIST_ROUNDS; r++) {
    const unsigned long long slot = g * PF_DIST_GROUP_WAVES + r * (PF_DIST_BLOCK / 64) + wave;
    size_t addr = 0;
    unsigned int pos = 0;
    bool take = pf_dist_cell(t, slot, lane, &addr, &pos);
    if (take && map) take = (map[pos >> 5] >> (pos & 31u)) & 1u;   // get_map_bit / get_mapup_bit: UINTLEN = 32
    if (take) take = fmax[addr] >= thr;                            // NaN compares false
    const unsigned long long m = __ballot(take);
    if (lane == 0) masks[slot] = m;
    cnt += (unsigned int)__popcll(m);
  }
  if (lane == 0 && cnt) atomicAdd(&total, cnt);
  __syncthreads();
  if (threadIdx.x == 0) counts[g] = total;
}

// offs[i] = counts[0] + ... + counts[i - 1], offs[ngroups] = the total; one workgroup, tiles of 4096 counts (a tile sums to 2^24 at most)
__global__ void __launch_bounds__(1024) k_dist_scan(const unsigned int *counts, unsigned long long ngroups, unsigned long long *offs) {
  __shared__ unsigned int wsum[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  unsigned long long carry = 0;
  for (unsigned long long base = 0; base < ngroups; base += 4096) {
    const unsigned long long i0 = base + 4ull * tid;
    unsigned int v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = i0 + k < ngroups ? counts[i0 + k] : 0u;
    const unsigned int s = v[0] + v[1] + v[2] + v[3];
    unsigned int incl = s;
    for (int o = 1; o < 64; o <<= 1) { const unsigned int x = __shfl_up(incl, o, 64); if (lane >= o) incl += x; }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    unsigned int wbase = 0, tot = 0;
    for (int q = 0; q < 16; q++) { const unsigned int x = wsum[q]; if (q < w) wbase += x; tot += x; }
    unsigned long long run = carry + wbase + (incl - s);
#pragma unroll
    for (int k = 0; k < 4; k++) if (i0 + k < ngroups) { offs[i0 + k] = run; run += v[k]; }
    carry += tot;
    __syncthreads();
  }
  if (tid == 0) offs[ngroups] = carry;
}

struct PfDistCols { const unsigned int *fmax, *vel; const int *rmax; size_t ncell_total; };

// word `code` (PfDistRecord) of the record of cell `addr`; WPE: 4-byte words of a PRODFLOAT
template <int WPE>
__device__ __forceinline__ unsigned int dist_word(const PfDistCols &c, int code, size_t addr) {
  if (code < 0) return 0u;
  if (code == 0) return (unsigned int)c.rmax[addr];
  if (code < 4) return c.fmax[addr * WPE + (code - 1)];
  const int k = (code - 4) >> 1, h = (code - 4) & 1;
  return c.vel[((size_t)k * c.ncell_total + addr) * WPE + h];
}

template <typename PR, bool LDS>
__global__ void __launch_bounds__(PF_DIST_BLOCK) k_dist_pack(PfDistTable t, const unsigned long long *masks, const unsigned long long *offs,
                                                             PfDistCols cols, PfDistRecord rec, size_t stride_words, unsigned long long first,
                                                             unsigned long long cnt, unsigned int *aos, unsigned int *frag_pos, unsigned int *cell_index) {
  constexpr int WPE = sizeof(PR) / 4;
  extern __shared__ unsigned int stage[];               // LDS: PF_DIST_BLOCK records
  __shared__ unsigned int woff[PF_DIST_GROUP_WAVES + 1];  // exclusive scan of the group's popcounts
  const unsigned long long g = blockIdx.x;
  const unsigned long long og = offs[g], cg = offs[g + 1] - og, last = first + cnt;
  if (!cg || og >= last || og + cg <= first) return;    // (the whole workgroup: nothing of it lies in this piece)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (tid < 64) {
    const unsigned int c = (unsigned int)__popcll(masks[g * PF_DIST_GROUP_WAVES + tid]);
    unsigned int incl = c;
    for (int o = 1; o < 64; o <<= 1) { const unsigned int x = __shfl_up(incl, o, 64); if (lane >= o) incl += x; }
    woff[tid] = incl - c;
    if (tid == 63) woff[64] = incl;
  }
  __syncthreads();
  const int nwords = rec.nwords;
  for (int r = 0; r < PF_DIST_ROUNDS; r++) {
    const int s0 = r * (PF_DIST_BLOCK / 64);
    const unsigned int rb = woff[s0], re = woff[s0 + PF_DIST_BLOCK / 64];
    if (rb == re || og + re <= first || og + rb >= last) continue;   // (uniform over the workgroup)
    const unsigned long long slot = g * PF_DIST_GROUP_WAVES + s0 + wave;
    const unsigned long long m = masks[slot];
    if ((m >> lane) & 1ull) {
      size_t addr = 0;
      unsigned int pos = 0;
      pf_dist_cell(t, slot, lane, &addr, &pos);
      const unsigned int rank = woff[s0 + wave] + (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
      const unsigned long long recno = og + rank;
      if (recno >= first && recno < last) {
        const unsigned long long j = recno - first;
        if (frag_pos) frag_pos[j] = pos;
        if (cell_index) cell_index[j] = (unsigned int)addr;
        if (aos) {
          if (LDS) {
            unsigned int *dst = stage + (size_t)(rank - rb) * nwords;
            for (int q = 0; q < nwords; q++) dst[q] = dist_word<WPE>(cols, rec.src[q], addr);
          } else {
            unsigned int *dst = aos + j * stride_words;
            for (int q = 0; q < rec.nnamed; q++) dst[rec.named_off[q]] = dist_word<WPE>(cols, rec.named_src[q], addr);
          }
        }
      }
    }
    if (LDS && aos) {
      __syncthreads();
      // the round's records that lie in this piece, as consecutive words
      const unsigned long long lo = og + rb > first ? og + rb : first, hi = og + re < last ? og + re : last;
      const unsigned int nw = (unsigned int)(hi - lo) * nwords;
      const unsigned int *src = stage + (size_t)(lo - (og + rb)) * nwords;
      unsigned int *dst = aos + (lo - first) * stride_words;
      for (unsigned int q = tid; q < nw; q += PF_DIST_BLOCK) dst[q] = src[q];
      __syncthreads();
    }
  }
}

// the smallest value t of the product type with (double)t >= flast: F >= t is then "(double)F >= flast" (outputs.Flast is a double)
static float dist_thr(double flast, float) {
  float t = (float)flast;
  if ((double)t < flast) t = nextafterf(t, INFINITY);
  return t;
}
static double dist_thr(double flast, double) { return flast; }

int pf_dist_table(int n, int x0, int nxl, const pf_subbox *sub, PfDistTable *t, int *bad) {
  return pf_dist_table_fill(n, x0, nxl, sub->start, sub->len, t, bad);
}

int pf_dist_record(int pb, const pf_product_layout *l, PfDistRecord *r) {
  memset(r, 0, sizeof(*r));
  if (l->stride < 4 || l->stride % 4 || l->stride / 4 > 0x7fffffffu) return 1;
  const int wpe = pb / 4;
  r->nwords = (int)(l->stride / 4);
  for (int q = 0; q < PF_DIST_MAX_WORDS; q++) r->src[q] = -1;
  struct Fld { int off, words, code0; };
  Fld f[6]; int nf = 0;
  if (l->off_Rmax >= 0) f[nf++] = Fld{l->off_Rmax, 1, 0};
  if (l->off_Fmax >= 0) f[nf++] = Fld{l->off_Fmax, wpe, 1};
  const int ov[4] = {l->off_Vel, l->off_Vel_2LPT, l->off_Vel_3LPT_1, l->off_Vel_3LPT_2};
  for (int o = 0; o < 4; o++) if (ov[o] >= 0) f[nf++] = Fld{ov[o], 3 * wpe, 4 + 6 * o};
  for (int a = 0; a < nf; a++) {
    if (f[a].off % 4 || (size_t)f[a].off + 4 * (size_t)f[a].words > l->stride) return 1;
    for (int b = 0; b < a; b++)
      if (f[a].off < f[b].off + 4 * f[b].words && f[b].off < f[a].off + 4 * f[a].words) return 2;
  }
  for (int a = 0; a < nf; a++)
    for (int q = 0; q < f[a].words; q++) {
      // displacement o: components e = 0..2 are columns 3 o + e, a component of wpe words: code 4 + 2 (3 o + e) + h
      const int code = f[a].code0 < 4 ? f[a].code0 + q : f[a].code0 + (wpe == 2 ? q : 2 * q);
      const int w = f[a].off / 4 + q;
      r->named_off[r->nnamed] = w; r->named_src[r->nnamed] = (signed char)code; r->nnamed++;
      if (w < PF_DIST_MAX_WORDS) r->src[w] = (signed char)code;
    }
  return 0;
}

void pf_dist_release(PfDistScratch *s) {
  hipFree(s->map); hipFree(s->masks); hipFree(s->counts); hipFree(s->offs);
  memset(s, 0, sizeof(*s));
}

int pf_dist_select(const PfDistTable &t, int pb, const void *fmax, double flast, const unsigned int *map_host, const unsigned int *map_dev,
                   PfDistScratch *s, hipStream_t st, unsigned long long *count) {
  memset(s, 0, sizeof(*s));
  *count = 0;
  if (!t.ngroups) return 0;   // the sub-box misses the slab
  const unsigned long long cells = (unsigned long long)t.slen[0] * t.slen[1] * t.slen[2];
  const size_t map_words = (size_t)((cells + 31) / 32);
  bool ok = hipMalloc((void **)&s->masks, (size_t)t.ngroups * PF_DIST_GROUP_WAVES * sizeof(unsigned long long)) == hipSuccess &&
            hipMalloc((void **)&s->counts, (size_t)t.ngroups * sizeof(unsigned int)) == hipSuccess &&
            hipMalloc((void **)&s->offs, (size_t)(t.ngroups + 1) * sizeof(unsigned long long)) == hipSuccess;
  if (ok && map_host) ok = hipMalloc((void **)&s->map, map_words * sizeof(unsigned int)) == hipSuccess &&
                           hipMemcpyAsync(s->map, map_host, map_words * sizeof(unsigned int), hipMemcpyHostToDevice, st) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); pf_dist_release(s); return 1; }
  const dim3 grid((unsigned int)t.ngroups), block(PF_DIST_BLOCK);
  const unsigned int *map = map_host ? s->map : map_dev;   // (a resident map, pf_map.hip, is read where it lies)
  if (pb == 8) hipLaunchKernelGGL(k_dist_flag<double>, grid, block, 0, st, t, (const double *)fmax, dist_thr(flast, double()), map, s->masks, s->counts);
  else hipLaunchKernelGGL(k_dist_flag<float>, grid, block, 0, st, t, (const float *)fmax, dist_thr(flast, float()), map, s->masks, s->counts);
  hipLaunchKernelGGL(k_dist_scan, dim3(1), dim3(1024), 0, st, s->counts, t.ngroups, s->offs);
  if (hipGetLastError() != hipSuccess ||
      hipMemcpyAsync(count, s->offs + t.ngroups, sizeof(unsigned long long), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) { pf_dist_release(s); return 1; }
  return 0;
}

int pf_dist_pack(const PfDistTable &t, const PfDistScratch &s, int pb, const void *fmax, const int *rmax, const void *vel12,
                 size_t ncell_total, const PfDistRecord &r, size_t stride, unsigned long long first, unsigned long long cnt, char *aos,
                 unsigned int *frag_pos, unsigned int *cell_index, bool lds, hipStream_t st) {
  if (!cnt || !t.ngroups) return 0;
  if (r.nwords > PF_DIST_MAX_WORDS || !aos) lds = false;
  PfDistCols c;
  c.fmax = (const unsigned int *)fmax; c.vel = (const unsigned int *)vel12; c.rmax = rmax; c.ncell_total = ncell_total;
  const dim3 grid((unsigned int)t.ngroups), block(PF_DIST_BLOCK);
  const size_t sw = stride / 4, shm = lds ? (size_t)PF_DIST_BLOCK * r.nwords * sizeof(unsigned int) : 0;
  unsigned int *out = (unsigned int *)aos;
  if (pb == 8) {
    if (lds) hipLaunchKernelGGL((k_dist_pack<double, true>), grid, block, shm, st, t, s.masks, s.offs, c, r, sw, first, cnt, out, frag_pos, cell_index);
    else hipLaunchKernelGGL((k_dist_pack<double, false>), grid, block, 0, st, t, s.masks, s.offs, c, r, sw, first, cnt, out, frag_pos, cell_index);
  } else {
    if (lds) hipLaunchKernelGGL((k_dist_pack<float, true>), grid, block, shm, st, t, s.masks, s.offs, c, r, sw, first, cnt, out, frag_pos, cell_index);
    else hipLaunchKernelGGL((k_dist_pack<float, false>), grid, block, 0, st, t, s.masks, s.offs, c, r, sw, first, cnt, out, frag_pos, cell_index);
  }
  return hipGetLastError() != hipSuccess;
}
