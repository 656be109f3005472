// pf_neighbours.hip -- the neighbour table of the stored particles: every find_location() (src/fragment.c:592-603) of the loops of
// count_peaks() (:605-706), quick_build_groups() (src/build_groups.c:1916-2004) and build_groups() (:245-343) answered in one call.
// The reference searches all Nstored positions six times per particle, in Fmax order, three times over; none of it depends on the
// group state.  Here the searches run once, in POSITION order: thread p owns rank p of sorted_pos, consecutive lanes are
// neighbours in z and what they look up lies in the same or adjacent lines.
//
//  k_neigh_fpos   Fmax into position order, once: fpos[p] = Fmax of particle indices[p] (a scattered read per particle); every
//                 comparison afterwards reads fpos at the rank the lookup has found, beside the sorted_pos entry it has just read.
//  k_neigh_rows   rowstart[r], r = 0 .. Lx Ly: the lower bound of r Lz in sorted_pos -- the ranks of z-row r = y + Ly x are
//                 [rowstart[r], rowstart[r + 1]).  One thread and one full-range search per row, Lx Ly + 1 of them.
//  k_neigh        one particle per lane.  z-/z+: rank p -/+ 1 when its position is pos -/+ 1; a periodic wrap in z lands on the
//                 first / last rank of the particle's own row.  x-/x+/y-/y+: a search of [rowstart[r'], rowstart[r' + 1]) of the
//                 neighbour's row r', at most Lz entries that the lanes of a wavefront share.  The record of particle
//                 iz = indices[p] -- six ints, 24 bytes -- is written whole, flags[iz] beside it.  Counts per lane, a wavefront
//                 reduction and one 64-bit atomic per wavefront and counter (as k_peaks): integer sums, the same whatever the
//                 schedule.  ROWS = false (PF_NEIGH_ROWS=0, read per call) is the plain form kept for the A/B: one search of the
//                 whole of sorted_pos per neighbour, the reference's way, still in position order; same output.
//
// Every index is in range by construction: positions are below Lx Ly Lz (checked on the host while they are staged, or produced by
// the distribute kernels), so a row id is below Lx Ly; rowstart holds ranks in [0, m]; a search reads inside its [lo, hi); p -/+ 1
// is tested against [0, m); indices holds a permutation of [0, m) made on the device.
//
// Scratch per particle of pf_neighbours: positions and their ranks through the pair sort of pf_organize.hip (4 x 4), Fmax as staged
// and in position order (2 K, K = 4 or 8), the table and the flags (24 + 1): 49 bytes (57), plus 4 (Lx Ly + 1) of rowstart and the
// sort's histograms.  The fused call adds K + 25 per returned record to what pf_distribute_sorted holds.
#include <hip/hip_runtime.h>

#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pf_internal.h"
#include "pf_map_core.h"
#include "pf_neigh_core.h"

#define PF_NEIGH_BLOCK 256

// ---------------------------------------------------------------------------------------------------------- kernels ----
template <typename T>
__global__ void __launch_bounds__(PF_NEIGH_BLOCK) k_neigh_fpos(unsigned int m, const unsigned int *__restrict__ indices, const unsigned int *__restrict__ perm,
                                                               const unsigned int *__restrict__ cell, const T *__restrict__ src, T *__restrict__ fpos) {
  const unsigned long long p = (unsigned long long)blockIdx.x * PF_NEIGH_BLOCK + threadIdx.x;
  if (p >= m) return;
  size_t a = indices[p];
  if (perm) a = perm[a];
  if (cell) a = cell[a];
  fpos[p] = src[a];
}

__global__ void __launch_bounds__(PF_NEIGH_BLOCK) k_neigh_rows(unsigned int m, const unsigned int *__restrict__ spos, unsigned int nrows, unsigned int lz,
                                                               unsigned int *__restrict__ rowstart) {
  const unsigned long long r = (unsigned long long)blockIdx.x * PF_NEIGH_BLOCK + threadIdx.x;
  if (r > nrows) return;
  rowstart[r] = pf_neigh_lower_bound(spos, m, r * (unsigned long long)lz);
}

template <typename T, bool ROWS>
__global__ void __launch_bounds__(PF_NEIGH_BLOCK) k_neigh(PfNeighBox b, unsigned int m, const unsigned int *__restrict__ spos, const unsigned int *__restrict__ indices,
                                                          const T *__restrict__ fpos, const unsigned int *__restrict__ rowstart, int *__restrict__ neigh,
                                                          unsigned char *__restrict__ flags, unsigned long long *__restrict__ counters) {
  const unsigned long long pl = (unsigned long long)blockIdx.x * PF_NEIGH_BLOCK + threadIdx.x;
  unsigned long long c0 = 0, c1 = 0;
  if (pl < m) {
    const unsigned int p = (unsigned int)pl, pos = spos[p];
    int c[3], out[6] = {-1, -1, -1, -1, -1, -1};
    pf_neigh_coord(b, pos, c);
    const bool skip = pf_neigh_skip(b, c), good = pf_neigh_good(b, c);
    bool peak = !skip;
    if (!skip) {
      const T f = fpos[p];
      const unsigned int *rs = ROWS ? rowstart : nullptr;
#pragma unroll
      for (int nn = 0; nn < 6; nn++) {
        const long long r = pf_neigh_rank(b, m, spos, rs, p, c, nn);
        if (r >= 0) {
          out[nn] = (int)indices[r];
          peak = peak && (f > fpos[r]);   // the C comparison in the product precision: a NaN on either side clears it
        }
      }
    }
    const unsigned int iz = indices[p];
    if (neigh) {
      int2 *dst = (int2 *)(neigh + 6 * (size_t)iz);   // (24 iz bytes into an allocation: 8-byte aligned)
      dst[0] = make_int2(out[0], out[1]); dst[1] = make_int2(out[2], out[3]); dst[2] = make_int2(out[4], out[5]);
    }
    if (flags) flags[iz] = (unsigned char)((skip ? PF_NEIGH_SKIP : 0) | (good ? PF_NEIGH_GOOD : 0) | (peak ? PF_NEIGH_PEAK : 0));
    c0 = peak ? 1u : 0u;
    c1 = (peak && good) ? 1u : 0u;
  }
  for (int o = 32; o > 0; o >>= 1) { c0 += __shfl_down(c0, o, 64); c1 += __shfl_down(c1, o, 64); }
  if ((threadIdx.x & 63) == 0) {
    if (c0) atomicAdd(counters, c0);
    if (c1) atomicAdd(counters + 1, c1);
  }
}

// ------------------------------------------------------------------------------------------------------------ launches ----
static unsigned int neigh_blocks(unsigned long long threads) { return (unsigned int)((threads + PF_NEIGH_BLOCK - 1) / PF_NEIGH_BLOCK); }

// what a call holds on the device beside the position index (neigh_release)
struct PfNeighScratch {
  unsigned int *buf[4];             // pf_neighbours: the four buffers of the position sort (positions staged in buf[0])
  void *fs, *fpos;                  // Fmax as staged (pf_neighbours), and in position order
  unsigned int *rowstart;
  int *neigh; unsigned char *flags;
  unsigned long long *counters;
  void *tmp;                        // rocPRIM's
};
static void neigh_release(PfNeighScratch *s) {
  for (int i = 0; i < 4; i++) hipFree(s->buf[i]);
  hipFree(s->fs); hipFree(s->fpos); hipFree(s->rowstart); hipFree(s->neigh); hipFree(s->flags); hipFree(s->counters); hipFree(s->tmp);
  memset(s, 0, sizeof(*s));
}
struct NeighGuard { PfNeighScratch *s; ~NeighGuard() { neigh_release(s); } };

static size_t neigh_scratch_bytes(size_t m, int pb, unsigned long long nrows, bool own_index, bool rows, bool neigh, bool flags) {
  return m * (size_t)((own_index ? 16 + pb : 0) + pb + (neigh ? 24 : 0) + (flags ? 1 : 0)) + (rows ? (size_t)(nrows + 1) * 4 : 0) + 16;
}
static int neigh_alloc(PfNeighScratch *s, size_t m, int pb, unsigned long long nrows, bool own_index, bool rows, bool neigh, bool flags) {
  bool ok = hipMalloc(&s->fpos, m * (size_t)pb) == hipSuccess && hipMalloc((void **)&s->counters, 2 * sizeof(unsigned long long)) == hipSuccess;
  if (ok && own_index) {
    for (int i = 0; i < 4 && ok; i++) ok = hipMalloc((void **)&s->buf[i], m * 4) == hipSuccess;
    ok = ok && hipMalloc(&s->fs, m * (size_t)pb) == hipSuccess;
  }
  if (ok && rows) ok = hipMalloc((void **)&s->rowstart, (size_t)(nrows + 1) * 4) == hipSuccess;
  if (ok && neigh) ok = hipMalloc((void **)&s->neigh, m * 24) == hipSuccess;
  if (ok && flags) ok = hipMalloc((void **)&s->flags, m) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); neigh_release(s); return 1; }
  return 0;
}

// the three kernels on the position index of m particles (0 < m < 2^31); fsrc: Fmax of particle i at element cell[perm[i]] (either
// may be null)
static int neigh_run(const PfNeighBox &b, size_t m, const unsigned int *spos, const unsigned int *indices, const unsigned int *perm, const unsigned int *cell,
                     const void *fsrc, int pb, bool rows, PfNeighScratch *s, hipStream_t st) {
  const unsigned int mm = (unsigned int)m, nrows = (unsigned int)b.len[0] * (unsigned int)b.len[1];
  const dim3 grid(neigh_blocks(m)), block(PF_NEIGH_BLOCK);
  if (hipMemsetAsync(s->counters, 0, 2 * sizeof(unsigned long long), st) != hipSuccess) return 1;
  if (pb == 8) hipLaunchKernelGGL(k_neigh_fpos<double>, grid, block, 0, st, mm, indices, perm, cell, (const double *)fsrc, (double *)s->fpos);
  else hipLaunchKernelGGL(k_neigh_fpos<float>, grid, block, 0, st, mm, indices, perm, cell, (const float *)fsrc, (float *)s->fpos);
  if (hipGetLastError() != hipSuccess) return 1;
  if (rows) {
    hipLaunchKernelGGL(k_neigh_rows, dim3(neigh_blocks((unsigned long long)nrows + 1)), block, 0, st, mm, spos, nrows, (unsigned int)b.len[2], s->rowstart);
    if (hipGetLastError() != hipSuccess) return 1;
  }
  auto launch = [&](auto kernel, auto *f) { hipLaunchKernelGGL(kernel, grid, block, 0, st, b, mm, spos, indices, f, s->rowstart, s->neigh, s->flags, s->counters); };
  if (pb == 8) { if (rows) launch(k_neigh<double, true>, (const double *)s->fpos); else launch(k_neigh<double, false>, (const double *)s->fpos); }
  else { if (rows) launch(k_neigh<float, true>, (const float *)s->fpos); else launch(k_neigh<float, false>, (const float *)s->fpos); }
  return hipGetLastError() != hipSuccess;
}

static bool neigh_rows_form() {   // PF_NEIGH_ROWS, read per call
  const char *e = getenv("PF_NEIGH_ROWS");
  return !(e && atoi(e) == 0);
}
static unsigned int neigh_bits(unsigned long long cells) {   // positions lie below `cells`
  unsigned int b = 1;
  while (b < 32 && (1ull << b) < cells) b++;
  return b;
}
// measurement aid (profiles/tools/neigh_time.py): under PF_NEIGH_STATS=1 a context-free pf_neighbours brackets its position sort and
// its table kernels with HIP events; pf_debug_neigh_ms hands the two spans of the calling thread's last such call out
static thread_local float neigh_last_ms[2] = {-1.0f, -1.0f};
struct NeighEvents {
  hipEvent_t e[3]; bool on;
  explicit NeighEvents(bool want) : on(want) {
    for (int i = 0; i < 3; i++) e[i] = nullptr;
    for (int i = 0; i < 3 && on; i++) on = hipEventCreate(&e[i]) == hipSuccess;
  }
  void mark(int i) { if (on) hipEventRecord(e[i], nullptr); }
  void read() {
    neigh_last_ms[0] = neigh_last_ms[1] = -1.0f;
    if (on && hipEventSynchronize(e[2]) == hipSuccess) { hipEventElapsedTime(&neigh_last_ms[0], e[0], e[1]); hipEventElapsedTime(&neigh_last_ms[1], e[1], e[2]); }
  }
  ~NeighEvents() { for (int i = 0; i < 3; i++) if (e[i]) hipEventDestroy(e[i]); }
};
extern "C" int pf_debug_neigh_ms(double *sort_ms, double *table_ms) {
  if (!sort_ms || !table_ms) return pf_fail(0, "pf_debug_neigh_ms: null argument");
  if (neigh_last_ms[0] < 0) return pf_fail(0, "pf_debug_neigh_ms: no context-free pf_neighbours of this thread ran under PF_NEIGH_STATS=1");
  *sort_ms = neigh_last_ms[0]; *table_ms = neigh_last_ms[1];
  return 0;
}
// the timers of a context; nothing without one
struct NeighTimer {
  void *t; int phase;
  NeighTimer(pf_ctx *c, int phase_, double bytes = 0, hipStream_t st = nullptr) : t(c ? pf_ctx_timer_begin(c, phase_, bytes, st) : nullptr), phase(phase_) {}
  ~NeighTimer() { if (t) pf_ctx_timer_end(t, phase); }
};
static double neigh_kernel_bytes(size_t m, int pb, bool neigh, bool flags) {   // index and Fmax read (the latter twice), table written
  return (double)m * (12.0 + 2.0 * pb + (neigh ? 24.0 : 0.0) + (flags ? 1.0 : 0.0));
}

#define NEIGHHIP(task, who, call)                                                                                      \
  do {                                                                                                                 \
    hipError_t e__ = (call);                                                                                           \
    if (e__ != hipSuccess) return pf_fail(task, "%s: %s failed: %s", who, #call, hipGetErrorString(e__));             \
  } while (0)

// the results of a call with a context: the table through the hand-off pieces, the counts behind the kernels
static int neigh_leave(pf_ctx *c, const PfCtxView &v, const char *who, size_t m, PfNeighScratch *s, int *neigh, unsigned char *flags, unsigned long long *peaks) {
  unsigned long long h[2] = {0, 0};
  NEIGHHIP(v.rank, who, hipMemcpyAsync(h, s->counters, sizeof(h), hipMemcpyDeviceToHost, v.stream));
  NEIGHHIP(v.rank, who, hipStreamSynchronize(v.stream));
  if (neigh && pf_ctx_d2h(c, neigh, s->neigh, m * 24)) return 1;
  if (flags && pf_ctx_d2h(c, flags, s->flags, m)) return 1;
  if (peaks) { peaks[0] = h[0]; peaks[1] = h[1]; }
  return 0;
}

int pf_neigh_from_index(pf_ctx *c, const PfCtxView &v, const char *who, const PfNeighOut &nb, size_t m, const unsigned int *sorted_pos,
                        const unsigned int *indices, const unsigned int *perm, const unsigned int *cell, const void *fmax) {
  PfNeighBox b;
  for (int d = 0; d < 3; d++) { b.len[d] = nb.len[d]; b.pbc[d] = nb.pbc[d]; b.safe[d] = nb.safe[d]; }
  const unsigned long long nrows = (unsigned long long)b.len[0] * (unsigned long long)b.len[1];
  PfNeighScratch s;
  memset(&s, 0, sizeof(s));
  NeighGuard guard{&s};
  if (neigh_alloc(&s, m, v.pb, nrows, false, nb.rows, nb.neigh != nullptr, nb.flags != nullptr))
    return pf_fail(v.rank, "%s: cannot allocate %zu bytes of scratch on the device for the neighbour table of %zu records", who,
                   neigh_scratch_bytes(m, v.pb, nrows, false, nb.rows, nb.neigh != nullptr, nb.flags != nullptr), m);
  {
    NeighTimer kt(c, 0, neigh_kernel_bytes(m, v.pb, nb.neigh != nullptr, nb.flags != nullptr), v.stream);
    if (neigh_run(b, m, sorted_pos, indices, perm, cell, fmax, v.pb, nb.rows, &s, v.stream)) return pf_fail(v.rank, "%s: launch failed", who);
  }
  return neigh_leave(c, v, who, m, &s, nb.neigh, nb.flags, nb.peaks);
}

// -------------------------------------------------------------------------------------------------------- entry points ----
extern "C" int pf_neighbours(pf_ctx *c, const pf_peak_region *box, size_t count, const unsigned int *frag_pos, const void *fmax, size_t fmax_stride,
                             int *neigh, unsigned char *flags, unsigned long long peaks[2]) {
  const char *who = "pf_neighbours";
  PfCtxView v;
  memset(&v, 0, sizeof(v));
  v.pb = 4;
  if (c) pf_ctx_view(c, &v);
  if (!box || !peaks || (count && (!frag_pos || !fmax))) return pf_fail(v.rank, "%s: null argument", who);
  PfMapBox mb;
  unsigned long long cells = 1;
  if (pf_map_box_check(who, v.rank, c ? v.n : 0, box, &mb, &cells)) return 1;
  if (count > 0x7FFFFFFFull) return pf_fail(v.rank, "%s: %zu records: the table is int like indices[], 2^31 - 1 records at most", who, count);
  const size_t elem = (size_t)v.pb;
  if (fmax_stride % elem) return pf_fail(v.rank, "%s: a stride of %zu bytes is no multiple of the %zu bytes of an Fmax", who, fmax_stride, elem);
  if (!count) { peaks[0] = peaks[1] = 0; return 0; }
  PfNeighBox b;
  for (int d = 0; d < 3; d++) { b.len[d] = mb.len[d]; b.pbc[d] = mb.pbc[d]; b.safe[d] = box->safe[d]; }
  const unsigned long long nrows = (unsigned long long)b.len[0] * (unsigned long long)b.len[1];
  const bool rows = neigh_rows_form();
  NeighTimer pt(c, 1);
  PfNeighScratch s;
  memset(&s, 0, sizeof(s));
  NeighGuard guard{&s};
  if (neigh_alloc(&s, count, v.pb, nrows, true, rows, neigh != nullptr, flags != nullptr))
    return pf_fail(v.rank, "%s: cannot allocate %zu bytes of scratch on the device for %zu records", who,
                   neigh_scratch_bytes(count, v.pb, nrows, true, rows, neigh != nullptr, flags != nullptr), count);
  // staging: positions are checked, the strided Fmax packed, on the way into the upload
  size_t bad = 0;
  if (c) {
    const int rc = pf_ctx_h2d_packed(c, s.buf[0], frag_pos, count, 4, 4, cells, &bad);
    if (rc == 2) return pf_fail(v.rank, "%s: frag_pos[%zu] = %u lies outside the box of %llu cells", who, bad, frag_pos[bad], cells);
    if (rc || pf_ctx_h2d_packed(c, s.fs, fmax, count, elem, fmax_stride, 0, &bad)) return 1;
  } else {
    for (size_t i = 0; i < count; i++)
      if (frag_pos[i] >= cells) return pf_fail(0, "%s: frag_pos[%zu] = %u lies outside the box of %llu cells", who, i, frag_pos[i], cells);
    std::vector<char> packed;
    const void *src = fmax;
    if (fmax_stride != elem) {
      packed.resize(count * elem);
      for (size_t i = 0; i < count; i++) memcpy(packed.data() + i * elem, (const char *)fmax + i * fmax_stride, elem);
      src = packed.data();
    }
    NEIGHHIP(0, who, hipMemcpy(s.buf[0], frag_pos, count * 4, hipMemcpyHostToDevice));
    NEIGHHIP(0, who, hipMemcpy(s.fs, src, count * elem, hipMemcpyHostToDevice));
  }
  unsigned int *spos = nullptr, *indices = nullptr;
  const char *se = getenv("PF_NEIGH_STATS");
  NeighEvents ev(!c && se && atoi(se) != 0);
  {
    const unsigned int bits = neigh_bits(cells);
    NeighTimer kt(c, 0, (double)count * (16.0 * ((bits + 7) / 8)) + neigh_kernel_bytes(count, v.pb, neigh != nullptr, flags != nullptr), v.stream);
    ev.mark(0);
    if (pf_org_position_sort(s.buf[0], s.buf[1], s.buf[2], s.buf[3], count, bits, &s.tmp, v.stream, &spos, &indices))
      return pf_fail(v.rank, "%s: position sort failed (out of memory?)", who);
    ev.mark(1);
    if (neigh_run(b, count, spos, indices, nullptr, nullptr, s.fs, v.pb, rows, &s, v.stream)) return pf_fail(v.rank, "%s: launch failed", who);
    ev.mark(2);
  }
  if (c) return neigh_leave(c, v, who, count, &s, neigh, flags, peaks);
  unsigned long long h[2] = {0, 0};
  NEIGHHIP(0, who, hipStreamSynchronize(nullptr));
  ev.read();
  NEIGHHIP(0, who, hipMemcpy(h, s.counters, sizeof(h), hipMemcpyDeviceToHost));
  if (neigh) NEIGHHIP(0, who, hipMemcpy(neigh, s.neigh, count * 24, hipMemcpyDeviceToHost));
  if (flags) NEIGHHIP(0, who, hipMemcpy(flags, s.flags, count, hipMemcpyDeviceToHost));
  peaks[0] = h[0]; peaks[1] = h[1];
  return 0;
}

extern "C" int pf_distribute_sorted_neighbours_map(pf_ctx *c, double flast, pf_map *m, int which, const pf_product_layout *l, size_t capacity, void *frag,
                                                   unsigned int *frag_pos, unsigned int *sorted_pos, int *indices, int *neigh, unsigned char *flags,
                                                   unsigned long long peaks[2], size_t *count) {
  const char *who = "pf_distribute_sorted_neighbours_map";
  if (!c) return pf_fail(0, "%s: null argument", who);
  PfCtxView v;
  pf_ctx_view(c, &v);
  PfMapView mv;
  if (pf_map_view(who, c, v.rank, m, which, &mv)) return 1;
  pf_subbox sub;
  PfNeighOut nb;
  for (int d = 0; d < 3; d++) {
    sub.start[d] = mv.start[d]; sub.len[d] = mv.len[d];
    nb.len[d] = mv.len[d]; nb.pbc[d] = mv.len[d] == v.n; nb.safe[d] = mv.safe[d];
  }
  nb.rows = neigh_rows_form(); nb.neigh = neigh; nb.flags = flags; nb.peaks = peaks;
  size_t taken = 0;
  return pf_distribute_sorted_impl(who, c, flast, &sub, nullptr, mv.bits, l, capacity, frag, frag_pos, sorted_pos, indices, count ? count : &taken, &nb);
}
