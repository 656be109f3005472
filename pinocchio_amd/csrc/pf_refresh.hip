// pf_refresh.hip -- the velocities of the stored particles of a sub-box after a new redshift segment (src/fragment.c:398-430).  The
// reference runs a whole second distribute() + sort_and_organize() to bring Vel* and Vel*_prev into frag[]; the stored set and its
// order cannot have changed, so here it is a gather by position, the mirror image of the scatter of pf_back.hip: 24 numbers per
// particle -- the twelve displacement columns and their copies of the segment before (vel12_prev, pf_shift_displacements).
//
//  k_refresh_flag    one particle per lane, in the particles' own order: whether the cell of its position lies in this slab
//                    (pf_refresh_core.h: no good_particle test), as one ballot per wave and one count per block of PF_REFRESH_BLOCK.
//  k_refresh_scan    exclusive scan of the block counts by one workgroup (the pattern of k_dist_scan), 64-bit totals.
//  k_refresh_gather  slot j of a found particle i = the found particles before it: the output is in ascending i whatever the thread
//                    order.  Two forms.  Natural (ORDERED false): thread t takes particle t; the found particles of a workgroup have
//                    consecutive slots, so their 24 values are staged in LDS (one column per padded row: the writes of a wave fall
//                    into distinct banks) and leave as contiguous 16-byte stores, as k_dist_pack writes its records; the 24 column
//                    reads per particle are scattered lines.  Ordered: thread t takes particle order[t], the caller's indices[] of
//                    sort_and_organize -- consecutive threads are z-neighbours, the column reads of a wave fall into few lines -- and
//                    each lane writes its own 96 (192) bytes as 16-byte stores at its slot.
//
// Every index is in range by construction: positions are below Lx Ly Lz and order entries below count -- checked on the host while
// they are staged, before anything is launched --, pf_refresh_cell gives an address only for a cell of the slab, and a slot is
// written only below the capacity the buffers were allocated for.
// Not tuned: the found particles' output lies whole on the device (4 + 24 PRODFLOAT bytes each) before it travels in the hand-off
// pieces (profiles/refresh_notes.md).
#include <hip/hip_runtime.h>

#include <stdlib.h>
#include <string.h>

#include "pf_internal.h"
#include "pf_map_core.h"
#include "pf_distribute_boxes.h"
#include "pf_refresh_core.h"

#define PF_REFRESH_PAD (PF_REFRESH_BLOCK + 1)   // words of a staged column: 257, so that (column, particle) -> bank (column + particle) % 32

// ---------------------------------------------------------------------------------------------------------- kernels ----
__global__ void __launch_bounds__(PF_REFRESH_BLOCK) k_refresh_flag(PfBackBox b, unsigned long long count, const unsigned int *__restrict__ pos,
                                                                   unsigned long long *__restrict__ masks, unsigned int *__restrict__ counts) {
  __shared__ unsigned int wcount[PF_REFRESH_WAVES];
  const unsigned long long i = (unsigned long long)blockIdx.x * PF_REFRESH_BLOCK + threadIdx.x;
  bool found = false;
  if (i < count) {
    size_t addr;
    found = pf_refresh_cell(b, pos[i], &addr);
  }
  const unsigned long long m = __ballot(found);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    masks[(unsigned long long)blockIdx.x * PF_REFRESH_WAVES + wave] = m;
    wcount[wave] = (unsigned int)__popcll(m);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int s = 0;
    for (int w = 0; w < PF_REFRESH_WAVES; w++) s += wcount[w];
    counts[blockIdx.x] = s;
  }
}

// offs[i] = counts[0] + ... + counts[i - 1], offs[nblocks] = the total; one workgroup, tiles of 4096 counts (a tile sums to 2^20 at most)
__global__ void __launch_bounds__(1024) k_refresh_scan(const unsigned int *__restrict__ counts, unsigned long long nblocks, unsigned long long *__restrict__ offs) {
  __shared__ unsigned int wsum[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  unsigned long long carry = 0;
  for (unsigned long long base = 0; base < nblocks; base += 4096) {
    const unsigned long long i0 = base + 4ull * tid;
    unsigned int v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = i0 + k < nblocks ? counts[i0 + k] : 0u;
    const unsigned int s = v[0] + v[1] + v[2] + v[3];
    unsigned int incl = s;
    for (int o = 1; o < 64; o <<= 1) { const unsigned int x = __shfl_up(incl, o, 64); if (lane >= o) incl += x; }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    unsigned int wbase = 0, tot = 0;
    for (int q = 0; q < 16; q++) { const unsigned int x = wsum[q]; if (q < w) wbase += x; tot += x; }
    unsigned long long run = carry + wbase + (incl - s);
#pragma unroll
    for (int k = 0; k < 4; k++) if (i0 + k < nblocks) { offs[i0 + k] = run; run += v[k]; }
    carry += tot;
    __syncthreads();
  }
  if (tid == 0) offs[nblocks] = carry;
}

// the columns as 4-byte words: PfRefreshCols (pf_internal.h)
// word w (0 .. 24 WPE - 1) of the output of the particle whose cell is addr: value k = w / WPE -- current column k, or prev column
// k - 12 --, half h = w % WPE of it
template <int WPE>
__device__ __forceinline__ unsigned int refresh_word(const PfRefreshCols &c, int w, size_t addr) {
  const int k = w / WPE, h = w % WPE, col = k < 12 ? k : k - 12;
  const unsigned int *set = k < 12 ? c.cur : c.prev;
  if (!set || col >= c.kmax) return 0u;
  return set[((size_t)col * c.ncell + addr) * WPE + h];
}

template <int WPE, bool ORDERED>
__global__ void __launch_bounds__(PF_REFRESH_BLOCK) k_refresh_gather(PfBackBox b, unsigned long long count, const unsigned int *__restrict__ pos,
                                                                     const int *__restrict__ order, const unsigned long long *__restrict__ masks,
                                                                     const unsigned long long *__restrict__ offs, PfRefreshCols cols,
                                                                     unsigned long long cap, unsigned int *__restrict__ index,
                                                                     unsigned int *__restrict__ vel) {
  constexpr int NW = 24 * WPE;   // words of a particle's output
  const unsigned long long t = (unsigned long long)blockIdx.x * PF_REFRESH_BLOCK + threadIdx.x;
  if (ORDERED) {
    if (t >= count) return;
    const unsigned long long i = (unsigned long long)(unsigned int)order[t];
    if (!pf_refresh_found(masks, i)) return;
    const unsigned long long j = offs[i / PF_REFRESH_BLOCK] + pf_refresh_rank_in_block(masks, i);
    if (j >= cap) return;
    size_t addr = 0;
    pf_refresh_cell(b, pos[i], &addr);
    if (index) index[j] = (unsigned int)i;
    if (vel) {
      uint4 *dst = (uint4 *)(vel + j * NW);   // 96 j or 192 j bytes behind a base that hipMalloc aligned
#pragma unroll
      for (int q = 0; q < NW / 4; q++) {
        uint4 o;
        o.x = refresh_word<WPE>(cols, 4 * q, addr); o.y = refresh_word<WPE>(cols, 4 * q + 1, addr);
        o.z = refresh_word<WPE>(cols, 4 * q + 2, addr); o.w = refresh_word<WPE>(cols, 4 * q + 3, addr);
        dst[q] = o;
      }
    }
  } else {
    __shared__ unsigned int stage[NW * PF_REFRESH_PAD];
    const unsigned long long g = blockIdx.x, og = offs[g], cg = offs[g + 1] - og;
    if (!cg || og >= cap) return;   // (the whole workgroup)
    if (t < count && pf_refresh_found(masks, t)) {
      const unsigned int rank = pf_refresh_rank_in_block(masks, t);
      if (og + rank < cap) {
        if (index) index[og + rank] = (unsigned int)t;
        if (vel) {
          size_t addr = 0;
          pf_refresh_cell(b, pos[t], &addr);
#pragma unroll
          for (int w = 0; w < NW; w++) stage[w * PF_REFRESH_PAD + rank] = refresh_word<WPE>(cols, w, addr);
        }
      }
    }
    if (!vel) return;
    __syncthreads();
    // the workgroup's particles below the capacity as consecutive 16-byte pieces: piece q holds words 4 (q % (NW / 4)) .. + 3 of
    // particle q / (NW / 4)
    const unsigned int nrec = (unsigned int)(cap - og < cg ? cap - og : cg), npiece = nrec * (NW / 4);
    uint4 *dst = (uint4 *)(vel + og * NW);
    for (unsigned int q = threadIdx.x; q < npiece; q += PF_REFRESH_BLOCK) {
      const unsigned int r = q / (NW / 4), w0 = 4 * (q % (NW / 4));
      uint4 o;
      o.x = stage[w0 * PF_REFRESH_PAD + r]; o.y = stage[(w0 + 1) * PF_REFRESH_PAD + r];
      o.z = stage[(w0 + 2) * PF_REFRESH_PAD + r]; o.w = stage[(w0 + 3) * PF_REFRESH_PAD + r];
      dst[q] = o;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ launches ----
#define REFHIP(task, who, call)                                                                                        \
  do {                                                                                                                 \
    hipError_t e__ = (call);                                                                                           \
    if (e__ != hipSuccess) return pf_fail(task, "%s: %s failed: %s", who, #call, hipGetErrorString(e__));             \
  } while (0)

// what a call holds on the device beside the columns: PfRefreshScratch (pf_internal.h)
static void refresh_release(PfRefreshScratch *s) {
  hipFree(s->pos); hipFree(s->order); hipFree(s->masks); hipFree(s->offs); hipFree(s->counts); hipFree(s->index); hipFree(s->vel);
  memset(s, 0, sizeof(*s));
}
struct RefreshGuard { PfRefreshScratch *s; ~RefreshGuard() { refresh_release(s); } };
static size_t refresh_blocks(size_t count) { return (count + PF_REFRESH_BLOCK - 1) / PF_REFRESH_BLOCK; }
static size_t refresh_in_bytes(size_t count, bool with_order) {
  const size_t nb = refresh_blocks(count);
  return count * (size_t)(with_order ? 8 : 4) + nb * (PF_REFRESH_WAVES * 8 + 4) + (nb + 1) * 8;
}
static int refresh_alloc_in(PfRefreshScratch *s, size_t count, bool with_order) {
  const size_t nb = refresh_blocks(count);
  bool ok = hipMalloc((void **)&s->pos, count * 4) == hipSuccess && hipMalloc((void **)&s->masks, nb * PF_REFRESH_WAVES * 8) == hipSuccess &&
            hipMalloc((void **)&s->counts, nb * 4) == hipSuccess && hipMalloc((void **)&s->offs, (nb + 1) * 8) == hipSuccess;
  if (ok && with_order) ok = hipMalloc((void **)&s->order, count * 4) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); return 1; }
  return 0;
}
static int refresh_alloc_out(PfRefreshScratch *s, size_t m, int pb, bool want_index, bool want_vel) {
  bool ok = true;
  if (want_index) ok = hipMalloc((void **)&s->index, m * 4) == hipSuccess;
  if (ok && want_vel) ok = hipMalloc(&s->vel, m * 24 * (size_t)pb) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); return 1; }
  return 0;
}

// flag + scan, behind positions that lie on the device; *found after a synchronisation of the stream (it sizes what follows)
static int refresh_select(const char *who, int task, const PfBackBox &b, size_t count, const PfRefreshScratch &s, hipStream_t st, unsigned long long *found) {
  const size_t nb = refresh_blocks(count);
  hipLaunchKernelGGL(k_refresh_flag, dim3((unsigned int)nb), dim3(PF_REFRESH_BLOCK), 0, st, b, (unsigned long long)count, s.pos, s.masks, s.counts);
  hipLaunchKernelGGL(k_refresh_scan, dim3(1), dim3(1024), 0, st, s.counts, (unsigned long long)nb, s.offs);
  if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  REFHIP(task, who, hipMemcpyAsync(found, s.offs + nb, sizeof(*found), hipMemcpyDeviceToHost, st));
  REFHIP(task, who, hipStreamSynchronize(st));
  return 0;
}
static int refresh_gather(int pb, const PfBackBox &b, size_t count, const PfRefreshScratch &s, const PfRefreshCols &cols, unsigned long long cap, hipStream_t st) {
  const dim3 grid((unsigned int)refresh_blocks(count)), block(PF_REFRESH_BLOCK);
  unsigned int *vel = (unsigned int *)s.vel;
  const unsigned long long n = count;
  if (pb == 8) {
    if (s.order) hipLaunchKernelGGL((k_refresh_gather<2, true>), grid, block, 0, st, b, n, s.pos, s.order, s.masks, s.offs, cols, cap, s.index, vel);
    else hipLaunchKernelGGL((k_refresh_gather<2, false>), grid, block, 0, st, b, n, s.pos, s.order, s.masks, s.offs, cols, cap, s.index, vel);
  } else {
    if (s.order) hipLaunchKernelGGL((k_refresh_gather<1, true>), grid, block, 0, st, b, n, s.pos, s.order, s.masks, s.offs, cols, cap, s.index, vel);
    else hipLaunchKernelGGL((k_refresh_gather<1, false>), grid, block, 0, st, b, n, s.pos, s.order, s.masks, s.offs, cols, cap, s.index, vel);
  }
  return hipGetLastError() != hipSuccess;
}

// the box of a call: checked as pf_map_create checks its box, the start reduced as pf_distribute reduces it
static int refresh_box(const char *who, int rank, int n, int x0, int nxl, const pf_peak_region *box, PfBackBox *b, unsigned long long *cells) {
  PfMapBox mb;
  if (pf_map_box_check(who, rank, n, box, &mb, cells)) return 1;
  for (int d = 0; d < 3; d++) { b->box.len[d] = mb.len[d]; b->box.pbc[d] = mb.pbc[d]; b->box.safe[d] = box->safe[d]; b->start[d] = pf_dist_wrap(box->start[d], n); }
  b->n = n; b->x0 = x0; b->nxl = nxl;
  return 0;
}
// the first entry that is not below its limit (the staging threads know of one such entry, not of the first)
static size_t refresh_first_bad(const unsigned int *a, size_t upto, unsigned long long limit) {
  for (size_t i = 0; i < upto; i++) if (a[i] >= limit) return i;
  return upto;
}

// the fields of a record the refresh writes: slot s = 0..3 the current Vel, Vel_2LPT, Vel_3LPT_1, Vel_3LPT_2, 4..7 their *_prev;
// three PRODFLOATs each, values 3 s .. 3 s + 2 of a particle's 24 (PfRefreshFields, pf_internal.h)
static int refresh_fields(const char *who, int rank, int pb, int shifts, const pf_product_layout *l, const pf_prev_layout *p, PfRefreshFields *f) {
  f->nf = 0;
  if (l->stride < 4 || l->stride % 4 || l->stride / 4 > 0x7fffffffu)
    return pf_fail(rank, "%s: bad layout: stride %zu and the offsets must be multiples of four, fields inside the record", who, l->stride);
  const int ov[8] = {l->off_Vel, l->off_Vel_2LPT, l->off_Vel_3LPT_1, l->off_Vel_3LPT_2, p ? p->off_Vel_prev : -1, p ? p->off_Vel_2LPT_prev : -1,
                     p ? p->off_Vel_3LPT_1_prev : -1, p ? p->off_Vel_3LPT_2_prev : -1};
  const int len = 3 * pb;
  for (int s = 0; s < 8; s++) {
    if (ov[s] < 0) continue;
    if (s >= 4 && !shifts) return pf_fail(rank, "%s: the layout names a *_prev field but there is no pf_shift_displacements yet", who);
    if (ov[s] % 4 || (size_t)ov[s] + (size_t)len > l->stride)
      return pf_fail(rank, "%s: bad layout: stride %zu and the offsets must be multiples of four, fields inside the record", who, l->stride);
    for (int a = 0; a < f->nf; a++)
      if (ov[s] < f->off[a] + len && f->off[a] < ov[s] + len)
        return pf_fail(rank, "%s: fields of the layout overlap (%s at byte %d and %s at byte %d)", who, f->slot[a] < 4 ? "a Vel field" : "a *_prev field", f->off[a],
                       s < 4 ? "a Vel field" : "a *_prev field", ov[s]);
    f->off[f->nf] = ov[s]; f->slot[f->nf] = s; f->nf++;
  }
  return 0;
}

// what both entry points with a context do up to the gather: arguments, box, upload and checks, selection, the gather into s->index /
// s->vel for the first m = min(found, capacity) found particles
static int refresh_run(pf_ctx *c, const PfCtxView &v, const char *who, const pf_peak_region *box, size_t count, const unsigned int *frag_pos, const int *order,
                       size_t capacity, bool want_index, bool want_vel, PfRefreshScratch *s, size_t *found, size_t *m_out) {
  *found = 0; *m_out = 0;
  if (!box || (count && !frag_pos)) return pf_fail(v.rank, "%s: null argument", who);
  if (!v.products_init) return pf_fail(v.rank, "%s: products not computed", who);
  if (count > 0x7FFFFFFFull) return pf_fail(v.rank, "%s: %zu particles: indices[] is int as in the reference, 2^31 - 1 particles at most", who, count);
  PfBackBox b;
  unsigned long long cells = 1;
  if (refresh_box(who, v.rank, v.n, v.rank * v.nxl, v.nxl, box, &b, &cells)) return 1;
  if (!count) return 0;
  const void *prev = nullptr; int shifts = 0, lpt_order = 3;
  pf_ctx_prev_view(c, &prev, &shifts, &lpt_order);
  if (pf_ctx_velocities_ready(c)) return 1;
  PfScopedTimer pt(c, 1);
  if (refresh_alloc_in(s, count, order != nullptr))
    return pf_fail(v.rank, "%s: cannot allocate %zu bytes of scratch on the device for %zu particles", who, refresh_in_bytes(count, order != nullptr), count);
  size_t bad = 0;
  int rc = pf_ctx_h2d_packed(c, s->pos, frag_pos, count, 4, 4, cells, &bad);
  if (rc == 2) {
    bad = refresh_first_bad(frag_pos, bad, cells);
    return pf_fail(v.rank, "%s: frag_pos[%zu] = %u lies outside the %llu cells of the box", who, bad, frag_pos[bad], cells);
  }
  if (rc) return 1;
  if (order) {
    rc = pf_ctx_h2d_packed(c, s->order, order, count, 4, 4, (unsigned long long)count, &bad);
    if (rc == 2) {
      bad = refresh_first_bad((const unsigned int *)order, bad, count);
      return pf_fail(v.rank, "%s: order[%zu] = %d is no index of the %zu particles", who, bad, order[bad], count);
    }
    if (rc) return 1;
  }
  unsigned long long h = 0;
  {
    PfScopedTimer kt(c, 0, (double)count * 4.0 + (double)refresh_blocks(count) * 56.0, v.stream);
    if (refresh_select(who, v.rank, b, count, *s, v.stream, &h)) return 1;
  }
  *found = (size_t)h;
  const size_t m = h < capacity ? (size_t)h : capacity;
  *m_out = m;
  if (!m || (!want_index && !want_vel)) return 0;
  if (refresh_alloc_out(s, m, v.pb, want_index, want_vel))
    return pf_fail(v.rank, "%s: cannot allocate %zu bytes on the device for the velocities of %zu particles", who, m * ((want_index ? 4 : 0) + (want_vel ? 24 * (size_t)v.pb : 0)), m);
  if (order) {   // an order that is no permutation omits particles: their entries then read 0xFFFFFFFF / zero, not what the memory held
    if (s->index) REFHIP(v.rank, who, hipMemsetAsync(s->index, 0xFF, m * 4, v.stream));
    if (s->vel) REFHIP(v.rank, who, hipMemsetAsync(s->vel, 0, m * 24 * (size_t)v.pb, v.stream));
  }
  PfRefreshCols cols;
  cols.cur = (const unsigned int *)v.vel12; cols.prev = (const unsigned int *)prev; cols.ncell = v.ncell; cols.kmax = lpt_order >= 3 ? 12 : lpt_order == 2 ? 6 : 3;   // columns 3 o .. 3 o + 2 of order o: 0 Zel'dovich, 1 2LPT, 2 3LPT(a), 3 3LPT(b)
  {
    PfScopedTimer kt(c, 0, (double)count * (order ? 24.0 : 20.0) + (double)m * (4.0 + 48.0 * v.pb), v.stream);
    if (refresh_gather(v.pb, b, count, *s, cols, m, v.stream)) return pf_fail(v.rank, "%s: launch failed", who);
  }
  return 0;
}

// what a host thread does with entries [a, e) of a piece that has arrived: the named fields of entry j into record idx[j].  An entry
// an `order` that is no permutation left unwritten (idx = 0xFFFFFFFF, not below count) is skipped
struct RefreshScatter { const unsigned int *idx; const char *val; char *rec; size_t stride, vb, pb, count; PfRefreshFields f; };
static void refresh_scatter(void *user, size_t a, size_t e) {
  const RefreshScatter &r = *(const RefreshScatter *)user;
  for (size_t j = a; j < e; j++) {
    if (r.idx[j] >= r.count) continue;
    char *dst = r.rec + (size_t)r.idx[j] * r.stride;
    const char *src = r.val + j * r.vb;
    for (int u = 0; u < r.f.nf; u++) memcpy(dst + r.f.off[u], src + (size_t)r.f.slot[u] * 3 * r.pb, 3 * r.pb);
  }
}

// the first m entries of s.index / s.vel into the caller's records: index and values of a piece in one pinned buffer, the values
// behind the indices (8-byte aligned); the host threads scatter the named fields into the records while the next piece travels
static int refresh_to_records(pf_ctx *c, const PfCtxView &v, const char *who, const PfRefreshScratch &s, size_t m, size_t count, void *frag, size_t stride,
                              const PfRefreshFields &f) {
  PfScopedTimer pt(c, 1);
  PfHandoffView h;
  if (pf_ctx_handoff_begin(c, &h)) return 1;
  const size_t pb = (size_t)v.pb, vb = 24 * pb;
  const size_t per = (h.chunk / (4 + vb)) & ~(size_t)1;
  if (!per) return pf_fail(v.rank, "%s: a particle does not fit the staging pieces", who);
  const size_t np = (m + per - 1) / per;
  auto issue = [&](size_t k) -> int {
    const int q = (int)(k & 1);
    const size_t first = k * per, cnt = m - first < per ? m - first : per;
    REFHIP(v.rank, who, hipMemcpyAsync(h.pin[q], s.index + first, cnt * 4, hipMemcpyDeviceToHost, h.st[q]));
    REFHIP(v.rank, who, hipMemcpyAsync(h.pin[q] + per * 4, (const char *)s.vel + first * vb, cnt * vb, hipMemcpyDeviceToHost, h.st[q]));
    return 0;
  };
  if (issue(0)) return 1;
  for (size_t k = 0; k < np; k++) {
    if (k + 1 < np && issue(k + 1)) return 1;
    const int q = (int)(k & 1);
    REFHIP(v.rank, who, hipStreamSynchronize(h.st[q]));
    const size_t first = k * per, cnt = m - first < per ? m - first : per;
    const unsigned int *idx = (const unsigned int *)h.pin[q];
    const char *val = h.pin[q] + per * 4;
    char *rec = (char *)frag;
    RefreshScatter job{idx, val, rec, stride, vb, pb, count, f};
    pf_ctx_host_run(c, cnt, refresh_scatter, &job);
  }
  return 0;
}

// -------------------------------------------------------------------------------------------------------- entry points ----
extern "C" int pf_gather_velocities(pf_ctx *c, const pf_peak_region *box, size_t count, const unsigned int *frag_pos, const int *order, size_t capacity,
                                    unsigned int *index, void *vel24, size_t *found) {
  const char *who = "pf_gather_velocities";
  if (!c) return pf_fail(0, "%s: null argument", who);
  PfCtxView v;
  pf_ctx_view(c, &v);
  PfRefreshScratch s;
  memset(&s, 0, sizeof(s));
  RefreshGuard guard{&s};
  size_t nfound = 0, m = 0;
  if (refresh_run(c, v, who, box, count, frag_pos, order, capacity, index != nullptr, vel24 != nullptr, &s, &nfound, &m)) return 1;
  if (m && index && pf_ctx_d2h(c, index, s.index, m * 4)) return 1;
  if (m && vel24 && pf_ctx_d2h(c, vel24, s.vel, m * 24 * (size_t)v.pb)) return 1;
  if (found) *found = nfound;
  return 0;
}

extern "C" int pf_refresh_velocities(pf_ctx *c, const pf_peak_region *box, size_t count, const unsigned int *frag_pos, const int *order, void *frag,
                                     const pf_product_layout *layout, const pf_prev_layout *prev, size_t *found) {
  const char *who = "pf_refresh_velocities";
  if (!c) return pf_fail(0, "%s: null argument", who);
  PfCtxView v;
  pf_ctx_view(c, &v);
  if (!layout || (count && !frag)) return pf_fail(v.rank, "%s: null argument", who);
  const void *pcols = nullptr; int shifts = 0, lpt_order = 3;
  pf_ctx_prev_view(c, &pcols, &shifts, &lpt_order);
  PfRefreshFields f;
  if (refresh_fields(who, v.rank, v.pb, shifts, layout, prev, &f)) return 1;
  PfRefreshScratch s;
  memset(&s, 0, sizeof(s));
  RefreshGuard guard{&s};
  size_t nfound = 0, m = 0;
  if (refresh_run(c, v, who, box, count, frag_pos, order, count, f.nf > 0, f.nf > 0, &s, &nfound, &m)) return 1;
  if (found) *found = nfound;
  if (!m || !f.nf) return 0;
  return refresh_to_records(c, v, who, s, m, count, frag, layout->stride, f);
}

// test tap without a context: the same kernels on a caller's columns, on the default stream
extern "C" int pf_debug_gather_velocities(int n, int x0, int nxl, int pb, const void *cols24, const pf_peak_region *box, size_t count,
                                          const unsigned int *frag_pos, const int *order, unsigned int *index, void *vel24, size_t *found) {
  const char *who = "pf_debug_gather_velocities";
  if (!box || !cols24 || (count && !frag_pos)) return pf_fail(0, "%s: null argument", who);
  if (pb != 4 && pb != 8) return pf_fail(0, "%s: a PRODFLOAT of %d bytes (4 or 8)", who, pb);
  if (n < 1 || n > 2048 || x0 < 0 || nxl < 1 || x0 + nxl > n) return pf_fail(0, "%s: planes %d .. %d of a box of %d^3 cells", who, x0, x0 + nxl - 1, n);
  if (count > 0x7FFFFFFFull) return pf_fail(0, "%s: %zu particles: indices[] is int as in the reference, 2^31 - 1 particles at most", who, count);
  PfBackBox b;
  unsigned long long cells = 1;
  if (refresh_box(who, 0, n, x0, nxl, box, &b, &cells)) return 1;
  for (size_t i = 0; i < count; i++)
    if (frag_pos[i] >= cells) return pf_fail(0, "%s: frag_pos[%zu] = %u lies outside the %llu cells of the box", who, i, frag_pos[i], cells);
  if (order)
    for (size_t i = 0; i < count; i++)
      if ((unsigned int)order[i] >= count) return pf_fail(0, "%s: order[%zu] = %d is no index of the %zu particles", who, i, order[i], count);
  if (found) *found = 0;
  if (!count) return 0;
  const size_t ncell = (size_t)nxl * n * n, colbytes = 24 * ncell * (size_t)pb;
  void *dcols = nullptr;
  PfRefreshScratch s;
  memset(&s, 0, sizeof(s));
  struct Columns { void **p; ~Columns() { hipFree(*p); } } columns{&dcols};
  RefreshGuard guard{&s};
  if (hipMalloc(&dcols, colbytes) != hipSuccess || refresh_alloc_in(&s, count, order != nullptr) || refresh_alloc_out(&s, count, pb, true, true)) {
    (void)hipGetLastError();
    return pf_fail(0, "%s: cannot allocate %zu bytes on the device", who, colbytes + refresh_in_bytes(count, order != nullptr) + count * (4 + 24 * (size_t)pb));
  }
  REFHIP(0, who, hipMemcpy(dcols, cols24, colbytes, hipMemcpyHostToDevice));
  REFHIP(0, who, hipMemcpy(s.pos, frag_pos, count * 4, hipMemcpyHostToDevice));
  if (order) REFHIP(0, who, hipMemcpy(s.order, order, count * 4, hipMemcpyHostToDevice));
  unsigned long long h = 0;
  if (refresh_select(who, 0, b, count, s, nullptr, &h)) return 1;
  PfRefreshCols cols;
  cols.cur = (const unsigned int *)dcols; cols.prev = cols.cur + 12 * ncell * (size_t)(pb / 4); cols.ncell = ncell; cols.kmax = 12;
  if (h) {
    if (refresh_gather(pb, b, count, s, cols, h, nullptr)) return pf_fail(0, "%s: launch failed", who);
    REFHIP(0, who, hipDeviceSynchronize());
    if (index) REFHIP(0, who, hipMemcpy(index, s.index, (size_t)h * 4, hipMemcpyDeviceToHost));
    if (vel24) REFHIP(0, who, hipMemcpy(vel24, s.vel, (size_t)h * 24 * (size_t)pb, hipMemcpyDeviceToHost));
  }
  if (found) *found = (size_t)h;
  return 0;
}

// ---- what pf_groupvel.hip uses of the above (pf_internal.h) ----
void pf_refresh_release(PfRefreshScratch *s) { refresh_release(s); }
size_t pf_refresh_blocks(size_t count) { return refresh_blocks(count); }
size_t pf_refresh_in_bytes(size_t count, bool with_order) { return refresh_in_bytes(count, with_order); }
int pf_refresh_alloc_in(PfRefreshScratch *s, size_t count, bool with_order) { return refresh_alloc_in(s, count, with_order); }
int pf_refresh_alloc_out(PfRefreshScratch *s, size_t m, int pb, bool want_index, bool want_vel) { return refresh_alloc_out(s, m, pb, want_index, want_vel); }
int pf_refresh_scan(const unsigned int *counts, size_t nblocks, unsigned long long *offs, hipStream_t st) {
  hipLaunchKernelGGL(k_refresh_scan, dim3(1), dim3(1024), 0, st, counts, (unsigned long long)nblocks, offs);
  return hipGetLastError() != hipSuccess;
}
int pf_refresh_select(const char *who, int task, const PfBackBox &b, size_t count, const PfRefreshScratch &s, hipStream_t st, unsigned long long *found) {
  return refresh_select(who, task, b, count, s, st, found);
}
int pf_refresh_gather(int pb, const PfBackBox &b, size_t count, const PfRefreshScratch &s, const PfRefreshCols &cols, unsigned long long cap, hipStream_t st) {
  return refresh_gather(pb, b, count, s, cols, cap, st);
}
int pf_refresh_box(const char *who, int rank, int n, int x0, int nxl, const pf_peak_region *box, PfBackBox *b, unsigned long long *cells) {
  return refresh_box(who, rank, n, x0, nxl, box, b, cells);
}
size_t pf_refresh_first_bad(const unsigned int *a, size_t upto, unsigned long long limit) { return refresh_first_bad(a, upto, limit); }
int pf_refresh_fields(const char *who, int rank, int pb, int shifts, const pf_product_layout *l, const pf_prev_layout *p, PfRefreshFields *f) {
  return refresh_fields(who, rank, pb, shifts, l, p, f);
}
int pf_refresh_to_records(pf_ctx *c, const PfCtxView &v, const char *who, const PfRefreshScratch &s, size_t m, size_t count, void *frag, size_t stride,
                          const PfRefreshFields &f) {
  return refresh_to_records(c, v, who, s, m, count, frag, stride, f);
}
