// pf_organize.hip -- sort_and_organize() (src/fragment.c:484-520) on the device: the call of fragment() (:193-346) that follows
// distribute().  The reference qsorts an index array by descending Fmax (index_compare_F :118-126), moves the product_data records
// and frag_pos into that order by cycle-following (reorder :533-564), qsorts again by frag_pos (index_compare_P :128-136) and
// leaves sorted_pos[] / indices[], which find_location() (:592-603) binary-searches for every neighbour lookup.  Here the records
// are never moved: they do not exist before they are written in their final order.
//
//  k_org_keys    one key per record j of the input (distribute()) order from the bits of its Fmax (pf_organize_core.h: 32 bits for
//                float products, 64 for double; -0.0 as +0.0, NaN last), carried value j.
//  sort          stable LSD radix sort of the (key, j) pairs (rocPRIM, the primitive pf_select_sort.hip uses): perm[i] = the input
//                index of output record i; equal Fmax stay in input order, the tie rule of pf_keys.h.
//  k_org_gather  the bandwidth kernel.  Output record i takes j = perm[i]; frag_pos_out[i] = frag_pos[j]; its words come from the
//                SoA columns at cell_index[j], or (pf_organize) from record j of an AoS buffer in device memory.  The source cells of
//                neighbouring outputs are unrelated -- every column read is a scattered 4-byte load whatever the kernel does -- so
//                only the writes can be coalesced: a workgroup takes a round of 256 consecutive output records, stages what a
//                record needs to be FOUND (its cell address, 4 bytes; and once per workgroup the column of every word of the
//                layout) in LDS, and then lane t produces output WORD t, t + 256, ... of the round: consecutive lanes write
//                consecutive words.  Against staging the gathered words themselves (k_dist_pack<.., true>) this keeps the
//                coalesced stores and drops the LDS round trip of the payload with its bank conflicts (a 26-word record strides
//                the 32 write banks two-way).  From an AoS source the same form reads each record as one run of consecutive words.
//                The plain form -- one lane per record, named words into a cleared buffer -- is kept for the A/B
//                (PF_DISTRIBUTE_LDS=0) and serves column records longer than PF_DIST_MAX_WORDS words.  A call packs the records
//                [first, first + cnt) of the sorted order, so that a large result leaves in staging pieces.
//  index         frag_pos_out of the records that are returned (k_org_gather without records) and i, a stable radix sort of the
//                pairs by the 32-bit position: sorted_pos[] and indices[].
//
// Scratch per selected record: cell_index and frag_pos (4 + 4), two key and two value buffers of the pair sort (2 K + 8, K = 4 or 8)
// and one more value buffer for the second sort, whose other three buffers are the first one's dead ones: 28 bytes (36 with double
// products), plus the sort's histograms.  pf_organize holds no cell_index (24 / 32) beside the records themselves.
#include <hip/hip_runtime.h>

#include <string.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "pf_internal.h"
#include "pf_organize_core.h"

#define PF_ORG_BLOCK 256

// the records in input (distribute()) order, on the device
struct PfOrgIn {
  int pb;                           // bytes of a PRODFLOAT
  const unsigned int *frag_pos;     // [total]
  // columns: cell_index[j] = slab address of record j (null: j itself)
  const unsigned int *cell_index;
  const void *fmax, *vel12; const int *rmax; size_t ncell;
  // or an AoS buffer (non-null) of records of aos_words words, Fmax at word fmax_word
  const unsigned int *aos; unsigned int aos_words, fmax_word;
};

// device memory of one call (org_release)
struct PfOrgScratch {
  unsigned int *cell, *pos;         // [total] the selection in input order
  void *kbuf[2];                    // [total] keys
  unsigned int *vbuf[2], *extra;    // [total] values; [m] the fourth buffer of the position sort
  void *tmp; size_t tmp_bytes;      // rocPRIM's own
  char *records;                    // pf_organize: the caller's records
  unsigned int *perm;               // -> one of vbuf: new -> old
  unsigned int *spare;              // -> the other one
  unsigned int *sorted_pos, *indices;
};
static void org_release(PfOrgScratch *o) {
  hipFree(o->cell); hipFree(o->pos); hipFree(o->kbuf[0]); hipFree(o->kbuf[1]); hipFree(o->vbuf[0]); hipFree(o->vbuf[1]); hipFree(o->extra);
  hipFree(o->tmp); hipFree(o->records);
  memset(o, 0, sizeof(*o));
}
struct OrgGuard { PfOrgScratch *o; ~OrgGuard() { org_release(o); } };
struct OrgDistGuard { PfDistScratch *s; ~OrgDistGuard() { pf_dist_release(s); } };

static size_t org_scratch_bytes(size_t total, size_t m, int pb, bool cell, bool index, size_t record_bytes) {
  return total * (size_t)(4 + (cell ? 4 : 0) + 2 * pb + 8) + (index ? 4 * m : 0) + record_bytes;
}
static int org_alloc(PfOrgScratch *o, size_t total, size_t m, int pb, bool cell, bool index, size_t record_bytes) {
  bool ok = hipMalloc((void **)&o->pos, total * 4) == hipSuccess && (!cell || hipMalloc((void **)&o->cell, total * 4) == hipSuccess);
  for (int b = 0; b < 2 && ok; b++)
    ok = hipMalloc(&o->kbuf[b], total * (size_t)pb) == hipSuccess && hipMalloc((void **)&o->vbuf[b], total * 4) == hipSuccess;
  if (ok && index) ok = hipMalloc((void **)&o->extra, m * 4) == hipSuccess;
  if (ok && record_bytes) ok = hipMalloc((void **)&o->records, record_bytes) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); org_release(o); return 1; }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------- kernels ----
template <typename K>
__global__ void __launch_bounds__(PF_ORG_BLOCK) k_org_keys(const unsigned int *__restrict__ fwords, size_t mult, const unsigned int *__restrict__ cell_index,
                                                           size_t total, K *__restrict__ keys, unsigned int *__restrict__ vals) {
  for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (size_t)gridDim.x * blockDim.x) {
    const size_t a = (cell_index ? (size_t)cell_index[j] : j) * mult;
    if constexpr (sizeof(K) == 8) keys[j] = (K)pf_org_key64((unsigned long long)fwords[a] | ((unsigned long long)fwords[a + 1] << 32));
    else keys[j] = (K)pf_org_key32(fwords[a]);
    vals[j] = (unsigned int)j;
  }
}

__global__ void __launch_bounds__(PF_ORG_BLOCK) k_org_iota(size_t m, unsigned int *__restrict__ v) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (size_t)gridDim.x * blockDim.x) v[i] = (unsigned int)i;
}

// the column of every word of a record: entry q gives word off[q] (the staged form: off[q] = q, every word of the record has an
// entry) as base[q][cell * mult[q]]; a null base is a zero word
struct PfOrgTab {
  const unsigned int *base[PF_DIST_MAX_WORDS];
  unsigned int off[PF_DIST_MAX_WORDS];
  unsigned char mult[PF_DIST_MAX_WORDS];
  int n;
};

template <bool AOS, bool STAGED>
__global__ void __launch_bounds__(PF_ORG_BLOCK)
    k_org_gather(const unsigned int *__restrict__ perm, const unsigned int *__restrict__ cell_index, const unsigned int *__restrict__ frag_pos, PfOrgTab tab,
                 const unsigned int *__restrict__ src, unsigned int nwords, unsigned long long first, unsigned long long cnt,
                 unsigned int *__restrict__ aos, unsigned int *__restrict__ frag_pos_out) {
  __shared__ const unsigned int *s_base[PF_DIST_MAX_WORDS];
  __shared__ unsigned int s_off[PF_DIST_MAX_WORDS], s_mult[PF_DIST_MAX_WORDS];
  __shared__ unsigned int s_addr[PF_ORG_BLOCK];   // where record r of the round comes from: cell address, or record index of the AoS source
  const unsigned int tid = threadIdx.x;
  const unsigned long long base = (unsigned long long)blockIdx.x * PF_ORG_BLOCK;   // (< cnt: the grid is ceil(cnt / PF_ORG_BLOCK))
  const unsigned int nrec = cnt - base < PF_ORG_BLOCK ? (unsigned int)(cnt - base) : PF_ORG_BLOCK;
  if (!AOS && (int)tid < tab.n) { s_base[tid] = tab.base[tid]; s_off[tid] = tab.off[tid]; s_mult[tid] = tab.mult[tid]; }
  if (tid < nrec) {
    const unsigned int j = perm[first + base + tid];
    if (frag_pos_out) frag_pos_out[base + tid] = frag_pos[j];
    s_addr[tid] = (!AOS && cell_index) ? cell_index[j] : j;
  }
  if (!aos) return;   // (the whole grid: positions only)
  __syncthreads();
  unsigned int *out = aos + base * nwords;
  if (STAGED) {
    // lane t writes word t, t + 256, ... of the round's records: word w is word q = w % nwords of record r = w / nwords
    const unsigned int nw = nrec * nwords;
#pragma unroll 4   // (independent scattered loads: several in flight per lane)
    for (unsigned int w = tid; w < nw; w += PF_ORG_BLOCK) {
      const unsigned int r = w / nwords, q = w - r * nwords;
      unsigned int v;
      if (AOS) v = src[(size_t)s_addr[r] * nwords + q];
      else { const unsigned int *b = s_base[q]; v = b ? b[(size_t)s_addr[r] * s_mult[q]] : 0u; }
      out[w] = v;
    }
  } else if (tid < nrec) {
    unsigned int *dst = out + (size_t)tid * nwords;
    const size_t a = s_addr[tid];
    if (AOS) for (unsigned int q = 0; q < nwords; q++) dst[q] = src[a * nwords + q];
    else for (int q = 0; q < tab.n; q++) dst[s_off[q]] = s_base[q][a * s_mult[q]];   // (named words only: the buffer was cleared)
  }
}

// ------------------------------------------------------------------------------------------------------------ launches ----
static int org_grid(size_t n) {
  size_t b = (n + PF_ORG_BLOCK - 1) / PF_ORG_BLOCK;
  if (b < 1) b = 1;
  if (b > 4096) b = 4096;
  return (int)b;
}

template <typename K>
static int org_sort_pairs(K *k0, K *k1, unsigned int *v0, unsigned int *v1, size_t n, unsigned int end_bit, PfOrgScratch *o, hipStream_t st,
                          K **kout, unsigned int **vout, unsigned int **vother) {
  rocprim::double_buffer<K> keys(k0, k1);
  rocprim::double_buffer<unsigned int> vals(v0, v1);
  size_t bytes = 0;
  if (rocprim::radix_sort_pairs(nullptr, bytes, keys, vals, n, 0u, end_bit, st) != hipSuccess) return 1;
  if (!bytes) bytes = 8;
  if (bytes > o->tmp_bytes) {
    hipFree(o->tmp); o->tmp = nullptr; o->tmp_bytes = 0;
    if (hipMalloc(&o->tmp, bytes) != hipSuccess) { (void)hipGetLastError(); return 1; }
    o->tmp_bytes = bytes;
  }
  if (rocprim::radix_sort_pairs(o->tmp, bytes, keys, vals, n, 0u, end_bit, st) != hipSuccess) return 1;
  *kout = keys.current(); *vout = vals.current(); *vother = vals.alternate();
  return 0;
}

// o->perm: the input index of every record of the sorted order
static int org_order(const PfOrgIn &in, size_t total, PfOrgScratch *o, hipStream_t st) {
  const unsigned int *fw = in.aos ? in.aos + in.fmax_word : (const unsigned int *)in.fmax;
  const size_t mult = in.aos ? in.aos_words : (size_t)(in.pb / 4);
  const dim3 grid(org_grid(total)), block(PF_ORG_BLOCK);
  if (in.pb == 8) {
    unsigned long long *ko;
    hipLaunchKernelGGL(k_org_keys<unsigned long long>, grid, block, 0, st, fw, mult, in.cell_index, total, (unsigned long long *)o->kbuf[0], o->vbuf[0]);
    if (hipGetLastError() != hipSuccess) return 1;
    return org_sort_pairs((unsigned long long *)o->kbuf[0], (unsigned long long *)o->kbuf[1], o->vbuf[0], o->vbuf[1], total, 64u, o, st, &ko, &o->perm, &o->spare);
  }
  unsigned int *ko;
  hipLaunchKernelGGL(k_org_keys<unsigned int>, grid, block, 0, st, fw, mult, in.cell_index, total, (unsigned int *)o->kbuf[0], o->vbuf[0]);
  if (hipGetLastError() != hipSuccess) return 1;
  return org_sort_pairs((unsigned int *)o->kbuf[0], (unsigned int *)o->kbuf[1], o->vbuf[0], o->vbuf[1], total, 32u, o, st, &ko, &o->perm, &o->spare);
}

static void org_tab(const PfOrgIn &in, const PfDistRecord &r, bool staged, PfOrgTab *t) {
  memset(t, 0, sizeof(*t));
  if (in.aos) return;
  const int wpe = in.pb / 4;
  t->n = staged ? r.nwords : r.nnamed;
  for (int q = 0; q < t->n; q++) {
    const int code = staged ? r.src[q] : r.named_src[q];   // PfDistRecord: -1 zero, 0 Rmax, 1 + h Fmax, 4 + 2 k + h displacement column k
    t->off[q] = staged ? (unsigned int)q : (unsigned int)r.named_off[q];
    if (code < 0) continue;
    if (code == 0) { t->base[q] = (const unsigned int *)in.rmax; t->mult[q] = 1; }
    else if (code < 4) { t->base[q] = (const unsigned int *)in.fmax + (code - 1); t->mult[q] = (unsigned char)wpe; }
    else {
      const int k = (code - 4) >> 1, h = (code - 4) & 1;
      t->base[q] = (const unsigned int *)in.vel12 + (size_t)k * in.ncell * wpe + h; t->mult[q] = (unsigned char)wpe;
    }
  }
}

// records [first, first + cnt) of the sorted order: aos (null: none; cnt records of r.nwords words) and frag_pos_out (null: none).
// staged: the word-per-lane form (column records of up to PF_DIST_MAX_WORDS words); else one lane per record -- from columns the
// named words only, into a buffer the caller has cleared
static int org_gather(const PfOrgIn &in, const unsigned int *perm, const PfDistRecord &r, unsigned long long first, unsigned long long cnt,
                      char *aos, unsigned int *frag_pos_out, bool staged, hipStream_t st) {
  if (!cnt) return 0;
  if (!in.aos && r.nwords > PF_DIST_MAX_WORDS) staged = false;
  PfOrgTab t;
  org_tab(in, r, staged, &t);
  const dim3 grid((unsigned int)((cnt + PF_ORG_BLOCK - 1) / PF_ORG_BLOCK)), block(PF_ORG_BLOCK);
  const unsigned int nwords = in.aos ? in.aos_words : (unsigned int)r.nwords;
  unsigned int *out = (unsigned int *)aos;
  if (in.aos) {
    if (staged) hipLaunchKernelGGL((k_org_gather<true, true>), grid, block, 0, st, perm, in.cell_index, in.frag_pos, t, in.aos, nwords, first, cnt, out, frag_pos_out);
    else hipLaunchKernelGGL((k_org_gather<true, false>), grid, block, 0, st, perm, in.cell_index, in.frag_pos, t, in.aos, nwords, first, cnt, out, frag_pos_out);
  } else {
    if (staged) hipLaunchKernelGGL((k_org_gather<false, true>), grid, block, 0, st, perm, in.cell_index, in.frag_pos, t, in.aos, nwords, first, cnt, out, frag_pos_out);
    else hipLaunchKernelGGL((k_org_gather<false, false>), grid, block, 0, st, perm, in.cell_index, in.frag_pos, t, in.aos, nwords, first, cnt, out, frag_pos_out);
  }
  return hipGetLastError() != hipSuccess;
}

// o->sorted_pos / o->indices of the first m records of the sorted order; positions below 2^pos_bits.  Reuses the three buffers the
// first sort has left dead
static int org_index(const PfOrgIn &in, size_t m, unsigned int pos_bits, PfOrgScratch *o, hipStream_t st) {
  PfDistRecord none;
  memset(&none, 0, sizeof(none));
  unsigned int *p0 = (unsigned int *)o->kbuf[0], *p1 = (unsigned int *)o->kbuf[1], *other;
  if (org_gather(in, o->perm, none, 0, m, nullptr, p0, false, st)) return 1;
  hipLaunchKernelGGL(k_org_iota, dim3(org_grid(m)), dim3(PF_ORG_BLOCK), 0, st, m, o->spare);
  if (hipGetLastError() != hipSuccess) return 1;
  return org_sort_pairs(p0, p1, o->spare, o->extra, m, pos_bits, o, st, &o->sorted_pos, &o->indices, &other);
}

// -------------------------------------------------------------------------------------------------------- entry points ----
#define ORGHIP(task, who, call)                                                                                        \
  do {                                                                                                                 \
    hipError_t e__ = (call);                                                                                           \
    if (e__ != hipSuccess) return pf_fail(task, "%s: %s failed: %s", who, #call, hipGetErrorString(e__));             \
  } while (0)

static int org_layout(int task, const char *who, int pb, const pf_product_layout *l, PfDistRecord *rec) {
  const int why = pf_dist_record(pb, l, rec);
  if (why == 1) return pf_fail(task, "%s: bad layout: stride %zu and the offsets must be multiples of four, fields inside the record", who, l->stride);
  if (why) return pf_fail(task, "%s: fields of the layout overlap", who);
  return 0;
}

// the first m records of the sorted order through the hand-off pieces, as pf_distribute sends its own: piece k is gathered into one
// of the two staging fields (records, then their frag_pos) and copied into its pinned buffer while the host threads move piece
// k - 1 into the caller's arrays
static int org_leave(pf_ctx *c, const PfCtxView &v, const char *who, const PfOrgIn &in, const unsigned int *perm, const PfDistRecord &rec, size_t stride,
                     size_t m, void *frag, unsigned int *frag_pos, bool staged) {
  PfHandoffView h;
  if (pf_ctx_handoff_begin(c, &h)) return 1;
  if (!frag) stride = 0;
  const size_t per = h.chunk / (stride + (frag_pos ? 4 : 0));
  if (!per) return pf_fail(v.rank, "%s: a record of %zu bytes does not fit the staging pieces", who, stride);
  const size_t np = (m + per - 1) / per;
  const bool clear = frag && !in.aos && !(staged && rec.nwords <= PF_DIST_MAX_WORDS);
  auto issue = [&](size_t k) -> int {
    const int b = (int)(k & 1);
    const size_t first = k * per, cnt = m - first < per ? m - first : per;
    char *stage = h.dev[b];
    unsigned int *pos_dev = (unsigned int *)(stage + per * stride);
    {
      PfScopedTimer kt(c, 0, (double)cnt * (2.0 * stride + 8.0 + (frag_pos ? 8.0 : 0.0)), h.st[b]);
      if (clear) ORGHIP(v.rank, who, hipMemsetAsync(stage, 0, cnt * stride, h.st[b]));
      if (org_gather(in, perm, rec, first, cnt, frag ? stage : nullptr, frag_pos ? pos_dev : nullptr, staged, h.st[b]))
        return pf_fail(v.rank, "%s: launch failed", who);
    }
    if (frag) ORGHIP(v.rank, who, hipMemcpyAsync(h.pin[b], stage, cnt * stride, hipMemcpyDeviceToHost, h.st[b]));
    if (frag_pos) ORGHIP(v.rank, who, hipMemcpyAsync(h.pin[b] + per * stride, pos_dev, cnt * sizeof(unsigned int), hipMemcpyDeviceToHost, h.st[b]));
    return 0;
  };
  if (issue(0)) return 1;
  for (size_t k = 0; k < np; k++) {
    if (k + 1 < np && issue(k + 1)) return 1;
    const int b = (int)(k & 1);
    ORGHIP(v.rank, who, hipStreamSynchronize(h.st[b]));
    const size_t first = k * per, cnt = m - first < per ? m - first : per;
    if (frag) pf_ctx_host_copy(c, (char *)frag + first * stride, h.pin[b], cnt * stride);
    if (frag_pos) pf_ctx_host_copy(c, frag_pos + first, h.pin[b] + per * stride, cnt * sizeof(unsigned int));
  }
  return 0;
}

// sorted_pos / indices of the first m records to the caller
static int org_index_leave(pf_ctx *c, const PfCtxView &v, const char *who, const PfOrgIn &in, size_t m, unsigned int pos_bits, PfOrgScratch *o,
                           unsigned int *sorted_pos, int *indices) {
  {
    PfScopedTimer kt(c, 0, (double)m * (16.0 + 16.0 * ((pos_bits + 7) / 8)), v.stream);
    if (org_index(in, m, pos_bits, o, v.stream)) return pf_fail(v.rank, "%s: position sort failed (out of memory?)", who);
  }
  if (sorted_pos && pf_ctx_d2h(c, sorted_pos, o->sorted_pos, m * sizeof(unsigned int))) return 1;
  if (indices && pf_ctx_d2h(c, indices, o->indices, m * sizeof(int))) return 1;
  return 0;
}

static unsigned int bits_for(unsigned long long cells) {   // positions lie below `cells`
  unsigned int b = 1;
  while (b < 32 && (1ull << b) < cells) b++;
  return b;
}

// the position sort alone, for positions the caller has put on the device (pf_neighbours.hip)
int pf_org_position_sort(unsigned int *k0, unsigned int *k1, unsigned int *v0, unsigned int *v1, size_t m, unsigned int pos_bits, void **tmp,
                         hipStream_t st, unsigned int **sorted_pos, unsigned int **indices) {
  PfOrgScratch o;
  memset(&o, 0, sizeof(o));
  unsigned int *other;
  hipLaunchKernelGGL(k_org_iota, dim3(org_grid(m)), dim3(PF_ORG_BLOCK), 0, st, m, v0);
  if (hipGetLastError() != hipSuccess) return 1;
  const int rc = org_sort_pairs(k0, k1, v0, v1, m, pos_bits, &o, st, sorted_pos, indices, &other);
  *tmp = o.tmp;
  return rc;
}

int pf_distribute_sorted_impl(const char *who, pf_ctx *c, double flast, const pf_subbox *sub, const unsigned int *map, const unsigned int *map_dev,
                              const pf_product_layout *l, size_t capacity, void *frag, unsigned int *frag_pos, unsigned int *sorted_pos, int *indices,
                              size_t *count, const PfNeighOut *nb) {
  if (!c) return pf_fail(0, "%s: null argument", who);
  PfCtxView v;
  pf_ctx_view(c, &v);
  if (!sub || !count || (frag && !l)) return pf_fail(v.rank, "%s: null argument", who);
  if (!v.products_init) return pf_fail(v.rank, "%s: products not computed", who);
  PfDistTable t;
  if (pf_dist_table_checked(v.rank, who, v.n, v.rank * v.nxl, v.nxl, sub, &t)) return 1;
  PfDistRecord rec;
  memset(&rec, 0, sizeof(rec));
  size_t stride = 0;
  if (frag) {
    if (org_layout(v.rank, who, v.pb, l, &rec)) return 1;
    stride = l->stride;
    if (l->off_Vel >= 0 || l->off_Vel_2LPT >= 0 || l->off_Vel_3LPT_1 >= 0 || l->off_Vel_3LPT_2 >= 0)
      if (pf_ctx_velocities_ready(c)) return 1;
  }
  PfScopedTimer pt(c, 1);
  PfDistScratch s;
  memset(&s, 0, sizeof(s));
  OrgDistGuard dguard{&s};
  unsigned long long total = 0;
  const double cells = 64.0 * (double)t.wave0[t.nbox];
  {
    PfScopedTimer kt(c, 0, cells * (v.pb + 0.125 + (map || map_dev ? 0.125 : 0.0)));
    if (pf_dist_select(t, v.pb, v.fmax, flast, map, map_dev, &s, v.stream, &total)) return pf_fail(v.rank, "%s: selection failed (out of memory?)", who);
  }
  *count = (size_t)total;
  if (total > 0x7FFFFFFFull)
    return pf_fail(v.rank, "%s: %llu records in one sub-box: indices[] is int as in the reference, 2^31 - 1 records at most", who, total);
  const size_t m = *count < capacity ? *count : capacity;
  const bool table = nb && (nb->neigh || nb->flags || nb->peaks);
  if (!m && nb && nb->peaks) nb->peaks[0] = nb->peaks[1] = 0;
  if (!m || (!frag && !frag_pos && !sorted_pos && !indices && !table)) return 0;
  const bool index = sorted_pos || indices || table;
  PfOrgScratch o;
  memset(&o, 0, sizeof(o));
  OrgGuard guard{&o};
  if (org_alloc(&o, (size_t)total, m, v.pb, true, index, 0))
    return pf_fail(v.rank, "%s: cannot allocate %zu bytes of scratch on the device for %llu records", who,
                   org_scratch_bytes((size_t)total, m, v.pb, true, index, 0), total);
  PfOrgIn in;
  memset(&in, 0, sizeof(in));
  in.pb = v.pb; in.frag_pos = o.pos; in.cell_index = o.cell; in.fmax = v.fmax; in.vel12 = v.vel12; in.rmax = v.rmax; in.ncell = v.ncell;
  {
    // the selection in distribute()'s order, then the order of sort_and_organize
    PfScopedTimer kt(c, 0, (double)t.ngroups * PF_DIST_GROUP_WAVES * 8.0 + (double)total * (8.0 + v.pb + 64.0 + (v.pb + 4.0) * 2.0 * v.pb));
    if (pf_dist_pack(t, s, v.pb, v.fmax, nullptr, nullptr, v.ncell, rec, 0, 0, total, nullptr, o.pos, o.cell, false, v.stream) ||
        org_order(in, (size_t)total, &o, v.stream))
      return pf_fail(v.rank, "%s: sort failed (out of memory?)", who);
  }
  if (index && org_index_leave(c, v, who, in, m, bits_for((unsigned long long)t.slen[0] * t.slen[1] * t.slen[2]), &o, sorted_pos, indices)) return 1;
  if (table && pf_neigh_from_index(c, v, who, *nb, m, o.sorted_pos, o.indices, o.perm, o.cell, v.fmax)) return 1;
  if (!frag && !frag_pos) { ORGHIP(v.rank, who, hipStreamSynchronize(v.stream)); return 0; }
  return org_leave(c, v, who, in, o.perm, rec, stride, m, frag, frag_pos, v.distribute_lds);
}

extern "C" int pf_distribute_sorted(pf_ctx *c, double flast, const pf_subbox *sub, const unsigned int *map, const pf_product_layout *l, size_t capacity,
                                    void *frag, unsigned int *frag_pos, unsigned int *sorted_pos, int *indices, size_t *count) {
  return pf_distribute_sorted_impl("pf_distribute_sorted", c, flast, sub, map, nullptr, l, capacity, frag, frag_pos, sorted_pos, indices, count);
}

extern "C" int pf_organize(pf_ctx *c, const pf_product_layout *l, size_t count, void *frag, unsigned int *frag_pos, unsigned int *sorted_pos, int *indices) {
  const char *who = "pf_organize";
  if (!c) return pf_fail(0, "%s: null argument", who);
  PfCtxView v;
  pf_ctx_view(c, &v);
  if (!l || (count && (!frag || !frag_pos))) return pf_fail(v.rank, "%s: null argument", who);
  if (l->off_Fmax < 0) return pf_fail(v.rank, "%s: the layout names no Fmax to sort by (off_Fmax = %d)", who, l->off_Fmax);
  PfDistRecord rec;
  if (org_layout(v.rank, who, v.pb, l, &rec)) return 1;
  if (count > 0x7FFFFFFFull)
    return pf_fail(v.rank, "%s: %zu records: indices[] is int as in the reference, 2^31 - 1 records at most", who, count);
  if (!count) return 0;
  const size_t stride = l->stride;
  const bool index = sorted_pos || indices;
  PfScopedTimer pt(c, 1);
  PfOrgScratch o;
  memset(&o, 0, sizeof(o));
  OrgGuard guard{&o};
  if (org_alloc(&o, count, count, v.pb, false, index, count * stride))
    return pf_fail(v.rank, "%s: cannot allocate %zu bytes on the device for %zu records of %zu bytes (%zu for the records, the rest scratch of the sorts)",
                   who, org_scratch_bytes(count, count, v.pb, false, index, count * stride), count, stride, count * stride);
  if (pf_ctx_h2d(c, o.records, frag, count * stride) || pf_ctx_h2d(c, o.pos, frag_pos, count * sizeof(unsigned int))) return 1;
  PfOrgIn in;
  memset(&in, 0, sizeof(in));
  in.pb = v.pb; in.frag_pos = o.pos; in.aos = (const unsigned int *)o.records; in.aos_words = (unsigned int)(stride / 4); in.fmax_word = (unsigned int)(l->off_Fmax / 4);
  {
    PfScopedTimer kt(c, 0, (double)count * (v.pb + 64.0 + (v.pb + 4.0) * 2.0 * v.pb));
    if (org_order(in, count, &o, v.stream)) return pf_fail(v.rank, "%s: sort failed (out of memory?)", who);
  }
  if (index && org_index_leave(c, v, who, in, count, 32u, &o, sorted_pos, indices)) return 1;
  return org_leave(c, v, who, in, o.perm, rec, stride, count, frag, frag_pos, v.distribute_lds);
}

// context-free tap: the ordering on a caller's fp32 Fmax (an AoS source of one-word records) and frag_pos
extern "C" int pf_debug_organize(size_t count, const float *fmax, const unsigned int *frag_pos, unsigned int *order, unsigned int *sorted_pos, int *indices) {
  const char *who = "pf_debug_organize";
  if (count && (!fmax || !frag_pos)) return pf_fail(0, "%s: null argument", who);
  if (count > 0x7FFFFFFFull) return pf_fail(0, "%s: %zu records: indices[] is int as in the reference, 2^31 - 1 records at most", who, count);
  if (!count) return 0;
  PfOrgScratch o;
  memset(&o, 0, sizeof(o));
  OrgGuard guard{&o};
  if (org_alloc(&o, count, count, 4, false, true, count * sizeof(float))) return pf_fail(0, "%s: device allocation failed", who);
  PfOrgIn in;
  memset(&in, 0, sizeof(in));
  in.pb = 4; in.frag_pos = o.pos; in.aos = (const unsigned int *)o.records; in.aos_words = 1; in.fmax_word = 0;
  const size_t b4 = count * 4;
  int rc = 1;
  if (hipMemcpy(o.records, fmax, b4, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(o.pos, frag_pos, b4, hipMemcpyHostToDevice) == hipSuccess &&
      !org_order(in, count, &o, nullptr) && !org_index(in, count, 32u, &o, nullptr) && hipDeviceSynchronize() == hipSuccess &&
      (!order || hipMemcpy(order, o.perm, b4, hipMemcpyDeviceToHost) == hipSuccess) &&
      (!sorted_pos || hipMemcpy(sorted_pos, o.sorted_pos, b4, hipMemcpyDeviceToHost) == hipSuccess) &&
      (!indices || hipMemcpy(indices, o.indices, b4, hipMemcpyDeviceToHost) == hipSuccess)) rc = 0;
  return rc ? pf_fail(0, "%s: device pass failed", who) : 0;
}
