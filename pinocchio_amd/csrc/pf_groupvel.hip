// pf_groupvel.hip -- the group velocities of a redshift segment (recompute_group_velocities(), src/fragment.c:852-909) as a segmented
// sum on the device, and with them the whole step of src/fragment.c:416-427 for a host that keeps frag[] and groups[]: the records of
// the particles that are still loose (group_ID below first_group: 0 and FILAMENT) are refreshed as pf_refresh_velocities refreshes
// them, the grouped particles' 24 numbers never leave the device -- only 24 doubles per group come back.
//
//  k_groupvel_flag    one particle per lane, in the particles' own order: not found / loose / counted (found: pf_refresh_core.h, no
//                     good_particle test), as two ballots per wave and two counts per block of PF_REFRESH_BLOCK, and the largest
//                     counted ID (an integer atomic per wave).  The loose set then goes through k_refresh_scan and k_refresh_gather.
//  k_groupvel_keys    slot of a counted particle = the counted ones before it; its key (pf_groupvel_core.h) = group ID above the cell
//                     index of the slab.  The keys are sorted by rocPRIM's radix sort over the bits in use; no values travel with them.
//  k_groupvel_heads   head flags of the sorted keys in the same ballot / count form; their scan gives every group its output slot and
//                     the number of groups.
//  k_groupvel_reduce  wave64, PF_GV_TILE sorted keys per workgroup, PF_GV_ROUNDS units of 64 per wave.  A lane decodes its cell, issues
//                     its 24 column loads (consecutive lanes are z-neighbours of one group: the loads of a wave fall into runs),
//                     widens them to fp64, and the wave runs a segmented inclusive scan over the head flags (shuffles, log steps).
//                     Segments that begin and end in the unit go to their slot; the parts that reach or leave the unit go to LDS,
//                     where wave 0 walks the units in order (pf_gv_combine) -- complete groups to their slots, the first and last
//                     part of the tile to the carries.
//  k_groupvel_fold    a wave per tile that a group leaves: its L part plus the F parts of the tiles behind it, in tile order.
// No floating-point atomics: the tree of additions of a group depends on the sorted array alone, so the sums depend on the set of
// (group, cell, value) and on nothing else.
//
// Every index is in range by construction: positions below Lx Ly Lz and IDs in [0, 2^31) (or [0, ngroups]) are checked on the host
// while they are staged, before anything is launched; a cell address exists only for a cell of the slab; a slot is below the number
// of heads, which sized the output; a tile index is below the number of tiles, which sized the carries.
// Not tuned (profiles/groupvel_notes.md).
#include <hip/hip_runtime.h>

#include <stdlib.h>
#include <string.h>

#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "pf_internal.h"
#include "pf_map_core.h"
#include "pf_distribute_boxes.h"
#include "pf_refresh_core.h"
#include "pf_groupvel_core.h"

// ---------------------------------------------------------------------------------------------------------- kernels ----
__global__ void __launch_bounds__(PF_REFRESH_BLOCK)
    k_groupvel_flag(PfBackBox b, unsigned long long count, const unsigned int *__restrict__ pos, const int *__restrict__ gid, int first_group,
                    unsigned long long *__restrict__ lmasks, unsigned int *__restrict__ lcounts, unsigned long long *__restrict__ cmasks,
                    unsigned int *__restrict__ ccounts, unsigned int *maxid) {
  __shared__ unsigned int wl[PF_REFRESH_WAVES], wc[PF_REFRESH_WAVES];
  const unsigned long long i = (unsigned long long)blockIdx.x * PF_REFRESH_BLOCK + threadIdx.x;
  bool loose = false, counted = false;
  unsigned int id = 0;
  if (i < count) {
    size_t addr;
    if (pf_refresh_cell(b, pos[i], &addr)) {
      const int g = gid[i];
      counted = g >= first_group;
      loose = !counted;
      if (counted) id = (unsigned int)g;
    }
  }
  const unsigned long long ml = __ballot(loose), mc = __ballot(counted);
  for (int o = 32; o > 0; o >>= 1) { const unsigned int x = __shfl_xor(id, o, 64); id = x > id ? x : id; }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    lmasks[(unsigned long long)blockIdx.x * PF_REFRESH_WAVES + wave] = ml;
    cmasks[(unsigned long long)blockIdx.x * PF_REFRESH_WAVES + wave] = mc;
    wl[wave] = (unsigned int)__popcll(ml);
    wc[wave] = (unsigned int)__popcll(mc);
    if (mc) atomicMax(maxid, id);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int sl = 0, sc = 0;
    for (int w = 0; w < PF_REFRESH_WAVES; w++) { sl += wl[w]; sc += wc[w]; }
    lcounts[blockIdx.x] = sl;
    ccounts[blockIdx.x] = sc;
  }
}

__global__ void __launch_bounds__(PF_REFRESH_BLOCK)
    k_groupvel_keys(PfBackBox b, unsigned long long count, const unsigned int *__restrict__ pos, const int *__restrict__ gid,
                    const unsigned long long *__restrict__ cmasks, const unsigned long long *__restrict__ coffs, unsigned int cellbits,
                    unsigned long long *__restrict__ keys) {
  const unsigned long long i = (unsigned long long)blockIdx.x * PF_REFRESH_BLOCK + threadIdx.x;
  if (i >= count || !pf_refresh_found(cmasks, i)) return;
  const unsigned long long j = coffs[i / PF_REFRESH_BLOCK] + pf_refresh_rank_in_block(cmasks, i);
  size_t addr = 0;
  pf_refresh_cell(b, pos[i], &addr);
  keys[j] = pf_gv_key((unsigned int)gid[i], addr, cellbits);
}

__global__ void __launch_bounds__(PF_REFRESH_BLOCK)
    k_groupvel_heads(const unsigned long long *__restrict__ keys, unsigned long long m, unsigned int cellbits, unsigned long long *__restrict__ hmasks,
                     unsigned int *__restrict__ hcounts) {
  __shared__ unsigned int wh[PF_REFRESH_WAVES];
  const unsigned long long j = (unsigned long long)blockIdx.x * PF_REFRESH_BLOCK + threadIdx.x;
  const unsigned long long mh = __ballot(j < m && pf_gv_head(keys, j, cellbits));
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    hmasks[(unsigned long long)blockIdx.x * PF_REFRESH_WAVES + wave] = mh;
    wh[wave] = (unsigned int)__popcll(mh);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int s = 0;
    for (int w = 0; w < PF_REFRESH_WAVES; w++) s += wh[w];
    hcounts[blockIdx.x] = s;
  }
}

// column k (0..11 current, 12..23 prev) of the cell addr as a double; zero where the set or the LPT order is absent
template <int WPE>
__device__ __forceinline__ double groupvel_value(const PfRefreshCols &c, int k, size_t addr) {
  const int col = k < 12 ? k : k - 12;
  const unsigned int *set = k < 12 ? c.cur : c.prev;
  if (!set || col >= c.kmax) return 0.0;
  if (WPE == 2) return ((const double *)set)[(size_t)col * c.ncell + addr];
  return (double)((const float *)set)[(size_t)col * c.ncell + addr];
}

template <int WPE>
__global__ void __launch_bounds__(PF_GV_WAVES * PF_GV_WAVE)
    k_groupvel_reduce(const unsigned long long *__restrict__ keys, unsigned long long m, unsigned int cellbits, PfRefreshCols cols,
                      const unsigned long long *__restrict__ hmasks, const unsigned long long *__restrict__ hoffs, int *__restrict__ group, PfGvOut o) {
  __shared__ double sF[PF_GV_UNITS * PF_GV_NV], sL[PF_GV_UNITS * PF_GV_NV];
  __shared__ unsigned int sSlot[PF_GV_UNITS], sFlags[PF_GV_UNITS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long t = blockIdx.x;
  for (int r = 0; r < PF_GV_ROUNDS; r++) {
    const int u = wave * PF_GV_ROUNDS + r;
    const unsigned long long j = t * PF_GV_TILE + (unsigned long long)u * PF_GV_WAVE + lane;
    const bool valid = j < m;
    // a lane beyond the array is a segment of its own that writes nothing
    const unsigned long long key = valid ? keys[j] : 0ull;
    const bool head = valid ? pf_gv_head(keys, j, cellbits) : true, tail = valid ? pf_gv_tail(keys, m, j, cellbits) : true;
    double v[PF_GV_NV];
    if (valid) {
      const size_t addr = (size_t)pf_gv_cell(key, cellbits);
#pragma unroll
      for (int k = 0; k < 24; k++) v[k] = groupvel_value<WPE>(cols, k, addr);
      v[24] = 1.0;
    } else {
#pragma unroll
      for (int k = 0; k < PF_GV_NV; k++) v[k] = 0.0;
    }
    // the segmented inclusive scan: s = the lane the segment of this lane begins at in the unit (0 when it reaches the unit from before)
    const unsigned long long hm = __ballot(head);
    const unsigned long long upto = hm & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
    const bool began_here = upto != 0ull;
    const int s = began_here ? 63 - __clzll((long long)upto) : 0;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const bool take = lane - off >= s;
#pragma unroll
      for (int k = 0; k < PF_GV_NV; k++) { const double x = __shfl_up(v[k], off, 64); if (take) v[k] += x; }
    }
    unsigned int slot = 0;
    if (valid) {
      slot = (unsigned int)(hoffs[j / PF_REFRESH_BLOCK] + pf_refresh_rank_in_block(hmasks, j)) + (head ? 1u : 0u) - 1u;
      if (head) group[slot] = (int)pf_gv_group(key, cellbits);
    }
    const unsigned long long tm = __ballot(valid && tail), open63 = __ballot(valid && !tail) >> 63;
    const bool hasF = !(hm & 1ull);
    const unsigned long long before_first = hm ? ((1ull << __builtin_ctzll(hm)) - 1ull) : ~0ull;
    const bool Fcloses = hasF && (tm & before_first) != 0ull, hasL = open63 && hm != 0ull;
    if (valid && tail) {
      if (began_here) {
#pragma unroll
        for (int k = 0; k < PF_GV_NV; k++) pf_gv_emit(o, slot, k, v[k]);
      } else {
#pragma unroll
        for (int k = 0; k < PF_GV_NV; k++) sF[PF_GV_NV * u + k] = v[k];
      }
    }
    if (lane == 63 && valid && !tail) {
      if (began_here) {
#pragma unroll
        for (int k = 0; k < PF_GV_NV; k++) sL[PF_GV_NV * u + k] = v[k];
        sSlot[u] = slot;
      } else {
#pragma unroll
        for (int k = 0; k < PF_GV_NV; k++) sF[PF_GV_NV * u + k] = v[k];
      }
    }
    if (lane == 0) sFlags[u] = (hasF ? PF_GV_HAS_F : 0u) | (Fcloses ? PF_GV_F_CLOSES : 0u) | (hasL ? PF_GV_HAS_L : 0u);
  }
  __syncthreads();
  if (threadIdx.x < PF_GV_NV) pf_gv_combine(o, t, PF_GV_UNITS, sF, sL, sSlot, sFlags, (int)threadIdx.x);
}

__global__ void __launch_bounds__(PF_GV_WAVES * PF_GV_WAVE) k_groupvel_fold(unsigned long long ntiles, PfGvOut o) {
  const unsigned long long t = (unsigned long long)blockIdx.x * PF_GV_WAVES + (threadIdx.x >> 6);
  const int k = threadIdx.x & 63;
  if (t < ntiles && k < PF_GV_NV) pf_gv_fold(o, t, ntiles, k);
}

// ------------------------------------------------------------------------------------------------------------ launches ----
#define GVHIP(task, who, call)                                                                                         \
  do {                                                                                                                 \
    hipError_t e__ = (call);                                                                                           \
    if (e__ != hipSuccess) return pf_fail(task, "%s: %s failed: %s", who, #call, hipGetErrorString(e__));             \
  } while (0)

// what a call holds on the device beside the columns and the scratch of the refresh
struct PfGvScratch {
  int *gid; unsigned long long *cmasks, *coffs; unsigned int *ccounts, *maxid;
  unsigned long long *keys[2]; void *tmp; unsigned long long *hmasks, *hoffs; unsigned int *hcounts;
  int *group; unsigned int *npart; double *sum, *carryF, *carryL; unsigned int *slotL, *tflags;
};
static void gv_release(PfGvScratch *g) {
  hipFree(g->gid); hipFree(g->cmasks); hipFree(g->coffs); hipFree(g->ccounts); hipFree(g->maxid); hipFree(g->keys[0]); hipFree(g->keys[1]); hipFree(g->tmp);
  hipFree(g->hmasks); hipFree(g->hoffs); hipFree(g->hcounts); hipFree(g->group); hipFree(g->npart); hipFree(g->sum); hipFree(g->carryF); hipFree(g->carryL);
  hipFree(g->slotL); hipFree(g->tflags);
  memset(g, 0, sizeof(*g));
}
struct GvGuard { PfGvScratch *g; PfRefreshScratch *s; ~GvGuard() { gv_release(g); pf_refresh_release(s); } };

static size_t gv_in_bytes(size_t count) {
  const size_t nb = pf_refresh_blocks(count);
  return count * 4 + nb * (PF_REFRESH_WAVES * 8 + 4) + (nb + 1) * 8 + 4;
}
static int gv_alloc_in(PfGvScratch *g, size_t count) {
  const size_t nb = pf_refresh_blocks(count);
  const bool ok = hipMalloc((void **)&g->gid, count * 4) == hipSuccess && hipMalloc((void **)&g->cmasks, nb * PF_REFRESH_WAVES * 8) == hipSuccess &&
                  hipMalloc((void **)&g->ccounts, nb * 4) == hipSuccess && hipMalloc((void **)&g->coffs, (nb + 1) * 8) == hipSuccess &&
                  hipMalloc((void **)&g->maxid, 4) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); return 1; }
  return 0;
}
static size_t gv_tiles(size_t m) { return (m + PF_GV_TILE - 1) / PF_GV_TILE; }
// the keys, their copy for the sort, the head flags and the carries of m counted particles (rocPRIM's own scratch comes on top)
static size_t gv_sort_bytes(size_t m) {
  const size_t nb = pf_refresh_blocks(m), nt = gv_tiles(m);
  return m * 16 + nb * (PF_REFRESH_WAVES * 8 + 4) + (nb + 1) * 8 + nt * (2 * PF_GV_NV * 8 + 8);
}
static size_t gv_out_bytes(size_t groups) { return groups * (4 + 4 + 24 * 8); }

// flag + the two scans, behind positions and IDs that lie on the device; the three numbers after a synchronisation of the stream
static int gv_select(const char *who, int task, const PfBackBox &b, size_t count, int first_group, const PfRefreshScratch &s, const PfGvScratch &g,
                     hipStream_t st, unsigned long long *loose, unsigned long long *counted, unsigned int *maxid) {
  const size_t nb = pf_refresh_blocks(count);
  GVHIP(task, who, hipMemsetAsync(g.maxid, 0, 4, st));
  hipLaunchKernelGGL(k_groupvel_flag, dim3((unsigned int)nb), dim3(PF_REFRESH_BLOCK), 0, st, b, (unsigned long long)count, s.pos, g.gid, first_group, s.masks,
                     s.counts, g.cmasks, g.ccounts, g.maxid);
  if (hipGetLastError() != hipSuccess || pf_refresh_scan(s.counts, nb, s.offs, st) || pf_refresh_scan(g.ccounts, nb, g.coffs, st))
    return pf_fail(task, "%s: launch failed", who);
  GVHIP(task, who, hipMemcpyAsync(loose, s.offs + nb, 8, hipMemcpyDeviceToHost, st));
  GVHIP(task, who, hipMemcpyAsync(counted, g.coffs + nb, 8, hipMemcpyDeviceToHost, st));
  GVHIP(task, who, hipMemcpyAsync(maxid, g.maxid, 4, hipMemcpyDeviceToHost, st));
  GVHIP(task, who, hipStreamSynchronize(st));
  return 0;
}

// PF_GROUPVEL_TIMES=1: the device time of the last call's stages -- keys + sort, head flags + scan, reduce + fold -- between events on
// its stream, at the price of one more synchronisation (profiles/tools/groupvel_time.py; pf_debug_groupvel_times)
static double gv_last_ms[3] = {0.0, 0.0, 0.0};
struct GvStage {
  hipEvent_t a, b; hipStream_t st; int which; bool on;
  GvStage(bool on_, int which_, hipStream_t st_) : a(nullptr), b(nullptr), st(st_), which(which_), on(on_) {
    if (on) on = hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess && hipEventRecord(a, st) == hipSuccess;
  }
  void end() {
    float ms = 0.0f;
    if (on && hipEventRecord(b, st) == hipSuccess && hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&ms, a, b) == hipSuccess) gv_last_ms[which] = ms;
    on = false;
  }
  ~GvStage() { end(); if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); }
};
extern "C" int pf_debug_groupvel_times(double *ms3) {
  if (!ms3) return 1;
  for (int i = 0; i < 3; i++) ms3[i] = gv_last_ms[i];
  return 0;
}

// the sums of the m counted particles into g->group / npart / sum; *groups after a synchronisation (it sizes the output)
static int gv_sums(const char *who, int task, int pb, const PfBackBox &b, size_t count, size_t ncell, const PfRefreshScratch &s, PfGvScratch *g,
                   const PfRefreshCols &cols, size_t m, unsigned int maxid, hipStream_t st, unsigned long long *groups) {
  *groups = 0;
  if (!m) return 0;
  const size_t nb = pf_refresh_blocks(count), nbm = pf_refresh_blocks(m), nt = gv_tiles(m);
  const unsigned int cellbits = pf_gv_bits(ncell - 1), endbit = cellbits + pf_gv_bits(maxid);
  bool ok = hipMalloc((void **)&g->keys[0], m * 8) == hipSuccess && hipMalloc((void **)&g->keys[1], m * 8) == hipSuccess &&
            hipMalloc((void **)&g->hmasks, nbm * PF_REFRESH_WAVES * 8) == hipSuccess && hipMalloc((void **)&g->hcounts, nbm * 4) == hipSuccess &&
            hipMalloc((void **)&g->hoffs, (nbm + 1) * 8) == hipSuccess && hipMalloc((void **)&g->carryF, nt * PF_GV_NV * 8) == hipSuccess &&
            hipMalloc((void **)&g->carryL, nt * PF_GV_NV * 8) == hipSuccess && hipMalloc((void **)&g->slotL, nt * 4) == hipSuccess &&
            hipMalloc((void **)&g->tflags, nt * 4) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); return pf_fail(task, "%s: cannot allocate %zu bytes of scratch on the device for %zu grouped particles", who, gv_sort_bytes(m), m); }
  const char *env = getenv("PF_GROUPVEL_TIMES");
  const bool times = env && atoi(env) != 0;
  GvStage sort_stage(times, 0, st);
  hipLaunchKernelGGL(k_groupvel_keys, dim3((unsigned int)nb), dim3(PF_REFRESH_BLOCK), 0, st, b, (unsigned long long)count, s.pos, g->gid, g->cmasks, g->coffs,
                     cellbits, g->keys[0]);
  if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  const unsigned long long *sorted = g->keys[0];
  if (endbit && m > 1) {
    rocprim::double_buffer<unsigned long long> db(g->keys[0], g->keys[1]);
    size_t bytes = 0;
    GVHIP(task, who, rocprim::radix_sort_keys(nullptr, bytes, db, m, 0u, endbit, st));
    if (!bytes) bytes = 8;
    if (hipMalloc(&g->tmp, bytes) != hipSuccess) { (void)hipGetLastError(); return pf_fail(task, "%s: cannot allocate %zu bytes of scratch on the device for the sort of %zu keys", who, bytes, m); }
    GVHIP(task, who, rocprim::radix_sort_keys(g->tmp, bytes, db, m, 0u, endbit, st));
    sorted = db.current();
  }
  sort_stage.end();
  GvStage head_stage(times, 1, st);
  hipLaunchKernelGGL(k_groupvel_heads, dim3((unsigned int)nbm), dim3(PF_REFRESH_BLOCK), 0, st, sorted, (unsigned long long)m, cellbits, g->hmasks, g->hcounts);
  if (hipGetLastError() != hipSuccess || pf_refresh_scan(g->hcounts, nbm, g->hoffs, st)) return pf_fail(task, "%s: launch failed", who);
  unsigned long long G = 0;
  GVHIP(task, who, hipMemcpyAsync(&G, g->hoffs + nbm, 8, hipMemcpyDeviceToHost, st));
  GVHIP(task, who, hipStreamSynchronize(st));
  head_stage.end();
  ok = hipMalloc((void **)&g->group, G * 4) == hipSuccess && hipMalloc((void **)&g->npart, G * 4) == hipSuccess && hipMalloc((void **)&g->sum, G * 24 * 8) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); return pf_fail(task, "%s: cannot allocate %zu bytes on the device for the sums of %llu groups", who, gv_out_bytes((size_t)G), G); }
  PfGvOut o;
  o.sum = g->sum; o.npart = g->npart; o.carryF = g->carryF; o.carryL = g->carryL; o.slotL = g->slotL; o.tflags = g->tflags;
  const dim3 block(PF_GV_WAVES * PF_GV_WAVE);
  GvStage reduce_stage(times, 2, st);
  if (pb == 8) hipLaunchKernelGGL(k_groupvel_reduce<2>, dim3((unsigned int)nt), block, 0, st, sorted, (unsigned long long)m, cellbits, cols, g->hmasks, g->hoffs, g->group, o);
  else hipLaunchKernelGGL(k_groupvel_reduce<1>, dim3((unsigned int)nt), block, 0, st, sorted, (unsigned long long)m, cellbits, cols, g->hmasks, g->hoffs, g->group, o);
  hipLaunchKernelGGL(k_groupvel_fold, dim3((unsigned int)((nt + PF_GV_WAVES - 1) / PF_GV_WAVES)), block, 0, st, (unsigned long long)nt, o);
  if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  reduce_stage.end();
  *groups = G;
  return 0;
}

// the first ID that is negative or above `last` (the staging threads know of one such entry, not of the first)
static size_t gv_first_bad_id(const int *group_id, size_t stride, size_t upto, long long last) {
  for (size_t i = 0; i < upto; i++) {
    const int g = *(const int *)((const char *)group_id + i * stride);
    if (g < 0 || g > last) return i;
  }
  return upto;
}
static int gv_bad_id(const char *who, int rank, const int *group_id, size_t stride, size_t bad, long long last) {
  bad = gv_first_bad_id(group_id, stride, bad, last);
  const int g = *(const int *)((const char *)group_id + bad * stride);
  if (g < 0) return pf_fail(rank, "%s: group_id[%zu] = %d is negative", who, bad, g);
  return pf_fail(rank, "%s: group_id[%zu] = %d lies above the %lld groups", who, bad, g, last);
}

// what both entry points with a context do up to the sums: arguments, box, upload and checks, the three classes, the sums on the
// device.  last_id: the largest ID that is legal
static int gv_run(pf_ctx *c, const PfCtxView &v, const char *who, const pf_peak_region *box, size_t count, const unsigned int *frag_pos, const int *order,
                  const int *group_id, size_t group_stride, int first_group, long long last_id, bool want_sums, PfBackBox *b, PfRefreshCols *cols,
                  PfRefreshScratch *s, PfGvScratch *g, unsigned long long *loose, unsigned long long *counted, unsigned long long *groups) {
  *loose = *counted = *groups = 0;
  if (!box || (count && (!frag_pos || !group_id))) return pf_fail(v.rank, "%s: null argument", who);
  if (!v.products_init) return pf_fail(v.rank, "%s: products not computed", who);
  if (count > 0x7FFFFFFFull) return pf_fail(v.rank, "%s: %zu particles: indices[] is int as in the reference, 2^31 - 1 particles at most", who, count);
  if (group_stride % 4) return pf_fail(v.rank, "%s: a stride of %zu bytes is no multiple of the 4 bytes of a group_ID", who, group_stride);
  if ((unsigned long long)v.ncell > 0x100000000ull) return pf_fail(v.rank, "%s: a slab of %zu cells: a key holds a cell index below 2^32", who, v.ncell);
  unsigned long long cells = 1;
  if (pf_refresh_box(who, v.rank, v.n, v.rank * v.nxl, v.nxl, box, b, &cells)) return 1;
  if (!count) return 0;
  const void *prev = nullptr; int shifts = 0, lpt_order = 3;
  pf_ctx_prev_view(c, &prev, &shifts, &lpt_order);
  if (pf_ctx_velocities_ready(c)) return 1;
  PfScopedTimer pt(c, 1);
  if (pf_refresh_alloc_in(s, count, order != nullptr) || gv_alloc_in(g, count))
    return pf_fail(v.rank, "%s: cannot allocate %zu bytes of scratch on the device for %zu particles", who, pf_refresh_in_bytes(count, order != nullptr) + gv_in_bytes(count), count);
  size_t bad = 0;
  int rc = pf_ctx_h2d_packed(c, s->pos, frag_pos, count, 4, 4, cells, &bad);
  if (rc == 2) {
    bad = pf_refresh_first_bad(frag_pos, bad, cells);
    return pf_fail(v.rank, "%s: frag_pos[%zu] = %u lies outside the %llu cells of the box", who, bad, frag_pos[bad], cells);
  }
  if (rc) return 1;
  rc = pf_ctx_h2d_packed(c, g->gid, group_id, count, 4, group_stride, (unsigned long long)last_id + 1ull, &bad);   // (a negative ID is a large unsigned one)
  if (rc == 2) return gv_bad_id(who, v.rank, group_id, group_stride, bad, last_id);
  if (rc) return 1;
  if (order) {
    rc = pf_ctx_h2d_packed(c, s->order, order, count, 4, 4, (unsigned long long)count, &bad);
    if (rc == 2) {
      bad = pf_refresh_first_bad((const unsigned int *)order, bad, count);
      return pf_fail(v.rank, "%s: order[%zu] = %d is no index of the %zu particles", who, bad, order[bad], count);
    }
    if (rc) return 1;
  }
  unsigned int maxid = 0;
  {
    PfScopedTimer kt(c, 0, (double)count * 8.0 + (double)pf_refresh_blocks(count) * 112.0, v.stream);
    if (gv_select(who, v.rank, *b, count, first_group, *s, *g, v.stream, loose, counted, &maxid)) return 1;
  }
  cols->cur = (const unsigned int *)v.vel12; cols->prev = (const unsigned int *)prev; cols->ncell = v.ncell; cols->kmax = lpt_order >= 3 ? 12 : lpt_order == 2 ? 6 : 3;
  if (!want_sums) return 0;
  PfScopedTimer kt(c, 0, (double)*counted * (8.0 + 32.0 + 8.0 + 24.0 * v.pb), v.stream);
  return gv_sums(who, v.rank, v.pb, *b, count, v.ncell, *s, g, *cols, (size_t)*counted, maxid, v.stream, groups);
}

// -------------------------------------------------------------------------------------------------------- entry points ----
extern "C" int pf_group_velocity_sums(pf_ctx *c, const pf_peak_region *box, size_t count, const unsigned int *frag_pos, const int *group_id, size_t group_stride,
                                      int first_group, size_t capacity, int *group, unsigned int *npart, double *sum24, size_t *groups_found,
                                      size_t *particles_found) {
  const char *who = "pf_group_velocity_sums";
  if (!c) return pf_fail(0, "%s: null argument", who);
  PfCtxView v;
  pf_ctx_view(c, &v);
  PfRefreshScratch s;
  PfGvScratch g;
  memset(&s, 0, sizeof(s));
  memset(&g, 0, sizeof(g));
  GvGuard guard{&g, &s};
  PfBackBox b;
  PfRefreshCols cols;
  unsigned long long loose = 0, counted = 0, G = 0;
  if (gv_run(c, v, who, box, count, frag_pos, nullptr, group_id, group_stride, first_group, 0x7FFFFFFFll, true, &b, &cols, &s, &g, &loose, &counted, &G)) return 1;
  const size_t m = G < capacity ? (size_t)G : capacity;
  if (m && group && pf_ctx_d2h(c, group, g.group, m * 4)) return 1;
  if (m && npart && pf_ctx_d2h(c, npart, g.npart, m * 4)) return 1;
  if (m && sum24 && pf_ctx_d2h(c, sum24, g.sum, m * 24 * 8)) return 1;
  if (groups_found) *groups_found = (size_t)G;
  if (particles_found) *particles_found = (size_t)counted;
  return 0;
}

// the fields of a group record the means go to: slot s as in pf_refresh.hip (0..3 current, 4..7 prev), three PRODFLOATs each
struct PfGvFields { int nf; long off[8]; int slot[8]; };
static int gv_group_fields(const char *who, int rank, int pb, const pf_group_layout *gl, PfGvFields *f) {
  f->nf = 0;
  const char *rule = "%s: bad group layout: stride %zu and the offsets must be multiples of four, fields inside the record";
  if (gl->stride < 4 || gl->stride % 4) return pf_fail(rank, rule, who, gl->stride);
  const long ov[8] = {gl->off_Vel, gl->off_Vel_2LPT, gl->off_Vel_3LPT_1, gl->off_Vel_3LPT_2, gl->off_Vel_prev, gl->off_Vel_2LPT_prev, gl->off_Vel_3LPT_1_prev,
                      gl->off_Vel_3LPT_2_prev};
  const long len = 3 * pb;
  if (gl->off_Mass >= 0 && (gl->off_Mass % 4 || (size_t)gl->off_Mass + 4 > gl->stride)) return pf_fail(rank, rule, who, gl->stride);
  for (int s = 0; s < 8; s++) {
    if (ov[s] < 0) continue;
    if (ov[s] % 4 || (size_t)ov[s] + (size_t)len > gl->stride) return pf_fail(rank, rule, who, gl->stride);
    if (gl->off_Mass >= 0 && ov[s] < gl->off_Mass + 4 && gl->off_Mass < ov[s] + len)
      return pf_fail(rank, "%s: fields of the group layout overlap (Mass at byte %ld and a field at byte %ld)", who, gl->off_Mass, ov[s]);
    for (int a = 0; a < f->nf; a++)
      if (ov[s] < f->off[a] + len && f->off[a] < ov[s] + len)
        return pf_fail(rank, "%s: fields of the group layout overlap (at byte %ld and at byte %ld)", who, f->off[a], ov[s]);
    f->off[f->nf] = ov[s]; f->slot[f->nf] = s; f->nf++;
  }
  return 0;
}

extern "C" int pf_refresh_segment(pf_ctx *c, const pf_peak_region *box, size_t count, const unsigned int *frag_pos, const int *order, const int *group_id,
                                  size_t group_stride, int first_group, void *frag, const pf_product_layout *layout, const pf_prev_layout *prev, void *groups,
                                  size_t ngroups, const pf_group_layout *gl, size_t *loose_out, size_t *grouped_out, size_t *mass_mismatch) {
  const char *who = "pf_refresh_segment";
  if (!c) return pf_fail(0, "%s: null argument", who);
  PfCtxView v;
  pf_ctx_view(c, &v);
  if ((frag && !layout) || (groups && !gl)) return pf_fail(v.rank, "%s: null argument", who);
  if (ngroups > 0x7FFFFFFFull) return pf_fail(v.rank, "%s: %zu groups: a group_ID is an int", who, ngroups);
  const void *pcols = nullptr; int shifts = 0, lpt_order = 3;
  pf_ctx_prev_view(c, &pcols, &shifts, &lpt_order);
  PfRefreshFields f;
  f.nf = 0;
  if (frag && pf_refresh_fields(who, v.rank, v.pb, shifts, layout, prev, &f)) return 1;
  PfGvFields gf;
  gf.nf = 0;
  if (groups && gv_group_fields(who, v.rank, v.pb, gl, &gf)) return 1;
  PfRefreshScratch s;
  PfGvScratch g;
  memset(&s, 0, sizeof(s));
  memset(&g, 0, sizeof(g));
  GvGuard guard{&g, &s};
  PfBackBox b;
  PfRefreshCols cols;
  unsigned long long loose = 0, counted = 0, G = 0;
  if (gv_run(c, v, who, box, count, frag_pos, order, group_id, group_stride, first_group, (long long)ngroups, groups != nullptr, &b, &cols, &s, &g, &loose, &counted, &G))
    return 1;
  if (loose_out) *loose_out = (size_t)loose;
  if (grouped_out) *grouped_out = (size_t)counted;
  if (mass_mismatch) *mass_mismatch = 0;
  // the group half first: its transfer is small, and the device is free for the gather of the loose half meanwhile
  std::vector<int> hgroup;
  std::vector<unsigned int> hnpart;
  std::vector<double> hsum;
  if (groups && G) {
    hgroup.resize((size_t)G); hnpart.resize((size_t)G); hsum.resize((size_t)G * 24);
    if (pf_ctx_d2h(c, hgroup.data(), g.group, (size_t)G * 4) || pf_ctx_d2h(c, hnpart.data(), g.npart, (size_t)G * 4) || pf_ctx_d2h(c, hsum.data(), g.sum, (size_t)G * 24 * 8))
      return 1;
  }
  // the loose half: the gather of pf_refresh.hip on the loose flags, and its scatter into the records
  if (frag && f.nf && loose) {
    const size_t m = (size_t)loose;
    if (pf_refresh_alloc_out(&s, m, v.pb, true, true))
      return pf_fail(v.rank, "%s: cannot allocate %zu bytes on the device for the velocities of %zu particles", who, m * (4 + 24 * (size_t)v.pb), m);
    if (order) {   // an order that is no permutation omits particles (pf_refresh.hip)
      GVHIP(v.rank, who, hipMemsetAsync(s.index, 0xFF, m * 4, v.stream));
      GVHIP(v.rank, who, hipMemsetAsync(s.vel, 0, m * 24 * (size_t)v.pb, v.stream));
    }
    {
      PfScopedTimer kt(c, 0, (double)count * (order ? 24.0 : 20.0) + (double)m * (4.0 + 48.0 * v.pb), v.stream);
      if (pf_refresh_gather(v.pb, b, count, s, cols, m, v.stream)) return pf_fail(v.rank, "%s: launch failed", who);
    }
    if (pf_refresh_to_records(c, v, who, s, m, count, frag, layout->stride, f)) return 1;
  }
  if (groups && G) {
    size_t mismatch = 0;
    char *rec = (char *)groups;
    for (size_t j = 0; j < (size_t)G; j++) {
      char *dst = rec + (size_t)hgroup[j] * gl->stride;
      if (gl->off_Mass >= 0) {
        int mass;
        memcpy(&mass, dst + gl->off_Mass, 4);
        if ((long long)mass != (long long)hnpart[j]) mismatch++;
      }
      const double np = (double)hnpart[j];
      for (int u = 0; u < gf.nf; u++)
        for (int e = 0; e < 3; e++) {
          const double mean = hsum[24 * j + 3 * gf.slot[u] + e] / np;
          if (v.pb == 8) memcpy(dst + gf.off[u] + 8 * e, &mean, 8);
          else { const float fm = (float)mean; memcpy(dst + gf.off[u] + 4 * e, &fm, 4); }
        }
    }
    if (mass_mismatch) *mass_mismatch = mismatch;
  }
  return 0;
}

// test tap without a context: the same kernels on a caller's columns, on the default stream
extern "C" int pf_debug_group_velocity_sums(int n, int x0, int nxl, int pb, const void *cols24, const pf_peak_region *box, size_t count,
                                            const unsigned int *frag_pos, const int *group_id, int first_group, int *group, unsigned int *npart,
                                            double *sum24, size_t *groups_found, size_t *particles_found) {
  const char *who = "pf_debug_group_velocity_sums";
  if (!box || !cols24 || (count && (!frag_pos || !group_id))) return pf_fail(0, "%s: null argument", who);
  if (pb != 4 && pb != 8) return pf_fail(0, "%s: a PRODFLOAT of %d bytes (4 or 8)", who, pb);
  if (n < 1 || n > 2048 || x0 < 0 || nxl < 1 || x0 + nxl > n) return pf_fail(0, "%s: planes %d .. %d of a box of %d^3 cells", who, x0, x0 + nxl - 1, n);
  if (count > 0x7FFFFFFFull) return pf_fail(0, "%s: %zu particles: indices[] is int as in the reference, 2^31 - 1 particles at most", who, count);
  const size_t ncell = (size_t)nxl * n * n;
  if ((unsigned long long)ncell > 0x100000000ull) return pf_fail(0, "%s: a slab of %zu cells: a key holds a cell index below 2^32", who, ncell);
  PfBackBox b;
  unsigned long long cells = 1;
  if (pf_refresh_box(who, 0, n, x0, nxl, box, &b, &cells)) return 1;
  for (size_t i = 0; i < count; i++)
    if (frag_pos[i] >= cells) return pf_fail(0, "%s: frag_pos[%zu] = %u lies outside the %llu cells of the box", who, i, frag_pos[i], cells);
  for (size_t i = 0; i < count; i++)
    if (group_id[i] < 0) return pf_fail(0, "%s: group_id[%zu] = %d is negative", who, i, group_id[i]);
  if (groups_found) *groups_found = 0;
  if (particles_found) *particles_found = 0;
  if (!count) return 0;
  const size_t colbytes = 24 * ncell * (size_t)pb;
  void *dcols = nullptr;
  PfRefreshScratch s;
  PfGvScratch g;
  memset(&s, 0, sizeof(s));
  memset(&g, 0, sizeof(g));
  struct Columns { void **p; ~Columns() { hipFree(*p); } } columns{&dcols};
  GvGuard guard{&g, &s};
  if (hipMalloc(&dcols, colbytes) != hipSuccess || pf_refresh_alloc_in(&s, count, false) || gv_alloc_in(&g, count)) {
    (void)hipGetLastError();
    return pf_fail(0, "%s: cannot allocate %zu bytes on the device", who, colbytes + pf_refresh_in_bytes(count, false) + gv_in_bytes(count));
  }
  GVHIP(0, who, hipMemcpy(dcols, cols24, colbytes, hipMemcpyHostToDevice));
  GVHIP(0, who, hipMemcpy(s.pos, frag_pos, count * 4, hipMemcpyHostToDevice));
  GVHIP(0, who, hipMemcpy(g.gid, group_id, count * 4, hipMemcpyHostToDevice));
  unsigned long long loose = 0, counted = 0, G = 0;
  unsigned int maxid = 0;
  if (gv_select(who, 0, b, count, first_group, s, g, nullptr, &loose, &counted, &maxid)) return 1;
  PfRefreshCols cols;
  cols.cur = (const unsigned int *)dcols; cols.prev = cols.cur + 12 * ncell * (size_t)(pb / 4); cols.ncell = ncell; cols.kmax = 12;
  if (gv_sums(who, 0, pb, b, count, ncell, s, &g, cols, (size_t)counted, maxid, nullptr, &G)) return 1;
  if (G) {
    GVHIP(0, who, hipDeviceSynchronize());
    if (group) GVHIP(0, who, hipMemcpy(group, g.group, (size_t)G * 4, hipMemcpyDeviceToHost));
    if (npart) GVHIP(0, who, hipMemcpy(npart, g.npart, (size_t)G * 4, hipMemcpyDeviceToHost));
    if (sum24) GVHIP(0, who, hipMemcpy(sum24, g.sum, (size_t)G * 24 * 8, hipMemcpyDeviceToHost));
  }
  if (groups_found) *groups_found = (size_t)G;
  if (particles_found) *particles_found = (size_t)counted;
  return 0;
}
