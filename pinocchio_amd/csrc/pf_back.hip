// pf_back.hip -- distribute_back() (src/distribute.c:703-946): zacc and group_ID of the good particles of a sub-box, as build_groups()
// left them in frag[], back into the two per-cell columns of this rank's FFT slab that write_timeless_snapshot()
// (src/write_snapshot.c:859-905) reads for its ZACC and GRUP blocks.
//
//  k_back_fill      zacc := -1, group_ID := 0 (src/allocations.c:519-524), one cell per lane.
//  k_back_scatter   one particle per lane.  With a box: keep_data_back() (:806-834) / the loop of send_data_back() (:859-896) -- the
//                   cell arithmetic of pf_back_core.h decides whether this slab takes the particle and where --; without one:
//                   recv_data_back() (:935-939), the position in the slab is given.  Two scattered stores per particle that is taken
//                   (the value of the product precision, the int), nothing else is written.  The count of what was stored: a
//                   wavefront reduction and one 64-bit atomic per wavefront, an integer sum that is the same whatever the schedule.
//
// Every index is in range by construction: positions are below Lx Ly Lz, or below the cells of the slab for the direct form -- checked
// on the host while they are staged, before anything is launched --, and pf_back_cell gives an address only for a cell of the slab.
// Not tuned: 12 bytes per particle cross the host link for two 4-byte stores (profiles/back_notes.md).
#include <hip/hip_runtime.h>

#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pf_internal.h"
#include "pf_map_core.h"
#include "pf_distribute_boxes.h"
#include "pf_back_core.h"

#define PF_BACK_BLOCK 256

// ---------------------------------------------------------------------------------------------------------- kernels ----
template <typename T>
__global__ void __launch_bounds__(PF_BACK_BLOCK) k_back_fill(size_t ncell, T *__restrict__ zacc, int *__restrict__ group) {
  const size_t i = (size_t)blockIdx.x * PF_BACK_BLOCK + threadIdx.x;
  if (i >= ncell) return;
  zacc[i] = (T)-1;
  group[i] = 0;
}

// pos null: particle iz lies at position iz (CLASSIC_FRAGMENTATION, :808-809).  direct: pos[iz] is the cell of the slab itself
template <typename T>
__global__ void __launch_bounds__(PF_BACK_BLOCK) k_back_scatter(PfBackBox b, int direct, unsigned long long count, const unsigned int *__restrict__ pos,
                                                                 const T *__restrict__ zacc, const int *__restrict__ gid, T *__restrict__ zcol,
                                                                 int *__restrict__ gcol, unsigned long long *__restrict__ stored) {
  const unsigned long long iz = (unsigned long long)blockIdx.x * PF_BACK_BLOCK + threadIdx.x;
  unsigned long long taken = 0;
  if (iz < count) {
    const unsigned int p = pos ? pos[iz] : (unsigned int)iz;
    size_t addr = p;
    if (direct || pf_back_cell(b, p, &addr)) {
      zcol[addr] = zacc[iz];
      gcol[addr] = gid[iz];
      taken = 1;
    }
  }
  if (stored) {
    for (int o = 32; o > 0; o >>= 1) taken += __shfl_down(taken, o, 64);
    if ((threadIdx.x & 63) == 0 && taken) atomicAdd(stored, taken);
  }
}

// ------------------------------------------------------------------------------------------------------------ launches ----
static unsigned int back_blocks(unsigned long long threads) { return (unsigned int)((threads + PF_BACK_BLOCK - 1) / PF_BACK_BLOCK); }

int pf_launch_back_fill(int pb, void *zacc, int *group, size_t ncell, hipStream_t st) {
  if (!ncell) return 0;
  const dim3 grid(back_blocks(ncell)), block(PF_BACK_BLOCK);
  if (pb == 8) hipLaunchKernelGGL(k_back_fill<double>, grid, block, 0, st, ncell, (double *)zacc, group);
  else hipLaunchKernelGGL(k_back_fill<float>, grid, block, 0, st, ncell, (float *)zacc, group);
  return hipGetLastError() != hipSuccess;
}

// 0 < count <= 2^32
static int back_launch_scatter(int pb, const PfBackBox &b, bool direct, unsigned long long count, const unsigned int *pos, const void *zacc, const int *gid,
                               void *zcol, int *gcol, unsigned long long *stored, hipStream_t st) {
  const dim3 grid(back_blocks(count)), block(PF_BACK_BLOCK);
  if (pb == 8) hipLaunchKernelGGL(k_back_scatter<double>, grid, block, 0, st, b, direct ? 1 : 0, count, pos, (const double *)zacc, gid, (double *)zcol, gcol, stored);
  else hipLaunchKernelGGL(k_back_scatter<float>, grid, block, 0, st, b, direct ? 1 : 0, count, pos, (const float *)zacc, gid, (float *)zcol, gcol, stored);
  return hipGetLastError() != hipSuccess;
}

// what a call holds on the device beside the columns
struct PfBackScratch { unsigned int *pos; void *zacc; int *gid; unsigned long long *stored; };
static void back_release(PfBackScratch *s) {
  hipFree(s->pos); hipFree(s->zacc); hipFree(s->gid); hipFree(s->stored);
  memset(s, 0, sizeof(*s));
}
struct BackGuard { PfBackScratch *s; ~BackGuard() { back_release(s); } };
static size_t back_scratch_bytes(size_t count, int pb, bool with_pos) { return count * (size_t)((with_pos ? 4 : 0) + pb + 4) + 8; }
static int back_alloc(PfBackScratch *s, size_t count, int pb, bool with_pos) {
  bool ok = hipMalloc(&s->zacc, count * (size_t)pb) == hipSuccess && hipMalloc((void **)&s->gid, count * 4) == hipSuccess &&
            hipMalloc((void **)&s->stored, sizeof(unsigned long long)) == hipSuccess;
  if (ok && with_pos) ok = hipMalloc((void **)&s->pos, count * 4) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); back_release(s); return 1; }
  return 0;
}

#define BACKHIP(task, who, call)                                                                                       \
  do {                                                                                                                 \
    hipError_t e__ = (call);                                                                                           \
    if (e__ != hipSuccess) return pf_fail(task, "%s: %s failed: %s", who, #call, hipGetErrorString(e__));             \
  } while (0)

// the box of a call: checked as pf_map_create checks its box, the start reduced as pf_distribute reduces it
static int back_box(const char *who, int rank, int n, int x0, int nxl, const pf_peak_region *box, PfBackBox *b, unsigned long long *cells) {
  PfMapBox mb;
  if (pf_map_box_check(who, rank, n, box, &mb, cells)) return 1;
  for (int d = 0; d < 3; d++) { b->box.len[d] = mb.len[d]; b->box.pbc[d] = mb.pbc[d]; b->box.safe[d] = box->safe[d]; b->start[d] = pf_dist_wrap(box->start[d], n); }
  b->n = n; b->x0 = x0; b->nxl = nxl;
  return 0;
}
// what every entry point refuses before it touches the device
static int back_args(const char *who, int rank, int pb, size_t count, const void *zacc, size_t zacc_stride, const int *group_id, size_t group_stride) {
  if (count && (!zacc || !group_id)) return pf_fail(rank, "%s: null argument", who);
  if (count > (1ull << 32)) return pf_fail(rank, "%s: %zu entries: positions are 32-bit as in the reference, 2^32 entries at most", who, count);
  if (zacc_stride % (size_t)pb) return pf_fail(rank, "%s: a stride of %zu bytes is no multiple of the %d bytes of a zacc", who, zacc_stride, pb);
  if (group_stride % 4) return pf_fail(rank, "%s: a stride of %zu bytes is no multiple of the 4 bytes of a group_ID", who, group_stride);
  return 0;
}

// the scatter of a call with a context: the three arrays go up through the hand-off pieces, packed by the host threads (the positions
// are checked against `limit` on the way); then ONE launch on the context's stream, behind everything uploaded.  b null: the direct form
static int back_run(pf_ctx *c, const PfCtxView &v, const char *who, const PfBackBox *b, unsigned long long limit, const char *limit_what, size_t count,
                    const unsigned int *pos, size_t pos_stride, const void *zacc, size_t zacc_stride, const int *group_id, size_t group_stride,
                    unsigned long long *stored) {
  void *zcol = nullptr; int *gcol = nullptr; bool fresh = false;
  if (pf_ctx_back_columns(c, who, &zcol, &gcol, &fresh)) return 1;
  PfScopedTimer pt(c, 1);
  PfBackScratch s;
  memset(&s, 0, sizeof(s));
  BackGuard guard{&s};
  if (back_alloc(&s, count, v.pb, pos != nullptr))
    return pf_fail(v.rank, "%s: cannot allocate %zu bytes of scratch on the device for %zu entries", who, back_scratch_bytes(count, v.pb, pos != nullptr), count);
  size_t bad = 0;
  if (pos) {
    const int rc = pf_ctx_h2d_packed(c, s.pos, pos, count, 4, pos_stride, limit, &bad);
    if (rc == 2) {
      unsigned int p;
      memcpy(&p, (const char *)pos + bad * pos_stride, sizeof(p));
      return pf_fail(v.rank, "%s: %s[%zu] = %u lies outside the %llu cells of %s", who, b ? "frag_pos" : "pos", bad, p, limit, limit_what);
    }
    if (rc) return 1;
  }
  if (pf_ctx_h2d_packed(c, s.zacc, zacc, count, (size_t)v.pb, zacc_stride, 0, &bad) || pf_ctx_h2d_packed(c, s.gid, group_id, count, 4, group_stride, 0, &bad)) return 1;
  BACKHIP(v.rank, who, hipMemsetAsync(s.stored, 0, sizeof(unsigned long long), v.stream));
  PfBackBox none;
  memset(&none, 0, sizeof(none));
  {
    PfScopedTimer kt(c, 0, (double)count * (double)((pos ? 4 : 0) + 2 * (v.pb + 4)), v.stream);
    if (back_launch_scatter(v.pb, b ? *b : none, b == nullptr, count, s.pos, s.zacc, s.gid, zcol, gcol, s.stored, v.stream)) return pf_fail(v.rank, "%s: launch failed", who);
  }
  unsigned long long h = 0;
  BACKHIP(v.rank, who, hipMemcpyAsync(&h, s.stored, sizeof(h), hipMemcpyDeviceToHost, v.stream));
  BACKHIP(v.rank, who, hipStreamSynchronize(v.stream));
  if (stored) *stored = h;
  return 0;
}

// -------------------------------------------------------------------------------------------------------- entry points ----
extern "C" int pf_back_reset(pf_ctx *c) {
  const char *who = "pf_back_reset";
  if (!c) return pf_fail(0, "%s: null argument", who);
  PfCtxView v;
  pf_ctx_view(c, &v);
  void *zcol = nullptr; int *gcol = nullptr; bool fresh = false;
  if (pf_ctx_back_columns(c, who, &zcol, &gcol, &fresh)) return 1;
  if (fresh) return 0;   // columns that have just come into being hold -1 / 0
  if (pf_launch_back_fill(v.pb, zcol, gcol, v.ncell, v.stream)) return pf_fail(v.rank, "%s: launch failed", who);
  return 0;
}

extern "C" int pf_distribute_back(pf_ctx *c, const pf_peak_region *box, size_t count, const unsigned int *frag_pos, const void *zacc, size_t zacc_stride,
                                  const int *group_id, size_t group_stride, size_t *stored) {
  const char *who = "pf_distribute_back";
  if (!c) return pf_fail(0, "%s: null argument", who);
  PfCtxView v;
  pf_ctx_view(c, &v);
  if (!box) return pf_fail(v.rank, "%s: null argument", who);
  if (back_args(who, v.rank, v.pb, count, zacc, zacc_stride, group_id, group_stride)) return 1;
  PfBackBox b;
  unsigned long long cells = 1;
  if (back_box(who, v.rank, v.n, v.rank * v.nxl, v.nxl, box, &b, &cells)) return 1;
  if (!frag_pos && count > cells) return pf_fail(v.rank, "%s: %zu particles at the positions 0 .. count - 1 of a box of %llu cells", who, count, cells);
  if (!count) { if (stored) *stored = 0; return 0; }
  unsigned long long h = 0;
  if (back_run(c, v, who, &b, cells, "the box", count, frag_pos, 4, zacc, zacc_stride, group_id, group_stride, &h)) return 1;
  if (stored) *stored = (size_t)h;
  return 0;
}

extern "C" int pf_back_apply(pf_ctx *c, size_t count, const unsigned int *pos, size_t pos_stride, const void *zacc, size_t zacc_stride, const int *group_id,
                             size_t group_stride) {
  const char *who = "pf_back_apply";
  if (!c) return pf_fail(0, "%s: null argument", who);
  PfCtxView v;
  pf_ctx_view(c, &v);
  if (count && !pos) return pf_fail(v.rank, "%s: null argument", who);
  if (back_args(who, v.rank, v.pb, count, zacc, zacc_stride, group_id, group_stride)) return 1;
  if (pos_stride % 4) return pf_fail(v.rank, "%s: a stride of %zu bytes is no multiple of the 4 bytes of a position", who, pos_stride);
  if (!count) return 0;
  return back_run(c, v, who, nullptr, (unsigned long long)v.ncell, "the slab", count, pos, pos_stride, zacc, zacc_stride, group_id, group_stride, nullptr);
}

// test tap without a context: the same kernel on columns of its own, on the default stream
extern "C" int pf_debug_distribute_back(int n, int x0, int nxl, const pf_peak_region *box, size_t count, const unsigned int *frag_pos, const float *zacc,
                                        const int *group_id, float *zacc_out, int *group_out, size_t *stored) {
  const char *who = "pf_debug_distribute_back";
  if (!box || !zacc_out || !group_out) return pf_fail(0, "%s: null argument", who);
  if (n < 1 || n > 2048 || x0 < 0 || nxl < 1 || x0 + nxl > n) return pf_fail(0, "%s: planes %d .. %d of a box of %d^3 cells", who, x0, x0 + nxl - 1, n);
  if (back_args(who, 0, 4, count, zacc, 4, group_id, 4)) return 1;
  PfBackBox b;
  unsigned long long cells = 1;
  if (back_box(who, 0, n, x0, nxl, box, &b, &cells)) return 1;
  if (!frag_pos && count > cells) return pf_fail(0, "%s: %zu particles at the positions 0 .. count - 1 of a box of %llu cells", who, count, cells);
  if (frag_pos)
    for (size_t i = 0; i < count; i++)
      if (frag_pos[i] >= cells) return pf_fail(0, "%s: frag_pos[%zu] = %u lies outside the %llu cells of the box", who, i, frag_pos[i], cells);
  const size_t ncell = (size_t)nxl * n * n;
  float *zcol = nullptr; int *gcol = nullptr;
  PfBackScratch s;
  memset(&s, 0, sizeof(s));
  struct Columns { float **z; int **g; ~Columns() { hipFree(*z); hipFree(*g); } } columns{&zcol, &gcol};
  BackGuard guard{&s};
  if (hipMalloc((void **)&zcol, ncell * 4) != hipSuccess || hipMalloc((void **)&gcol, ncell * 4) != hipSuccess || (count && back_alloc(&s, count, 4, frag_pos != nullptr))) {
    (void)hipGetLastError();
    return pf_fail(0, "%s: cannot allocate %zu bytes on the device", who, ncell * 8 + back_scratch_bytes(count, 4, frag_pos != nullptr));
  }
  if (pf_launch_back_fill(4, zcol, gcol, ncell, nullptr)) return pf_fail(0, "%s: launch failed", who);
  unsigned long long h = 0;
  if (count) {
    if (frag_pos) BACKHIP(0, who, hipMemcpy(s.pos, frag_pos, count * 4, hipMemcpyHostToDevice));
    BACKHIP(0, who, hipMemcpy(s.zacc, zacc, count * 4, hipMemcpyHostToDevice));
    BACKHIP(0, who, hipMemcpy(s.gid, group_id, count * 4, hipMemcpyHostToDevice));
    BACKHIP(0, who, hipMemset(s.stored, 0, sizeof(unsigned long long)));
    if (back_launch_scatter(4, b, false, count, s.pos, s.zacc, s.gid, zcol, gcol, s.stored, nullptr)) return pf_fail(0, "%s: launch failed", who);
    BACKHIP(0, who, hipMemcpy(&h, s.stored, sizeof(h), hipMemcpyDeviceToHost));
  }
  BACKHIP(0, who, hipMemcpy(zacc_out, zcol, ncell * 4, hipMemcpyDeviceToHost));
  BACKHIP(0, who, hipMemcpy(group_out, gcol, ncell * 4, hipMemcpyDeviceToHost));
  if (stored) *stored = (size_t)h;
  return 0;
}
