// pf_points.hip -- the state of every stored particle of a sub-box at its own collapse time (src/build_groups.c:1286-1317 and what it
// calls: virial :1023-1051, set_point :1464-1520, set_weight :1411-1444, q2x :1554-1603), from the Fmax and velocity columns in HBM.
// The arithmetic is pf_points_core.h; this file holds the kernel and the entry points.
//
//  (k_refresh_flag, k_refresh_scan of pf_refresh.hip: which particles have their cell in this slab, and their slots in ascending
//   particle index)
//  k_point_states  one particle per lane.  A found particle whose slot is below the capacity gathers F from the Fmax column and the
//                  velocity columns the order reads (3, 6 or 12, as many again from the prev columns with myseg >= 1), evaluates
//                  its state with the spline tables in LDS -- the knot interval is found once per particle for all tables
//                  (PfPlcX) -- and writes the record of 8 PRODFLOATs at its slot.  Two forms, as k_refresh_gather has them.
//                  Natural: thread t takes particle t; the records of a workgroup have consecutive slots, are staged in LDS (one
//                  value per padded row) and leave as contiguous 16-byte stores.  Ordered: thread t takes particle order[t] -- the
//                  caller's indices[] of sort_and_organize, ascending position, which is also how callers that walk in Fmax order
//                  keep neighbours together -- and each lane writes its own 32 (64) bytes as 16-byte stores.
// The output is decided by the scan and by per-particle arithmetic alone: no atomics, identical from run to run and in both forms.
//
// The tables.  The call copies the tables it reads -- pf_point_plan: at most ten of the 2 + 8 nk -- into one small array of the form
// of the full one; every workgroup stages its first PF_POINT_LDS_DOUBLES doubles in LDS, PfPlcTab::at reads the rest from memory.
// The growing modes at the segment's redshifts are computed once per call on the host from the same small array and travel as a
// kernel argument.
//
// Every index is in range by construction: positions are below Lx Ly Lz and order entries below count -- checked on the host before
// anything is launched --; pf_refresh_cell gives an address only for a cell of the slab, which sized the Fmax column and each of the
// twelve (twenty-four) velocity columns; the prev columns are read only with myseg >= 1, which is refused without them; a slot is
// written only below the capacity that sized index and states; the staging rows hold PF_REFRESH_BLOCK ranks and a rank is below the
// workgroup's count; a table index is below the doubles of the small array (the knot search stays inside [0, n - 1], the tables of
// a family are 2 + nb f + {0, 1} with nb = 2 exactly when a PfPlcK has `both`); the staging loop copies min(doubles,
// PF_POINT_LDS_DOUBLES) doubles into an LDS array of that size.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pf_internal.h"
#include "pf_points_core.h"

#define PTHIP(task, who, call)                                                                                         \
  do {                                                                                                                 \
    hipError_t e__ = (call);                                                                                           \
    if (e__ != hipSuccess) return pf_fail(task, "%s: %s failed: %s", who, #call, hipGetErrorString(e__));             \
  } while (0)

#define PF_POINT_PAD (PF_REFRESH_BLOCK + 1)   // values of a staged row: 257
#define PF_POINT_LDS_DOUBLES 6000             // doubles of the tables a workgroup stages: 48000 bytes beside 16448 of staged records

// ---------------------------------------------------------------------------------------------------------- kernel ----
// the columns of the slab: fmax [ncell], cur / prev twelve columns of ncell each (prev null without myseg)
template <class PR> struct PfPointCols { const PR *fmax, *cur, *prev; size_t ncell; };

template <class PR>
__device__ __forceinline__ void point_record(const PfBackBox &b, unsigned int pos, const PfPointCols<PR> &cols, const PfPlcTab &tab, const PfPointGeom &g,
                                             const PfPlcSegIn &sg, const PfPlcK &kp, const PfPlcK &ks, const PfPlcSeg &seg, PR rec[PF_POINT_NREC]) {
  size_t addr = 0;
  pf_refresh_cell(b, pos, &addr);
  int c[3];
  pf_neigh_coord(b.box, pos, c);
  PfPlcObj<PR> o;
  o.M = 1;
#pragma unroll
  for (int d = 0; d < 3; d++) o.q[d] = (PR)((double)c[d] + PF_POINT_SHIFT);
  const int nfam = sg.order > 2 ? 4 : sg.order;   // families q2x reads: v; v, v2; all four
#pragma unroll
  for (int s = 0; s < 4; s++)
#pragma unroll
    for (int e = 0; e < 3; e++) {
      o.v[s][e] = s < nfam ? cols.cur[(size_t)(3 * s + e) * cols.ncell + addr] : (PR)0;
      o.v[4 + s][e] = (s < nfam && sg.myseg) ? cols.prev[(size_t)(3 * s + e) * cols.ncell + addr] : (PR)0;
    }
  const PR F = cols.fmax[addr];
  pf_point_state<PR>(tab, g, sg, kp, ks, seg, o, F, rec);
}

template <class PR, bool ORDERED>
__global__ void __launch_bounds__(PF_REFRESH_BLOCK)
    k_point_states(PfBackBox b, unsigned long long count, const unsigned int *__restrict__ pos, const int *__restrict__ order,
                   const unsigned long long *__restrict__ masks, const unsigned long long *__restrict__ offs, PfPointCols<PR> cols, PfPlcTab tab, int tab_doubles,
                   PfPointGeom g, PfPlcSegIn sg, PfPlcK kp, PfPlcK ks, PfPlcSeg seg, unsigned long long cap, unsigned int *__restrict__ index, PR *__restrict__ states) {
  extern __shared__ double lds[];
  constexpr int VPP = 16 / (int)sizeof(PR), NP = PF_POINT_NREC / VPP;   // values of a 16-byte piece, pieces of a record
  const unsigned long long t = (unsigned long long)blockIdx.x * PF_REFRESH_BLOCK + threadIdx.x;
  if constexpr (!ORDERED) {
    const unsigned long long og = offs[blockIdx.x], cg = offs[blockIdx.x + 1] - og;
    if (!cg || og >= cap) return;   // (the whole workgroup)
  }
  if (states) {   // (uniform)
    const int ns = tab_doubles < PF_POINT_LDS_DOUBLES ? tab_doubles : PF_POINT_LDS_DOUBLES;
    for (int i = threadIdx.x; i < ns; i += PF_REFRESH_BLOCK) lds[i] = tab.g[i];
    __syncthreads();
    tab.s = lds; tab.ns = ns;
  }
  if constexpr (ORDERED) {
    if (t >= count) return;
    const unsigned long long i = (unsigned long long)(unsigned int)order[t];
    if (!pf_refresh_found(masks, i)) return;
    const unsigned long long j = offs[i / PF_REFRESH_BLOCK] + pf_refresh_rank_in_block(masks, i);
    if (j >= cap) return;
    if (index) index[j] = (unsigned int)i;
    if (states) {
      PR rec[PF_POINT_NREC];
      point_record<PR>(b, pos[i], cols, tab, g, sg, kp, ks, seg, rec);
      uint4 *dst = (uint4 *)(states + j * PF_POINT_NREC);   // 32 j or 64 j bytes behind a base that hipMalloc aligned
#pragma unroll
      for (int q = 0; q < NP; q++) {
        uint4 o;
        __builtin_memcpy(&o, rec + VPP * q, 16);
        dst[q] = o;
      }
    }
  } else {
    __shared__ PR stage[PF_POINT_NREC * PF_POINT_PAD];
    const unsigned long long og = offs[blockIdx.x], cg = offs[blockIdx.x + 1] - og;
    if (t < count && pf_refresh_found(masks, t)) {
      const unsigned int rank = pf_refresh_rank_in_block(masks, t);
      if (og + rank < cap) {
        if (index) index[og + rank] = (unsigned int)t;
        if (states) {
          PR rec[PF_POINT_NREC];
          point_record<PR>(b, pos[t], cols, tab, g, sg, kp, ks, seg, rec);
#pragma unroll
          for (int w = 0; w < PF_POINT_NREC; w++) stage[w * PF_POINT_PAD + rank] = rec[w];
        }
      }
    }
    if (!states) return;
    __syncthreads();
    // the workgroup's records below the capacity as consecutive 16-byte pieces: piece q holds values VPP (q % NP) .. of record q / NP
    const unsigned int nrec = (unsigned int)(cap - og < cg ? cap - og : cg), npiece = nrec * NP;
    uint4 *dst = (uint4 *)(states + og * PF_POINT_NREC);
    for (unsigned int q = threadIdx.x; q < npiece; q += PF_REFRESH_BLOCK) {
      const unsigned int r = q / NP, w0 = VPP * (q % NP);
      PR tmp[VPP];
#pragma unroll
      for (int k = 0; k < VPP; k++) tmp[k] = stage[(w0 + k) * PF_POINT_PAD + r];
      uint4 o;
      __builtin_memcpy(&o, tmp, 16);
      dst[q] = o;
    }
  }
}

// PF_POINT_TIMES=1: device ms of the last call's select + scan passes and of its state pass (profiles/tools/points_time.py)
static double point_last_ms[2] = {0.0, 0.0};
struct PointStage {
  hipEvent_t a, b; hipStream_t st; int which; bool on;
  PointStage(bool on_, int which_, hipStream_t st_) : a(nullptr), b(nullptr), st(st_), which(which_), on(on_) {
    if (on) on = hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess && hipEventRecord(a, st) == hipSuccess;
  }
  void end() {
    float ms = 0.0f;
    if (on && hipEventRecord(b, st) == hipSuccess && hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&ms, a, b) == hipSuccess) point_last_ms[which] = ms;
    on = false;
  }
  ~PointStage() { end(); if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); }
};
extern "C" int pf_debug_point_times(double *ms2) {
  if (!ms2) return 1;
  ms2[0] = point_last_ms[0]; ms2[1] = point_last_ms[1];
  return 0;
}
static bool point_times_on() {
  const char *env = getenv("PF_POINT_TIMES");
  return env && atoi(env) != 0;
}

// ------------------------------------------------------------------------------------------------------------ launches ----
// what a call holds on the device beside the columns of a context: the selection scratch of pf_refresh.hip (its `vel` holds the
// states), the small table array and, in the tap, the caller's columns
struct PointScratch { PfRefreshScratch r; double *tab; void *fmax, *cols; };
struct PointGuard {
  PointScratch *s;
  ~PointGuard() { pf_refresh_release(&s->r); hipFree(s->tab); hipFree(s->fmax); hipFree(s->cols); s->tab = nullptr; s->fmax = s->cols = nullptr; }
};

// what the kernel needs beside the particles
struct PointCall { PfPlcTab tab; int tab_doubles; PfPointGeom g; PfPlcSegIn sg; PfPlcK kp, ks; PfPlcSeg seg; };

// the checks of seg and par that need no device; lpt_order: the order whose columns exist
static int point_args(const char *who, int rank, const pf_plc_segment *seg, const pf_point_params *par, bool have_prev) {
  if (seg->myseg < 0) return pf_fail(rank, "%s: myseg = %d", who, seg->myseg);
  if (seg->myseg >= 1 && !have_prev) return pf_fail(rank, "%s: myseg = %d reads the Vel*_prev columns but there is no pf_shift_displacements yet", who, seg->myseg);
  if (par->order < 1 || par->order > 3) return pf_fail(rank, "%s: order = %d (1 to 3)", who, par->order);
  const double v[3] = {par->sigma0, par->k_sigma, par->k_point};
  const char *nm[3] = {"sigma0", "k_sigma", "k_point"};
  for (int i = 0; i < 3; i++)
    if (!(v[i] > 0.0) || v[i] - v[i] != 0.0) return pf_fail(rank, "%s: %s = %g must be positive and finite", who, nm[i], v[i]);
  return 0;
}

// the small table array of the call on the device (s->tab), the segment's growing modes and the rest of PointCall
static int point_prepare(const char *who, int rank, const PfPlcTab &full, const pf_plc_segment *seg, const pf_point_params *par, int lpt_order, const PfBackBox &b,
                         PointScratch *s, PointCall *pc) {
  const PfPointPlan plan = pf_point_plan(full, par->k_point, par->k_sigma);
  const int n = full.n;
  std::vector<double> h((size_t)plan.doubles, 0.0);
  PTHIP(rank, who, hipMemcpy(h.data(), full.g, (size_t)n * 8, hipMemcpyDeviceToHost));
  for (int j = 0; j < plan.ntab; j++)
    if (plan.src[j] >= 0)
      PTHIP(rank, who, hipMemcpy(h.data() + n + (size_t)4 * n * j, full.g + n + (size_t)4 * n * plan.src[j], (size_t)4 * n * 8, hipMemcpyDeviceToHost));
  if (hipMalloc((void **)&s->tab, (size_t)plan.doubles * 8) != hipSuccess) {
    (void)hipGetLastError();
    return pf_fail(rank, "%s: cannot allocate %zu bytes on the device for the tables of the call", who, (size_t)plan.doubles * 8);
  }
  PTHIP(rank, who, hipMemcpy(s->tab, h.data(), (size_t)plan.doubles * 8, hipMemcpyHostToDevice));
  pc->sg.myseg = seg->myseg; pc->sg.use_v31 = seg->use_v31 != 0; pc->sg.order = par->order < lpt_order ? par->order : lpt_order;
  pc->sg.z_seg = seg->z_seg; pc->sg.z_prev = seg->z_prev;
  pc->g.nw = lpt_order >= 3 ? 4 : lpt_order == 2 ? 2 : 1;
  pc->g.sigma0 = par->sigma0;
  for (int d = 0; d < 3; d++) { pc->g.box[d] = (double)b.box.len[d]; pc->g.pbc[d] = b.box.pbc[d]; }
  pc->kp = plan.kp; pc->ks = plan.ks;
  const PfPlcTab host = pf_point_tab(full, plan, h.data());
  pc->seg = pf_point_segment_modes(host, pc->sg, pc->kp, pc->g.nw);
  pc->tab = pf_point_tab(full, plan, s->tab);
  pc->tab_doubles = plan.doubles;
  return 0;
}

template <class PR>
static int point_launch(const PfBackBox &b, size_t count, const PfRefreshScratch &r, const void *fmax, const void *cur, const void *prev, size_t ncell,
                        const PointCall &pc, unsigned long long cap, hipStream_t st) {
  const dim3 grid((unsigned int)pf_refresh_blocks(count)), block(PF_REFRESH_BLOCK);
  const int ns = pc.tab_doubles < PF_POINT_LDS_DOUBLES ? pc.tab_doubles : PF_POINT_LDS_DOUBLES;
  const size_t lds = r.vel ? (size_t)ns * 8 : 0;
  PfPointCols<PR> cols{(const PR *)fmax, (const PR *)cur, (const PR *)prev, ncell};
  const unsigned long long n = count;
  if (r.order)
    hipLaunchKernelGGL((k_point_states<PR, true>), grid, block, lds, st, b, n, r.pos, r.order, r.masks, r.offs, cols, pc.tab, pc.tab_doubles, pc.g, pc.sg, pc.kp, pc.ks, pc.seg, cap,
                       r.index, (PR *)r.vel);
  else
    hipLaunchKernelGGL((k_point_states<PR, false>), grid, block, lds, st, b, n, r.pos, r.order, r.masks, r.offs, cols, pc.tab, pc.tab_doubles, pc.g, pc.sg, pc.kp, pc.ks, pc.seg, cap,
                       r.index, (PR *)r.vel);
  return hipGetLastError() != hipSuccess;
}
static int point_states(int pb, const PfBackBox &b, size_t count, const PfRefreshScratch &r, const void *fmax, const void *cur, const void *prev, size_t ncell,
                        const PointCall &pc, unsigned long long cap, hipStream_t st) {
  return pb == 8 ? point_launch<double>(b, count, r, fmax, cur, prev, ncell, pc, cap, st) : point_launch<float>(b, count, r, fmax, cur, prev, ncell, pc, cap, st);
}
static int point_alloc_out(PfRefreshScratch *r, size_t m, int pb, bool want_index, bool want_states) {
  bool ok = true;
  if (want_index) ok = hipMalloc((void **)&r->index, m * 4) == hipSuccess;
  if (ok && want_states) ok = hipMalloc(&r->vel, m * PF_POINT_NREC * (size_t)pb) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); return 1; }
  return 0;
}

// -------------------------------------------------------------------------------------------------------- entry points ----
extern "C" int pf_point_states(pf_ctx *c, const pf_plc_segment *seg, const pf_peak_region *box, const pf_point_params *par, size_t count, const unsigned int *frag_pos,
                               const int *order, size_t capacity, unsigned int *index, void *states, size_t *found) {
  const char *who = "pf_point_states";
  if (found) *found = 0;
  if (!c) return pf_fail(0, "%s: null argument", who);
  PfCtxView v;
  pf_ctx_view(c, &v);
  if (!seg || !box || !par || (count && !frag_pos)) return pf_fail(v.rank, "%s: null argument", who);
  PfPlcTab full;
  int full_doubles = 0;
  if (!pf_plc_tables(c, &full, &full_doubles)) return pf_fail(v.rank, "%s: no cosmology set (pf_plc_set_cosmology)", who);
  if (!v.products_init) return pf_fail(v.rank, "%s: products not computed", who);
  const void *prev = nullptr; int shifts = 0, lpt_order = 3;
  pf_ctx_prev_view(c, &prev, &shifts, &lpt_order);
  if (point_args(who, v.rank, seg, par, prev != nullptr)) return 1;
  if (count > 0x7FFFFFFFull) return pf_fail(v.rank, "%s: %zu particles: indices[] is int as in the reference, 2^31 - 1 particles at most", who, count);
  PfBackBox b;
  unsigned long long cells = 1;
  if (pf_refresh_box(who, v.rank, v.n, v.rank * v.nxl, v.nxl, box, &b, &cells)) return 1;
  if (!count) return 0;
  if (pf_ctx_velocities_ready(c)) return 1;
  PointScratch s;
  memset(&s, 0, sizeof(s));
  PointGuard guard{&s};
  PfScopedTimer pt(c, 1);
  if (pf_refresh_alloc_in(&s.r, count, order != nullptr))
    return pf_fail(v.rank, "%s: cannot allocate %zu bytes of scratch on the device for %zu particles", who, pf_refresh_in_bytes(count, order != nullptr), count);
  size_t bad = 0;
  int rc = pf_ctx_h2d_packed(c, s.r.pos, frag_pos, count, 4, 4, cells, &bad);
  if (rc == 2) {
    bad = pf_refresh_first_bad(frag_pos, bad, cells);
    return pf_fail(v.rank, "%s: frag_pos[%zu] = %u lies outside the %llu cells of the box", who, bad, frag_pos[bad], cells);
  }
  if (rc) return 1;
  if (order) {
    rc = pf_ctx_h2d_packed(c, s.r.order, order, count, 4, 4, (unsigned long long)count, &bad);
    if (rc == 2) {
      bad = pf_refresh_first_bad((const unsigned int *)order, bad, count);
      return pf_fail(v.rank, "%s: order[%zu] = %d is no index of the %zu particles", who, bad, order[bad], count);
    }
    if (rc) return 1;
  }
  const bool times = point_times_on();
  unsigned long long h = 0;
  {
    PfScopedTimer kt(c, 0, (double)count * 4.0 + (double)pf_refresh_blocks(count) * 56.0, v.stream);
    PointStage stage(times, 0, v.stream);
    if (pf_refresh_select(who, v.rank, b, count, s.r, v.stream, &h)) return 1;
  }
  const size_t m = h < capacity ? (size_t)h : capacity;
  if (m && (index || states)) {
    const size_t pb = (size_t)v.pb;
    if (point_alloc_out(&s.r, m, v.pb, index != nullptr, states != nullptr))
      return pf_fail(v.rank, "%s: cannot allocate %zu bytes on the device for the states of %zu particles", who, m * ((index ? 4 : 0) + (states ? PF_POINT_NREC * pb : 0)), m);
    if (order) {   // an order that is no permutation omits particles: their entries then read 0xFFFFFFFF / zero, not what the memory held
      if (s.r.index) PTHIP(v.rank, who, hipMemsetAsync(s.r.index, 0xFF, m * 4, v.stream));
      if (s.r.vel) PTHIP(v.rank, who, hipMemsetAsync(s.r.vel, 0, m * PF_POINT_NREC * pb, v.stream));
    }
    PointCall pc;
    memset(&pc, 0, sizeof(pc));
    if (states && point_prepare(who, v.rank, full, seg, par, lpt_order, b, &s, &pc)) return 1;
    {
      PfScopedTimer kt(c, 0, (double)count * (order ? 24.0 : 20.0) + (double)m * (4.0 + (double)pb * (1 + 6 * pc.sg.order * (seg->myseg ? 2 : 1) + PF_POINT_NREC)), v.stream);
      PointStage stage(times, 1, v.stream);
      if (point_states(v.pb, b, count, s.r, v.fmax, v.vel12, prev, v.ncell, pc, m, v.stream)) return pf_fail(v.rank, "%s: launch failed", who);
      if (times) PTHIP(v.rank, who, hipStreamSynchronize(v.stream));
    }
    if (index && pf_ctx_d2h(c, index, s.r.index, m * 4)) return 1;
    if (states && pf_ctx_d2h(c, states, s.r.vel, m * PF_POINT_NREC * pb)) return 1;
  }
  if (found) *found = (size_t)h;
  return 0;
}

// test tap on a caller's columns, on the default stream; tables_ctx supplies the cosmology tables alone
extern "C" int pf_debug_point_states(int n, int x0, int nxl, int pb, const void *fmax_col, const void *cols24, pf_ctx *tables_ctx, const pf_plc_segment *seg,
                                     const pf_peak_region *box, const pf_point_params *par, size_t count, const unsigned int *frag_pos, const int *order,
                                     unsigned int *index, void *states, size_t *found) {
  const char *who = "pf_debug_point_states";
  if (found) *found = 0;
  if (!fmax_col || !cols24 || !tables_ctx || !seg || !box || !par || (count && !frag_pos)) return pf_fail(0, "%s: null argument", who);
  if (pb != 4 && pb != 8) return pf_fail(0, "%s: a PRODFLOAT of %d bytes (4 or 8)", who, pb);
  if (n < 1 || n > 2048 || x0 < 0 || nxl < 1 || x0 + nxl > n) return pf_fail(0, "%s: planes %d .. %d of a box of %d^3 cells", who, x0, x0 + nxl - 1, n);
  PfPlcTab full;
  int full_doubles = 0;
  if (!pf_plc_tables(tables_ctx, &full, &full_doubles)) return pf_fail(0, "%s: no cosmology set (pf_plc_set_cosmology)", who);
  if (point_args(who, 0, seg, par, true)) return 1;
  if (count > 0x7FFFFFFFull) return pf_fail(0, "%s: %zu particles: indices[] is int as in the reference, 2^31 - 1 particles at most", who, count);
  PfBackBox b;
  unsigned long long cells = 1;
  if (pf_refresh_box(who, 0, n, x0, nxl, box, &b, &cells)) return 1;
  for (size_t i = 0; i < count; i++)
    if (frag_pos[i] >= cells) return pf_fail(0, "%s: frag_pos[%zu] = %u lies outside the %llu cells of the box", who, i, frag_pos[i], cells);
  if (order)
    for (size_t i = 0; i < count; i++)
      if ((unsigned int)order[i] >= count) return pf_fail(0, "%s: order[%zu] = %d is no index of the %zu particles", who, i, order[i], count);
  if (!count) return 0;
  const size_t ncell = (size_t)nxl * n * n, colbytes = 24 * ncell * (size_t)pb, fbytes = ncell * (size_t)pb;
  PointScratch s;
  memset(&s, 0, sizeof(s));
  PointGuard guard{&s};
  if (hipMalloc(&s.cols, colbytes) != hipSuccess || hipMalloc(&s.fmax, fbytes) != hipSuccess || pf_refresh_alloc_in(&s.r, count, order != nullptr) ||
      point_alloc_out(&s.r, count, pb, true, true)) {
    (void)hipGetLastError();
    return pf_fail(0, "%s: cannot allocate %zu bytes on the device", who, colbytes + fbytes + pf_refresh_in_bytes(count, order != nullptr) + count * (4 + PF_POINT_NREC * (size_t)pb));
  }
  PTHIP(0, who, hipMemcpy(s.cols, cols24, colbytes, hipMemcpyHostToDevice));
  PTHIP(0, who, hipMemcpy(s.fmax, fmax_col, fbytes, hipMemcpyHostToDevice));
  PTHIP(0, who, hipMemcpy(s.r.pos, frag_pos, count * 4, hipMemcpyHostToDevice));
  if (order) PTHIP(0, who, hipMemcpy(s.r.order, order, count * 4, hipMemcpyHostToDevice));
  unsigned long long h = 0;
  if (pf_refresh_select(who, 0, b, count, s.r, nullptr, &h)) return 1;
  if (h) {
    PointCall pc;
    memset(&pc, 0, sizeof(pc));
    if (point_prepare(who, 0, full, seg, par, 3, b, &s, &pc)) return 1;
    if (order) {
      PTHIP(0, who, hipMemset(s.r.index, 0xFF, (size_t)h * 4));
      PTHIP(0, who, hipMemset(s.r.vel, 0, (size_t)h * PF_POINT_NREC * (size_t)pb));
    }
    const char *cur = (const char *)s.cols;
    if (point_states(pb, b, count, s.r, s.fmax, cur, cur + 12 * ncell * (size_t)pb, ncell, pc, h, nullptr)) return pf_fail(0, "%s: launch failed", who);
    PTHIP(0, who, hipDeviceSynchronize());
    if (index) PTHIP(0, who, hipMemcpy(index, s.r.index, (size_t)h * 4, hipMemcpyDeviceToHost));
    if (states) PTHIP(0, who, hipMemcpy(states, s.r.vel, (size_t)h * PF_POINT_NREC * (size_t)pb, hipMemcpyDeviceToHost));
  }
  if (found) *found = (size_t)h;
  return 0;
}
