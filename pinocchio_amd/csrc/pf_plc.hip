// pf_plc.hip -- the past-light-cone test of build_groups() (src/build_groups.c:356-448, :783-868) on the device.  The arithmetic is
// pf_plc_core.h; this file holds the state a context keeps for it, the kernels and the entry points.
//
//  k_plc_ends   one candidate per lane.  A candidate that passes the filter gets its own k, the growing modes at the segment's
//               redshifts, and position + comoving distance at both ends of its interval -- two evaluations that serve every
//               replication.  Then the replications loop over two distances each and the crossing pairs are counted.
//  k_plc_list   after the scan of the counts: the same loop on the stored ends (same inputs, same instructions, same decisions)
//               writes the (candidate, replication) pairs at the candidate's offset, in replication order.
//  k_plc_root   one crossing pair per lane: the root finder and store_PLC.  Only lanes with work are here, so a wavefront is not
//               held by one lane's iterations of a pair among sixty-three that do not cross.
//  k_plc_pack   after the scan of the stored flags: the records that passed the aperture move to their slots; the n(z) histogram
//               is counted in integers.
// The order of the output is decided by the two scans alone.  The integer atomics (histogram, unconverged pairs) add counts.
//
// The spline tables are staged in LDS by every workgroup of k_plc_ends and k_plc_root: all of them where they fit
// PF_PLC_LDS_DOUBLES (the scale-independent build: ten tables), their first PF_PLC_LDS_DOUBLES doubles -- the knots, the comoving
// distance the root finder reads most, Hubble and the first growth tables -- otherwise; PfPlcTab::at reads the rest from memory.
//
// Every index is in range by construction: a lane works on i < ncand (p < npairs); a replication index is below nrep, which sized
// the array; a pair slot is below the candidate's next offset, and the offsets end at npairs, which sized the pair arrays; a record
// slot is below the number of stored pairs and is written only below the capacity that sized the output; a table index is below
// pf_plc_tab_doubles (the knot search stays inside [0, n - 1], the k-bin and the smoothing index are clamped in pf_plc_core.h); a
// histogram bin is checked against nzbins.
#include <hip/hip_runtime.h>

#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pf_internal.h"
#include "pf_collapse_core.h"   // pf_spline_coeffs, pf_spline_bd (host)
#include "pf_plc_core.h"

#define PLCHIP(task, who, call)                                                                                        \
  do {                                                                                                                 \
    hipError_t e__ = (call);                                                                                           \
    if (e__ != hipSuccess) return pf_fail(task, "%s: %s failed: %s", who, #call, hipGetErrorString(e__));             \
  } while (0)

// ---------------------------------------------------------------------------------------------------------- kernels ----
// candidate i as the kernels read it: val[k ncand + i], k as in PF_PLC_NVAL
template <class T> struct PfPlcCand { const T *val; const int *mass; const unsigned char *pass; unsigned long long n; };
// ends[(6) ncand] positions (lo 0..2, hi 3..5), dist[(2) ncand]
template <class T> struct PfPlcEnds { T *P; double *D; };

__device__ __forceinline__ PfPlcTab plc_stage(PfPlcTab t, int total, double *lds) {
  const int ns = total < PF_PLC_LDS_DOUBLES ? total : PF_PLC_LDS_DOUBLES;
  for (int i = threadIdx.x; i < ns; i += blockDim.x) lds[i] = t.g[i];
  __syncthreads();
  t.s = lds; t.ns = ns;
  return t;
}
template <class T> __device__ __forceinline__ PfPlcObj<T> plc_load(const PfPlcCand<T> &c, unsigned long long i) {
  PfPlcObj<T> o;
  o.M = c.mass[i];
#pragma unroll
  for (int e = 0; e < 3; e++) o.q[e] = c.val[(unsigned long long)e * c.n + i];
#pragma unroll
  for (int s = 0; s < 8; s++)
#pragma unroll
    for (int e = 0; e < 3; e++) o.v[s][e] = c.val[(unsigned long long)(3 + 3 * s + e) * c.n + i];
  return o;
}
template <class T> __device__ __forceinline__ T plc_flo(const PfPlcCand<T> &c, const PfPlcGeom &g, int events, unsigned long long i) {
  return events ? c.val[(unsigned long long)PF_PLC_V_FLO * c.n + i] : (T)g.Fstop;
}
template <class T> __device__ __forceinline__ void plc_read_ends(const PfPlcEnds<T> &e, unsigned long long n, unsigned long long i, PfPlcEnd<T> *lo, PfPlcEnd<T> *hi) {
#pragma unroll
  for (int k = 0; k < 3; k++) { lo->P[k] = e.P[(unsigned long long)k * n + i]; hi->P[k] = e.P[(unsigned long long)(3 + k) * n + i]; }
  lo->D = e.D[i]; hi->D = e.D[n + i];
}
// the replications of one candidate: f(r, kind) for every crossing pair, in replication order
template <class T, class F> __device__ __forceinline__ void plc_pairs(const PfPlcGeom &g, int events, T Flo, T Flast, const PfPlcEnd<T> &lo, const PfPlcEnd<T> &hi, F f) {
  for (int r = 0; r < g.nrep; r++) {
    const PfPlcRep rep = g.rep[r];
    if (!pf_plc_tried<T>(events, Flo, Flast, rep)) continue;
    const double bb = pf_plc_condition<T>(g, lo, rep);
    const double aa = bb > 0. ? pf_plc_condition<T>(g, hi, rep) : 0.0;
    const int kind = pf_plc_decide(bb, aa);
    if (kind) f(r, kind);
  }
}

template <class T>
__global__ void __launch_bounds__(PF_PLC_BLOCK)
    k_plc_ends(PfPlcTab tab, int tab_doubles, PfPlcGeom g, PfPlcSegIn sg, int events, int min_mass, PfPlcCand<T> c, PfPlcEnds<T> ends, unsigned int *__restrict__ counts) {
  extern __shared__ double lds[];
  tab = plc_stage(tab, tab_doubles, lds);
  const unsigned long long i = (unsigned long long)blockIdx.x * PF_PLC_BLOCK + threadIdx.x;
  if (i >= c.n) return;
  unsigned int cnt = 0;
  if (c.pass[i] && c.mass[i] >= min_mass) {
    const PfPlcObj<T> o = plc_load<T>(c, i);
    const T Flast = c.val[(unsigned long long)PF_PLC_V_FLAST * c.n + i], Flo = plc_flo<T>(c, g, events, i);
    const PfPlcK k = pf_plc_group_k<T>(tab, o.M, g.ipd);
    const PfPlcSeg s = pf_plc_segment_modes(tab, sg, k);
    const PfPlcEnd<T> lo = pf_plc_end<T>(tab, g, sg, k, s, o, Flo, nullptr), hi = pf_plc_end<T>(tab, g, sg, k, s, o, Flast, nullptr);
#pragma unroll
    for (int e = 0; e < 3; e++) { ends.P[(unsigned long long)e * c.n + i] = lo.P[e]; ends.P[(unsigned long long)(3 + e) * c.n + i] = hi.P[e]; }
    ends.D[i] = lo.D; ends.D[c.n + i] = hi.D;
    plc_pairs<T>(g, events, Flo, Flast, lo, hi, [&](int, int) { cnt++; });
  }
  counts[i] = cnt;
}

template <class T>
__global__ void __launch_bounds__(PF_PLC_BLOCK)
    k_plc_list(PfPlcGeom g, int events, PfPlcCand<T> c, PfPlcEnds<T> ends, const unsigned int *__restrict__ counts, const unsigned long long *__restrict__ offs,
               unsigned int *__restrict__ pair_c, int *__restrict__ pair_r) {
  const unsigned long long i = (unsigned long long)blockIdx.x * PF_PLC_BLOCK + threadIdx.x;
  if (i >= c.n || !counts[i]) return;
  const T Flast = c.val[(unsigned long long)PF_PLC_V_FLAST * c.n + i], Flo = plc_flo<T>(c, g, events, i);
  PfPlcEnd<T> lo, hi;
  plc_read_ends<T>(ends, c.n, i, &lo, &hi);
  unsigned long long at = offs[i];
  const unsigned long long end = offs[i + 1];
  plc_pairs<T>(g, events, Flo, Flast, lo, hi, [&](int r, int) {
    if (at < end) { pair_c[at] = (unsigned int)i; pair_r[at] = r; }
    at++;
  });
}

// rec[(7) npairs]: z, x[3], v[3] of pair p at rec[k npairs + p]; ok[p] = 1 when stored; bin[p] its histogram bin or -1
template <class T>
__global__ void __launch_bounds__(PF_PLC_BLOCK)
    k_plc_root(PfPlcTab tab, int tab_doubles, PfPlcGeom g, PfPlcSegIn sg, int events, PfPlcCand<T> c, PfPlcEnds<T> ends, unsigned long long npairs,
               const unsigned int *__restrict__ pair_c, const int *__restrict__ pair_r, T *__restrict__ rec, unsigned int *__restrict__ ok, int *__restrict__ bin,
               unsigned long long *unconverged) {
  extern __shared__ double lds[];
  tab = plc_stage(tab, tab_doubles, lds);
  const unsigned long long p = (unsigned long long)blockIdx.x * PF_PLC_BLOCK + threadIdx.x;
  if (p >= npairs) return;
  const unsigned long long i = pair_c[p];
  const PfPlcRep rep = g.rep[pair_r[p]];
  const PfPlcObj<T> o = plc_load<T>(c, i);
  const T Flast = c.val[(unsigned long long)PF_PLC_V_FLAST * c.n + i], Flo = plc_flo<T>(c, g, events, i);
  const PfPlcK k = pf_plc_group_k<T>(tab, o.M, g.ipd);
  const PfPlcSeg s = pf_plc_segment_modes(tab, sg, k);
  PfPlcEnd<T> lo, hi;
  plc_read_ends<T>(ends, c.n, i, &lo, &hi);
  const double bb = pf_plc_condition<T>(g, lo, rep);
  T F = Flo;
  bool found = true;
  if (bb != 0.0) {
    found = pf_plc_root<T>(tab, g, sg, k, s, o, rep, Flo, Flast, bb, pf_plc_condition<T>(g, hi, rep), &F);
    if (!found) atomicAdd(unconverged, 1ull);
  }
  T out[7];
  int iz = -1;
  const bool stored = found && pf_plc_store<T>(tab, g, sg, k, s, o, rep, F, out, &iz);
  ok[p] = stored ? 1u : 0u;
  bin[p] = iz;
  if (stored) {
#pragma unroll
    for (int q = 0; q < 7; q++) rec[(unsigned long long)q * npairs + p] = out[q];
  }
}

// the stored pairs to their slots: out[7 slot + q], the pair beside them
template <class T>
__global__ void __launch_bounds__(PF_PLC_BLOCK)
    k_plc_pack(unsigned long long npairs, unsigned long long cap, const unsigned int *__restrict__ pair_c, const int *__restrict__ pair_r, const T *__restrict__ rec,
               const unsigned int *__restrict__ ok, const int *__restrict__ bin, const unsigned long long *__restrict__ slots, T *__restrict__ out,
               unsigned int *__restrict__ out_c, int *__restrict__ out_r, unsigned long long *__restrict__ hist, int nzbins) {
  const unsigned long long p = (unsigned long long)blockIdx.x * PF_PLC_BLOCK + threadIdx.x;
  if (p >= npairs || !ok[p]) return;
  const unsigned long long slot = slots[p];
  if (slot >= cap) return;
#pragma unroll
  for (int q = 0; q < 7; q++) out[7 * slot + q] = rec[(unsigned long long)q * npairs + p];
  out_c[slot] = pair_c[p];
  out_r[slot] = pair_r[p];
  const int b = bin[p];
  if (b >= 0 && b < nzbins) atomicAdd(&hist[b], 1ull);
}

// ------------------------------------------------------------------------------------------------ state of a context ----
struct PfPlcState {
  bool have_cosmo, have_geom;
  double *dtab; PfPlcRep *drep;
  int tab_doubles;
  PfPlcTab tab;
  PfPlcGeom geom;
};
void pf_plc_release(void *state) {
  PfPlcState *s = (PfPlcState *)state;
  if (!s) return;
  hipFree(s->dtab); hipFree(s->drep);
  delete s;
}
static PfPlcState *plc_state(pf_ctx *c) {
  void **slot = pf_ctx_plc_slot(c);
  if (!*slot) {
    PfPlcState *s = new PfPlcState();
    memset(s, 0, sizeof(*s));
    *slot = s;
  }
  return (PfPlcState *)*slot;
}

// what pf_catalog.hip reads of the state: the tables as pf_plc_set_cosmology left them on the device; false while there are none
bool pf_plc_tables(pf_ctx *c, PfPlcTab *tab, int *tab_doubles) {
  const PfPlcState *s = (const PfPlcState *)*pf_ctx_plc_slot(c);
  if (!s || !s->have_cosmo) return false;
  *tab = s->tab; *tab_doubles = s->tab_doubles;
  return true;
}

extern "C" int pf_plc_set_cosmology(pf_ctx *c, const pf_plc_cosmology *cs) {
  const char *who = "pf_plc_set_cosmology";
  if (!c || !cs) return pf_fail(0, "%s: null argument", who);
  PfCtxView v;
  pf_ctx_view(c, &v);
  if (!cs->x || !cs->comvdist || !cs->hubble) return pf_fail(v.rank, "%s: null argument", who);
  for (int f = 0; f < 4; f++)
    if (!cs->grow[f] || !cs->fomega[f]) return pf_fail(v.rank, "%s: null argument", who);
  const int n = cs->n, nk = cs->nk;
  if (n < 3 || n > PF_KNOT_CAP) return pf_fail(v.rank, "%s: %d knots (3 to %d)", who, n, PF_KNOT_CAP);
  if (nk < 1 || nk > PF_PLC_MAX_NK) return pf_fail(v.rank, "%s: nk = %d (1, or up to %d k-bins)", who, nk, PF_PLC_MAX_NK);
  for (int i = 0; i + 1 < n; i++)
    if (!(cs->x[i + 1] > cs->x[i])) return pf_fail(v.rank, "%s: the knots do not increase at x[%d] = %g, x[%d] = %g", who, i, cs->x[i], i + 1, cs->x[i + 1]);
  int nsmooth = 0;
  if (nk > 1) {
    if (!cs->k_gm_displ) return pf_fail(v.rank, "%s: null argument", who);
    if (cs->nsmooth < 2 || cs->nsmooth > 4096) return pf_fail(v.rank, "%s: nsmooth = %d (2 to 4096)", who, cs->nsmooth);
    if (!(cs->rad_gm0 > 0.0) || !(cs->deltalogk > 0.0)) return pf_fail(v.rank, "%s: Rad_GM[0] = %g and deltalogk = %g must be positive", who, cs->rad_gm0, cs->deltalogk);
    nsmooth = cs->nsmooth;
    for (int j = 0; j < nsmooth; j++)
      if (!(cs->k_gm_displ[j] > 0.0)) return pf_fail(v.rank, "%s: k_GM_displ[%d] = %g is not positive", who, j, cs->k_gm_displ[j]);
  }
  const int total = pf_plc_tab_doubles(n, nk, nsmooth);
  std::vector<double> h((size_t)total);
  memcpy(h.data(), cs->x, (size_t)n * 8);
  auto put = [&](int table, const double *y) -> int {
    double *dst = h.data() + n + (size_t)4 * n * table;
    memcpy(dst, y, (size_t)n * 8);
    if (pf_spline_coeffs(cs->x, y, n, dst + n)) return 1;
    pf_spline_bd(cs->x, y, dst + n, n, dst + 2 * n, dst + 3 * n);
    return 0;
  };
  int bad = put(0, cs->comvdist) | put(1, cs->hubble);
  for (int f = 0; f < 4; f++)
    for (int j = 0; j < nk; j++) bad |= put(2 + nk * f + j, cs->grow[f] + (size_t)j * n) | put(2 + nk * (4 + f) + j, cs->fomega[f] + (size_t)j * n);
  if (bad) return pf_fail(v.rank, "%s: spline set-up failed", who);
  for (int j = 0; j < nsmooth; j++) h[(size_t)total - nsmooth + j] = cs->k_gm_displ[j];
  for (int i = 0; i < total; i++)
    if (!(h[i] == h[i]) || h[i] - h[i] != 0.0) return pf_fail(v.rank, "%s: a table holds a value that is not finite", who);
  PfPlcState *s = plc_state(c);
  PLCHIP(v.rank, who, hipStreamSynchronize(v.stream));
  double *d = nullptr;
  if (hipMalloc((void **)&d, (size_t)total * 8) != hipSuccess) { (void)hipGetLastError(); return pf_fail(v.rank, "%s: cannot allocate %zu bytes on the device", who, (size_t)total * 8); }
  if (hipMemcpy(d, h.data(), (size_t)total * 8, hipMemcpyHostToDevice) != hipSuccess) { hipFree(d); return pf_fail(v.rank, "%s: upload failed", who); }
  hipFree(s->dtab);
  s->dtab = d; s->tab_doubles = total;
  PfPlcTab &t = s->tab;
  t.g = d; t.s = nullptr; t.ns = 0; t.n = n; t.nk = nk;
  t.logkmin = cs->logkmin; t.dlogk = cs->deltalogk; t.kmin = pow(10., cs->logkmin); t.kmax = pow(10., cs->logkmin + (nk - 1) * cs->deltalogk);   // cosmo.c:169-170
  t.k_for_GM = cs->k_for_GM; t.rad_gm0 = cs->rad_gm0; t.nsmooth = nsmooth; t.kgm_at = total - nsmooth;
  s->have_cosmo = true;
  return 0;
}

extern "C" int pf_plc_set_geometry(pf_ctx *c, const pf_plc_geometry *gm) {
  const char *who = "pf_plc_set_geometry";
  if (!c || !gm) return pf_fail(0, "%s: null argument", who);
  PfCtxView v;
  pf_ctx_view(c, &v);
  if (!gm->nrep) return pf_fail(v.rank, "%s: no replications", who);
  if (!gm->repls) return pf_fail(v.rank, "%s: null argument", who);
  if (gm->nrep > 0x7FFFFFFFull) return pf_fail(v.rank, "%s: %zu replications (2^31 - 1 at most)", who, gm->nrep);
  if (!(gm->InterPartDist > 0.0)) return pf_fail(v.rank, "%s: InterPartDist = %g must be positive", who, gm->InterPartDist);
  if (gm->nzbins < 0 || gm->nzbins > (1 << 20) || (gm->nzbins && !(gm->delta_z > 0.0)))
    return pf_fail(v.rank, "%s: a histogram of %d bins of width %g", who, gm->nzbins, gm->delta_z);
  std::vector<PfPlcRep> h(gm->nrep);
  for (size_t r = 0; r < gm->nrep; r++) {
    h[r].i = gm->repls[r].i; h[r].j = gm->repls[r].j; h[r].k = gm->repls[r].k;
    if (v.pb == 8) { h[r].F1 = gm->repls[r].F1; h[r].F2 = gm->repls[r].F2; }
    else { h[r].F1 = (double)(float)gm->repls[r].F1; h[r].F2 = (double)(float)gm->repls[r].F2; }
  }
  PfPlcState *s = plc_state(c);
  PLCHIP(v.rank, who, hipStreamSynchronize(v.stream));
  PfPlcRep *d = nullptr;
  if (hipMalloc((void **)&d, gm->nrep * sizeof(PfPlcRep)) != hipSuccess) { (void)hipGetLastError(); return pf_fail(v.rank, "%s: cannot allocate %zu bytes on the device", who, gm->nrep * sizeof(PfPlcRep)); }
  if (hipMemcpy(d, h.data(), gm->nrep * sizeof(PfPlcRep), hipMemcpyHostToDevice) != hipSuccess) { hipFree(d); return pf_fail(v.rank, "%s: upload failed", who); }
  hipFree(s->drep);
  s->drep = d;
  PfPlcGeom &g = s->geom;
  for (int i = 0; i < 3; i++) { g.center[i] = gm->center[i]; g.xvers[i] = gm->xvers[i]; g.yvers[i] = gm->yvers[i]; g.zvers[i] = gm->zvers[i]; g.gs[i] = gm->GSglobal[i]; g.stabl[i] = 0; }
  g.aperture = gm->aperture; g.Fstop = gm->Fstop; g.ipd = gm->InterPartDist; g.lastz = gm->LastzForPLC; g.delta_z = gm->delta_z; g.nzbins = gm->nzbins;
  g.nrep = (int)gm->nrep; g.rep = d;
  s->have_geom = true;
  return 0;
}

// PF_PLC_TIMES=1: device ms of the last call's candidate passes and of its root + store passes (profiles/tools/plc_time.py)
static double plc_last_ms[2] = {0.0, 0.0};
struct PlcStage {
  hipEvent_t a, b; hipStream_t st; int which; bool on;
  PlcStage(bool on_, int which_, hipStream_t st_) : a(nullptr), b(nullptr), st(st_), which(which_), on(on_) {
    if (on) on = hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess && hipEventRecord(a, st) == hipSuccess;
  }
  void end() {
    float ms = 0.0f;
    if (on && hipEventRecord(b, st) == hipSuccess && hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&ms, a, b) == hipSuccess) plc_last_ms[which] = ms;
    on = false;
  }
  ~PlcStage() { end(); if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); }
};
extern "C" int pf_debug_plc_times(double *ms2) {
  if (!ms2) return 1;
  ms2[0] = plc_last_ms[0]; ms2[1] = plc_last_ms[1];
  return 0;
}

// ------------------------------------------------------------------------------------------------------ the test ----
struct PlcScratch {
  void *val; int *mass; unsigned char *pass; void *endP; double *endD; unsigned int *counts; unsigned long long *offs;
  unsigned int *pair_c; int *pair_r; void *rec; unsigned int *ok; int *bin; unsigned long long *slots, *unconv, *hist;
  void *out; unsigned int *out_c; int *out_r;
};
static void plc_scratch_release(PlcScratch *s) {
  hipFree(s->val); hipFree(s->mass); hipFree(s->pass); hipFree(s->endP); hipFree(s->endD); hipFree(s->counts); hipFree(s->offs); hipFree(s->pair_c); hipFree(s->pair_r);
  hipFree(s->rec); hipFree(s->ok); hipFree(s->bin); hipFree(s->slots); hipFree(s->unconv); hipFree(s->hist); hipFree(s->out); hipFree(s->out_c); hipFree(s->out_r);
  memset(s, 0, sizeof(*s));
}
struct PlcGuard { PlcScratch *s; ~PlcGuard() { plc_scratch_release(s); } };

// the host threads pack candidates [a, b): the 29 values as PRODFLOAT columns, Mass, and good / point folded into one byte
struct PlcPackJob {
  const char *groups; const pf_plc_group_layout *gl; const char *f_lo; size_t f_lo_stride; size_t n, pb; char *val; int *mass; unsigned char *pass;
};
static void plc_pack(void *user, size_t a, size_t b) {
  const PlcPackJob &j = *(const PlcPackJob *)user;
  const pf_plc_group_layout &gl = *j.gl;
  const long ov[8] = {gl.off_Vel, gl.off_Vel_2LPT, gl.off_Vel_3LPT_1, gl.off_Vel_3LPT_2, gl.off_Vel_prev, gl.off_Vel_2LPT_prev, gl.off_Vel_3LPT_1_prev, gl.off_Vel_3LPT_2_prev};
  for (size_t i = a; i < b; i++) {
    const char *r = j.groups + i * gl.stride;
    memcpy(&j.mass[i], r + gl.off_Mass, 4);
    int good = 1, point = 0;
    if (gl.off_good >= 0) memcpy(&good, r + gl.off_good, 4);
    if (gl.off_point >= 0) memcpy(&point, r + gl.off_point, 4);
    j.pass[i] = (point >= 0 && good) ? 1 : 0;
    for (int e = 0; e < 3; e++) memcpy(j.val + ((size_t)e * j.n + i) * j.pb, r + gl.off_Pos + e * j.pb, j.pb);
    for (int s = 0; s < 8; s++)
      for (int e = 0; e < 3; e++) {
        char *dst = j.val + ((size_t)(3 + 3 * s + e) * j.n + i) * j.pb;
        if (ov[s] >= 0) memcpy(dst, r + ov[s] + e * j.pb, j.pb);
        else memset(dst, 0, j.pb);
      }
    memcpy(j.val + ((size_t)PF_PLC_V_FLAST * j.n + i) * j.pb, r + gl.off_Flast, j.pb);
    char *dst = j.val + ((size_t)PF_PLC_V_FLO * j.n + i) * j.pb;
    if (j.f_lo) memcpy(dst, j.f_lo + i * j.f_lo_stride, j.pb);
    else memset(dst, 0, j.pb);
  }
}

static int plc_layout_check(const char *who, int rank, int pb, const pf_plc_group_layout *gl) {
  const long pl = 3 * pb;
  const long off[14] = {gl->off_Mass, gl->off_Pos, gl->off_name, gl->off_Flast, gl->off_good, gl->off_point, gl->off_Vel, gl->off_Vel_2LPT, gl->off_Vel_3LPT_1,
                        gl->off_Vel_3LPT_2, gl->off_Vel_prev, gl->off_Vel_2LPT_prev, gl->off_Vel_3LPT_1_prev, gl->off_Vel_3LPT_2_prev};
  const long len[14] = {4, pl, 8, pb, 4, 4, pl, pl, pl, pl, pl, pl, pl, pl};
  if (gl->off_Mass < 0 || gl->off_Pos < 0 || gl->off_Flast < 0) return pf_fail(rank, "%s: the group layout must name Mass, Pos and Flast", who);
  for (int k = 0; k < 14; k++)
    if (off[k] >= 0 && (size_t)off[k] + (size_t)len[k] > gl->stride)
      return pf_fail(rank, "%s: bad group layout: the field at byte %ld leaves the record of %zu bytes", who, off[k], gl->stride);
  return 0;
}

template <class T>
static int plc_device(pf_ctx *c, const PfCtxView &v, const char *who, const PfPlcState &st, const PfPlcGeom &g, const PfPlcSegIn &sg, int events, int min_mass,
                      size_t ncand, size_t capacity, PlcScratch *s, unsigned long long *count, unsigned long long *unconv, size_t *written) {
  const hipStream_t q = v.stream;
  const unsigned int nb = (unsigned int)((ncand + PF_PLC_BLOCK - 1) / PF_PLC_BLOCK);
  const int ns = st.tab_doubles < PF_PLC_LDS_DOUBLES ? st.tab_doubles : PF_PLC_LDS_DOUBLES;
  const size_t lds = (size_t)ns * 8;
  const char *env = getenv("PF_PLC_TIMES");
  const bool times = env && atoi(env) != 0;
  bool ok = hipMalloc(&s->endP, ncand * 6 * sizeof(T)) == hipSuccess && hipMalloc((void **)&s->endD, ncand * 16) == hipSuccess &&
            hipMalloc((void **)&s->counts, ncand * 4) == hipSuccess && hipMalloc((void **)&s->offs, (ncand + 1) * 8) == hipSuccess &&
            hipMalloc((void **)&s->unconv, 8) == hipSuccess && hipMalloc((void **)&s->hist, ((size_t)g.nzbins + 1) * 8) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); return pf_fail(v.rank, "%s: cannot allocate %zu bytes of scratch on the device for %zu candidates", who, ncand * (6 * sizeof(T) + 28), ncand); }
  PfPlcCand<T> cd{(const T *)s->val, s->mass, s->pass, (unsigned long long)ncand};
  PfPlcEnds<T> ends{(T *)s->endP, s->endD};
  unsigned long long npairs = 0;
  {
    PfScopedTimer kt(c, 0, (double)ncand * (PF_PLC_NVAL * sizeof(T) + 5.0 + 6 * sizeof(T) + 16 + 4), q);
    PlcStage stage(times, 0, q);
    PLCHIP(v.rank, who, hipMemsetAsync(s->unconv, 0, 8, q));
    PLCHIP(v.rank, who, hipMemsetAsync(s->hist, 0, ((size_t)g.nzbins + 1) * 8, q));
    hipLaunchKernelGGL(k_plc_ends<T>, dim3(nb), dim3(PF_PLC_BLOCK), lds, q, st.tab, st.tab_doubles, g, sg, events, min_mass, cd, ends, s->counts);
    if (hipGetLastError() != hipSuccess || pf_refresh_scan(s->counts, ncand, s->offs, q)) return pf_fail(v.rank, "%s: launch failed", who);
    PLCHIP(v.rank, who, hipMemcpyAsync(&npairs, s->offs + ncand, 8, hipMemcpyDeviceToHost, q));
    PLCHIP(v.rank, who, hipStreamSynchronize(q));
    stage.end();
  }
  *count = 0; *unconv = 0; *written = 0;
  if (!npairs) return 0;
  if (npairs > 0x7FFFFFFFull) return pf_fail(v.rank, "%s: %llu crossing pairs (2^31 - 1 at most in one call)", who, npairs);
  const size_t P = (size_t)npairs;
  ok = hipMalloc((void **)&s->pair_c, P * 4) == hipSuccess && hipMalloc((void **)&s->pair_r, P * 4) == hipSuccess && hipMalloc(&s->rec, P * 7 * sizeof(T)) == hipSuccess &&
       hipMalloc((void **)&s->ok, P * 4) == hipSuccess && hipMalloc((void **)&s->bin, P * 4) == hipSuccess && hipMalloc((void **)&s->slots, (P + 1) * 8) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); return pf_fail(v.rank, "%s: cannot allocate %zu bytes of scratch on the device for %zu crossing pairs", who, P * (24 + 7 * sizeof(T)), P); }
  const unsigned int npb = (unsigned int)((P + PF_PLC_BLOCK - 1) / PF_PLC_BLOCK);
  unsigned long long stored = 0;
  PfScopedTimer kt(c, 0, (double)P * (PF_PLC_NVAL * sizeof(T) + 24.0 + 14 * sizeof(T)), q);
  PlcStage stage(times, 1, q);
  hipLaunchKernelGGL(k_plc_list<T>, dim3(nb), dim3(PF_PLC_BLOCK), 0, q, g, events, cd, ends, s->counts, s->offs, s->pair_c, s->pair_r);
  hipLaunchKernelGGL(k_plc_root<T>, dim3(npb), dim3(PF_PLC_BLOCK), lds, q, st.tab, st.tab_doubles, g, sg, events, cd, ends, npairs, s->pair_c, s->pair_r, (T *)s->rec, s->ok,
                     s->bin, s->unconv);
  if (hipGetLastError() != hipSuccess || pf_refresh_scan(s->ok, P, s->slots, q)) return pf_fail(v.rank, "%s: launch failed", who);
  PLCHIP(v.rank, who, hipMemcpyAsync(&stored, s->slots + P, 8, hipMemcpyDeviceToHost, q));
  PLCHIP(v.rank, who, hipMemcpyAsync(unconv, s->unconv, 8, hipMemcpyDeviceToHost, q));
  PLCHIP(v.rank, who, hipStreamSynchronize(q));
  *count = stored;
  const size_t m = stored < capacity ? (size_t)stored : capacity;
  *written = m;
  if (!m) return 0;
  ok = hipMalloc(&s->out, m * 7 * sizeof(T)) == hipSuccess && hipMalloc((void **)&s->out_c, m * 4) == hipSuccess && hipMalloc((void **)&s->out_r, m * 4) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); return pf_fail(v.rank, "%s: cannot allocate %zu bytes on the device for %zu records", who, m * (8 + 7 * sizeof(T)), m); }
  hipLaunchKernelGGL(k_plc_pack<T>, dim3(npb), dim3(PF_PLC_BLOCK), 0, q, npairs, (unsigned long long)m, s->pair_c, s->pair_r, (const T *)s->rec, s->ok, s->bin, s->slots, (T *)s->out,
                     s->out_c, s->out_r, s->hist, g.nzbins);
  if (hipGetLastError() != hipSuccess) return pf_fail(v.rank, "%s: launch failed", who);
  PLCHIP(v.rank, who, hipStreamSynchronize(q));
  stage.end();
  return 0;
}

extern "C" int pf_plc_cross(pf_ctx *c, int mode, const pf_plc_segment *seg, const pf_peak_region *box, size_t ncand, const void *groups,
                            const pf_plc_group_layout *gl, const void *f_lo, size_t f_lo_stride, int min_mass, size_t capacity, void *plcgroups,
                            const pf_plc_out_layout *ol, unsigned int *cand_of, int *rep_of, double *nz, size_t *count, size_t *unconverged) {
  const char *who = "pf_plc_cross";
  if (!c) return pf_fail(0, "%s: null argument", who);
  PfCtxView v;
  pf_ctx_view(c, &v);
  if (count) *count = 0;
  if (unconverged) *unconverged = 0;
  if (!seg || !box || !gl || (ncand && !groups) || (capacity && plcgroups && !ol)) return pf_fail(v.rank, "%s: null argument", who);
  if (mode != PF_PLC_LAST_CHECK && mode != PF_PLC_EVENTS) return pf_fail(v.rank, "%s: mode %d (PF_PLC_LAST_CHECK or PF_PLC_EVENTS)", who, mode);
  const PfPlcState *st = (const PfPlcState *)*pf_ctx_plc_slot(c);
  if (!st || !st->have_cosmo) return pf_fail(v.rank, "%s: no cosmology set (pf_plc_set_cosmology)", who);
  if (!st->have_geom) return pf_fail(v.rank, "%s: no geometry set (pf_plc_set_geometry)", who);
  if (mode == PF_PLC_EVENTS && ncand && !f_lo) return pf_fail(v.rank, "%s: PF_PLC_EVENTS needs the lower end of every interval in f_lo", who);
  if (mode == PF_PLC_EVENTS && f_lo_stride < (size_t)v.pb) return pf_fail(v.rank, "%s: an f_lo stride of %zu bytes is below a PRODFLOAT of %d", who, f_lo_stride, v.pb);
  if (seg->myseg < 0) return pf_fail(v.rank, "%s: myseg = %d", who, seg->myseg);
  if (ncand > 0x7FFFFFFFull) return pf_fail(v.rank, "%s: %zu candidates (2^31 - 1 at most)", who, ncand);
  if (plc_layout_check(who, v.rank, v.pb, gl)) return 1;
  if (plcgroups && ol) {
    const long off[5] = {ol->off_Mass, ol->off_name, ol->off_z, ol->off_x, ol->off_v};
    const long len[5] = {4, 8, v.pb, 3 * v.pb, 3 * v.pb};
    for (int k = 0; k < 5; k++)
      if (off[k] >= 0 && (size_t)off[k] + (size_t)len[k] > ol->stride)
        return pf_fail(v.rank, "%s: bad output layout: the field at byte %ld leaves the record of %zu bytes", who, off[k], ol->stride);
  }
  if (!ncand) return 0;
  const void *prev = nullptr; int shifts = 0, lpt_order = 3;
  pf_ctx_prev_view(c, &prev, &shifts, &lpt_order);
  PfPlcSegIn sg;
  sg.myseg = seg->myseg; sg.use_v31 = seg->use_v31 != 0; sg.order = lpt_order < 3 ? lpt_order : 3; sg.z_seg = seg->z_seg; sg.z_prev = seg->z_prev;
  PfPlcGeom g = st->geom;
  for (int i = 0; i < 3; i++) g.stabl[i] = box->start[i];
  const int events = mode == PF_PLC_EVENTS;
  const size_t pb = (size_t)v.pb;
  PlcScratch s;
  memset(&s, 0, sizeof(s));
  PlcGuard guard{&s};
  unsigned long long found = 0, unconv = 0;
  size_t m = 0;
  {
    PfScopedTimer pt(c, 1);
    const size_t vb = ncand * PF_PLC_NVAL * pb;
    std::vector<char> hval(vb);
    std::vector<int> hmass(ncand);
    std::vector<unsigned char> hpass(ncand);
    PfHandoffView hv;
    if (pf_ctx_handoff_begin(c, &hv)) return 1;
    PlcPackJob job{(const char *)groups, gl, events ? (const char *)f_lo : nullptr, f_lo_stride, ncand, pb, hval.data(), hmass.data(), hpass.data()};
    pf_ctx_host_run(c, ncand, plc_pack, &job);
    if (hipMalloc(&s.val, vb) != hipSuccess || hipMalloc((void **)&s.mass, ncand * 4) != hipSuccess || hipMalloc((void **)&s.pass, ncand) != hipSuccess) {
      (void)hipGetLastError();
      return pf_fail(v.rank, "%s: cannot allocate %zu bytes on the device for %zu candidates", who, vb + ncand * 5, ncand);
    }
    if (pf_ctx_h2d(c, s.val, hval.data(), vb) || pf_ctx_h2d(c, s.mass, hmass.data(), ncand * 4) || pf_ctx_h2d(c, s.pass, hpass.data(), ncand)) return 1;
  }
  const int rc = v.pb == 8 ? plc_device<double>(c, v, who, *st, g, sg, events, min_mass, ncand, capacity, &s, &found, &unconv, &m)
                           : plc_device<float>(c, v, who, *st, g, sg, events, min_mass, ncand, capacity, &s, &found, &unconv, &m);
  if (rc) return 1;
  if (count) *count = (size_t)found;
  if (unconverged) *unconverged = (size_t)unconv;
  if (!m) return 0;
  std::vector<char> hout(m * 7 * pb);
  std::vector<unsigned int> hc(m);
  std::vector<int> hr(m);
  std::vector<unsigned long long> hh((size_t)g.nzbins + 1);
  if (pf_ctx_d2h(c, hout.data(), s.out, m * 7 * pb) || pf_ctx_d2h(c, hc.data(), s.out_c, m * 4) || pf_ctx_d2h(c, hr.data(), s.out_r, m * 4) ||
      pf_ctx_d2h(c, hh.data(), s.hist, ((size_t)g.nzbins + 1) * 8))
    return 1;
  if (plcgroups && ol)
    for (size_t j = 0; j < m; j++) {
      char *dst = (char *)plcgroups + j * ol->stride;
      const char *src = (const char *)groups + (size_t)hc[j] * gl->stride, *rec = hout.data() + j * 7 * pb;
      if (ol->off_Mass >= 0) memcpy(dst + ol->off_Mass, src + gl->off_Mass, 4);
      if (ol->off_name >= 0) { if (gl->off_name >= 0) memcpy(dst + ol->off_name, src + gl->off_name, 8); else memset(dst + ol->off_name, 0, 8); }
      if (ol->off_z >= 0) memcpy(dst + ol->off_z, rec, pb);
      if (ol->off_x >= 0) memcpy(dst + ol->off_x, rec + pb, 3 * pb);
      if (ol->off_v >= 0) memcpy(dst + ol->off_v, rec + 4 * pb, 3 * pb);
    }
  if (cand_of) memcpy(cand_of, hc.data(), m * 4);
  if (rep_of) memcpy(rep_of, hr.data(), m * 4);
  if (nz)
    for (int b = 0; b < g.nzbins; b++) nz[b] += (double)hh[b];
  return 0;
}
