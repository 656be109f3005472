// pf_catalog.hip -- the output step of build_groups() (src/build_groups.c:899-905) on the device: the records of write_catalog()
// (src/write_halos.c:268-318) and the two local arrays of compute_mf() (:46-65).  The arithmetic is pf_catalog_core.h, which also
// says how the mass function is binned without a log10 on the device and how far its integer sums lie from the reference's running
// sum of doubles: massinbin[b] = (double)sumMass[b] * ParticleMass differs from it by at most (n_b + 1) 2^-53 relative and does
// not depend on the order of groups[].  The spline tables are those pf_plc_set_cosmology left on the device.
//
//  k_cat_flag     one group per lane: the filter point >= 0 && good && Mass >= min_mass as a 0 / 1 flag, and the group's bin of the
//                 mass function (binary search in the thresholds), -1 where it does not count
//  (pf_refresh_scan over the flags: slot of a passing group = the passing groups before it)
//  k_cat_hist     count and 64-bit sum of Mass per bin with integer atomics; a workgroup adds up in LDS first where nbin fits
//                 PF_CAT_LDS_BINS and then adds its non-empty bins to memory
//  k_cat_records  one group per lane: a passing group whose slot is below the capacity gets its own k, the growing modes at the
//                 segment's redshifts, weights and velocity factors at F, and writes M, x, v, q as ten columns at its slot, its
//                 batch index beside them
// The order of the output is decided by the scan alone: ascending batch index.  The atomics add integers, which commute; no
// floating-point atomic anywhere.
//
// The spline tables are staged in LDS by every workgroup of k_cat_records as the light-cone kernels stage them: all of them where
// they fit PF_PLC_LDS_DOUBLES, their first PF_PLC_LDS_DOUBLES doubles otherwise; PfPlcTab::at reads the rest from memory.
//
// Every index is in range by construction: a lane works on group i < n, which sized val (27 columns of n), mass, pass, flag, bin and
// offs (n + 1); a slot is offs[i] < offs[n] = the count, and is written only below m = min(count, capacity), which sized the ten
// output columns and the index; a bin is -1 or the result of pf_cat_bin, which is below nbin, and nbin sized both histogram arrays
// (the LDS copy is used only when nbin <= PF_CAT_LDS_BINS, its size); the thresholds are nbin + 1 and the search stays inside
// [0, nbin]; a table index is below pf_plc_tab_doubles (the knot search stays inside [0, n - 1], the k-bin and the smoothing index
// are clamped in pf_plc_core.h); the staging loop copies min(total, PF_PLC_LDS_DOUBLES) doubles into an LDS array of that size.
#include <hip/hip_runtime.h>

#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "pf_internal.h"
#include "pf_catalog_core.h"

#define CATHIP(task, who, call)                                                                                        \
  do {                                                                                                                 \
    hipError_t e__ = (call);                                                                                           \
    if (e__ != hipSuccess) return pf_fail(task, "%s: %s failed: %s", who, #call, hipGetErrorString(e__));             \
  } while (0)

#define PF_CAT_HIST_PER_LANE 16   // groups a lane of k_cat_hist adds up before its workgroup flushes

// ---------------------------------------------------------------------------------------------------------- kernels ----
// group i as the kernels read it: val[k n + i], k = 0..2 Pos, 3 + 3 s + e velocity s
template <class T> struct PfCatGroups { const T *val; const int *mass; const unsigned char *pass; unsigned long long n; };

__device__ __forceinline__ PfPlcTab cat_stage(PfPlcTab t, int total, double *lds) {
  const int ns = total < PF_PLC_LDS_DOUBLES ? total : PF_PLC_LDS_DOUBLES;
  for (int i = threadIdx.x; i < ns; i += blockDim.x) lds[i] = t.g[i];
  __syncthreads();
  t.s = lds; t.ns = ns;
  return t;
}

__global__ void __launch_bounds__(PF_CAT_BLOCK)
    k_cat_flag(unsigned long long n, const int *__restrict__ mass, const unsigned char *__restrict__ pass, int min_mass, const unsigned int *__restrict__ thr, int nbin,
               unsigned int *__restrict__ flag, int *__restrict__ bin) {
  const unsigned long long i = (unsigned long long)blockIdx.x * PF_CAT_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int M = mass[i];
  const bool ok = pass[i] && M >= min_mass;
  flag[i] = ok ? 1u : 0u;
  if (bin) bin[i] = ok ? pf_cat_bin(thr, nbin, M) : -1;
}

__global__ void __launch_bounds__(PF_CAT_BLOCK)
    k_cat_hist(unsigned long long n, const int *__restrict__ mass, const int *__restrict__ bin, int nbin, unsigned int *__restrict__ cnt, unsigned long long *__restrict__ sum) {
  __shared__ unsigned int lcnt[PF_CAT_LDS_BINS];
  __shared__ unsigned long long lsum[PF_CAT_LDS_BINS];
  const bool in_lds = nbin <= PF_CAT_LDS_BINS;
  if (in_lds) {
    for (int b = threadIdx.x; b < nbin; b += PF_CAT_BLOCK) { lcnt[b] = 0u; lsum[b] = 0ull; }
    __syncthreads();
  }
  const unsigned long long base = (unsigned long long)blockIdx.x * (PF_CAT_BLOCK * PF_CAT_HIST_PER_LANE);
  for (int r = 0; r < PF_CAT_HIST_PER_LANE; r++) {
    const unsigned long long i = base + (unsigned long long)r * PF_CAT_BLOCK + threadIdx.x;
    if (i >= n) break;
    const int b = bin[i];
    if (b < 0 || b >= nbin) continue;
    const unsigned long long M = (unsigned long long)(unsigned int)mass[i];   // (a counted group has Mass >= 1)
    if (in_lds) { atomicAdd(&lcnt[b], 1u); atomicAdd(&lsum[b], M); }
    else { atomicAdd(&cnt[b], 1u); atomicAdd(&sum[b], M); }
  }
  if (in_lds) {
    __syncthreads();
    for (int b = threadIdx.x; b < nbin; b += PF_CAT_BLOCK)
      if (lcnt[b]) { atomicAdd(&cnt[b], lcnt[b]); atomicAdd(&sum[b], lsum[b]); }
  }
}

// out[(PF_CAT_NREC) m]: value k of the record in slot s at out[k m + s]; index[s] its group
template <class T>
__global__ void __launch_bounds__(PF_CAT_BLOCK)
    k_cat_records(PfPlcTab tab, int tab_doubles, PfCatGeom g, PfPlcSegIn sg, T F, PfCatGroups<T> c, const unsigned int *__restrict__ flag,
                  const unsigned long long *__restrict__ offs, unsigned long long m, T *__restrict__ out, unsigned int *__restrict__ index) {
  extern __shared__ double lds[];
  tab = cat_stage(tab, tab_doubles, lds);
  const unsigned long long i = (unsigned long long)blockIdx.x * PF_CAT_BLOCK + threadIdx.x;
  if (i >= c.n || !flag[i]) return;
  const unsigned long long slot = offs[i];
  if (slot >= m) return;
  PfPlcObj<T> o;
  o.M = c.mass[i];
#pragma unroll
  for (int e = 0; e < 3; e++) o.q[e] = c.val[(unsigned long long)e * c.n + i];
#pragma unroll
  for (int s = 0; s < 8; s++)
#pragma unroll
    for (int e = 0; e < 3; e++) o.v[s][e] = c.val[(unsigned long long)(3 + 3 * s + e) * c.n + i];
  const PfPlcK k = pf_plc_group_k<T>(tab, o.M, g.ipd);
  const PfPlcSeg s = pf_plc_segment_modes(tab, sg, k);
  T rec[PF_CAT_NREC];
  pf_cat_record<T>(tab, g, sg, k, s, o, F, rec);
#pragma unroll
  for (int q = 0; q < PF_CAT_NREC; q++) out[(unsigned long long)q * m + slot] = rec[q];
  index[slot] = (unsigned int)i;
}

// PF_CATALOG_TIMES=1: device ms of the last call's flag + scan passes and of its record + histogram passes (profiles/tools/catalog_time.py)
static double cat_last_ms[2] = {0.0, 0.0};
struct CatStage {
  hipEvent_t a, b; hipStream_t st; int which; bool on;
  CatStage(bool on_, int which_, hipStream_t st_) : a(nullptr), b(nullptr), st(st_), which(which_), on(on_) {
    if (on) on = hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess && hipEventRecord(a, st) == hipSuccess;
  }
  void end() {
    float ms = 0.0f;
    if (on && hipEventRecord(b, st) == hipSuccess && hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&ms, a, b) == hipSuccess) cat_last_ms[which] = ms;
    on = false;
  }
  ~CatStage() { end(); if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); }
};
extern "C" int pf_debug_catalog_times(double *ms2) {
  if (!ms2) return 1;
  ms2[0] = cat_last_ms[0]; ms2[1] = cat_last_ms[1];
  return 0;
}
// ... and the host's wall ms of the same call's parts: pack (thresholds included), upload, device (allocations and waits included), download + records
static double cat_part_ms[4] = {0.0, 0.0, 0.0, 0.0};
extern "C" int pf_debug_catalog_parts(double *ms4) {
  if (!ms4) return 1;
  for (int k = 0; k < 4; k++) ms4[k] = cat_part_ms[k];
  return 0;
}
struct CatClock {
  std::chrono::steady_clock::time_point t0;
  CatClock() : t0(std::chrono::steady_clock::now()) {}
  void lap(int which) {
    const auto t1 = std::chrono::steady_clock::now();
    cat_part_ms[which] = std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
  }
};

// ------------------------------------------------------------------------------------------------------ the call ----
struct CatScratch {
  void *val; int *mass; unsigned char *pass; unsigned int *thr, *flag; int *bin; unsigned long long *offs; unsigned int *cnt; unsigned long long *sum;
  void *out; unsigned int *index;
};
static void cat_scratch_release(CatScratch *s) {
  hipFree(s->val); hipFree(s->mass); hipFree(s->pass); hipFree(s->thr); hipFree(s->flag); hipFree(s->bin); hipFree(s->offs); hipFree(s->cnt); hipFree(s->sum);
  hipFree(s->out); hipFree(s->index);
  memset(s, 0, sizeof(*s));
}
struct CatGuard { CatScratch *s; ~CatGuard() { cat_scratch_release(s); } };

// the host threads pack groups [a, b): the 27 values as PRODFLOAT columns, Mass, and good / point folded into one byte
struct CatPackJob { const char *groups; const pf_plc_group_layout *gl; size_t n, pb; char *val; int *mass; unsigned char *pass; };
static void cat_pack(void *user, size_t a, size_t b) {
  const CatPackJob &j = *(const CatPackJob *)user;
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
  }
}

static int cat_layout_check(const char *who, int rank, int pb, const pf_plc_group_layout *gl) {
  const long pl = 3 * pb;
  const long off[14] = {gl->off_Mass, gl->off_Pos, gl->off_name, gl->off_Flast, gl->off_good, gl->off_point, gl->off_Vel, gl->off_Vel_2LPT, gl->off_Vel_3LPT_1,
                        gl->off_Vel_3LPT_2, gl->off_Vel_prev, gl->off_Vel_2LPT_prev, gl->off_Vel_3LPT_1_prev, gl->off_Vel_3LPT_2_prev};
  const long len[14] = {4, pl, 8, pb, 4, 4, pl, pl, pl, pl, pl, pl, pl, pl};
  if (gl->off_Mass < 0 || gl->off_Pos < 0) return pf_fail(rank, "%s: the group layout must name Mass and Pos", who);
  for (int k = 0; k < 14; k++)
    if (off[k] >= 0 && (size_t)off[k] + (size_t)len[k] > gl->stride)
      return pf_fail(rank, "%s: bad group layout: the field at byte %ld leaves the record of %zu bytes", who, off[k], gl->stride);
  return 0;
}

template <class T>
static int cat_device(pf_ctx *c, const PfCtxView &v, const char *who, const PfPlcTab &tab, int tab_doubles, const PfCatGeom &g, const PfPlcSegIn &sg, double F, int min_mass,
                      size_t n, size_t capacity, int nbin, CatScratch *s, unsigned long long *count, size_t *written) {
  const hipStream_t q = v.stream;
  const unsigned int nb = (unsigned int)((n + PF_CAT_BLOCK - 1) / PF_CAT_BLOCK);
  const int ns = tab_doubles < PF_PLC_LDS_DOUBLES ? tab_doubles : PF_PLC_LDS_DOUBLES;
  const char *env = getenv("PF_CATALOG_TIMES");
  const bool times = env && atoi(env) != 0;
  bool ok = hipMalloc((void **)&s->flag, n * 4) == hipSuccess && hipMalloc((void **)&s->offs, (n + 1) * 8) == hipSuccess;
  if (ok && nbin > 0)
    ok = hipMalloc((void **)&s->bin, n * 4) == hipSuccess && hipMalloc((void **)&s->cnt, (size_t)nbin * 4) == hipSuccess && hipMalloc((void **)&s->sum, (size_t)nbin * 8) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); return pf_fail(v.rank, "%s: cannot allocate %zu bytes of scratch on the device for %zu groups", who, n * 16 + (size_t)nbin * 12, n); }
  unsigned long long found = 0;
  {
    PfScopedTimer kt(c, 0, (double)n * (5.0 + 4 + 4 + 12), q);
    CatStage stage(times, 0, q);
    hipLaunchKernelGGL(k_cat_flag, dim3(nb), dim3(PF_CAT_BLOCK), 0, q, (unsigned long long)n, s->mass, s->pass, min_mass, s->thr, nbin, s->flag, s->bin);
    if (hipGetLastError() != hipSuccess || pf_refresh_scan(s->flag, n, s->offs, q)) return pf_fail(v.rank, "%s: launch failed", who);
    CATHIP(v.rank, who, hipMemcpyAsync(&found, s->offs + n, 8, hipMemcpyDeviceToHost, q));
    CATHIP(v.rank, who, hipStreamSynchronize(q));
    stage.end();
  }
  *count = found;
  const size_t m = found < capacity ? (size_t)found : capacity;
  *written = m;
  if (m) {
    ok = hipMalloc(&s->out, m * PF_CAT_NREC * sizeof(T)) == hipSuccess && hipMalloc((void **)&s->index, m * 4) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); return pf_fail(v.rank, "%s: cannot allocate %zu bytes on the device for %zu records", who, m * (4 + PF_CAT_NREC * sizeof(T)), m); }
  }
  if (!m && nbin <= 0) return 0;
  PfScopedTimer kt(c, 0, (double)n * 8.0 + (double)m * ((PF_CAT_NVAL + PF_CAT_NREC) * sizeof(T) + 8.0), q);
  CatStage stage(times, 1, q);
  if (nbin > 0) {
    CATHIP(v.rank, who, hipMemsetAsync(s->cnt, 0, (size_t)nbin * 4, q));
    CATHIP(v.rank, who, hipMemsetAsync(s->sum, 0, (size_t)nbin * 8, q));
    const size_t per = (size_t)PF_CAT_BLOCK * PF_CAT_HIST_PER_LANE;
    hipLaunchKernelGGL(k_cat_hist, dim3((unsigned int)((n + per - 1) / per)), dim3(PF_CAT_BLOCK), 0, q, (unsigned long long)n, s->mass, s->bin, nbin, s->cnt, s->sum);
  }
  if (m) {
    PfCatGroups<T> cd{(const T *)s->val, s->mass, s->pass, (unsigned long long)n};
    hipLaunchKernelGGL(k_cat_records<T>, dim3(nb), dim3(PF_CAT_BLOCK), (size_t)ns * 8, q, tab, tab_doubles, g, sg, (T)F, cd, s->flag, s->offs, (unsigned long long)m, (T *)s->out,
                       s->index);
  }
  if (hipGetLastError() != hipSuccess) return pf_fail(v.rank, "%s: launch failed", who);
  CATHIP(v.rank, who, hipStreamSynchronize(q));
  stage.end();
  return 0;
}

extern "C" int pf_catalog(pf_ctx *c, const pf_plc_segment *seg, const pf_peak_region *box, const pf_catalog_params *par, size_t ngroups, const void *groups,
                          const pf_plc_group_layout *gl, size_t capacity, void *catalog, const pf_catalog_out_layout *ol, unsigned int *group_of, const pf_mf_bins *bins,
                          int *ninbin, double *massinbin, size_t *count) {
  const char *who = "pf_catalog";
  if (count) *count = 0;
  if (!c) return pf_fail(0, "%s: null argument", who);
  PfCtxView v;
  pf_ctx_view(c, &v);
  if (!seg || !box || !par || !gl || (ngroups && !groups) || (capacity && catalog && !ol) || (bins && bins->nbin > 0 && (!ninbin || !massinbin))) return pf_fail(v.rank, "%s: null argument", who);
  PfPlcTab tab;
  int tab_doubles = 0;
  if (!pf_plc_tables(c, &tab, &tab_doubles)) return pf_fail(v.rank, "%s: no cosmology set (pf_plc_set_cosmology)", who);
  if (seg->myseg < 0) return pf_fail(v.rank, "%s: myseg = %d", who, seg->myseg);
  if (!(par->F > 0.0) || par->F - par->F != 0.0) return pf_fail(v.rank, "%s: F = %g must be finite and positive", who, par->F);
  if (!(par->InterPartDist > 0.0) || !(par->hfactor > 0.0))
    return pf_fail(v.rank, "%s: InterPartDist = %g and hfactor = %g must be positive", who, par->InterPartDist, par->hfactor);
  const int nbin = bins ? bins->nbin : 0;
  if (bins) {
    if (nbin < 0 || nbin > (1 << 20)) return pf_fail(v.rank, "%s: a mass function of %d bins (0 to 2^20)", who, nbin);
    if (!(par->ParticleMass > 0.0) || !(bins->deltam > 0.0) || bins->mmin - bins->mmin != 0.0)
      return pf_fail(v.rank, "%s: ParticleMass = %g and deltam = %g must be positive and mmin = %g finite for the mass function", who, par->ParticleMass, bins->deltam, bins->mmin);
  }
  for (int i = 0; i < 3; i++)
    if (box->len[i] <= 0 || par->GSglobal[i] <= 0)
      return pf_fail(v.rank, "%s: len[%d] = %d and GSglobal[%d] = %lld must be positive", who, i, box->len[i], i, par->GSglobal[i]);
  if (ngroups > 0x7FFFFFFFull) return pf_fail(v.rank, "%s: %zu groups (2^31 - 1 at most)", who, ngroups);
  if (cat_layout_check(who, v.rank, v.pb, gl)) return 1;
  if (catalog && ol) {
    const long off[6] = {ol->off_name, ol->off_M, ol->off_x, ol->off_v, ol->off_q, ol->off_n};
    const long len[6] = {8, v.pb, 3 * v.pb, 3 * v.pb, 3 * v.pb, 4};
    for (int k = 0; k < 6; k++)
      if (off[k] >= 0 && (size_t)off[k] + (size_t)len[k] > ol->stride)
        return pf_fail(v.rank, "%s: bad output layout: the field at byte %ld leaves the record of %zu bytes", who, off[k], ol->stride);
  }
  for (int b = 0; b < nbin; b++) { ninbin[b] = 0; massinbin[b] = 0.0; }
  if (!ngroups) return 0;
  const void *prev = nullptr; int shifts = 0, lpt_order = 3;
  pf_ctx_prev_view(c, &prev, &shifts, &lpt_order);
  PfPlcSegIn sg;
  sg.myseg = seg->myseg; sg.use_v31 = seg->use_v31 != 0; sg.order = lpt_order < 3 ? lpt_order : 3; sg.z_seg = seg->z_seg; sg.z_prev = seg->z_prev;
  PfCatGeom g;
  for (int i = 0; i < 3; i++) { g.ggrid[i] = (double)par->GSglobal[i]; g.box[i] = (double)box->len[i]; g.stabl[i] = (double)box->start[i]; g.pbc[i] = par->pbc[i] != 0; }
  g.scale = par->InterPartDist * par->hfactor; g.ipd = par->InterPartDist; g.pmass = par->ParticleMass; g.hfactor = par->hfactor;
  const size_t pb = (size_t)v.pb, n = ngroups;
  CatScratch s;
  memset(&s, 0, sizeof(s));
  CatGuard guard{&s};
  CatClock clock;
  {
    PfScopedTimer pt(c, 1);
    const size_t vb = n * PF_CAT_NVAL * pb;
    std::vector<char> hval(vb);
    std::vector<int> hmass(n);
    std::vector<unsigned char> hpass(n);
    std::vector<unsigned int> hthr((size_t)nbin + 1);
    if (nbin > 0) pf_cat_thresholds(bins->mmin, bins->deltam, nbin, par->ParticleMass, hthr.data());
    PfHandoffView hv;
    if (pf_ctx_handoff_begin(c, &hv)) return 1;
    CatPackJob job{(const char *)groups, gl, n, pb, hval.data(), hmass.data(), hpass.data()};
    pf_ctx_host_run(c, n, cat_pack, &job);
    clock.lap(0);
    if (hipMalloc(&s.val, vb) != hipSuccess || hipMalloc((void **)&s.mass, n * 4) != hipSuccess || hipMalloc((void **)&s.pass, n) != hipSuccess ||
        hipMalloc((void **)&s.thr, ((size_t)nbin + 1) * 4) != hipSuccess) {
      (void)hipGetLastError();
      return pf_fail(v.rank, "%s: cannot allocate %zu bytes on the device for %zu groups", who, vb + n * 5 + ((size_t)nbin + 1) * 4, n);
    }
    if (pf_ctx_h2d(c, s.val, hval.data(), vb) || pf_ctx_h2d(c, s.mass, hmass.data(), n * 4) || pf_ctx_h2d(c, s.pass, hpass.data(), n)) return 1;
    if (nbin > 0 && pf_ctx_h2d(c, s.thr, hthr.data(), ((size_t)nbin + 1) * 4)) return 1;
    clock.lap(1);
  }
  // F as set_obj takes it: outputs.F[iout] rounded to PRODFLOAT
  unsigned long long found = 0;
  size_t m = 0;
  const int rc = v.pb == 8 ? cat_device<double>(c, v, who, tab, tab_doubles, g, sg, par->F, par->min_mass, n, capacity, nbin, &s, &found, &m)
                           : cat_device<float>(c, v, who, tab, tab_doubles, g, sg, par->F, par->min_mass, n, capacity, nbin, &s, &found, &m);
  if (rc) return 1;
  clock.lap(2);
  cat_part_ms[3] = 0.0;
  if (nbin > 0) {
    std::vector<unsigned int> hc((size_t)nbin);
    std::vector<unsigned long long> hs((size_t)nbin);
    if (pf_ctx_d2h(c, hc.data(), s.cnt, (size_t)nbin * 4) || pf_ctx_d2h(c, hs.data(), s.sum, (size_t)nbin * 8)) return 1;
    for (int b = 0; b < nbin; b++) { ninbin[b] = (int)hc[b]; massinbin[b] = (double)hs[b] * par->ParticleMass; }
  }
  if (count) *count = (size_t)found;
  if (!m) return 0;
  std::vector<char> hout(m * PF_CAT_NREC * pb);
  std::vector<unsigned int> hi(m);
  if (pf_ctx_d2h(c, hout.data(), s.out, m * PF_CAT_NREC * pb) || pf_ctx_d2h(c, hi.data(), s.index, m * 4)) return 1;
  if (catalog && ol) {
    const long dst_off[4] = {ol->off_M, ol->off_x, ol->off_v, ol->off_q};
    const int first[4] = {0, 1, 4, 7}, nval[4] = {1, 3, 3, 3};
    for (size_t j = 0; j < m; j++) {
      char *dst = (char *)catalog + j * ol->stride;
      const char *src = (const char *)groups + (size_t)hi[j] * gl->stride;
      if (ol->off_name >= 0) { if (gl->off_name >= 0) memcpy(dst + ol->off_name, src + gl->off_name, 8); else memset(dst + ol->off_name, 0, 8); }
      if (ol->off_n >= 0) memcpy(dst + ol->off_n, src + gl->off_Mass, 4);
      for (int f = 0; f < 4; f++)
        if (dst_off[f] >= 0)
          for (int e = 0; e < nval[f]; e++) memcpy(dst + dst_off[f] + e * pb, hout.data() + ((size_t)(first[f] + e) * m + j) * pb, pb);
    }
  }
  if (group_of) memcpy(group_of, hi.data(), m * 4);
  clock.lap(3);
  return 0;
}
