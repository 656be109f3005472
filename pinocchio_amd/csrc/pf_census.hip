// pf_census.hip -- the flavour census (include/pinfmax.h: pf_flavour_census, pf_debug_census): one streaming pass over the Fmax and
// Rmax columns of the fast and of the exact flavour of the collapse solve -- 16 bytes per cell with float products, 24 with double
// ones --, classified per cell by pf_census_core.h.  The sweeps that fill the columns are pf_api.hip's; this file holds the kernels
// and the tap on a caller's columns.
//
//  k_census_count    a grid of at most PF_CENSUS_MAXWG workgroups; workgroup b takes the tiles [b tpw, (b + 1) tpw) of
//                    PF_CENSUS_TILE consecutive cells, thread t of a tile its cells 4 t .. 4 t + 3: one 16-byte load per Rmax
//                    column and one (float) or two (double) per Fmax column where the whole group of four lies below `count`,
//                    single loads in the tail group (the columns are allocations of their own, so 16-byte aligned).  Counting is by
//                    wave: a ballot and a population count per common bin (0..3) and per flag, in scalar registers; the rare bins
//                    (>= 4) go one distinct bin at a time -- ballot of the lanes that share the first lane's bin -- into the wave's
//                    own row of an LDS table, written by lane 0 alone.  The maxima travel per lane as (d, cell) and u, are reduced
//                    by shuffles with the tie rule "lower cell" and leave as one partial per workgroup.  Workgroup b writes entry b
//                    of every column of the partial counts: PF_CENSUS_NCNT 64-bit integers and its outliers (bins >= 3 + nonfinite).
//  k_census_final    one workgroup: the sums of the columns (a column per wave, contiguous reads), the reduction of the partial
//                    maxima with the same tie rule, the exclusive scan of the workgroups' outlier counts, the pf_census itself.
//  k_census_records  the same walk once more, by the workgroups whose outliers begin below the capacity: the rank of an outlier
//                    inside its tile from four ballots (the cells of lane l come before those of lane l + 1), the waves' totals
//                    through LDS, the running count of the workgroup on top of its scanned offset; a record is written, as two
//                    16-byte stores, when its slot is below the capacity.  Ascending cell index by construction.
// No atomics of any kind: every sum is of integers, every partial has one writer, and the maxima are decided by comparisons with a
// total order -- the result does not depend on the schedule.  Cell indices and counts are 64 bits throughout.
//
// Every index is in range by construction: a load reads elements i .. i + 3 only when i + 4 <= count and single elements only below
// count; entry b of a column of the partials is written by workgroup b < grid, the grid that sized them; the LDS rows are indexed by
// the wave (< PF_CENSUS_WAVES) and by a bin that pf_census_bin holds to [0, PF_CENSUS_NBIN); k_census_final reads entries below the
// grid of the PF_CENSUS_NCNT + 1 columns and writes offs[0 .. grid]; a record slot is below min(outliers, capacity), which sized the record array.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include "pf_internal.h"
#include "pf_census_core.h"

static_assert(PF_CENSUS_NBIN == PF_CENSUS_BINS, "the bins of the core header are those of the interface");
static_assert(sizeof(pf_census_cell) == 32, "a record is two 16-byte pieces");

#define CNHIP(task, who, call)                                                                                         \
  do {                                                                                                                 \
    hipError_t e__ = (call);                                                                                           \
    if (e__ != hipSuccess) return pf_fail(task, "%s: %s failed: %s", who, #call, hipGetErrorString(e__));             \
  } while (0)

#define PF_CENSUS_BLOCK 256
#define PF_CENSUS_WAVES (PF_CENSUS_BLOCK / 64)
#define PF_CENSUS_TILE (4 * PF_CENSUS_BLOCK)     // cells of a tile: four per thread
#define PF_CENSUS_MAXWG 2048                     // workgroups of the grid at most: eight per CU
#define PF_CENSUS_NCNT (PF_CENSUS_NBIN + 3)      // the bins, then differing_bits, rmax_differing, nonfinite
// the partial counts: [PF_CENSUS_NCNT + 1][workgroups] -- a column per count, and CN_OUT, the outliers of each workgroup
enum { CN_DIFF = PF_CENSUS_NBIN, CN_RDIFF = PF_CENSUS_NBIN + 1, CN_NONFIN = PF_CENSUS_NBIN + 2, CN_OUT = PF_CENSUS_NCNT };

typedef unsigned long long u64;

template <class PR> struct CensusCols { const PR *ff, *fe; const int *rf, *re; };
struct CensusWalk { u64 first_cell, count, ntiles, tiles_per_wg; };

// the four cells i .. i + 3 of a thread (i a multiple of four) -> how many of them lie below count; the rest read as zeros
template <class PR>
__device__ __forceinline__ int census_load(const CensusCols<PR> &c, u64 i, u64 count, PR f[4], PR e[4], int rf[4], int re[4]) {
  const u64 left = i < count ? count - i : 0;
  if (left >= 4) {
    const int4 a = *(const int4 *)(c.rf + i), b = *(const int4 *)(c.re + i);
    rf[0] = a.x; rf[1] = a.y; rf[2] = a.z; rf[3] = a.w;
    re[0] = b.x; re[1] = b.y; re[2] = b.z; re[3] = b.w;
    if constexpr (sizeof(PR) == 4) {
      const float4 x = *(const float4 *)(c.ff + i), y = *(const float4 *)(c.fe + i);
      f[0] = x.x; f[1] = x.y; f[2] = x.z; f[3] = x.w;
      e[0] = y.x; e[1] = y.y; e[2] = y.z; e[3] = y.w;
    } else {
      const double2 x0 = *(const double2 *)(c.ff + i), x1 = *(const double2 *)(c.ff + i + 2);
      const double2 y0 = *(const double2 *)(c.fe + i), y1 = *(const double2 *)(c.fe + i + 2);
      f[0] = x0.x; f[1] = x0.y; f[2] = x1.x; f[3] = x1.y;
      e[0] = y0.x; e[1] = y0.y; e[2] = y1.x; e[3] = y1.y;
    }
    return 4;
  }
  const int nv = left < 4 ? (int)left : 4;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const bool on = j < nv;
    f[j] = on ? c.ff[i + j] : (PR)0; e[j] = on ? c.fe[i + j] : (PR)0;
    rf[j] = on ? c.rf[i + j] : 0; re[j] = on ? c.re[i + j] : 0;
  }
  return nv;
}

// (d, cell) ordered by larger d, then lower cell: a total order, so that any reduction tree gives the same winner
__device__ __forceinline__ void census_better(double &d, u64 &cell, double od, u64 ocell) {
  if (od > d || (od == d && ocell < cell)) { d = od; cell = ocell; }
}

template <class PR>
__global__ void __launch_bounds__(PF_CENSUS_BLOCK)
    k_census_count(CensusCols<PR> c, CensusWalk w, u64 *__restrict__ partials, double *__restrict__ maxpart, u64 *__restrict__ maxcell) {
  __shared__ u64 rows[PF_CENSUS_WAVES][PF_CENSUS_NCNT];
  __shared__ double smax[PF_CENSUS_WAVES][2];
  __shared__ u64 scell[PF_CENSUS_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = threadIdx.x; k < PF_CENSUS_WAVES * PF_CENSUS_NCNT; k += PF_CENSUS_BLOCK) (&rows[0][0])[k] = 0;
  __syncthreads();
  u64 h0 = 0, h1 = 0, h2 = 0, h3 = 0, nd = 0, nr = 0, nn = 0;   // the same in every lane of a wave
  double bd = -1.0, bu = -1.0;                                // -1: no finite cell yet
  u64 bc = ~0ull;
  const u64 t0 = (u64)blockIdx.x * w.tiles_per_wg, t1 = t0 + w.tiles_per_wg < w.ntiles ? t0 + w.tiles_per_wg : w.ntiles;
  for (u64 tile = t0; tile < t1; tile++) {
    const u64 i = tile * PF_CENSUS_TILE + 4ull * threadIdx.x;
    PR f[4], e[4];
    int rf[4], re[4];
    const int nv = census_load<PR>(c, i, w.count, f, e, rf, re);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const bool on = j < nv;
      const PfCensusCell q = pf_census_classify<PR>(f[j], e[j], rf[j], re[j]);
      const int bin = on ? q.bin : -2;
      h0 += __popcll(__ballot(bin == 0)); h1 += __popcll(__ballot(bin == 1));
      h2 += __popcll(__ballot(bin == 2)); h3 += __popcll(__ballot(bin == 3));
      nd += __popcll(__ballot(on && q.differ)); nr += __popcll(__ballot(on && q.rdiffer)); nn += __popcll(__ballot(bin == -1));
      u64 rare = __ballot(bin >= 4);
      while (rare) {   // one distinct bin per turn
        const int bk = __shfl(bin, __ffsll((long long)rare) - 1);
        const u64 m = __ballot(bin == bk);
        if (lane == 0) rows[wave][bk] += (u64)__popcll(m);
        rare &= ~m;
      }
      if (bin >= 0) {   // the cells of a thread ascend: a later one wins only when it is larger
        if (q.d > bd) { bd = q.d; bc = w.first_cell + i + j; }
        if (q.u > bu) bu = q.u;
      }
    }
  }
  if (lane == 0) {
    rows[wave][0] += h0; rows[wave][1] += h1; rows[wave][2] += h2; rows[wave][3] += h3;
    rows[wave][CN_DIFF] = nd; rows[wave][CN_RDIFF] = nr; rows[wave][CN_NONFIN] = nn;
  }
  for (int off = 32; off; off >>= 1) {
    const double od = __shfl_xor(bd, off), ou = __shfl_xor(bu, off);
    const u64 oc = __shfl_xor(bc, off);
    census_better(bd, bc, od, oc);
    if (ou > bu) bu = ou;
  }
  if (lane == 0) { smax[wave][0] = bd; smax[wave][1] = bu; scell[wave] = bc; }
  __syncthreads();
  for (int k = threadIdx.x; k < PF_CENSUS_NCNT; k += PF_CENSUS_BLOCK) {
    u64 s = 0;
#pragma unroll
    for (int v = 0; v < PF_CENSUS_WAVES; v++) s += rows[v][k];
    partials[(u64)k * gridDim.x + blockIdx.x] = s;
  }
  if (threadIdx.x == PF_CENSUS_BLOCK - 1) {   // the outliers of this workgroup, what k_census_final scans
    u64 o = 0;
    for (int v = 0; v < PF_CENSUS_WAVES; v++) {
      for (int q = 3; q < PF_CENSUS_NBIN; q++) o += rows[v][q];
      o += rows[v][CN_NONFIN];
    }
    partials[(u64)CN_OUT * gridDim.x + blockIdx.x] = o;
  }
  if (threadIdx.x == 0) {
    for (int v = 1; v < PF_CENSUS_WAVES; v++) {
      census_better(bd, bc, smax[v][0], scell[v]);
      if (smax[v][1] > bu) bu = smax[v][1];
    }
    maxpart[2 * blockIdx.x] = bd; maxpart[2 * blockIdx.x + 1] = bu; maxcell[blockIdx.x] = bc;
  }
}

// one workgroup of PF_CENSUS_BLOCK threads; nwg <= PF_CENSUS_MAXWG
__global__ void __launch_bounds__(PF_CENSUS_BLOCK)
    k_census_final(const u64 *__restrict__ partials, const double *__restrict__ maxpart, const u64 *__restrict__ maxcell, int nwg, u64 count, pf_census *__restrict__ out,
                   u64 *__restrict__ offs) {
  constexpr int PER = PF_CENSUS_MAXWG / PF_CENSUS_BLOCK;   // workgroups a thread scans
  __shared__ u64 tot[PF_CENSUS_NCNT];
  __shared__ u64 scan[PF_CENSUS_BLOCK];
  __shared__ double sd[PF_CENSUS_BLOCK], su[PF_CENSUS_BLOCK];
  __shared__ u64 sc[PF_CENSUS_BLOCK];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int k = wave; k < PF_CENSUS_NCNT; k += PF_CENSUS_WAVES) {   // a column per wave: contiguous reads, an integer sum by shuffles
    u64 s = 0;
    for (int b = lane; b < nwg; b += 64) s += partials[(u64)k * nwg + b];
    for (int off = 32; off; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) tot[k] = s;
  }
  // outliers of the workgroups PER t .. PER t + PER - 1, then the scan over the threads
  u64 mine[PER], sum = 0;
#pragma unroll
  for (int k = 0; k < PER; k++) {
    const int b = PER * t + k;
    const u64 o = b < nwg ? partials[(u64)CN_OUT * nwg + b] : 0;
    mine[k] = o; sum += o;
  }
  scan[t] = sum;
  double bd = -1.0, bu = -1.0;
  u64 bc = ~0ull;
  for (int b = t; b < nwg; b += PF_CENSUS_BLOCK) {
    census_better(bd, bc, maxpart[2 * b], maxcell[b]);
    if (maxpart[2 * b + 1] > bu) bu = maxpart[2 * b + 1];
  }
  sd[t] = bd; su[t] = bu; sc[t] = bc;
  __syncthreads();
  for (int off = 1; off < PF_CENSUS_BLOCK; off <<= 1) {   // inclusive scan
    const u64 add = t >= off ? scan[t - off] : 0;
    __syncthreads();
    scan[t] += add;
    __syncthreads();
  }
  u64 run = scan[t] - sum;
#pragma unroll
  for (int k = 0; k < PER; k++) {
    const int b = PER * t + k;
    if (b < nwg) offs[b] = run;
    run += mine[k];
  }
  for (int off = PF_CENSUS_BLOCK / 2; off; off >>= 1) {
    if (t < off) {
      census_better(sd[t], sc[t], sd[t + off], sc[t + off]);
      if (su[t + off] > su[t]) su[t] = su[t + off];
    }
    __syncthreads();
  }
  if (t == 0) {
    const u64 total = scan[PF_CENSUS_BLOCK - 1];
    offs[nwg] = total;
    u64 beyond = 0;
    for (int q = 0; q < PF_CENSUS_NBIN; q++) {
      out->hist[q] = tot[q];
      if (q >= 3) beyond += tot[q];
    }
    out->cells = count;
    out->differing_bits = tot[CN_DIFF]; out->rmax_differing = tot[CN_RDIFF]; out->nonfinite = tot[CN_NONFIN];
    out->beyond_2ulp = beyond; out->outliers = total;
    const bool any = sd[0] >= 0.0;   // a cell that is not nonfinite exists
    out->max_abs = any ? sd[0] : 0.0; out->max_ulps = any ? su[0] : 0.0; out->max_abs_cell = sc[0];
  }
}

template <class PR>
__global__ void __launch_bounds__(PF_CENSUS_BLOCK)
    k_census_records(CensusCols<PR> c, CensusWalk w, const u64 *__restrict__ offs, u64 cap, pf_census_cell *__restrict__ rec) {
  __shared__ unsigned int wtot[PF_CENSUS_WAVES];
  const u64 og = offs[blockIdx.x], end = offs[blockIdx.x + 1];
  if (end == og || og >= cap) return;   // (the whole workgroup)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 below = lane ? ~0ull >> (64 - lane) : 0;   // the lanes before this one
  u64 run = og;
  const u64 t0 = (u64)blockIdx.x * w.tiles_per_wg, t1 = t0 + w.tiles_per_wg < w.ntiles ? t0 + w.tiles_per_wg : w.ntiles;
  for (u64 tile = t0; tile < t1 && run < end && run < cap; tile++) {   // (run is the same in every thread)
    const u64 i = tile * PF_CENSUS_TILE + 4ull * threadIdx.x;
    PR f[4], e[4];
    int rf[4], re[4];
    const int nv = census_load<PR>(c, i, w.count, f, e, rf, re);
    bool o[4];
    unsigned int before = 0, total = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      o[j] = j < nv && pf_census_classify<PR>(f[j], e[j], rf[j], re[j]).outlier;
      const u64 m = __ballot(o[j]);
      before += (unsigned int)__popcll(m & below); total += (unsigned int)__popcll(m);
    }
    if (lane == 0) wtot[wave] = total;
    __syncthreads();
    u64 slot = run + before, all = 0;
#pragma unroll
    for (int v = 0; v < PF_CENSUS_WAVES; v++) {
      if (v < wave) slot += wtot[v];
      all += wtot[v];
    }
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (o[j]) {
        if (slot < cap) {
          pf_census_cell r;
          r.cell = w.first_cell + i + j; r.fast = (double)f[j]; r.exact = (double)e[j]; r.rmax_fast = rf[j]; r.rmax_exact = re[j];
          uint4 p[2];
          __builtin_memcpy(p, &r, 32);
          uint4 *dst = (uint4 *)(rec + slot);   // 32 slot bytes behind a base that hipMalloc aligned
          dst[0] = p[0]; dst[1] = p[1];
        }
        slot++;
      }
    __syncthreads();   // wtot is rewritten by the next tile
    run += all;
  }
}

// ------------------------------------------------------------------------------------------------------------ launches ----
struct CensusScratch { u64 *partials, *maxcell, *offs; double *maxpart; pf_census *out; pf_census_cell *rec; };
struct CensusGuard {
  CensusScratch *s;
  ~CensusGuard() { hipFree(s->partials); hipFree(s->maxcell); hipFree(s->offs); hipFree(s->maxpart); hipFree(s->out); hipFree(s->rec); memset(s, 0, sizeof(*s)); }
};

template <class PR>
static int census_count(const CensusCols<PR> &c, const CensusWalk &w, int nwg, const CensusScratch &s, hipStream_t st) {
  hipLaunchKernelGGL((k_census_count<PR>), dim3(nwg), dim3(PF_CENSUS_BLOCK), 0, st, c, w, s.partials, s.maxpart, s.maxcell);
  return hipGetLastError() != hipSuccess;
}
template <class PR>
static int census_records(const CensusCols<PR> &c, const CensusWalk &w, int nwg, const CensusScratch &s, u64 cap, hipStream_t st) {
  hipLaunchKernelGGL((k_census_records<PR>), dim3(nwg), dim3(PF_CENSUS_BLOCK), 0, st, c, w, s.offs, cap, s.rec);
  return hipGetLastError() != hipSuccess;
}

// the census of four columns that lie on the device; synchronises the stream twice (the outlier count sizes the record array)
int pf_census_device(const char *who, int task, int pb, unsigned long long first_cell, size_t count, const void *fmax_fast, const int *rmax_fast,
                     const void *fmax_exact, const int *rmax_exact, pf_census *out, size_t capacity, pf_census_cell *cells, hipStream_t st) {
  memset(out, 0, sizeof(*out));
  out->max_abs_cell = ~0ull;
  if (!count) return 0;
  CensusWalk w;
  w.first_cell = first_cell; w.count = count;
  w.ntiles = ((u64)count + PF_CENSUS_TILE - 1) / PF_CENSUS_TILE;
  w.tiles_per_wg = (w.ntiles + PF_CENSUS_MAXWG - 1) / PF_CENSUS_MAXWG;
  const int nwg = (int)((w.ntiles + w.tiles_per_wg - 1) / w.tiles_per_wg);   // 1 .. PF_CENSUS_MAXWG
  // (every caller's columns are allocations of their own: hipMalloc aligns them far beyond the 16 bytes the loads need)
  if (((uintptr_t)fmax_fast | (uintptr_t)fmax_exact | (uintptr_t)rmax_fast | (uintptr_t)rmax_exact) & 15) return pf_fail(task, "%s: a column is not 16-byte aligned (internal error)", who);
  CensusScratch s;
  memset(&s, 0, sizeof(s));
  CensusGuard guard{&s};
  const size_t pbytes = (size_t)nwg * (PF_CENSUS_NCNT + 1) * 8;
  if (hipMalloc((void **)&s.partials, pbytes) != hipSuccess || hipMalloc((void **)&s.maxpart, (size_t)nwg * 16) != hipSuccess ||
      hipMalloc((void **)&s.maxcell, (size_t)nwg * 8) != hipSuccess || hipMalloc((void **)&s.offs, ((size_t)nwg + 1) * 8) != hipSuccess ||
      hipMalloc((void **)&s.out, sizeof(pf_census)) != hipSuccess) {
    (void)hipGetLastError();
    return pf_fail(task, "%s: cannot allocate %zu bytes of scratch on the device", who, pbytes + (size_t)nwg * 32 + 8 + sizeof(pf_census));
  }
  int rc;
  if (pb == 8) rc = census_count<double>(CensusCols<double>{(const double *)fmax_fast, (const double *)fmax_exact, rmax_fast, rmax_exact}, w, nwg, s, st);
  else rc = census_count<float>(CensusCols<float>{(const float *)fmax_fast, (const float *)fmax_exact, rmax_fast, rmax_exact}, w, nwg, s, st);
  if (rc) return pf_fail(task, "%s: launch failed", who);
  hipLaunchKernelGGL(k_census_final, dim3(1), dim3(PF_CENSUS_BLOCK), 0, st, s.partials, s.maxpart, s.maxcell, nwg, (u64)count, s.out, s.offs);
  if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  CNHIP(task, who, hipMemcpyAsync(out, s.out, sizeof(pf_census), hipMemcpyDeviceToHost, st));
  CNHIP(task, who, hipStreamSynchronize(st));
  const u64 m = out->outliers < (u64)capacity ? out->outliers : (u64)capacity;
  if (m && cells) {
    if (hipMalloc((void **)&s.rec, (size_t)m * sizeof(pf_census_cell)) != hipSuccess) {
      (void)hipGetLastError();
      return pf_fail(task, "%s: cannot allocate %zu bytes on the device for %llu outlier records", who, (size_t)m * sizeof(pf_census_cell), m);
    }
    if (pb == 8) rc = census_records<double>(CensusCols<double>{(const double *)fmax_fast, (const double *)fmax_exact, rmax_fast, rmax_exact}, w, nwg, s, m, st);
    else rc = census_records<float>(CensusCols<float>{(const float *)fmax_fast, (const float *)fmax_exact, rmax_fast, rmax_exact}, w, nwg, s, m, st);
    if (rc) return pf_fail(task, "%s: launch failed", who);
    CNHIP(task, who, hipMemcpyAsync(cells, s.rec, (size_t)m * sizeof(pf_census_cell), hipMemcpyDeviceToHost, st));
    CNHIP(task, who, hipStreamSynchronize(st));
  }
  return 0;
}

// test tap on a caller's columns, on the default stream
extern "C" int pf_debug_census(int product_bytes, unsigned long long first_cell, size_t count, const void *fmax_fast, const int *rmax_fast, const void *fmax_exact,
                               const int *rmax_exact, pf_census *out, size_t capacity, pf_census_cell *cells) {
  const char *who = "pf_debug_census";
  if (!out || (capacity && !cells) || (count && (!fmax_fast || !rmax_fast || !fmax_exact || !rmax_exact))) return pf_fail(0, "%s: null argument", who);
  if (product_bytes != 4 && product_bytes != 8) return pf_fail(0, "%s: a PRODFLOAT of %d bytes (4 or 8)", who, product_bytes);
  if (first_cell + (unsigned long long)count < first_cell) return pf_fail(0, "%s: the cell indices %llu + %zu leave 64 bits", who, first_cell, count);
  if (!count) return pf_census_device(who, 0, product_bytes, first_cell, 0, nullptr, nullptr, nullptr, nullptr, out, capacity, cells, nullptr);
  const size_t fb = count * (size_t)product_bytes, rb = count * 4;
  struct Cols { void *p[4]; ~Cols() { for (int i = 0; i < 4; i++) hipFree(p[i]); } } d = {{nullptr, nullptr, nullptr, nullptr}};
  if (hipMalloc(&d.p[0], fb) != hipSuccess || hipMalloc(&d.p[1], fb) != hipSuccess || hipMalloc(&d.p[2], rb) != hipSuccess || hipMalloc(&d.p[3], rb) != hipSuccess) {
    (void)hipGetLastError();
    return pf_fail(0, "%s: cannot allocate %zu bytes on the device", who, 2 * (fb + rb));
  }
  CNHIP(0, who, hipMemcpy(d.p[0], fmax_fast, fb, hipMemcpyHostToDevice));
  CNHIP(0, who, hipMemcpy(d.p[1], fmax_exact, fb, hipMemcpyHostToDevice));
  CNHIP(0, who, hipMemcpy(d.p[2], rmax_fast, rb, hipMemcpyHostToDevice));
  CNHIP(0, who, hipMemcpy(d.p[3], rmax_exact, rb, hipMemcpyHostToDevice));
  return pf_census_device(who, 0, product_bytes, first_cell, count, d.p[0], (const int *)d.p[2], d.p[1], (const int *)d.p[3], out, capacity, cells, nullptr);
}
