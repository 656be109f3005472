// pf_bispec.hip -- the FFT estimator of the bispectrum (Scoccimarro 2000; Sefusatti et al. 2016) on a spectrum that lies on the device
// (include/pinfmax.h: pf_halo_bispectrum and its taps; pf_halo.hip calls pf_bispec_device).  Per k-bin i the spectrum is masked to
// the bin (data field) or replaced by N^3 inside it (count field), reversed by the context's transform and kept as a compact real
// field D_i(x) or I_i(x); then sum_x D_i D_j D_l for every ordered triple of bins that can close a triangle.  The integer side and
// the term are pf_bispec_core.h's, the fixed point pf_power_core.h's.  The reference has no counterpart.
//
//  k_bispec_mask     the form pass on the rows of this rank's ky-slab, one lane per stored mode (thread t at the columns kz = t, t +
//                    256, ... <= n/2): inside the bin the mode (times the window factor) or (N^3, 0), zero outside; a mode that is
//                    not finite is written as zero and counted; the Hermitian-weighted modes of the bin, counted in integers.  Per
//                    wave a shuffle reduction, then one integer atomic per counter into one of PF_BISPEC_SLOTS copies.
//  k_bispec_keep     one cell per lane: the reversed field out of the transform's rows of `pitch` reals into the compact store
//                    [nxl][n][n]; the largest |value| (an integer maximum of the bit pattern of the double) and the cells that are
//                    not finite, which are stored as zero.
//  k_bispec_triples  blockIdx.y names a group: one pair (i, j) and up to PF_BISPEC_LC consecutive l, so that a b is formed once per
//                    cell and 2 + LC fields are streamed for LC triples.  A lane walks the cells idx, idx + stride, ... and adds the
//                    three limbs of |t| under the triple's exponent to 64-bit registers, positive and negative apart; at its end a
//                    shuffle reduction and one integer atomic per wave and counter that has something to add, into the slot copy
//                    of the workgroup.  Nothing depends on the geometry of the launch: integer adds alone.
//  k_bispec_pairs    the same for sum_x D_i^2, blockIdx.y the bin.
//  k_bispec_fold     the slot copies -> one table.
//
// Every index is in range by construction: a mode is read and written in the workgroup's own rows (< rows) at a column kz <= n/2 <
// pitch; the deconvolution table is read at |kx|, |ky|, kz <= n/2, its length less one; a cell index is below ncell = nxl n^2, a
// field index below nk, which sized the stores; a group index is blockIdx.y < ngroups, its triples t0 + q < nt by construction of the
// list (bispec_groups); a counter lies in slot blockIdx.x mod PF_BISPEC_SLOTS of the tables pf_bispec_words sized.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pf_internal.h"
#include "pf_matter_core.h"
#include "pf_bispec_core.h"

#define BSHIP(task, who, call)                                                                                         \
  do {                                                                                                                 \
    hipError_t e__ = (call);                                                                                           \
    if (e__ != hipSuccess) return pf_fail(task, "%s: %s failed: %s", who, #call, hipGetErrorString(e__));             \
  } while (0)

#define PF_BISPEC_BLOCK 256
#ifndef PF_BISPEC_LC
#define PF_BISPEC_LC 4             // l per group: 24 64-bit sums in registers (profiles/bispec_notes.md: 1, 4 and 8 timed)
#endif
#ifndef PF_BISPEC_CELLS
#define PF_BISPEC_CELLS 16         // cells per lane a launch aims at, so that the reduction at the end of a lane is small beside its walk
#endif
#define PF_BISPEC_MAXWG_X 4096
#define PF_BISPEC_MAXWG_MASK 8192

static_assert(PF_BISPEC_KBINS == PF_BISPEC_MAX_KBINS, "pf_bispec_core.h and pinfmax.h disagree");

typedef unsigned long long u64;

__device__ __forceinline__ u64 bispec_wave_sum(u64 v) {
  for (int off = warpSize / 2; off; off >>= 1) v += __shfl_down(v, off);
  return v;
}
__device__ __forceinline__ u64 bispec_wave_max(u64 v) {
  for (int off = warpSize / 2; off; off >>= 1) { const u64 o = __shfl_down(v, off); v = o > v ? o : v; }
  return v;
}
__device__ __forceinline__ void bispec_add(u64 *p, u64 v) {
  if (v) (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// spec null: no input is read (the count field of a call); kind 0 data, 1 count
struct BispecMask { const void *spec; void *out; const double *C; int n, nyl, y0, kind; long long pitch; unsigned int rows, rows_per_wg; u64 lo2, hi2; double n3; };

template <class F>
__global__ void __launch_bounds__(PF_BISPEC_BLOCK) k_bispec_mask(BispecMask v, u64 *counters) {
  const unsigned int r0 = blockIdx.x * v.rows_per_wg, r1 = r0 + v.rows_per_wg < v.rows ? r0 + v.rows_per_wg : v.rows;
  const unsigned int half = (unsigned int)v.n / 2;
  u64 kmodes = 0, nonfin = 0;
  for (unsigned int row = r0; row < r1; row++) {
    const unsigned int kx = row / (unsigned int)v.nyl, yl = row - kx * (unsigned int)v.nyl;
    const int sx = pf_power_signed((int)kx, v.n), sy = pf_power_signed((int)yl + v.y0, v.n);
    const unsigned int kxy2 = (unsigned int)(sx * sx + sy * sy);
    const double cxy = v.C ? v.C[sx < 0 ? -sx : sx] * v.C[sy < 0 ? -sy : sy] : 1.0;
    for (unsigned int kz = threadIdx.x; kz <= half; kz += PF_BISPEC_BLOCK) {
      const long long at = 2 * ((long long)row * v.pitch + kz);
      double re = 0.0, im = 0.0;
      if (pf_bispec_in_bin((u64)kxy2 + (u64)kz * kz, v.lo2, v.hi2)) {
        const u64 w = (kz > 0 && kz < half) ? 2u : 1u;
        kmodes += w;
        bool fin = true;
        if (v.spec) {   // the mode as the data field holds it: times the window factor, rounded once to the field type
          double a, b;
          const F *e = (const F *)v.spec + at;
          if constexpr (sizeof(F) == 8) { const double2 x = *(const double2 *)e; a = x.x; b = x.y; }
          else { const float2 x = *(const float2 *)e; a = (double)x.x; b = (double)x.y; }
          const double c = v.C ? pf_matter_deconv(cxy, 1.0, v.C[kz]) : -1.0;
          re = (double)(F)pf_bispec_masked(a, c); im = (double)(F)pf_bispec_masked(b, c);
          fin = pf_power_finite(re) && pf_power_finite(im);
        }
        if (v.kind) { re = (double)(F)v.n3; im = 0.0; }
        if (!fin) { nonfin += w; re = im = 0.0; }
      }
      F *o = (F *)v.out + at;
      if constexpr (sizeof(F) == 8) *(double2 *)o = make_double2(re, im);
      else *(float2 *)o = make_float2((float)re, (float)im);
    }
  }
  kmodes = bispec_wave_sum(kmodes); nonfin = bispec_wave_sum(nonfin);
  if ((threadIdx.x & (warpSize - 1)) == 0) {
    u64 *slot = counters + (size_t)(blockIdx.x % PF_BISPEC_SLOTS) * 2;
    bispec_add(slot, kmodes); bispec_add(slot + 1, nonfin);
  }
}

template <class F>
__global__ void __launch_bounds__(PF_BISPEC_BLOCK) k_bispec_keep(const F *real, long long pitch, int n, size_t ncell, F *store, u64 *counters) {
  const size_t i = (size_t)blockIdx.x * PF_BISPEC_BLOCK + threadIdx.x;
  u64 mx = 0, bad = 0;
  if (i < ncell) {
    const size_t row = i / (unsigned int)n;
    F x = real[row * (size_t)pitch + (i - row * (unsigned int)n)];
    if (!pf_power_finite((double)x)) { bad = 1; x = (F)0; }
    store[i] = x;
    mx = (u64)__double_as_longlong(fabs((double)x));
  }
  mx = bispec_wave_max(mx); bad = bispec_wave_sum(bad);
  if ((threadIdx.x & (warpSize - 1)) == 0) {
    u64 *slot = counters + (size_t)(blockIdx.x % PF_BISPEC_SLOTS) * 2;
    if (mx > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(slot, mx);
    bispec_add(slot + 1, bad);
  }
}

// a group: the pair (i, j), the triples (i, j, l0 + q), q < nl <= PF_BISPEC_LC, which are t0 + q of the list
struct BispecGroup { int i, j, l0, nl, t0, pad[3]; };

// slots: PF_BISPEC_SLOTS copies of `len` counters; a triple t has the six counters 6 t + 3 s + limb, s = 0 positive, 1 negative
template <class F>
__global__ void __launch_bounds__(PF_BISPEC_BLOCK) k_bispec_triples(const F *stores, size_t ncell, const BispecGroup *groups, const int *exps, u64 *slots, size_t len) {
  const BispecGroup g = groups[blockIdx.y];
  const F *fa = stores + (size_t)g.i * ncell, *fb = stores + (size_t)g.j * ncell, *fl = stores + (size_t)g.l0 * ncell;
  int e[PF_BISPEC_LC];
  u64 acc[PF_BISPEC_LC][2][3];
#pragma unroll
  for (int q = 0; q < PF_BISPEC_LC; q++) {
    e[q] = q < g.nl ? exps[g.t0 + q] : 0;
#pragma unroll
    for (int k = 0; k < 3; k++) acc[q][0][k] = acc[q][1][k] = 0;
  }
  const size_t stride = (size_t)gridDim.x * PF_BISPEC_BLOCK;
  for (size_t idx = (size_t)blockIdx.x * PF_BISPEC_BLOCK + threadIdx.x; idx < ncell; idx += stride) {
    const double a = (double)fa[idx], b = (double)fb[idx];
#pragma unroll
    for (int q = 0; q < PF_BISPEC_LC; q++)
      if (q < g.nl) {
        const double t = pf_bispec_term(a, b, (double)fl[(size_t)q * ncell + idx]);
        const bool neg = t < 0.0;
        uint32_t l[3];
        pf_power_limbs(fabs(t), e[q], l);   // (a term of zero has limbs of zero)
#pragma unroll
        for (int k = 0; k < 3; k++) { acc[q][0][k] += neg ? 0u : l[k]; acc[q][1][k] += neg ? l[k] : 0u; }
      }
  }
  u64 *slot = slots + (size_t)(blockIdx.x % PF_BISPEC_SLOTS) * len;
  const bool first = (threadIdx.x & (warpSize - 1)) == 0;
#pragma unroll
  for (int q = 0; q < PF_BISPEC_LC; q++)
    if (q < g.nl)
#pragma unroll
      for (int s = 0; s < 2; s++)
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const u64 v = bispec_wave_sum(acc[q][s][k]);
          if (first) bispec_add(slot + 6 * (size_t)(g.t0 + q) + 3 * s + k, v);
        }
}

// the pair sums: the three counters of bin i at 6 nt + 3 i; their exponents at exps[nt + i]
template <class F>
__global__ void __launch_bounds__(PF_BISPEC_BLOCK) k_bispec_pairs(const F *stores, size_t ncell, int nt, const int *exps, u64 *slots, size_t len) {
  const int i = blockIdx.y;
  const F *fa = stores + (size_t)i * ncell;
  const int e = exps[nt + i];
  u64 acc[3] = {0, 0, 0};
  const size_t stride = (size_t)gridDim.x * PF_BISPEC_BLOCK;
  for (size_t idx = (size_t)blockIdx.x * PF_BISPEC_BLOCK + threadIdx.x; idx < ncell; idx += stride) {
    uint32_t l[3];
    pf_power_limbs(pf_bispec_pair((double)fa[idx]), e, l);
#pragma unroll
    for (int k = 0; k < 3; k++) acc[k] += l[k];
  }
  u64 *slot = slots + (size_t)(blockIdx.x % PF_BISPEC_SLOTS) * len + 6 * (size_t)nt + 3 * (size_t)i;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const u64 v = bispec_wave_sum(acc[k]);
    if ((threadIdx.x & (warpSize - 1)) == 0) bispec_add(slot + k, v);
  }
}

__global__ void __launch_bounds__(PF_BISPEC_BLOCK) k_bispec_fold(const u64 *slots, size_t len, u64 *table) {
  const size_t i = (size_t)blockIdx.x * PF_BISPEC_BLOCK + threadIdx.x;
  if (i >= len) return;
  u64 s = 0;
  for (int k = 0; k < PF_BISPEC_SLOTS; k++) s += slots[(size_t)k * len + i];
  table[i] = s;
}

// ------------------------------------------------------------------------------------------------------------ launches ----
// the groups of the closed triples, in the order of the list
static void bispec_groups(int kmin, int dk, int nk, std::vector<BispecGroup> *out) {
  int t = 0;
  for (int i = 0; i < nk; i++)
    for (int j = i; j < nk; j++) {
      const int last = pf_bispec_last(kmin, dk, nk, i, j);
      for (int l0 = j; l0 <= last; l0 += PF_BISPEC_LC) {
        const int nl = last - l0 + 1 < PF_BISPEC_LC ? last - l0 + 1 : PF_BISPEC_LC;
        if (out) out->push_back(BispecGroup{i, j, l0, nl, t, {0, 0, 0}});
        t += nl;
      }
    }
}
static size_t bispec_ngroups(int kmin, int dk, int nk) {
  std::vector<BispecGroup> g;
  bispec_groups(kmin, dk, nk, &g);
  return g.size();
}

// the tables of a call, 64-bit words one behind the other: the counters of the mask passes [nk][SLOTS][2] and of the keep passes
// likewise, the slot copies of the limb counters [SLOTS][len], their table [len] -- these are cleared per set of fields --, what the
// ranks agree on, the exponents (ints) and the groups
struct BispecWords { size_t len, mask, keep, slots, table, clear, agree, exps, groups, total; };
static BispecWords bispec_layout(int kmin, int dk, int nk, int P) {
  BispecWords w;
  const size_t nt = (size_t)pf_bispec_triangles(kmin, dk, nk, nullptr);
  w.len = 6 * nt + 3 * (size_t)nk;
  w.mask = 0; w.keep = w.mask + (size_t)nk * PF_BISPEC_SLOTS * 2; w.slots = w.keep + (size_t)nk * PF_BISPEC_SLOTS * 2;
  w.table = w.slots + PF_BISPEC_SLOTS * w.len; w.clear = w.table + w.len;
  w.agree = w.clear; w.exps = w.agree + (size_t)P * nk + nk + 2; w.groups = w.exps + (nt + nk + 1) / 2;
  w.total = w.groups + bispec_ngroups(kmin, dk, nk) * (sizeof(BispecGroup) / 8);
  return w;
}
size_t pf_bispec_words(int kmin, int dk, int nk, int P) { return bispec_layout(kmin, dk, nk, P).total; }

int pf_bispec_mask_device(const char *who, int task, int fb, const void *spec, void *out, int n, int y0, int nyl, long long pitch, const double *C, int kind, int kmin, int dk,
                          int bin, u64 *counters, hipStream_t st) {
  if (((uintptr_t)spec | (uintptr_t)out) & 15) return pf_fail(task, "%s: a spectrum is not 16-byte aligned (internal error)", who);
  BispecMask v;
  v.spec = spec; v.out = out; v.C = spec ? C : nullptr; v.n = n; v.nyl = nyl; v.y0 = y0; v.kind = kind; v.pitch = pitch;
  v.rows = (unsigned int)n * (unsigned int)nyl;
  v.rows_per_wg = (v.rows + PF_BISPEC_MAXWG_MASK - 1) / PF_BISPEC_MAXWG_MASK;
  v.lo2 = pf_bispec_edge2(kmin, dk, bin); v.hi2 = pf_bispec_edge2(kmin, dk, bin + 1);
  v.n3 = (double)n * (double)n * (double)n;
  const unsigned int nwg = (v.rows + v.rows_per_wg - 1) / v.rows_per_wg;
  hipLaunchKernelGGL(fb == 8 ? k_bispec_mask<double> : k_bispec_mask<float>, dim3(nwg), dim3(PF_BISPEC_BLOCK), 0, st, v, counters);
  if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  return 0;
}

static int pf_bispec_keep_device(const char *who, int task, int fb, const void *real, long long pitch, int n, size_t ncell, void *store, u64 *counters, hipStream_t st) {
  const size_t nblk = (ncell + PF_BISPEC_BLOCK - 1) / PF_BISPEC_BLOCK;
  if (nblk > 0x7fffffffull) return pf_fail(task, "%s: %zu cells are more than one launch takes (internal error)", who, ncell);
  const dim3 gr((unsigned int)nblk), bl(PF_BISPEC_BLOCK);
  if (fb == 8) hipLaunchKernelGGL(k_bispec_keep<double>, gr, bl, 0, st, (const double *)real, pitch, n, ncell, (double *)store, counters);
  else hipLaunchKernelGGL(k_bispec_keep<float>, gr, bl, 0, st, (const float *)real, pitch, n, ncell, (float *)store, counters);
  if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  return 0;
}

// a few words of the host summed over the ranks of the context, through `dev` on the context's stream
static int bispec_agree(const char *who, int task, pf_ctx *c, u64 *dev, std::vector<u64> &a, hipStream_t st) {
  BSHIP(task, who, hipMemcpyAsync(dev, a.data(), a.size() * 8, hipMemcpyHostToDevice, st));
  BSHIP(task, who, hipStreamSynchronize(st));
  if (pf_ctx_allreduce(c, dev, a.size(), 1)) return 1;
  BSHIP(task, who, hipMemcpyAsync(a.data(), dev, a.size() * 8, hipMemcpyDeviceToHost, st));
  BSHIP(task, who, hipStreamSynchronize(st));
  return 0;
}

// behind the mask and keep passes of nk fields: their counters -> kmodes, the maxima and the two counts, over the ranks of coll
// (null: this slab alone); then the triple pass (and the pair pass where out->pair is wanted) under the exponents of the maxima, the
// table over the ranks, and the sums on the host.  Synchronises the stream
static int pf_bispec_sums_device(const char *who, int task, pf_ctx *coll, int rank, int P, int fb, const PfBispecBins &kb, size_t ncell, const void *stores, u64 *words, PfBispecOut *out,
                          hipStream_t st) {
  const int nk = kb.nk, nt = pf_bispec_triangles(kb.kmin, kb.dk, nk, nullptr);
  const BispecWords w = bispec_layout(kb.kmin, kb.dk, nk, coll ? P : 1);
  std::vector<u64> cnt(w.slots);
  BSHIP(task, who, hipMemcpyAsync(cnt.data(), words, cnt.size() * 8, hipMemcpyDeviceToHost, st));
  BSHIP(task, who, hipStreamSynchronize(st));
  const int ranks = coll ? P : 1, me = coll ? rank : 0;
  std::vector<u64> a((size_t)ranks * nk + nk + 2, 0);   // the maxima in a slot per rank, kmodes, the modes and the cells that are not finite
  u64 *mx = a.data() + (size_t)me * nk, *km = a.data() + (size_t)ranks * nk, *bad = km + nk;
  for (int i = 0; i < nk; i++)
    for (int k = 0; k < PF_BISPEC_SLOTS; k++) {
      const u64 *m = cnt.data() + w.mask + ((size_t)i * PF_BISPEC_SLOTS + k) * 2, *p = cnt.data() + w.keep + ((size_t)i * PF_BISPEC_SLOTS + k) * 2;
      km[i] += m[0]; bad[0] += m[1]; bad[1] += p[1];
      if (p[0] > mx[i]) mx[i] = p[0];
    }
  if (coll && bispec_agree(who, task, coll, words + w.agree, a, st)) return 1;
  std::vector<double> M(nk, 0.0);
  for (int i = 0; i < nk; i++)
    for (int p = 0; p < ranks; p++) {
      double m;
      memcpy(&m, &a[(size_t)p * nk + i], 8);
      if (m > M[i]) M[i] = m;
    }
  // the exponents: of a triple from (M_i M_j) M_l, of a pair from M_i M_i, formed as the terms are; 0 where the scale is zero (every
  // term is)
  std::vector<int> ijl(3 * (size_t)nt), exps((size_t)nt + nk, 0);
  pf_bispec_triangles(kb.kmin, kb.dk, nk, ijl.data());
  for (int t = 0; t < nt + nk; t++) {
    const double m = t < nt ? pf_bispec_term(M[ijl[3 * t]], M[ijl[3 * t + 1]], M[ijl[3 * t + 2]]) : pf_bispec_pair(M[t - nt]);
    if (!pf_power_finite(m)) return pf_fail(task, "%s: the product of the largest values of the fields of k-bins overflows a double", who);
    if (m > 0.0) exps[t] = pf_power_exponent(m);
  }
  std::vector<BispecGroup> groups;
  bispec_groups(kb.kmin, kb.dk, nk, &groups);
  BSHIP(task, who, hipMemcpyAsync(words + w.exps, exps.data(), exps.size() * 4, hipMemcpyHostToDevice, st));
  BSHIP(task, who, hipMemcpyAsync(words + w.groups, groups.data(), groups.size() * sizeof(BispecGroup), hipMemcpyHostToDevice, st));
  BSHIP(task, who, hipStreamSynchronize(st));   // (pageable memory: the copies have left the vectors)
  size_t gx = (ncell + (size_t)PF_BISPEC_BLOCK * PF_BISPEC_CELLS - 1) / ((size_t)PF_BISPEC_BLOCK * PF_BISPEC_CELLS);
  gx = gx < 1 ? 1 : gx > PF_BISPEC_MAXWG_X ? PF_BISPEC_MAXWG_X : gx;
  if (groups.size() > 65535) return pf_fail(task, "%s: %zu groups of triples are more than one launch takes (internal error)", who, groups.size());
  const dim3 bl(PF_BISPEC_BLOCK), gt((unsigned int)gx, (unsigned int)groups.size()), gp((unsigned int)gx, (unsigned int)nk);
  const int *de = (const int *)(words + w.exps);
  const BispecGroup *dg = (const BispecGroup *)(words + w.groups);
  if (fb == 8) hipLaunchKernelGGL(k_bispec_triples<double>, gt, bl, 0, st, (const double *)stores, ncell, dg, de, words + w.slots, w.len);
  else hipLaunchKernelGGL(k_bispec_triples<float>, gt, bl, 0, st, (const float *)stores, ncell, dg, de, words + w.slots, w.len);
  if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  if (out->pair) {
    if (fb == 8) hipLaunchKernelGGL(k_bispec_pairs<double>, gp, bl, 0, st, (const double *)stores, ncell, nt, de, words + w.slots, w.len);
    else hipLaunchKernelGGL(k_bispec_pairs<float>, gp, bl, 0, st, (const float *)stores, ncell, nt, de, words + w.slots, w.len);
    if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  }
  hipLaunchKernelGGL(k_bispec_fold, dim3((unsigned int)((w.len + PF_BISPEC_BLOCK - 1) / PF_BISPEC_BLOCK)), bl, 0, st, words + w.slots, w.len, words + w.table);
  if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  if (coll && pf_ctx_allreduce(coll, words + w.table, w.len, 1)) return 1;
  std::vector<u64> tab(w.len);
  BSHIP(task, who, hipMemcpyAsync(tab.data(), words + w.table, w.len * 8, hipMemcpyDeviceToHost, st));
  BSHIP(task, who, hipStreamSynchronize(st));
  for (int t = 0; t < nt; t++) {
    const double pos = pf_power_from_limbs(&tab[6 * (size_t)t], 3, exps[t]), neg = pf_power_from_limbs(&tab[6 * (size_t)t + 3], 3, exps[t]);   // (counters of zero give zero)
    out->sums[t] = pos - neg;
    if (out->parts) { out->parts[t] = pos; out->parts[nt + t] = neg; }
  }
  for (int i = 0; i < nk; i++) {
    if (out->pair) out->pair[i] = pf_power_from_limbs(&tab[6 * (size_t)nt + 3 * (size_t)i], 3, exps[nt + i]);
    if (out->maxima) out->maxima[i] = M[i];
    if (out->kmodes) out->kmodes[i] = km[i];
  }
  out->nonfinite_modes = bad[0]; out->nonfinite_cells = bad[1];
  return 0;
}

int pf_bispec_device(const char *who, int task, pf_ctx *c, const PfBispecGeom &g, const PfBispecBins &kb, const void *spec, int kind, const double *C, void *work, void *stores,
                     u64 *words, void (*mark)(void *, int), void *user, PfBispecOut *out, hipStream_t st) {
  const BispecWords w = bispec_layout(kb.kmin, kb.dk, kb.nk, g.P);
  const size_t ncell = (size_t)g.nxl * g.n * g.n;
  BSHIP(task, who, hipMemsetAsync(words, 0, w.clear * 8, st));
  if (mark) mark(user, -1);
  for (int i = 0; i < kb.nk; i++) {
    if (pf_bispec_mask_device(who, task, g.fb, spec, work, g.n, g.y0, g.nyl, g.nzp, C, kind, kb.kmin, kb.dk, i, words + w.mask + (size_t)i * PF_BISPEC_SLOTS * 2, st)) return 1;
    if (mark) mark(user, PF_BISPEC_PH_MASK);
    if (pf_ctx_matter_reverse(c)) return 1;
    if (mark) mark(user, PF_BISPEC_PH_TRANSFORM);
    if (pf_bispec_keep_device(who, task, g.fb, work, g.rpitch, g.n, ncell, (char *)stores + (size_t)i * ncell * g.fb, words + w.keep + (size_t)i * PF_BISPEC_SLOTS * 2, st)) return 1;
    if (mark) mark(user, PF_BISPEC_PH_KEEP);
  }
  if (pf_bispec_sums_device(who, task, g.P > 1 ? c : nullptr, g.rank, g.P, g.fb, kb, ncell, stores, words, out, st)) return 1;
  if (mark) mark(user, PF_BISPEC_PH_TRIPLES);
  return 0;
}

extern "C" int pf_bispectrum_triangles(int kmin, int dk, int nk, int *ijl) {
  const int bad = pf_bispec_check(kmin, dk, nk, 0);
  if (bad) { pf_fail(0, "pf_bispectrum_triangles: k-bins from %d in %d steps of %d (kmin >= 1, dk >= 1, 1 <= nk <= %d)", kmin, nk, dk, PF_BISPEC_MAX_KBINS); return -1; }
  return pf_bispec_triangles(kmin, dk, nk, ijl);
}

// what both taps and the call refuse of the k-bins, with the message
int pf_bispec_check_bins(const char *who, int task, int kmin, int dk, int nk, int n) {
  const int bad = pf_bispec_check(kmin, dk, nk, n);
  if (bad == 1) return pf_fail(task, "%s: a kmin of %d (1 or more, in units of the fundamental)", who, kmin);
  if (bad == 2) return pf_fail(task, "%s: a dk of %d (1 or more, in units of the fundamental)", who, dk);
  if (bad == 3) return pf_fail(task, "%s: %d k-bins (1 to %d)", who, nk, PF_BISPEC_MAX_KBINS);
  if (bad == 4) return pf_fail(task, "%s: 3 kmax = 3 (%d + %d * %d) = %d is above the grid of %d: triangles would close modulo the grid", who, kmin, nk, dk, 3 * (kmin + nk * dk), n);
  return 0;
}

// ------------------------------------------------------------------------------------------------------------ taps ----
extern "C" int pf_debug_bispec_mask(int field_bytes, int n, int y0, int nyl, const double *spec, int flags, int kind, int kmin, int dk, int nk, int bin, double *spec_out,
                                    unsigned long long *kmodes, unsigned long long *nonfinite_modes) {
  const char *who = "pf_debug_bispec_mask";
  if (!spec || !spec_out || !kmodes || !nonfinite_modes) return pf_fail(0, "%s: null argument", who);
  if (flags & ~(PF_HALO_NGP | PF_HALO_DECONVOLVE)) return pf_fail(0, "%s: unknown flag bits 0x%x", who, (unsigned int)(flags & ~(PF_HALO_NGP | PF_HALO_DECONVOLVE)));
  if (kind < 0 || kind > 1) return pf_fail(0, "%s: field kind %d (0 data, 1 count)", who, kind);
  if (n < 2 || n > 2048 || (n & 1)) return pf_fail(0, "%s: a grid of %d (even, 2 to 2048)", who, n);
  if (pf_bispec_check_bins(who, 0, kmin, dk, nk, n)) return 1;
  if (bin < 0 || bin >= nk) return pf_fail(0, "%s: k-bin %d of %d", who, bin, nk);
  const size_t cnt_words = (size_t)PF_BISPEC_SLOTS * 2, nzh = (size_t)n / 2 + 1;
  PfSpecStage d = {};
  if (pf_stage_spectra(who, field_bytes, n, y0, nyl, 2, spec, nullptr, cnt_words + nzh, &d)) return 1;
  BSHIP(0, who, hipMemsetAsync(d.words, 0, cnt_words * 8, nullptr));
  const double *Ctab = nullptr;
  if (pf_corr_deconv_upload(who, 0, flags, n, (double *)(d.words + cnt_words), &Ctab, nullptr)) return 1;
  if (pf_bispec_mask_device(who, 0, field_bytes, d.spec[0], d.spec[1], n, y0, nyl, d.nzp, Ctab, kind, kmin, dk, bin, d.words, nullptr)) return 1;
  if (pf_launch_spec_export_t(field_bytes, d.spec[1], (double *)d.in, n, nyl, (int)nzh, d.nzp, nullptr)) return pf_fail(0, "%s: launch failed", who);
  u64 slots[PF_BISPEC_SLOTS * 2];
  BSHIP(0, who, hipMemcpyAsync(spec_out, d.in, (size_t)nyl * n * nzh * 16, hipMemcpyDeviceToHost, nullptr));
  BSHIP(0, who, hipMemcpyAsync(slots, d.words, sizeof(slots), hipMemcpyDeviceToHost, nullptr));
  BSHIP(0, who, hipStreamSynchronize(nullptr));
  *kmodes = *nonfinite_modes = 0;
  for (int k = 0; k < PF_BISPEC_SLOTS; k++) { *kmodes += slots[2 * k]; *nonfinite_modes += slots[2 * k + 1]; }
  return 0;
}

struct BispecStage { void *in, *field, *stores; u64 *words; ~BispecStage() { hipFree(in); hipFree(field); hipFree(stores); hipFree(words); } };
extern "C" int pf_debug_bispec_triples(int field_bytes, int n, int x0, int nxl, const double *fields, int kmin, int dk, int nk, double *sums, double *parts, double *pair,
                                       double *maxima, unsigned long long *nonfinite_cells) {
  const char *who = "pf_debug_bispec_triples";
  if (!fields || !sums || !parts || !pair || !maxima || !nonfinite_cells) return pf_fail(0, "%s: null argument", who);
  if (field_bytes != 4 && field_bytes != 8) return pf_fail(0, "%s: fields of %d bytes (4 or 8)", who, field_bytes);
  if (n < 2 || n > 2048 || (n & 1)) return pf_fail(0, "%s: a grid of %d (even, 2 to 2048)", who, n);
  if (n > 1024) return pf_fail(0, "%s: a grid of %d is above 1024: a limb counter takes n^3 terms below 2^32 and would pass 2^63", who, n);
  if (x0 < 0 || nxl < 1 || x0 + nxl > n) return pf_fail(0, "%s: planes %d .. %d leave the grid of %d", who, x0, x0 + nxl - 1, n);
  if (pf_bispec_check_bins(who, 0, kmin, dk, nk, 0)) return 1;
  // the production layout of a real field: rows of 2 (n/2 + 64 / field_bytes) reals, NaN patterns in the padding that no pass may see
  const long long pitch = 2 * ((long long)n / 2 + 64 / field_bytes), nrows = (long long)nxl * n;
  const size_t ncell = (size_t)nrows * n, in_bytes = ncell * 8, field = (size_t)nrows * pitch * field_bytes, store = (size_t)nk * ncell * field_bytes;
  const size_t words = pf_bispec_words(kmin, dk, nk, 1);
  const BispecWords w = bispec_layout(kmin, dk, nk, 1);
  BispecStage d = {nullptr, nullptr, nullptr, nullptr};
  if (hipMalloc(&d.in, in_bytes) != hipSuccess || hipMalloc(&d.field, field) != hipSuccess || hipMalloc(&d.stores, store) != hipSuccess ||
      hipMalloc((void **)&d.words, words * 8) != hipSuccess) {
    (void)hipGetLastError();
    return pf_fail(0, "%s: cannot allocate %zu bytes on the device", who, in_bytes + field + store + words * 8);
  }
  BSHIP(0, who, hipMemset(d.field, 0xff, field));
  BSHIP(0, who, hipMemset(d.words, 0, w.clear * 8));
  for (int i = 0; i < nk; i++) {
    BSHIP(0, who, hipMemcpy(d.in, fields + (size_t)i * ncell, in_bytes, hipMemcpyHostToDevice));
    if (pf_launch_real_import(field_bytes, (const double *)d.in, d.field, nrows, n, pitch, nullptr)) return pf_fail(0, "%s: launch failed", who);
    if (pf_bispec_keep_device(who, 0, field_bytes, d.field, pitch, n, ncell, (char *)d.stores + (size_t)i * ncell * field_bytes, d.words + w.keep + (size_t)i * PF_BISPEC_SLOTS * 2, nullptr))
      return 1;
    BSHIP(0, who, hipDeviceSynchronize());   // (the import has read `in`)
  }
  const PfBispecBins kb = {kmin, dk, nk};
  PfBispecOut out = {sums, parts, pair, maxima, nullptr, 0, 0};
  if (pf_bispec_sums_device(who, 0, nullptr, 0, 1, field_bytes, kb, ncell, d.stores, d.words, &out, nullptr)) return 1;
  *nonfinite_cells = out.nonfinite_cells;
  return 0;
}
