// pf_matter.hip -- the density of the LPT-displaced particles and its spectra (include/pinfmax.h: pf_matter_power and its taps): mass
// assignment of one particle per cell at the reference's initialize_POS positions (src/write_snapshot.c:907-954) into a grid of
// 64-bit integers, the density contrast into a scratch field, the context's own forward transform, and per-shell sums of
// |delta_m|^2 and Re(delta_m conj delta) with the resident delta(k).  The arithmetic of a particle and of a mode is pf_matter_core.h's;
// the fixed-point sums are pf_power_core.h's.  The reference has no counterpart beyond the plots it commits for its mode 3.
//
//  k_matter_deposit   one particle per lane, consecutive lanes along z: the twelve column loads of a wave are contiguous, and so,
//                     nearly, are its targets along z.  Up to eight 64-bit integer adds whose result is not used (relaxed, agent
//                     scope); a factor of zero adds nothing and is left out.  Integer adds: the grid is the same bits for any order.
//                     The three classes are counted per wave (ballots) and leave as one atomic per wave and class.
//  k_matter_deposit_lds
//                     the default where n is a multiple of 16 (PF_MATTER_LDS=0: the plain form): a brick of particles per workgroup
//                     through an LDS tile placed by the brick's mean displacement, described at the kernel.  The same grid, bit for bit.
//  k_matter_contrast  cell -> delta = cell / 2^48 - 1 in double, rounded once to the field type, into the real rows of the scratch
//                     field; in the same pass the largest cell, the empty cells and the sums of the high and low halves of the cells
//                     (integers: the same from run to run).
//  k_matter_scan /    the two passes of pf_power.hip over the rows of two spectra.  Three positive sums per shell (0 |delta_m|^2, 1 the
//  k_matter_acc       positive cross terms, 2 the negative ones): ONE scan takes the largest term of every shell for all three, with
//                     nmodes, k2sum and the modes whose terms are not finite (five LDS tables; where they do not fit, n above
//                     about 1800, a scan per sum); an accumulation per sum adds every term as three 32-bit limbs scaled to that
//                     maximum (LDS holds one sum's counters, so every grid up to 2048 fits).  Four passes over the two spectra
//                     (profiles/matter_notes.md).
//  k_matter_final     limbs -> double, times 1 / N^6; cross = positive - negative, formed once.
//
// Every index is in range by construction: a particle index is below ncell; a target plane is wrapped into [0, n) and deposited only
// when it lies in this slab's [x0, x0 + nxl) (always, with one rank); target rows and columns are wrapped into [0, n); a mode is read
// at a row below `rows` and a column kz <= n/2 < pitch; a shell is below pf_power_nbins(n), which sized every table; the
// deconvolution table is read at |kx|, |ky|, kz <= n/2, its length less one.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pf_internal.h"
#include "pf_matter_core.h"

#define MTHIP(task, who, call)                                                                                         \
  do {                                                                                                                 \
    hipError_t e__ = (call);                                                                                           \
    if (e__ != hipSuccess) return pf_fail(task, "%s: %s failed: %s", who, #call, hipGetErrorString(e__));             \
  } while (0)

#define PF_MATTER_BLOCK 256
#define PF_MATTER_MAXWG 8192     // workgroups of a shell pass at most (pf_power.hip: PF_POWER_MAXWG_SHELLS)
#define PF_MATTER_LDS_MAX 65536  // bytes of LDS a workgroup may ask for without an attribute
#define PF_MATTER_FLAGS (PF_MATTER_NGP | PF_MATTER_DECONVOLVE)
#define PF_MATTER_LDS_DEFAULT 1   // PF_MATTER_LDS unset: the LDS-staged deposit, 70 ms against 329 at 1024^3 (the A/B: profiles/matter_notes.md)

typedef unsigned long long u64;

// counters of a call on the device: PF_MATTER_SLOTS copies of each, a workgroup adds to the copy of its index -- one counter for all
// wavefronts of a 1024^3 call is 1.7e7 atomics on one address: the contrast pass took 778 ms that way and takes 8 (profiles/matter_notes.md);
// the copies are summed (MC_MAX: reduced) on the host
#define PF_MATTER_SLOTS 1024
enum { MC_DEPOSITED = 0, MC_NONFINITE, MC_OUTSIDE, MC_EMPTY, MC_MAX, MC_SUMHI, MC_SUMLO, MC_NONFIN_MODES, MC_COUNT };
#define MC_WORDS ((size_t)PF_MATTER_SLOTS * MC_COUNT)

struct MatterCols { const void *vel12; size_t ncell; int n, nxl, x0, kmax, use_w; double w[4]; };

__device__ __forceinline__ void matter_add(u64 *p, u64 v) {
  if (v) (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// a maximum only grows: a term that is not above what a relaxed read saw needs no atomic
__device__ __forceinline__ void matter_max(u64 *p, u64 v) {
  if (v > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, v);
}
__device__ __forceinline__ void matter_max_lds(u64 *p, u64 v) {
  if (v > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) atomicMax(p, v);
}
__device__ __forceinline__ void matter_count(bool flag, u64 *counter) {
  const u64 m = __ballot(flag);
  if (m && (threadIdx.x & (warpSize - 1)) == (unsigned int)(__ffsll((long long)m) - 1)) matter_add(counter, (u64)__popcll(m));
}

template <class T, int NGP>
__global__ void __launch_bounds__(PF_MATTER_BLOCK) k_matter_deposit(MatterCols c, u64 *grid, u64 *counters) {
  const size_t i = (size_t)blockIdx.x * PF_MATTER_BLOCK + threadIdx.x;
  int cls = -1;
  if (i < c.ncell) {
    const unsigned int n = (unsigned int)c.n;
    const size_t row = i / n;
    const int q[3] = {c.x0 + (int)(row / n), (int)(row % n), (int)(i - row * n)};
    const T *col = (const T *)c.vel12;
    const double *w = c.use_w ? c.w : nullptr;
    T pos[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
      T v[4];
#pragma unroll
      for (int o = 0; o < 4; o++) {
        const int k = 3 * o + j;
        v[o] = k < c.kmax ? pf_matter_column<T>(col[(size_t)k * c.ncell + i], w, o) : (T)0;
      }
      pos[j] = pf_matter_pos<T>(q[j], c.n, v[0], v[1], v[2], v[3]);
    }
    cls = pf_matter_class<T>(pos, c.n);
    if (cls == 0) {
      if (NGP) {
        const int lx = pf_matter_ngp_axis<T>(pos[0], c.n) - c.x0;
        if (lx >= 0 && lx < c.nxl)
          matter_add(grid + ((size_t)lx * n + (size_t)pf_matter_ngp_axis<T>(pos[1], c.n)) * n + (size_t)pf_matter_ngp_axis<T>(pos[2], c.n), PF_MATTER_ONE);
      } else {
        int cell[3][2];
        uint32_t wt[3][2];
#pragma unroll
        for (int j = 0; j < 3; j++) pf_matter_cic_axis<T>(pos[j], c.n, cell[j], wt[j]);
#pragma unroll
        for (int a = 0; a < 2; a++) {
          const int lx = cell[0][a] - c.x0;
          if (lx < 0 || lx >= c.nxl || !wt[0][a]) continue;
#pragma unroll
          for (int b = 0; b < 2; b++) {
            const u64 wxy = (u64)wt[0][a] * wt[1][b];
            u64 *rowp = grid + ((size_t)lx * n + (size_t)cell[1][b]) * n;
            matter_add(rowp + cell[2][0], wxy * wt[2][0]);
            matter_add(rowp + cell[2][1], wxy * wt[2][1]);
          }
        }
      }
    }
  }
  u64 *slot = counters + (size_t)(blockIdx.x % PF_MATTER_SLOTS) * MC_COUNT;
  matter_count(cls == 0, slot + MC_DEPOSITED);
  matter_count(cls == 1, slot + MC_NONFINITE);
  matter_count(cls == 2, slot + MC_OUTSIDE);
}

// ---- the LDS-staged form (PF_MATTER_LDS=1): a workgroup takes a brick of 4 x 4 x 16 particles (16 consecutive lanes along z) and adds
// into an LDS tile of the brick plus a margin of PF_ML_M cells on every side, placed by the brick's mean displacement (rounded to whole
// cells; any placement gives the same grid, a good one keeps the adds in LDS).  What falls outside the tile goes straight to the
// grid; the tile leaves with one global add per touched cell.  Integer adds in both places: the grid is that of the plain form, bit
// for bit.  Needs n a multiple of 16 and nxl a multiple of 4 (matter_deposit falls back to the plain form otherwise).
// Indices: a tile slot is used only after tx < TX, ty < TY, tz < TZ were checked; the flush maps a slot back through a
// non-negative remainder by n, so its cell is in [0, n)^3, and the plane is deposited only inside the slab, as in the plain form.
#define PF_ML_BX 4
#define PF_ML_BY 4
#define PF_ML_BZ 16
#define PF_ML_M 3
#define PF_ML_TX (PF_ML_BX + 2 * PF_ML_M)
#define PF_ML_TY (PF_ML_BY + 2 * PF_ML_M)
#define PF_ML_TZ (PF_ML_BZ + 2 * PF_ML_M)
#define PF_ML_CELLS (PF_ML_TX * PF_ML_TY * PF_ML_TZ)

__device__ __forceinline__ int matter_mod(int a, int n) { const int r = a % n; return r < 0 ? r + n : r; }

struct MatterTile {
  u64 *tile, *grid; const int *base; int n, nxl, x0;
  __device__ __forceinline__ void add(int cx, int cy, int cz, u64 w) const {
    if (!w) return;
    const int tx = matter_mod(cx - base[0], n), ty = matter_mod(cy - base[1], n), tz = matter_mod(cz - base[2], n);
    if (tx < PF_ML_TX && ty < PF_ML_TY && tz < PF_ML_TZ) { atomicAdd(&tile[(tx * PF_ML_TY + ty) * PF_ML_TZ + tz], w); return; }
    const int lx = cx - x0;
    if (lx >= 0 && lx < nxl) matter_add(grid + ((size_t)lx * n + (size_t)cy) * n + (size_t)cz, w);
  }
};

template <class T, int NGP>
__global__ void __launch_bounds__(PF_MATTER_BLOCK) k_matter_deposit_lds(MatterCols c, u64 *grid, u64 *counters) {
  __shared__ u64 tile[PF_ML_CELLS];
  __shared__ float dsum[3][PF_MATTER_BLOCK / 64];
  __shared__ int base[3];
  const unsigned int n = (unsigned int)c.n, nbz = n / PF_ML_BZ, nby = n / PF_ML_BY;
  unsigned int b = blockIdx.x;
  const unsigned int kz = b % nbz; b /= nbz;
  const unsigned int ky = b % nby, kx = b / nby;                 // kx < nxl / PF_ML_BX by the launch
  const unsigned int t = threadIdx.x;
  const int org[3] = {c.x0 + (int)(kx * PF_ML_BX), (int)(ky * PF_ML_BY), (int)(kz * PF_ML_BZ)};
  const int q[3] = {org[0] + (int)(t / (PF_ML_BY * PF_ML_BZ)), org[1] + (int)(t / PF_ML_BZ % PF_ML_BY), org[2] + (int)(t % PF_ML_BZ)};
  const size_t i = ((size_t)(q[0] - c.x0) * n + (size_t)q[1]) * n + (size_t)q[2];   // < ncell: every coordinate is inside the slab
  for (int k = t; k < PF_ML_CELLS; k += PF_MATTER_BLOCK) tile[k] = 0;
  const T *col = (const T *)c.vel12;
  const double *w = c.use_w ? c.w : nullptr;
  T pos[3];
  float d[3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    T v[4];
#pragma unroll
    for (int o = 0; o < 4; o++) {
      const int k = 3 * o + j;
      v[o] = k < c.kmax ? pf_matter_column<T>(col[(size_t)k * c.ncell + i], w, o) : (T)0;
    }
    pos[j] = pf_matter_pos<T>(q[j], c.n, v[0], v[1], v[2], v[3]);
    const float dj = (float)v[0] + (float)v[1] + (float)v[2] + (float)v[3];
    d[j] = fabsf(dj) < 1e6f ? dj : 0.0f;                          // (placement only: a value that is not finite counts as none)
    for (int off = warpSize / 2; off; off >>= 1) d[j] += __shfl_down(d[j], off);
    if ((t & (warpSize - 1)) == 0) dsum[j][t / warpSize] = d[j];
  }
  __syncthreads();
  if (t < 3) {
    float m = 0.0f;
    for (int k = 0; k < PF_MATTER_BLOCK / 64; k++) m += dsum[t][k];
    base[t] = org[t] + (int)floorf(m / (float)PF_MATTER_BLOCK + 0.5f) - PF_ML_M;   // |m / 256| < 1e6: no overflow
  }
  __syncthreads();
  const MatterTile mt = {tile, grid, base, c.n, c.nxl, c.x0};
  const int cls = pf_matter_class<T>(pos, c.n);
  if (cls == 0) {
    if (NGP) mt.add(pf_matter_ngp_axis<T>(pos[0], c.n), pf_matter_ngp_axis<T>(pos[1], c.n), pf_matter_ngp_axis<T>(pos[2], c.n), PF_MATTER_ONE);
    else {
      int cell[3][2];
      uint32_t wt[3][2];
#pragma unroll
      for (int j = 0; j < 3; j++) pf_matter_cic_axis<T>(pos[j], c.n, cell[j], wt[j]);
#pragma unroll
      for (int a = 0; a < 2; a++)
#pragma unroll
        for (int bb = 0; bb < 2; bb++) {
          const u64 wxy = (u64)wt[0][a] * wt[1][bb];
          mt.add(cell[0][a], cell[1][bb], cell[2][0], wxy * wt[2][0]);
          mt.add(cell[0][a], cell[1][bb], cell[2][1], wxy * wt[2][1]);
        }
    }
  }
  __syncthreads();
  for (int k = t; k < PF_ML_CELLS; k += PF_MATTER_BLOCK) {
    const u64 v = tile[k];
    if (!v) continue;
    const int tz = k % PF_ML_TZ, ty = k / PF_ML_TZ % PF_ML_TY, tx = k / (PF_ML_TZ * PF_ML_TY);
    const int lx = matter_mod(base[0] + tx, c.n) - c.x0;
    if (lx >= 0 && lx < c.nxl) matter_add(grid + ((size_t)lx * n + (size_t)matter_mod(base[1] + ty, c.n)) * n + (size_t)matter_mod(base[2] + tz, c.n), v);
  }
  u64 *slot = counters + (size_t)(blockIdx.x % PF_MATTER_SLOTS) * MC_COUNT;
  matter_count(cls == 0, slot + MC_DEPOSITED);
  matter_count(cls == 1, slot + MC_NONFINITE);
  matter_count(cls == 2, slot + MC_OUTSIDE);
}

__device__ __forceinline__ u64 matter_wave_sum(u64 v) {
  for (int off = warpSize / 2; off; off >>= 1) v += __shfl_down(v, off);
  return v;
}
__device__ __forceinline__ u64 matter_wave_max(u64 v) {
  for (int off = warpSize / 2; off; off >>= 1) { const u64 o = __shfl_down(v, off); v = o > v ? o : v; }
  return v;
}

// out null: the counters alone (pf_debug_matter_deposit)
template <class F>
__global__ void __launch_bounds__(PF_MATTER_BLOCK) k_matter_contrast(const u64 *grid, size_t ncell, int n, long long pitch, F *out, u64 *counters) {
  const size_t i = (size_t)blockIdx.x * PF_MATTER_BLOCK + threadIdx.x;
  u64 cell = 0, empty = 0, hi = 0, lo = 0;
  if (i < ncell) {
    cell = grid[i];
    empty = cell == 0; hi = cell >> 32; lo = cell & 0xffffffffull;
    if (out) {
      const size_t row = i / (unsigned int)n;
      const double d = ldexp((double)cell, -48) - 1.0;
      out[row * (size_t)pitch + (i - row * (unsigned int)n)] = (F)d;
    }
  }
  const u64 mx = matter_wave_max(cell);
  empty = matter_wave_sum(empty); hi = matter_wave_sum(hi); lo = matter_wave_sum(lo);
  if ((threadIdx.x & (warpSize - 1)) == 0) {
    u64 *slot = counters + (size_t)(blockIdx.x % PF_MATTER_SLOTS) * MC_COUNT;
    matter_max(slot + MC_MAX, mx);
    matter_add(slot + MC_EMPTY, empty); matter_add(slot + MC_SUMHI, hi); matter_add(slot + MC_SUMLO, lo);
  }
}

// ------------------------------------------------------------------------------------------------------------ shell sums ----
// rows [kx][ky_local] of `pitch` complex of both spectra; lin null: no cross sums; C null: no deconvolution
struct MatterView { const void *m, *lin; const double *C; int n, nyl, y0; long long pitch; unsigned int rows, rows_per_wg; };
// the tables in HBM, 64-bit words: one allocation, cleared before the first scan.  smax / pl: [3][nb] and [3][4 nb] by `which`
struct MatterTabs { u64 *smax, *nm, *k2, *pl; double *out; };

template <class F> __device__ __forceinline__ void matter_load(const void *spec, long long pitch, unsigned int row, unsigned int kz, double &re, double &im) {
  const F *e = (const F *)spec + 2 * ((long long)row * pitch + kz);
  if constexpr (sizeof(F) == 8) { const double2 x = *(const double2 *)e; re = x.x; im = x.y; }
  else { const float2 x = *(const float2 *)e; re = (double)x.x; im = (double)x.y; }
}

// the auto and the cross term of mode (row, kz); fin: both are finite (a mode with a term that is not is in no sum)
template <class F> __device__ __forceinline__ void matter_terms(const MatterView &v, unsigned int row, unsigned int kz, double cxy, double &ta, double &tc, bool &fin) {
  double a, b, p = 0.0, q = 0.0;
  matter_load<F>(v.m, v.pitch, row, kz, a, b);
  const double c = v.C ? pf_matter_deconv(cxy, 1.0, v.C[kz]) : -1.0;
  ta = pf_matter_auto(a, b, c);
  tc = 0.0;
  if (v.lin) { matter_load<F>(v.lin, v.pitch, row, kz, p, q); tc = pf_matter_cross(a, b, p, q, c); }
  fin = pf_power_finite(ta) && pf_power_finite(tc);
}
__device__ __forceinline__ unsigned int matter_abs(int s) { return (unsigned int)(s < 0 ? -s : s); }

// what both passes share: the rows of this workgroup one after the other, thread t at the columns kz = t, t + 256, ... <= n/2
template <class F, class OP> __device__ __forceinline__ void matter_walk(const MatterView &v, OP op) {
  const unsigned int r0 = blockIdx.x * v.rows_per_wg, r1 = r0 + v.rows_per_wg < v.rows ? r0 + v.rows_per_wg : v.rows;
  const unsigned int half = (unsigned int)v.n / 2;
  for (unsigned int row = r0; row < r1; row++) {
    const unsigned int kx = row / (unsigned int)v.nyl, yl = row - kx * (unsigned int)v.nyl;
    const int sx = pf_power_signed((int)kx, v.n), sy = pf_power_signed((int)yl + v.y0, v.n);
    const unsigned int kxy2 = (unsigned int)(sx * sx + sy * sy);
    const double cxy = v.C ? v.C[matter_abs(sx)] * v.C[matter_abs(sy)] : 1.0;
    for (unsigned int kz = threadIdx.x; kz <= half; kz += PF_MATTER_BLOCK) {
      const unsigned int k2 = kxy2 + kz * kz, w = (kz > 0 && kz < half) ? 2u : 1u;
      bool fin;
      double ta, tc;
      matter_terms<F>(v, row, kz, cxy, ta, tc, fin);
      op(pf_power_shell(k2), k2, w, ta, tc, fin);
    }
  }
}

// ALL: the maxima of the three sums in one pass (LDS: five tables of nb words, the launch says whether they fit); else that of `which`
// alone (three tables).  nmodes, k2sum and the modes that are not finite are counted by the pass that takes the maximum of sum 0
template <class F, bool ALL>
__global__ void __launch_bounds__(PF_MATTER_BLOCK) k_matter_scan(MatterView v, int which, int nb, MatterTabs g, u64 *counters) {
  extern __shared__ u64 lds[];
  constexpr int NS = ALL ? 3 : 1;
  u64 *smax = lds, *snm = lds + NS * nb, *sk2 = lds + (NS + 1) * nb;
  for (int k = threadIdx.x; k < (NS + 2) * nb; k += PF_MATTER_BLOCK) lds[k] = 0;
  __syncthreads();
  const bool count = ALL || which == 0;
  u64 nonfin = 0;
  matter_walk<F>(v, [&](int b, unsigned int k2, unsigned int w, double ta, double tc, bool fin) {
    if (count) {
      atomicAdd(&snm[b], (u64)w);
      if (k2) atomicAdd(&sk2[b], (u64)w * k2);
      if (!fin) nonfin += (u64)w;
    }
    if (!fin) return;
#pragma unroll
    for (int s = 0; s < NS; s++) {
      const double t = pf_matter_part(ALL ? s : which, ta, tc);
      if (t > 0.0) matter_max_lds(&smax[s * nb + b], (u64)__double_as_longlong(t));
    }
  });
  nonfin = matter_wave_sum(nonfin);
  if ((threadIdx.x & (warpSize - 1)) == 0) matter_add(counters + (size_t)(blockIdx.x % PF_MATTER_SLOTS) * MC_COUNT + MC_NONFIN_MODES, nonfin);
  __syncthreads();
  for (int b = threadIdx.x; b < nb; b += PF_MATTER_BLOCK) {
    if (count && snm[b]) { atomicAdd(&g.nm[b], snm[b]); atomicAdd(&g.k2[b], sk2[b]); }
#pragma unroll
    for (int s = 0; s < NS; s++)
      if (smax[s * nb + b]) atomicMax(&g.smax[(size_t)(ALL ? s : which) * nb + b], smax[s * nb + b]);
  }
}

template <class F>
__global__ void __launch_bounds__(PF_MATTER_BLOCK) k_matter_acc(MatterView v, int which, int nb, MatterTabs g) {
  extern __shared__ u64 lds[];
  u64 *sp = lds;
  int *se = (int *)(lds + 3 * nb);
  for (int k = threadIdx.x; k < 3 * nb; k += PF_MATTER_BLOCK) lds[k] = 0;
  for (int b = threadIdx.x; b < nb; b += PF_MATTER_BLOCK) {
    const u64 m = g.smax[(size_t)which * nb + b];
    se[b] = m ? pf_power_exponent(__longlong_as_double((long long)m)) : 0;
  }
  __syncthreads();
  matter_walk<F>(v, [&](int b, unsigned int, unsigned int w, double ta, double tc, bool fin) {
    const double t = pf_matter_part(which, ta, tc);
    if (!fin || !(t > 0.0)) return;
    uint32_t l[3];
    pf_power_limbs((double)w * t, se[b], l);
#pragma unroll
    for (int i = 0; i < 3; i++)
      if (l[i]) atomicAdd(&sp[3 * b + i], (u64)l[i]);
  });
  __syncthreads();
  // three counters of the workgroup (weights 2^0, 2^32, 2^64) -> four limbs below 2^32 each, added to the four counters in HBM
  for (int b = threadIdx.x; b < nb; b += PF_MATTER_BLOCK) {
    u64 c0 = sp[3 * b], c1 = sp[3 * b + 1], c2 = sp[3 * b + 2];
    if (!(c0 | c1 | c2)) continue;
    c1 += c0 >> 32; c2 += c1 >> 32;
    u64 *gl = g.pl + 4 * ((size_t)which * nb + b);
    matter_add(&gl[0], c0 & 0xffffffffull); matter_add(&gl[1], c1 & 0xffffffffull); matter_add(&gl[2], c2 & 0xffffffffull); matter_add(&gl[3], c2 >> 32);
  }
}

// out: [nb] power, [nb] cross
__global__ void __launch_bounds__(PF_MATTER_BLOCK) k_matter_final(int nb, double n6, MatterTabs g) {
  const int b = blockIdx.x * PF_MATTER_BLOCK + threadIdx.x;
  if (b >= nb) return;
  double s[3];
  for (int which = 0; which < 3; which++) {
    const u64 mx = g.smax[(size_t)which * nb + b];
    s[which] = mx ? pf_power_from_limbs(g.pl + 4 * ((size_t)which * nb + b), 4, pf_power_exponent(__longlong_as_double((long long)mx))) : 0.0;
  }
  g.out[b] = s[0] / n6;
  g.out[nb + b] = (s[1] - s[2]) / n6;
}

// ------------------------------------------------------------------------------------------------------------ launches ----
// PF_MATTER_TIMES=1: device ms of the phases of the last call -- deposit (the clearing of the grid included), contrast, transform,
// shell sums (profiles/tools/matter_time.py)
// (per host thread: two contexts on two threads do not overwrite each other's)
static thread_local double matter_last_ms[4] = {0.0, 0.0, 0.0, 0.0};
// what the calling thread's last call launched: the deposit (0 plain, 1 LDS-staged, -1 none yet) and the scans of its shell passes
static thread_local int matter_last_form = -1, matter_last_scans = 0;
extern "C" int pf_debug_matter_form(int *form) {
  if (!form) return 1;
  form[0] = matter_last_form; form[1] = matter_last_scans;
  return 0;
}
extern "C" int pf_debug_matter_times(double *ms) {
  if (!ms) return 1;
  for (int i = 0; i < 4; i++) ms[i] = matter_last_ms[i];
  return 0;
}
struct MatterTimer {
  hipEvent_t ev[6]; hipStream_t st; bool on; int marks;
  MatterTimer(hipStream_t st_) : st(st_), marks(0) {
    const char *env = getenv("PF_MATTER_TIMES");
    on = env && atoi(env) != 0;
    for (int i = 0; i < 6; i++) ev[i] = nullptr;
    for (int i = 0; i < 4; i++) matter_last_ms[i] = 0.0;
    for (int i = 0; on && i < 6; i++) on = hipEventCreate(&ev[i]) == hipSuccess;
    mark();
  }
  void mark() { if (on && marks < 6) on = hipEventRecord(ev[marks++], st) == hipSuccess; }
  // phase_of_mark[k - 1]: the phase that ended at mark k, -1: none; a phase that did not run keeps 0
  void end(const int *phase_of_mark) {
    if (on && hipEventSynchronize(ev[marks - 1]) == hipSuccess)
      for (int k = 1; k < marks; k++) {
        float ms = 0.0f;
        if (phase_of_mark[k - 1] >= 0 && hipEventElapsedTime(&ms, ev[k - 1], ev[k]) == hipSuccess) matter_last_ms[phase_of_mark[k - 1]] = ms;
      }
    on = false;
  }
  ~MatterTimer() { for (int i = 0; i < 6; i++) if (ev[i]) hipEventDestroy(ev[i]); }
};

struct MatterScratch { u64 *grid, *words; void *in; };
struct MatterGuard { MatterScratch *s; ~MatterGuard() { hipFree(s->grid); hipFree(s->words); hipFree(s->in); s->grid = s->words = nullptr; s->in = nullptr; } };

static bool matter_finite(double x) { return x - x == 0.0; }
static int matter_check_common(const char *who, int task, int flags, const double *weight, const pf_matter_info *info) {
  if (!info) return pf_fail(task, "%s: null argument", who);
  if (flags & ~PF_MATTER_FLAGS) return pf_fail(task, "%s: unknown flag bits 0x%x", who, (unsigned int)(flags & ~PF_MATTER_FLAGS));
  for (int k = 0; weight && k < 4; k++)
    if (!matter_finite(weight[k])) return pf_fail(task, "%s: weight %d is not finite", who, k);
  return 0;
}

// grid (cleared here) += the particles of the slab; counters: MC_WORDS words, cleared by the caller
static int matter_deposit(const char *who, int task, int pb, const MatterCols &c, int flags, u64 *grid, u64 *counters, hipStream_t st) {
  MTHIP(task, who, hipMemsetAsync(grid, 0, c.ncell * 8, st));
  const size_t nblk = (c.ncell + PF_MATTER_BLOCK - 1) / PF_MATTER_BLOCK;
  if (nblk > 0x7fffffffull) return pf_fail(task, "%s: %zu cells are more than one launch takes (internal error)", who, c.ncell);
  const dim3 gr((unsigned int)nblk), bl(PF_MATTER_BLOCK);
  const bool ngp = (flags & PF_MATTER_NGP) != 0;
  const char *env = getenv("PF_MATTER_LDS");
  if ((env ? atoi(env) != 0 : PF_MATTER_LDS_DEFAULT) && c.n % PF_ML_BZ == 0 && c.nxl % PF_ML_BX == 0) {   // (n a multiple of 16 is one of PF_ML_BY too)
    const dim3 gl((unsigned int)(c.ncell / PF_MATTER_BLOCK));
    if (pb == 8) { if (ngp) hipLaunchKernelGGL((k_matter_deposit_lds<double, 1>), gl, bl, 0, st, c, grid, counters); else hipLaunchKernelGGL((k_matter_deposit_lds<double, 0>), gl, bl, 0, st, c, grid, counters); }
    else { if (ngp) hipLaunchKernelGGL((k_matter_deposit_lds<float, 1>), gl, bl, 0, st, c, grid, counters); else hipLaunchKernelGGL((k_matter_deposit_lds<float, 0>), gl, bl, 0, st, c, grid, counters); }
    if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
    matter_last_form = 1;
    return 0;
  }
  matter_last_form = 0;
  if (pb == 8) { if (ngp) hipLaunchKernelGGL((k_matter_deposit<double, 1>), gr, bl, 0, st, c, grid, counters); else hipLaunchKernelGGL((k_matter_deposit<double, 0>), gr, bl, 0, st, c, grid, counters); }
  else { if (ngp) hipLaunchKernelGGL((k_matter_deposit<float, 1>), gr, bl, 0, st, c, grid, counters); else hipLaunchKernelGGL((k_matter_deposit<float, 0>), gr, bl, 0, st, c, grid, counters); }
  if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  return 0;
}
// fb 0: no field, the counters alone
static int matter_contrast(const char *who, int task, int fb, const u64 *grid, size_t ncell, int n, long long pitch, void *field, u64 *counters, hipStream_t st) {
  const dim3 gr((unsigned int)((ncell + PF_MATTER_BLOCK - 1) / PF_MATTER_BLOCK)), bl(PF_MATTER_BLOCK);
  if (fb == 8) hipLaunchKernelGGL((k_matter_contrast<double>), gr, bl, 0, st, grid, ncell, n, pitch, (double *)field, counters);
  else hipLaunchKernelGGL((k_matter_contrast<float>), gr, bl, 0, st, grid, ncell, n, pitch, (float *)(fb ? field : nullptr), counters);
  if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  return 0;
}
static void matter_cols(MatterCols *c, const void *vel12, size_t ncell, int n, int nxl, int x0, int kmax, const double *weight) {
  c->vel12 = vel12; c->ncell = ncell; c->n = n; c->nxl = nxl; c->x0 = x0; c->kmax = kmax; c->use_w = weight != nullptr;
  for (int k = 0; k < 4; k++) c->w[k] = weight ? weight[k] : 1.0;
}

// words of the shell tables: smax [3 nb], nm [nb], k2 [nb], pl [12 nb]; then out [2 nb] doubles and the deconvolution table [n/2 + 1]
static size_t matter_shell_words(int n) { return (size_t)19 * pf_power_nbins(n) + (size_t)(n / 2 + 1); }
// the rows y0 .. y0 + nyl - 1 of two spectra on the device -> this slab's sums in the tables at `words` (matter_shell_words(n) of them, not yet cleared).  Nothing is synchronised
static int matter_shells(const char *who, int task, int fb, const void *spec_m, const void *spec_lin, int n, int y0, int nyl, long long pitch, int flags, u64 *words,
                         u64 *counters, MatterTabs *g, hipStream_t st) {
  const int nb = pf_power_nbins(n), nzh = n / 2 + 1;
  MatterView v;
  v.m = spec_m; v.lin = spec_lin; v.C = nullptr; v.n = n; v.nyl = nyl; v.y0 = y0; v.pitch = pitch;
  v.rows = (unsigned int)n * (unsigned int)nyl;
  v.rows_per_wg = (v.rows + PF_MATTER_MAXWG - 1) / PF_MATTER_MAXWG;
  const unsigned int nwg = (v.rows + v.rows_per_wg - 1) / v.rows_per_wg;
  const size_t lds = (size_t)3 * nb * 8 + (size_t)nb * 4;
  if (lds > PF_MATTER_LDS_MAX) return pf_fail(task, "%s: the %d shells of a grid of %d do not fit the LDS tables", who, nb, n);
  if (((uintptr_t)spec_m | (uintptr_t)spec_lin) & 15) return pf_fail(task, "%s: a spectrum is not 16-byte aligned (internal error)", who);
  MTHIP(task, who, hipMemsetAsync(words, 0, (size_t)19 * nb * 8, st));
  g->smax = words; g->nm = g->smax + 3 * (size_t)nb; g->k2 = g->nm + nb; g->pl = g->k2 + nb; g->out = (double *)(g->pl + 12 * (size_t)nb);
  if (flags & PF_MATTER_DECONVOLVE) {
    std::vector<double> C(nzh);
    for (int j = 0; j < nzh; j++) C[j] = pf_matter_deconv_entry(j, n, (flags & PF_MATTER_NGP) ? 1 : 2);
    double *Cdev = g->out + 2 * (size_t)nb;   // (pageable memory: the copy has left C when the call returns)
    MTHIP(task, who, hipMemcpyAsync(Cdev, C.data(), (size_t)nzh * 8, hipMemcpyHostToDevice, st));
    MTHIP(task, who, hipStreamSynchronize(st));
    v.C = Cdev;
  }
  // with a second spectrum one scan takes the three maxima where its five tables fit (n up to about 1800); PF_MATTER_SCAN_EACH=1
  // (tests only) takes the way of the larger grids: a scan per sum
  const size_t lds_all = (size_t)5 * nb * 8;
  const char *each = getenv("PF_MATTER_SCAN_EACH");
  const bool fused = spec_lin && lds_all <= PF_MATTER_LDS_MAX && !(each && atoi(each) != 0);
  const dim3 gr(nwg), bl(PF_MATTER_BLOCK);
  if (fused) {
    if (fb == 8) hipLaunchKernelGGL((k_matter_scan<double, true>), gr, bl, lds_all, st, v, 0, nb, *g, counters);
    else hipLaunchKernelGGL((k_matter_scan<float, true>), gr, bl, lds_all, st, v, 0, nb, *g, counters);
  }
  for (int which = 0; which < (spec_lin ? 3 : 1); which++) {
    if (!fused) {
      if (fb == 8) hipLaunchKernelGGL((k_matter_scan<double, false>), gr, bl, lds, st, v, which, nb, *g, counters);
      else hipLaunchKernelGGL((k_matter_scan<float, false>), gr, bl, lds, st, v, which, nb, *g, counters);
    }
    if (fb == 8) hipLaunchKernelGGL((k_matter_acc<double>), gr, bl, lds, st, v, which, nb, *g);
    else hipLaunchKernelGGL((k_matter_acc<float>), gr, bl, lds, st, v, which, nb, *g);
    if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  }
  matter_last_scans = fused ? 1 : spec_lin ? 3 : 1;
  const double n3 = (double)n * (double)n * (double)n;
  hipLaunchKernelGGL(k_matter_final, dim3((unsigned int)((nb + PF_MATTER_BLOCK - 1) / PF_MATTER_BLOCK)), dim3(PF_MATTER_BLOCK), 0, st, nb, n3 * n3, *g);
  if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  return 0;
}

// the counters and, with g, the shell sums -> the caller's arrays
static int matter_fetch(const char *who, int task, int n, const u64 *counters, const MatterTabs *g, u64 modes, u64 *nmodes, u64 *k2sum, double *power, double *cross,
                        pf_matter_info *info, hipStream_t st) {
  std::vector<u64> slots((size_t)PF_MATTER_SLOTS * MC_COUNT);
  MTHIP(task, who, hipMemcpyAsync(slots.data(), counters, slots.size() * 8, hipMemcpyDeviceToHost, st));
  if (g) {
    const size_t nb = (size_t)pf_power_nbins(n);
    std::vector<u64> hu(2 * nb);
    std::vector<double> hd(2 * nb);
    MTHIP(task, who, hipMemcpyAsync(hu.data(), g->nm, hu.size() * 8, hipMemcpyDeviceToHost, st));
    MTHIP(task, who, hipMemcpyAsync(hd.data(), g->out, hd.size() * 8, hipMemcpyDeviceToHost, st));
    MTHIP(task, who, hipStreamSynchronize(st));
    memcpy(nmodes, hu.data(), nb * 8); memcpy(k2sum, hu.data() + nb, nb * 8);
    memcpy(power, hd.data(), nb * 8);
    if (cross) memcpy(cross, hd.data() + nb, nb * 8);
  } else MTHIP(task, who, hipStreamSynchronize(st));
  u64 hc[MC_COUNT] = {0};
  for (int k = 0; k < PF_MATTER_SLOTS; k++)
    for (int i = 0; i < MC_COUNT; i++) {
      const u64 v = slots[(size_t)k * MC_COUNT + i];
      if (i == MC_MAX) hc[i] = v > hc[i] ? v : hc[i]; else hc[i] += v;
    }
  info->deposited = hc[MC_DEPOSITED]; info->nonfinite = hc[MC_NONFINITE]; info->outside = hc[MC_OUTSIDE]; info->empty_cells = hc[MC_EMPTY];
  info->max_cell = hc[MC_MAX]; info->sum_hi32 = hc[MC_SUMHI]; info->sum_lo32 = hc[MC_SUMLO]; info->modes = modes; info->nonfinite_modes = hc[MC_NONFIN_MODES];
  return 0;
}

extern "C" int pf_matter_power(pf_ctx *c, int flags, const double *weight, unsigned long long *nmodes, unsigned long long *k2sum, double *power, double *cross,
                               double *density_host, pf_matter_info *info) {
  const char *who = "pf_matter_power";
  if (!c) return pf_fail(0, "%s: null argument", who);
  PfSpecView sv;
  pf_ctx_spec_geometry(c, &sv);
  if (!nmodes || !k2sum || !power) return pf_fail(sv.rank, "%s: null argument", who);
  if (matter_check_common(who, sv.rank, flags, weight, info)) return 1;
  if (sv.P > 1) return pf_fail(sv.rank, "%s: one rank only (this context is rank %d of %d): particles leave their x-slab", who, sv.rank, sv.P);
  if (cross && pf_ctx_spec_view(c, who, 0, &sv)) return 1;   // "density not set" (which = 0: nothing is launched)
  PfCtxView cv;
  pf_ctx_view(c, &cv);
  if (!cv.products_init) return pf_fail(sv.rank, "%s: products not computed", who);
  PfMatterCtx mc;
  pf_ctx_matter_view(c, &mc);
  if (pf_ctx_velocities_ready(c)) return 1;
  MatterScratch s = {nullptr, nullptr, nullptr};
  MatterGuard guard{&s};
  const size_t words = MC_WORDS + matter_shell_words(sv.n), bytes = cv.ncell * 8 + words * 8;
  if (hipMalloc((void **)&s.grid, cv.ncell * 8) != hipSuccess || hipMalloc((void **)&s.words, words * 8) != hipSuccess) {
    (void)hipGetLastError();
    return pf_fail(sv.rank, "%s: cannot allocate %zu bytes of scratch on the device", who, bytes);
  }
  u64 *counters = s.words;
  MTHIP(sv.rank, who, hipMemsetAsync(counters, 0, MC_WORDS * 8, sv.stream));
  MatterTimer timer(sv.stream);
  MatterCols cols;
  matter_cols(&cols, cv.vel12, cv.ncell, cv.n, cv.nxl, mc.x0, mc.lpt_order >= 3 ? 12 : mc.lpt_order == 2 ? 6 : 3, weight);
  if (matter_deposit(who, sv.rank, cv.pb, cols, flags, s.grid, counters, sv.stream)) return 1;
  timer.mark();
  if (matter_contrast(who, sv.rank, sv.fb, s.grid, cv.ncell, cv.n, mc.rpitch, mc.field, counters, sv.stream)) return 1;
  timer.mark();
  int phases[5] = {0, 1, 2, 3, 3}, np = 2;
  if (density_host) {   // the field as the transform will read it, widened to double; its time belongs to no phase
    if (pf_ctx_matter_export(c, density_host)) return 1;
    timer.mark();
    phases[np++] = -1;
  }
  if (pf_ctx_matter_forward(c)) return 1;
  timer.mark();
  phases[np++] = 2;
  MatterTabs g;
  if (matter_shells(who, sv.rank, sv.fb, mc.field, cross ? sv.spec : nullptr, sv.n, sv.y0, sv.nyl, sv.nzp, flags, counters + MC_WORDS, counters, &g, sv.stream)) return 1;
  timer.mark();
  phases[np++] = 3;
  timer.end(phases);
  return matter_fetch(who, sv.rank, sv.n, counters, &g, (u64)sv.n * sv.n * sv.n, nmodes, k2sum, power, cross, info, sv.stream);
}

extern "C" int pf_debug_matter_deposit(int pb, int n, const void *vel12_host, int flags, const double *weight, unsigned long long *grid_host, pf_matter_info *info) {
  const char *who = "pf_debug_matter_deposit";
  if (!vel12_host || !grid_host) return pf_fail(0, "%s: null argument", who);
  if (matter_check_common(who, 0, flags, weight, info)) return 1;
  if (pb != 4 && pb != 8) return pf_fail(0, "%s: products of %d bytes (4 or 8)", who, pb);
  if (n < 2 || n > 512) return pf_fail(0, "%s: a grid of %d (2 to 512)", who, n);
  const size_t ncell = (size_t)n * n * n;
  MatterScratch s = {nullptr, nullptr, nullptr};
  MatterGuard guard{&s};
  if (hipMalloc((void **)&s.grid, ncell * 8) != hipSuccess || hipMalloc((void **)&s.words, MC_WORDS * 8) != hipSuccess || hipMalloc(&s.in, 12 * ncell * pb) != hipSuccess) {
    (void)hipGetLastError();
    return pf_fail(0, "%s: cannot allocate %zu bytes on the device", who, ncell * 8 + MC_WORDS * 8 + 12 * ncell * pb);
  }
  MTHIP(0, who, hipMemcpy(s.in, vel12_host, 12 * ncell * pb, hipMemcpyHostToDevice));
  MTHIP(0, who, hipMemsetAsync(s.words, 0, MC_WORDS * 8, nullptr));
  MatterTimer timer(nullptr);
  MatterCols cols;
  matter_cols(&cols, s.in, ncell, n, n, 0, 12, weight);
  if (matter_deposit(who, 0, pb, cols, flags, s.grid, s.words, nullptr)) return 1;
  timer.mark();
  if (matter_contrast(who, 0, 0, s.grid, ncell, n, n, nullptr, s.words, nullptr)) return 1;
  timer.mark();
  const int phases[4] = {0, 1, 2, 3};
  timer.end(phases);
  MTHIP(0, who, hipMemcpyAsync(grid_host, s.grid, ncell * 8, hipMemcpyDeviceToHost, nullptr));
  return matter_fetch(who, 0, n, s.words, nullptr, 0, nullptr, nullptr, nullptr, nullptr, info, nullptr);
}

extern "C" int pf_debug_matter_shells(int field_bytes, int n, int y0, int nyl, const double *spec_m, const double *spec_lin, int flags, unsigned long long *nmodes,
                                      unsigned long long *k2sum, double *power, double *cross, pf_matter_info *info) {
  const char *who = "pf_debug_matter_shells";
  if (!spec_m || !nmodes || !k2sum || !power) return pf_fail(0, "%s: null argument", who);
  if (matter_check_common(who, 0, flags, nullptr, info)) return 1;
  if (cross && !spec_lin) return pf_fail(0, "%s: cross sums without a second spectrum", who);
  if (field_bytes != 4 && field_bytes != 8) return pf_fail(0, "%s: fields of %d bytes (4 or 8)", who, field_bytes);
  if (n < 2 || n > 2048 || (n & 1)) return pf_fail(0, "%s: a grid of %d (even, 2 to 2048)", who, n);
  if (y0 < 0 || nyl < 1 || y0 + nyl > n) return pf_fail(0, "%s: rows %d .. %d leave the grid of %d", who, y0, y0 + nyl - 1, n);
  // the production layout: rows of whole 128-byte lines, and NaN patterns in the padding that no sum may see
  const int nzh = n / 2 + 1, nzp = n / 2 + 64 / field_bytes;
  const long long nrows = (long long)nyl * n;
  const size_t in_bytes = (size_t)nrows * nzh * 16, field = (size_t)nrows * nzp * 2 * field_bytes;
  const bool two = spec_lin && cross;
  struct Bufs { void *in, *spec; ~Bufs() { hipFree(in); hipFree(spec); } } d = {nullptr, nullptr};
  MatterScratch s = {nullptr, nullptr, nullptr};
  MatterGuard guard{&s};
  const size_t words = MC_WORDS + matter_shell_words(n);
  if (hipMalloc(&d.in, in_bytes) != hipSuccess || hipMalloc(&d.spec, 2 * field) != hipSuccess || hipMalloc((void **)&s.words, words * 8) != hipSuccess) {
    (void)hipGetLastError();
    return pf_fail(0, "%s: cannot allocate %zu bytes on the device", who, in_bytes + 2 * field + words * 8);
  }
  MTHIP(0, who, hipMemset(d.spec, 0xff, 2 * field));
  void *dm = d.spec, *dl = (char *)d.spec + field;
  // [ky_local][kx][kz] of the caller -> [kx][ky_local][kz] rows of nzp
  MTHIP(0, who, hipMemcpy(d.in, spec_m, in_bytes, hipMemcpyHostToDevice));
  if (pf_launch_spec_import_t(field_bytes, (const double *)d.in, dm, n, nyl, nzh, nzp, nullptr)) return pf_fail(0, "%s: launch failed", who);
  if (two) {
    MTHIP(0, who, hipDeviceSynchronize());
    MTHIP(0, who, hipMemcpy(d.in, spec_lin, in_bytes, hipMemcpyHostToDevice));
    if (pf_launch_spec_import_t(field_bytes, (const double *)d.in, dl, n, nyl, nzh, nzp, nullptr)) return pf_fail(0, "%s: launch failed", who);
  }
  MTHIP(0, who, hipMemsetAsync(s.words, 0, MC_WORDS * 8, nullptr));
  MatterTimer timer(nullptr);
  MatterTabs g;
  if (matter_shells(who, 0, field_bytes, dm, two ? dl : nullptr, n, y0, nyl, nzp, flags, s.words + MC_WORDS, s.words, &g, nullptr)) return 1;
  timer.mark();
  const int phases[4] = {3, 3, 3, 3};
  timer.end(phases);
  return matter_fetch(who, 0, n, s.words, &g, (u64)nyl * n * n, nmodes, k2sum, power, cross, info, nullptr);
}
