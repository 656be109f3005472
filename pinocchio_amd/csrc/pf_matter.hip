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
//  k_matter_reach /   pf_matter_power_slabs, the call on more than one rank (at the end of this file): how many planes the particles of
//  k_matter_fold      a slab reach beyond it, and the 64-bit integer add of the ghost planes the other ranks sent into the owner's planes.
//
// Every index is in range by construction: a particle index is below ncell; a target plane is wrapped into [0, n) and deposited only
// when its window plane (plane - w0) mod n is below wn, the planes the grid was allocated with (always, with one rank); target rows and columns are wrapped into [0, n); a mode is read
// at a row below `rows` and a column kz <= n/2 < pitch; a shell is below pf_power_nbins(n), which sized every table; the
// deconvolution table is read at |kx|, |ky|, kz <= n/2, its length less one.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pf_internal.h"
#include "pf_matter_core.h"
#include "pf_matter_slabs_core.h"

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

// the particles are those of the slab [x0, x0 + nxl); the grid holds the wn planes w0, w0 + 1, ... (mod n) of the box -- the slab itself
// with one rank, the slab and its ghost planes or the whole box in pf_matter_power_slabs (pf_matter_slabs_core.h)
struct MatterCols { const void *vel12; size_t ncell; int n, nxl, x0, w0, wn, kmax, use_w; double w[4]; };

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
        const int lx = pf_matter_window_plane(pf_matter_ngp_axis<T>(pos[0], c.n), c.w0, c.wn, c.n);
        if (lx >= 0)
          matter_add(grid + ((size_t)lx * n + (size_t)pf_matter_ngp_axis<T>(pos[1], c.n)) * n + (size_t)pf_matter_ngp_axis<T>(pos[2], c.n), PF_MATTER_ONE);
      } else {
        int cell[3][2];
        uint32_t wt[3][2];
#pragma unroll
        for (int j = 0; j < 3; j++) pf_matter_cic_axis<T>(pos[j], c.n, cell[j], wt[j]);
#pragma unroll
        for (int a = 0; a < 2; a++) {
          const int lx = pf_matter_window_plane(cell[0][a], c.w0, c.wn, c.n);
          if (lx < 0 || !wt[0][a]) continue;
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
// non-negative remainder by n, so its cell is in [0, n)^3, and the plane is deposited only inside the window, as in the plain form.
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
  u64 *tile, *grid; const int *base; int n, w0, wn;
  __device__ __forceinline__ void add(int cx, int cy, int cz, u64 w) const {
    if (!w) return;
    const int tx = matter_mod(cx - base[0], n), ty = matter_mod(cy - base[1], n), tz = matter_mod(cz - base[2], n);
    if (tx < PF_ML_TX && ty < PF_ML_TY && tz < PF_ML_TZ) { atomicAdd(&tile[(tx * PF_ML_TY + ty) * PF_ML_TZ + tz], w); return; }
    const int lx = pf_matter_window_plane(cx, w0, wn, n);
    if (lx >= 0) matter_add(grid + ((size_t)lx * n + (size_t)cy) * n + (size_t)cz, w);
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
  const MatterTile mt = {tile, grid, base, c.n, c.w0, c.wn};
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
    const int lx = pf_matter_window_plane(matter_mod(base[0] + tx, c.n), c.w0, c.wn, c.n);
    if (lx >= 0) matter_add(grid + ((size_t)lx * n + (size_t)matter_mod(base[1] + ty, c.n)) * n + (size_t)matter_mod(base[2] + tz, c.n), v);
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

// ---- the slab form (pf_matter_power_slabs): how far the particles of this slab reach, and the fold of what the other ranks sent ----
// reach: [PF_MATTER_SLOTS][2] words, cleared by the caller: the largest Hlo and Hhi (pf_matter_slabs_core.h) of the workgroups of a
// slot.  One particle per lane as in k_matter_deposit, the four x columns alone (contiguous loads of a wave); a maximum per wave by
// shuffles, per workgroup through LDS, then one atomic per workgroup and side -- and none where the slot already holds as much.
// Indices: i < ncell; a slot is below PF_MATTER_SLOTS
template <class T, int NGP>
__global__ void __launch_bounds__(PF_MATTER_BLOCK) k_matter_reach(MatterCols c, u64 *reach) {
  __shared__ int part[2][PF_MATTER_BLOCK / 64];
  const size_t i = (size_t)blockIdx.x * PF_MATTER_BLOCK + threadIdx.x;
  int lo = 0, hi = 0;
  if (i < c.ncell) {
    const unsigned int n = (unsigned int)c.n;
    const int q0 = c.x0 + (int)(i / n / n);
    const T *col = (const T *)c.vel12;
    const double *w = c.use_w ? c.w : nullptr;
    T v[4];
#pragma unroll
    for (int o = 0; o < 4; o++) v[o] = 3 * o < c.kmax ? pf_matter_column<T>(col[(size_t)(3 * o) * c.ncell + i], w, o) : (T)0;
    int smin, smax;
    if (pf_matter_reach<T>(pf_matter_pos<T>(q0, c.n, v[0], v[1], v[2], v[3]), q0, c.n, NGP, &smin, &smax)) {
      lo = smin < 0 ? -smin : 0; hi = smax > 0 ? smax : 0;
    }
  }
  for (int off = warpSize / 2; off; off >>= 1) {
    const int a = __shfl_down(lo, off), b = __shfl_down(hi, off);
    lo = a > lo ? a : lo; hi = b > hi ? b : hi;
  }
  if ((threadIdx.x & (warpSize - 1)) == 0) { part[0][threadIdx.x / warpSize] = lo; part[1][threadIdx.x / warpSize] = hi; }
  __syncthreads();
  if (threadIdx.x < 2) {
    int m = 0;
    for (int k = 0; k < PF_MATTER_BLOCK / warpSize; k++) m = part[threadIdx.x][k] > m ? part[threadIdx.x][k] : m;
    matter_max(reach + (size_t)(blockIdx.x % PF_MATTER_SLOTS) * 2 + threadIdx.x, (u64)m);
  }
}

// own[l][..] += every received plane whose target is local plane l = blockIdx.y: sources first[l] .. first[l + 1] - 1 of `src`, each
// the index of a plane of `recv` (peer * B + slot).  A thread owns its two words of the plane: plain 16-byte loads and one store,
// 64-bit integer adds, no atomics.  pairs = n^2 / 2 (n is even).  Indices: l < nxl by the launch, a source below P B by the table,
// i < pairs
__global__ void __launch_bounds__(PF_MATTER_BLOCK) k_matter_fold(ulonglong2 *own, const ulonglong2 *recv, const int *first, const int *src, size_t pairs) {
  const int l = blockIdx.y, k0 = first[l], k1 = first[l + 1];
  if (k0 == k1) return;
  for (size_t i = (size_t)blockIdx.x * PF_MATTER_BLOCK + threadIdx.x; i < pairs; i += (size_t)gridDim.x * PF_MATTER_BLOCK) {
    ulonglong2 v = own[(size_t)l * pairs + i];
    for (int k = k0; k < k1; k++) {
      const ulonglong2 a = recv[(size_t)src[k] * pairs + i];
      v.x += a.x; v.y += a.y;
    }
    own[(size_t)l * pairs + i] = v;
  }
}

// out[i] = the largest of slots[p][i], p < P: the maximum over the ranks of `count` words, after the sum over the ranks of vectors in
// which every rank filled its own slot alone
__global__ void __launch_bounds__(PF_MATTER_BLOCK) k_matter_slot_max(const u64 *slots, int P, int count, u64 *out) {
  const int i = blockIdx.x * PF_MATTER_BLOCK + threadIdx.x;
  if (i >= count) return;
  u64 m = 0;
  for (int p = 0; p < P; p++) { const u64 v = slots[(size_t)p * count + i]; m = v > m ? v : m; }
  out[i] = m;
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

// grid (the wn planes of the window, cleared here) += the particles of the slab; counters: MC_WORDS words, cleared by the caller
static int matter_deposit(const char *who, int task, int pb, const MatterCols &c, int flags, u64 *grid, u64 *counters, hipStream_t st) {
  MTHIP(task, who, hipMemsetAsync(grid, 0, (size_t)c.wn * c.n * c.n * 8, st));
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
  c->vel12 = vel12; c->ncell = ncell; c->n = n; c->nxl = nxl; c->x0 = x0; c->w0 = x0; c->wn = nxl; c->kmax = kmax; c->use_w = weight != nullptr;
  for (int k = 0; k < 4; k++) c->w[k] = weight ? weight[k] : 1.0;
}

// words of the shell tables: smax [3 nb], nm [nb], k2 [nb], pl [12 nb]; then out [2 nb] doubles and the deconvolution table [n/2 + 1]
static size_t matter_shell_words(int n) { return (size_t)19 * pf_power_nbins(n) + (size_t)(n / 2 + 1); }
// the rows y0 .. y0 + nyl - 1 of two spectra on the device -> this slab's sums in the tables at `words` (matter_shell_words(n) of them, not yet cleared).  Nothing is synchronised
// coll (more than one rank, collective): the sums of the box on every rank -- the maxima of the scans over the ranks through `slots`
// (P x 3 nb words), then the integer tables summed over the ranks; every all-reduce runs on the context's stream, which is st
struct MatterColl { pf_ctx *c; int P, rank; u64 *slots; };
static int matter_shells(const char *who, int task, int fb, const void *spec_m, const void *spec_lin, int n, int y0, int nyl, long long pitch, int flags, u64 *words,
                         u64 *counters, MatterTabs *g, hipStream_t st, const MatterColl *coll = nullptr) {
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
  // more than one rank: every scan first, then the maxima of the box, so that every limb of every rank is formed under the box's exponent
  for (int pass = coll ? 0 : 1; pass < 2; pass++) {
    for (int which = 0; which < (spec_lin ? 3 : 1); which++) {
      if (!fused && (!coll || pass == 0)) {
        if (fb == 8) hipLaunchKernelGGL((k_matter_scan<double, false>), gr, bl, lds, st, v, which, nb, *g, counters);
        else hipLaunchKernelGGL((k_matter_scan<float, false>), gr, bl, lds, st, v, which, nb, *g, counters);
      }
      if (pass == 1) {
        if (fb == 8) hipLaunchKernelGGL((k_matter_acc<double>), gr, bl, lds, st, v, which, nb, *g);
        else hipLaunchKernelGGL((k_matter_acc<float>), gr, bl, lds, st, v, which, nb, *g);
      }
      if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
    }
    if (coll && pass == 0) {
      const size_t cnt = (size_t)3 * nb;
      MTHIP(task, who, hipMemsetAsync(coll->slots, 0, (size_t)coll->P * cnt * 8, st));
      MTHIP(task, who, hipMemcpyAsync(coll->slots + (size_t)coll->rank * cnt, g->smax, cnt * 8, hipMemcpyDeviceToDevice, st));
      if (pf_ctx_allreduce(coll->c, coll->slots, (size_t)coll->P * cnt, 1)) return 1;
      hipLaunchKernelGGL(k_matter_slot_max, dim3((unsigned int)((cnt + PF_MATTER_BLOCK - 1) / PF_MATTER_BLOCK)), bl, 0, st, coll->slots, coll->P, (int)cnt, g->smax);
      if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
    }
  }
  if (coll && pf_ctx_allreduce(coll->c, g->nm, (size_t)14 * nb, 1)) return 1;   // nm, k2 and the limbs pl lie one behind the other
  matter_last_scans = fused ? 1 : spec_lin ? 3 : 1;
  const double n3 = (double)n * (double)n * (double)n;
  hipLaunchKernelGGL(k_matter_final, dim3((unsigned int)((nb + PF_MATTER_BLOCK - 1) / PF_MATTER_BLOCK)), dim3(PF_MATTER_BLOCK), 0, st, nb, n3 * n3, *g);
  if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  return 0;
}

// a few words of the host summed over the ranks of the context, through `dev` (as many words on the device) on the context's stream
static int matter_agree(const char *who, int task, pf_ctx *c, u64 *dev, std::vector<u64> &a, hipStream_t st) {
  MTHIP(task, who, hipMemcpyAsync(dev, a.data(), a.size() * 8, hipMemcpyHostToDevice, st));
  MTHIP(task, who, hipStreamSynchronize(st));
  if (pf_ctx_allreduce(c, dev, a.size(), 1)) return 1;
  MTHIP(task, who, hipMemcpyAsync(a.data(), dev, a.size() * 8, hipMemcpyDeviceToHost, st));
  MTHIP(task, who, hipStreamSynchronize(st));
  return 0;
}

// the counters and, with g, the shell sums -> the caller's arrays; coll: the counters of the box (collective, through `agree`:
// MC_COUNT + P words on the device)
static int matter_fetch(const char *who, int task, int n, const u64 *counters, const MatterTabs *g, u64 modes, u64 *nmodes, u64 *k2sum, double *power, double *cross,
                        pf_matter_info *info, hipStream_t st, const MatterColl *coll = nullptr, u64 *agree = nullptr) {
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
  if (coll) {   // the box's: sums over the ranks, and the largest cell through a slot per rank
    std::vector<u64> a((size_t)MC_COUNT + coll->P, 0);
    for (int i = 0; i < MC_COUNT; i++) a[i] = i == MC_MAX ? 0 : hc[i];
    a[(size_t)MC_COUNT + coll->rank] = hc[MC_MAX];
    if (matter_agree(who, task, coll->c, agree, a, st)) return 1;
    for (int i = 0; i < MC_COUNT; i++) hc[i] = a[i];
    for (int p = 0; p < coll->P; p++) hc[MC_MAX] = a[(size_t)MC_COUNT + p] > hc[MC_MAX] ? a[(size_t)MC_COUNT + p] : hc[MC_MAX];
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

// ------------------------------------------------------------------------------------------------------------ slabs ----
// pf_matter_power_slabs: the call above on any number of ranks.  The particles of a slab leave it: every rank finds how far
// (k_matter_reach), the ranks agree on the largest reach both ways, every rank deposits into a window of its slab and that many
// ghost planes (or the whole box), the ghost planes travel to their owners in one all-to-all of the context and are added there
// (k_matter_fold).  Integer adds on every rank: the grid is the one-rank grid.  The plan is pf_matter_slabs_core.h's.
static thread_local u64 matter_last_exchange[6] = {0, 0, 0, 0, 0, 0};
extern "C" int pf_debug_matter_exchange(unsigned long long out[6]) {
  if (!out) return 1;
  for (int i = 0; i < 6; i++) out[i] = matter_last_exchange[i];
  return 0;
}

struct SlabBufs { u64 *win, *send, *recv, *words; int *tab; void *cols; };
struct SlabGuard {
  SlabBufs *b;
  ~SlabGuard() { hipFree(b->win); hipFree(b->send); hipFree(b->recv); hipFree(b->words); hipFree(b->tab); hipFree(b->cols); memset(b, 0, sizeof(*b)); }
};
// the words of a call beside the window and the blocks: the counters, the shell tables (shells: a whole call), the reach slots, the
// few words the ranks agree on, and the slots of the scans' maxima
struct SlabWords { size_t shell, reach, agree, slots, total; };
static SlabWords slab_words(int n, int P, bool shells) {
  SlabWords w;
  const size_t a = (size_t)2 * P + 1, b = (size_t)MC_COUNT + P;
  w.shell = MC_WORDS; w.reach = w.shell + (shells ? matter_shell_words(n) : 0); w.agree = w.reach + (size_t)2 * PF_MATTER_SLOTS;
  w.slots = w.agree + (a > b ? a : b);
  w.total = w.slots + (shells && P > 1 ? (size_t)P * 3 * pf_power_nbins(n) : 0);
  return w;
}

// a rank that refuses on its own (its message stands in pf_last_error) still meets the others in the first all-reduce, with its flag
static int slab_refuse(const char *who, pf_ctx *c, const PfSpecView &sv) {
  if (sv.P == 1) return 1;
  u64 *dev = nullptr;
  const size_t cnt = (size_t)2 * sv.P + 1;
  if (hipMalloc((void **)&dev, cnt * 8) != hipSuccess) { (void)hipGetLastError(); return 1; }
  std::vector<u64> a(cnt, 0);
  a[cnt - 1] = 1;
  (void)matter_agree(who, sv.rank, c, dev, a, sv.stream);   // (a successful all-reduce leaves the message as it is)
  hipFree(dev);
  return 1;
}

struct SlabPlan { int hlo, hhi, form, w0, wn, B, own; };

// the window of this rank's slab after deposit, exchange and fold: b->win, the rank's own planes from plane pl->own on.  cols: the
// particle slab (its window is set here); b->words is allocated (slab_words) and its counters are cleared.  Collective
static int slab_grid(const char *who, pf_ctx *c, const PfSpecView &sv, int pb, MatterCols cols, int flags, const SlabWords &sw, SlabBufs *b, SlabPlan *pl) {
  const int task = sv.rank, n = cols.n, P = sv.P, nxl = cols.nxl;
  hipStream_t st = sv.stream;
  u64 *reach = b->words + sw.reach, *agree = b->words + sw.agree;
  const bool ngp = (flags & PF_MATTER_NGP) != 0;
  // 1. the reach of this slab, then of every slab
  MTHIP(task, who, hipMemsetAsync(reach, 0, (size_t)2 * PF_MATTER_SLOTS * 8, st));
  const size_t nblk = (cols.ncell + PF_MATTER_BLOCK - 1) / PF_MATTER_BLOCK;
  if (nblk > 0x7fffffffull) return pf_fail(task, "%s: %zu cells are more than one launch takes (internal error)", who, cols.ncell);
  const dim3 gr((unsigned int)nblk), bl(PF_MATTER_BLOCK);
  if (pb == 8) { if (ngp) hipLaunchKernelGGL((k_matter_reach<double, 1>), gr, bl, 0, st, cols, reach); else hipLaunchKernelGGL((k_matter_reach<double, 0>), gr, bl, 0, st, cols, reach); }
  else { if (ngp) hipLaunchKernelGGL((k_matter_reach<float, 1>), gr, bl, 0, st, cols, reach); else hipLaunchKernelGGL((k_matter_reach<float, 0>), gr, bl, 0, st, cols, reach); }
  if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  std::vector<u64> hr((size_t)2 * PF_MATTER_SLOTS);
  MTHIP(task, who, hipMemcpyAsync(hr.data(), reach, hr.size() * 8, hipMemcpyDeviceToHost, st));
  MTHIP(task, who, hipStreamSynchronize(st));
  u64 hlo = 0, hhi = 0;
  for (int k = 0; k < PF_MATTER_SLOTS; k++) { hlo = hr[2 * k] > hlo ? hr[2 * k] : hlo; hhi = hr[2 * k + 1] > hhi ? hr[2 * k + 1] : hhi; }
  if (P > 1) {
    std::vector<u64> a((size_t)2 * P + 1, 0);
    a[sv.rank] = hlo; a[(size_t)P + sv.rank] = hhi;
    if (matter_agree(who, task, c, agree, a, st)) return 1;
    if (a[(size_t)2 * P]) return pf_fail(task, "%s: refused on another rank of the context", who);
    for (int p = 0; p < P; p++) { hlo = a[p] > hlo ? a[p] : hlo; hhi = a[(size_t)P + p] > hhi ? a[(size_t)P + p] : hhi; }
  }
  pl->hlo = (int)hlo; pl->hhi = (int)hhi;   // (each at most n / 2)
  // 2. the plan, the window and the blocks
  pl->form = pf_matter_exchange_form(n, P, pl->hlo, pl->hhi);
  pf_matter_window(n, nxl, cols.x0, pl->hlo, pl->hhi, &pl->w0, &pl->wn);
  pl->own = pf_matter_window_plane(cols.x0, pl->w0, pl->wn, n);
  pl->B = pl->form ? pf_matter_block_planes(n, P, pl->hlo, pl->hhi) : 0;
  const size_t plane = (size_t)n * n, block = (size_t)pl->B * plane;
  const size_t bytes = ((size_t)pl->wn + 2 * (size_t)P * pl->B) * plane * 8;
  // the fold's table: first[nxl + 1], then the sources by target plane
  std::vector<int> first(nxl + 1, 0), src, list(nxl);
  if (pl->form) {
    std::vector<std::vector<int>> by(nxl);
    for (int p = 0; p < P; p++) {
      if (p == sv.rank) continue;
      const int len = pf_matter_block_list(n, P, pl->hlo, pl->hhi, p, sv.rank, list.data());
      for (int j = 0; j < len; j++) by[list[j]].push_back(p * pl->B + j);
    }
    for (int l = 0; l < nxl; l++) { first[l + 1] = first[l] + (int)by[l].size(); src.insert(src.end(), by[l].begin(), by[l].end()); }
  }
  bool failed = hipMalloc((void **)&b->win, (size_t)pl->wn * plane * 8) != hipSuccess;
  if (pl->form && !failed)
    failed = hipMalloc((void **)&b->send, (size_t)P * block * 8) != hipSuccess || hipMalloc((void **)&b->recv, (size_t)P * block * 8) != hipSuccess ||
             hipMalloc((void **)&b->tab, (first.size() + src.size() + 1) * sizeof(int)) != hipSuccess;
  if (failed) { (void)hipGetLastError(); pf_fail(task, "%s: cannot allocate %zu bytes of scratch on the device", who, bytes + sw.total * 8); }
  if (P > 1) {
    std::vector<u64> a(1, failed ? 1 : 0);
    if (matter_agree(who, task, c, agree, a, st)) return 1;
    if (a[0] && !failed) return pf_fail(task, "%s: another rank of the context cannot allocate its scratch", who);
  }
  if (failed) return 1;
  matter_last_exchange[0] = (u64)pl->form; matter_last_exchange[1] = (u64)pl->hlo; matter_last_exchange[2] = (u64)pl->hhi;
  matter_last_exchange[3] = (u64)pl->wn; matter_last_exchange[4] = (u64)pl->B; matter_last_exchange[5] = (u64)block * 8;
  // 3. deposit, and what leaves and arrives
  cols.w0 = pl->w0; cols.wn = pl->wn;
  if (matter_deposit(who, task, pb, cols, flags, b->win, b->words, st)) return 1;
  if (!pl->form) return 0;
  MTHIP(task, who, hipMemcpyAsync(b->tab, first.data(), first.size() * sizeof(int), hipMemcpyHostToDevice, st));
  if (!src.empty()) MTHIP(task, who, hipMemcpyAsync(b->tab + first.size(), src.data(), src.size() * sizeof(int), hipMemcpyHostToDevice, st));
  MTHIP(task, who, hipStreamSynchronize(st));   // (pageable memory: the tables may go once the copies have left them)
  for (int q = 0; q < P; q++) {
    if (q == sv.rank) continue;
    const int len = pf_matter_block_list(n, P, pl->hlo, pl->hhi, sv.rank, q, list.data());
    for (int j = 0; j < len;) {   // slots j .. e - 1: planes that follow each other in the window too, one copy
      const int wp = pf_matter_window_plane(q * nxl + list[j], pl->w0, pl->wn, n);
      int e = j + 1;
      while (e < len && pf_matter_window_plane(q * nxl + list[e], pl->w0, pl->wn, n) == wp + (e - j)) e++;
      MTHIP(task, who, hipMemcpyAsync(b->send + ((size_t)q * pl->B + j) * plane, b->win + (size_t)wp * plane, (size_t)(e - j) * plane * 8, hipMemcpyDeviceToDevice, st));
      j = e;
    }
  }
  if (pf_ctx_alltoall(c, b->send, b->recv, block * 8)) return 1;
  if (!src.empty()) {
    const size_t pairs = plane / 2, want = (pairs + PF_MATTER_BLOCK - 1) / PF_MATTER_BLOCK;
    const dim3 gf((unsigned int)(want < 4096 ? want : 4096), (unsigned int)nxl);
    hipLaunchKernelGGL(k_matter_fold, gf, bl, 0, st, (ulonglong2 *)(b->win + (size_t)pl->own * plane), (const ulonglong2 *)b->recv, b->tab, b->tab + first.size(), pairs);
    if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  }
  return 0;
}

// what both entry points check before anything is launched -> 1 with the message set
static int slab_check(const char *who, pf_ctx *c, const PfSpecView &sv, int flags, const double *weight, const pf_matter_info *info) {
  if (matter_check_common(who, sv.rank, flags, weight, info)) return 1;
  if (sv.P > 1 && (sv.n & 1)) return pf_fail(sv.rank, "%s: a grid of %d on %d ranks (even sizes only: the fold adds two words at a time)", who, sv.n, sv.P);
  return 0;
}

extern "C" int pf_matter_power_slabs(pf_ctx *c, int flags, const double *weight, unsigned long long *nmodes, unsigned long long *k2sum, double *power, double *cross,
                                     double *density_host, pf_matter_info *info) {
  const char *who = "pf_matter_power_slabs";
  if (!c) return pf_fail(0, "%s: null argument", who);
  PfSpecView sv;
  pf_ctx_spec_geometry(c, &sv);
  if (sv.P > 1 && !pf_ctx_exchange_installed(c)) return pf_fail(sv.rank, "%s: no exchange installed for %d ranks (pf_set_exchange and pf_set_allreduce / pf_init_rccl)", who, sv.P);
  PfCtxView cv;
  pf_ctx_view(c, &cv);
  // every check a rank makes on its own; what it finds it tells the others before anything is launched
  int bad = 0;
  if (!nmodes || !k2sum || !power) bad = pf_fail(sv.rank, "%s: null argument", who);
  if (!bad) bad = slab_check(who, c, sv, flags, weight, info);
  if (!bad && cross) bad = pf_ctx_spec_view(c, who, 0, &sv);   // "density not set" (which = 0: nothing is launched)
  if (!bad && !cv.products_init) bad = pf_fail(sv.rank, "%s: products not computed", who);
  SlabBufs b;
  memset(&b, 0, sizeof(b));
  SlabGuard guard{&b};
  const SlabWords sw = slab_words(sv.n, sv.P, true);
  if (!bad && hipMalloc((void **)&b.words, sw.total * 8) != hipSuccess) {
    (void)hipGetLastError();
    bad = pf_fail(sv.rank, "%s: cannot allocate %zu bytes of scratch on the device", who, sw.total * 8);
  }
  if (bad) return slab_refuse(who, c, sv);
  PfMatterCtx mc;
  pf_ctx_matter_view(c, &mc);
  if (pf_ctx_velocities_ready(c)) return 1;
  u64 *counters = b.words;
  MTHIP(sv.rank, who, hipMemsetAsync(counters, 0, MC_WORDS * 8, sv.stream));
  MatterTimer timer(sv.stream);
  MatterCols cols;
  matter_cols(&cols, cv.vel12, cv.ncell, cv.n, cv.nxl, mc.x0, mc.lpt_order >= 3 ? 12 : mc.lpt_order == 2 ? 6 : 3, weight);
  SlabPlan pl;
  if (slab_grid(who, c, sv, cv.pb, cols, flags, sw, &b, &pl)) return 1;
  timer.mark();
  if (matter_contrast(who, sv.rank, sv.fb, b.win + (size_t)pl.own * cv.n * cv.n, cv.ncell, cv.n, mc.rpitch, mc.field, counters, sv.stream)) return 1;
  timer.mark();
  int phases[5] = {0, 1, 2, 3, 3}, np = 2;
  if (density_host) {
    if (pf_ctx_matter_export(c, density_host)) return 1;
    timer.mark();
    phases[np++] = -1;
  }
  if (pf_ctx_matter_forward(c)) return 1;
  timer.mark();
  phases[np++] = 2;
  MatterTabs g;
  const MatterColl coll = {c, sv.P, sv.rank, b.words + sw.slots};
  const MatterColl *cp = sv.P > 1 ? &coll : nullptr;
  if (matter_shells(who, sv.rank, sv.fb, mc.field, cross ? sv.spec : nullptr, sv.n, sv.y0, sv.nyl, sv.nzp, flags, b.words + sw.shell, counters, &g, sv.stream, cp)) return 1;
  timer.mark();
  phases[np++] = 3;
  timer.end(phases);
  return matter_fetch(who, sv.rank, sv.n, counters, &g, (u64)sv.n * sv.n * sv.n, nmodes, k2sum, power, cross, info, sv.stream, cp, b.words + sw.agree);
}

extern "C" int pf_debug_matter_slabs(pf_ctx *c, const void *vel12_slab_host, int flags, const double *weight, unsigned long long *grid_slab_host, pf_matter_info *info) {
  const char *who = "pf_debug_matter_slabs";
  if (!c) return pf_fail(0, "%s: null argument", who);
  PfSpecView sv;
  pf_ctx_spec_geometry(c, &sv);
  if (sv.P > 1 && !pf_ctx_exchange_installed(c)) return pf_fail(sv.rank, "%s: no exchange installed for %d ranks (pf_set_exchange and pf_set_allreduce / pf_init_rccl)", who, sv.P);
  PfCtxView cv;
  pf_ctx_view(c, &cv);
  int bad = 0;
  if (!vel12_slab_host || !grid_slab_host) bad = pf_fail(sv.rank, "%s: null argument", who);
  if (!bad) bad = slab_check(who, c, sv, flags, weight, info);
  SlabBufs b;
  memset(&b, 0, sizeof(b));
  SlabGuard guard{&b};
  const SlabWords sw = slab_words(sv.n, sv.P, false);
  const size_t col_bytes = 12 * cv.ncell * (size_t)cv.pb;
  if (!bad && (hipMalloc((void **)&b.words, sw.total * 8) != hipSuccess || hipMalloc(&b.cols, col_bytes) != hipSuccess)) {
    (void)hipGetLastError();
    bad = pf_fail(sv.rank, "%s: cannot allocate %zu bytes of scratch on the device", who, sw.total * 8 + col_bytes);
  }
  if (bad) return slab_refuse(who, c, sv);
  MTHIP(sv.rank, who, hipMemcpyAsync(b.cols, vel12_slab_host, col_bytes, hipMemcpyHostToDevice, sv.stream));
  MTHIP(sv.rank, who, hipMemsetAsync(b.words, 0, MC_WORDS * 8, sv.stream));
  MatterTimer timer(sv.stream);
  MatterCols cols;
  matter_cols(&cols, b.cols, cv.ncell, cv.n, cv.nxl, sv.rank * cv.nxl, 12, weight);
  SlabPlan pl;
  if (slab_grid(who, c, sv, cv.pb, cols, flags, sw, &b, &pl)) return 1;
  timer.mark();
  const u64 *own = b.win + (size_t)pl.own * cv.n * cv.n;
  if (matter_contrast(who, sv.rank, 0, own, cv.ncell, cv.n, cv.n, nullptr, b.words, sv.stream)) return 1;
  timer.mark();
  const int phases[4] = {0, 1, 2, 3};
  timer.end(phases);
  MTHIP(sv.rank, who, hipMemcpyAsync(grid_slab_host, own, cv.ncell * 8, hipMemcpyDeviceToHost, sv.stream));
  const MatterColl coll = {c, sv.P, sv.rank, nullptr};
  return matter_fetch(who, sv.rank, sv.n, b.words, nullptr, 0, nullptr, nullptr, nullptr, nullptr, info, sv.stream, sv.P > 1 ? &coll : nullptr, b.words + sw.agree);
}
