// pf_matter.hip -- the density of the LPT-displaced particles and its spectra (include/pinfmax.h: pf_matter_power and its taps): mass
// assignment of one particle per cell at the reference's initialize_POS positions (src/write_snapshot.c:907-954) into a grid of
// 64-bit integers, the density contrast into a scratch field, the context's own forward transform, and per-shell sums of
// |delta_m|^2 and Re(delta_m conj delta) with the resident delta(k).  The arithmetic of a particle is pf_matter_core.h's.
// The reference has no counterpart beyond the plots it commits for its mode 3.
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
//  k_matter_reach /   pf_matter_power_slabs, the call on more than one rank: how many planes the particles of a slab reach beyond it, and
//  k_matter_fold      the 64-bit integer add of the ghost planes the other ranks sent into the owner's planes.
// The shell sums of the two spectra are pf_power.hip's (pf_matter_shells_device, pf_internal.h): one scan, or a scan per sum, and an
// accumulation per sum -- four passes over the two spectra (profiles/matter_notes.md).
//
// Every index is in range by construction: a particle index is below ncell; a target plane is wrapped into [0, n) and deposited only
// when its window plane (plane - w0) mod n is below wn, the planes the grid was allocated with (always, with one rank); target rows
// and columns are wrapped into [0, n).
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
#define PF_MATTER_FLAGS (PF_MATTER_NGP | PF_MATTER_DECONVOLVE)
#define PF_MATTER_LDS_DEFAULT 1   // PF_MATTER_LDS unset: the LDS-staged deposit, 70 ms against 329 at 1024^3 (the A/B: profiles/matter_notes.md)

typedef unsigned long long u64;

// the counters of a call on the device (pf_internal.h): PF_MATTER_SLOTS copies of each
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

// what a call holds on the device beside the context's own: the window of the grid, the blocks that leave and arrive with the fold's
// table, the words (slab_words) and, in a tap, the caller's columns
struct MatterBufs { u64 *win, *send, *recv, *words; int *tab; void *cols; };
struct MatterGuard {
  MatterBufs *b;
  ~MatterGuard() { hipFree(b->win); hipFree(b->send); hipFree(b->recv); hipFree(b->words); hipFree(b->tab); hipFree(b->cols); memset(b, 0, sizeof(*b)); }
};
// the instantiation of a kernel template <class T, int NGP> for products of pb bytes and the assignment of the call
#define MATTER_KERNEL(k, pb, ngp) ((pb) == 8 ? ((ngp) ? k<double, 1> : k<double, 0>) : ((ngp) ? k<float, 1> : k<float, 0>))

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
    hipLaunchKernelGGL(MATTER_KERNEL(k_matter_deposit_lds, pb, ngp), gl, bl, 0, st, c, grid, counters);
    if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
    matter_last_form = 1;
    return 0;
  }
  matter_last_form = 0;
  hipLaunchKernelGGL(MATTER_KERNEL(k_matter_deposit, pb, ngp), gr, bl, 0, st, c, grid, counters);
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
static int matter_fetch(const char *who, int task, int n, const u64 *counters, const PfShellSums *g, u64 modes, u64 *nmodes, u64 *k2sum, double *power, double *cross,
                        pf_matter_info *info, hipStream_t st, pf_ctx *coll = nullptr, u64 *agree = nullptr) {
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
    PfSpecView sv;
    pf_ctx_spec_geometry(coll, &sv);
    std::vector<u64> a((size_t)MC_COUNT + sv.P, 0);
    for (int i = 0; i < MC_COUNT; i++) a[i] = i == MC_MAX ? 0 : hc[i];
    a[(size_t)MC_COUNT + sv.rank] = hc[MC_MAX];
    if (matter_agree(who, task, coll, agree, a, st)) return 1;
    for (int i = 0; i < MC_COUNT; i++) hc[i] = a[i];
    for (int p = 0; p < sv.P; p++) hc[MC_MAX] = a[(size_t)MC_COUNT + p] > hc[MC_MAX] ? a[(size_t)MC_COUNT + p] : hc[MC_MAX];
  }
  info->deposited = hc[MC_DEPOSITED]; info->nonfinite = hc[MC_NONFINITE]; info->outside = hc[MC_OUTSIDE]; info->empty_cells = hc[MC_EMPTY];
  info->max_cell = hc[MC_MAX]; info->sum_hi32 = hc[MC_SUMHI]; info->sum_lo32 = hc[MC_SUMLO]; info->modes = modes; info->nonfinite_modes = hc[MC_NONFIN_MODES];
  return 0;
}

// ------------------------------------------------------------------------------------------------------------ slabs ----
// the grid of a call on any number of ranks (pf_matter_power_slabs; pf_matter_power is its one-rank case without the reach pass).
// The particles of a slab leave it: every rank finds how far
// (k_matter_reach), the ranks agree on the largest reach both ways, every rank deposits into a window of its slab and that many
// ghost planes (or the whole box), the ghost planes travel to their owners in one all-to-all of the context and are added there
// (k_matter_fold).  Integer adds on every rank: the grid is the one-rank grid.  The plan is pf_matter_slabs_core.h's.
static thread_local u64 matter_last_exchange[6] = {0, 0, 0, 0, 0, 0};
extern "C" int pf_debug_matter_exchange(unsigned long long out[6]) {
  if (!out) return 1;
  for (int i = 0; i < 6; i++) out[i] = matter_last_exchange[i];
  return 0;
}

// the words of a call beside the window and the blocks: the counters, the words of the shell sums (shells: a whole call), the reach
// slots, and the few words the ranks agree on
struct SlabWords { size_t shell, reach, agree, total; };
static SlabWords slab_words(int n, int P, bool shells) {
  SlabWords w;
  const size_t a = (size_t)2 * P + 1, b = (size_t)MC_COUNT + P;
  w.shell = MC_WORDS; w.reach = w.shell + (shells ? pf_matter_shells_words(n, P) : 0); w.agree = w.reach + (size_t)2 * PF_MATTER_SLOTS;
  w.total = w.agree + (a > b ? a : b);
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
// particle slab (its window is set here); b->words is allocated (slab_words) and its counters are cleared.  Collective.
// reach false (pf_matter_power: one rank, whose window is its slab whatever the reach): no reach pass, and what
// pf_debug_matter_exchange reports stays
static int matter_grid(const char *who, pf_ctx *c, const PfSpecView &sv, int pb, MatterCols cols, int flags, bool reach, const SlabWords &sw, MatterBufs *b, SlabPlan *pl) {
  const int task = sv.rank, n = cols.n, P = sv.P, nxl = cols.nxl;
  hipStream_t st = sv.stream;
  u64 *agree = b->words + sw.agree;
  const dim3 bl(PF_MATTER_BLOCK);
  // 1. the reach of this slab, then of every slab
  u64 hlo = 0, hhi = 0;
  if (reach) {
    u64 *slots = b->words + sw.reach;
    MTHIP(task, who, hipMemsetAsync(slots, 0, (size_t)2 * PF_MATTER_SLOTS * 8, st));
    const size_t nblk = (cols.ncell + PF_MATTER_BLOCK - 1) / PF_MATTER_BLOCK;
    if (nblk > 0x7fffffffull) return pf_fail(task, "%s: %zu cells are more than one launch takes (internal error)", who, cols.ncell);
    hipLaunchKernelGGL(MATTER_KERNEL(k_matter_reach, pb, (flags & PF_MATTER_NGP) != 0), dim3((unsigned int)nblk), bl, 0, st, cols, slots);
    if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
    std::vector<u64> hr((size_t)2 * PF_MATTER_SLOTS);
    MTHIP(task, who, hipMemcpyAsync(hr.data(), slots, hr.size() * 8, hipMemcpyDeviceToHost, st));
    MTHIP(task, who, hipStreamSynchronize(st));
    for (int k = 0; k < PF_MATTER_SLOTS; k++) { hlo = hr[2 * k] > hlo ? hr[2 * k] : hlo; hhi = hr[2 * k + 1] > hhi ? hr[2 * k + 1] : hhi; }
  }
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
  bool failed = !b->win && hipMalloc((void **)&b->win, (size_t)pl->wn * plane * 8) != hipSuccess;   // (without a reach pass the caller brought it)
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
  if (reach) {
    matter_last_exchange[0] = (u64)pl->form; matter_last_exchange[1] = (u64)pl->hlo; matter_last_exchange[2] = (u64)pl->hhi;
    matter_last_exchange[3] = (u64)pl->wn; matter_last_exchange[4] = (u64)pl->B; matter_last_exchange[5] = (u64)block * 8;
  }
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

// what the calls on a context check before anything is launched -> 1 with the message set.  slabs false: pf_matter_power
static int slab_check(const char *who, const PfSpecView &sv, bool slabs, int flags, const double *weight, const pf_matter_info *info) {
  if (matter_check_common(who, sv.rank, flags, weight, info)) return 1;
  if (!slabs && sv.P > 1) return pf_fail(sv.rank, "%s: one rank only (this context is rank %d of %d): particles leave their x-slab", who, sv.rank, sv.P);
  if (sv.P > 1 && (sv.n & 1)) return pf_fail(sv.rank, "%s: a grid of %d on %d ranks (even sizes only: the fold adds two words at a time)", who, sv.n, sv.P);
  return 0;
}

// pf_matter_power (slabs false) and pf_matter_power_slabs: checks, scratch, deposit, contrast, the export on request, the forward
// transform, the shell sums, the fetch.  The first refuses more than one rank and then needs neither the reach pass nor an agreement
static int matter_power_call(const char *who, bool slabs, pf_ctx *c, int flags, const double *weight, u64 *nmodes, u64 *k2sum, double *power, double *cross,
                             double *density_host, pf_matter_info *info) {
  if (!c) return pf_fail(0, "%s: null argument", who);
  PfSpecView sv;
  pf_ctx_spec_geometry(c, &sv);
  if (slabs && sv.P > 1 && !pf_ctx_exchange_installed(c))
    return pf_fail(sv.rank, "%s: no exchange installed for %d ranks (pf_set_exchange and pf_set_allreduce / pf_init_rccl)", who, sv.P);
  PfCtxView cv;
  pf_ctx_view(c, &cv);
  // every check a rank makes on its own; what it finds it tells the others before anything is launched
  int bad = 0;
  if (!nmodes || !k2sum || !power) bad = pf_fail(sv.rank, "%s: null argument", who);
  if (!bad) bad = slab_check(who, sv, slabs, flags, weight, info);
  if (!bad && cross) bad = pf_ctx_spec_view(c, who, 0, &sv);   // "density not set" (which = 0: nothing is launched)
  if (!bad && !cv.products_init) bad = pf_fail(sv.rank, "%s: products not computed", who);
  MatterBufs b;
  memset(&b, 0, sizeof(b));
  MatterGuard guard{&b};
  const SlabWords sw = slab_words(sv.n, sv.P, true);
  // (the window of pf_matter_power is its slab: allocated here, before the timer, and not as the slab call's inside its deposit phase)
  const size_t bytes = sw.total * 8 + (slabs ? 0 : cv.ncell * 8);
  if (!bad && (hipMalloc((void **)&b.words, sw.total * 8) != hipSuccess || (!slabs && hipMalloc((void **)&b.win, cv.ncell * 8) != hipSuccess))) {
    (void)hipGetLastError();
    bad = pf_fail(sv.rank, "%s: cannot allocate %zu bytes of scratch on the device", who, bytes);
  }
  if (bad) return slabs ? slab_refuse(who, c, sv) : 1;
  PfMatterCtx mc;
  pf_ctx_matter_view(c, &mc);
  if (pf_ctx_velocities_ready(c)) return 1;
  u64 *counters = b.words;
  MTHIP(sv.rank, who, hipMemsetAsync(counters, 0, MC_WORDS * 8, sv.stream));
  MatterTimer timer(sv.stream);
  MatterCols cols;
  matter_cols(&cols, cv.vel12, cv.ncell, cv.n, cv.nxl, mc.x0, mc.lpt_order >= 3 ? 12 : mc.lpt_order == 2 ? 6 : 3, weight);
  SlabPlan pl;
  if (matter_grid(who, c, sv, cv.pb, cols, flags, slabs, sw, &b, &pl)) return 1;
  timer.mark();
  if (matter_contrast(who, sv.rank, sv.fb, b.win + (size_t)pl.own * cv.n * cv.n, cv.ncell, cv.n, mc.rpitch, mc.field, counters, sv.stream)) return 1;
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
  PfShellSums g;
  pf_ctx *coll = sv.P > 1 ? c : nullptr;
  if (pf_matter_shells_device(who, sv.rank, sv.fb, mc.field, cross ? sv.spec : nullptr, sv.n, sv.y0, sv.nyl, sv.nzp, flags, b.words + sw.shell, counters, coll, &g,
                              sv.stream))
    return 1;
  matter_last_scans = g.scans;
  timer.mark();
  phases[np++] = 3;
  timer.end(phases);
  return matter_fetch(who, sv.rank, sv.n, counters, &g, (u64)sv.n * sv.n * sv.n, nmodes, k2sum, power, cross, info, sv.stream, coll, b.words + sw.agree);
}
extern "C" int pf_matter_power(pf_ctx *c, int flags, const double *weight, unsigned long long *nmodes, unsigned long long *k2sum, double *power, double *cross,
                               double *density_host, pf_matter_info *info) {
  return matter_power_call("pf_matter_power", false, c, flags, weight, nmodes, k2sum, power, cross, density_host, info);
}
extern "C" int pf_matter_power_slabs(pf_ctx *c, int flags, const double *weight, unsigned long long *nmodes, unsigned long long *k2sum, double *power, double *cross,
                                     double *density_host, pf_matter_info *info) {
  return matter_power_call("pf_matter_power_slabs", true, c, flags, weight, nmodes, k2sum, power, cross, density_host, info);
}

// ------------------------------------------------------------------------------------------------------------ taps ----
// what the two deposit taps end with: the contrast pass without a field, the grid to the host, the counters
static int matter_tap_tail(const char *who, int task, MatterTimer &timer, const u64 *grid, size_t ncell, int n, u64 *counters, u64 *grid_host, pf_matter_info *info,
                           hipStream_t st, pf_ctx *coll = nullptr, u64 *agree = nullptr) {
  timer.mark();
  if (matter_contrast(who, task, 0, grid, ncell, n, n, nullptr, counters, st)) return 1;
  timer.mark();
  const int phases[4] = {0, 1, 2, 3};
  timer.end(phases);
  MTHIP(task, who, hipMemcpyAsync(grid_host, grid, ncell * 8, hipMemcpyDeviceToHost, st));
  return matter_fetch(who, task, n, counters, nullptr, 0, nullptr, nullptr, nullptr, nullptr, info, st, coll, agree);
}

extern "C" int pf_debug_matter_deposit(int pb, int n, const void *vel12_host, int flags, const double *weight, unsigned long long *grid_host, pf_matter_info *info) {
  const char *who = "pf_debug_matter_deposit";
  if (!vel12_host || !grid_host) return pf_fail(0, "%s: null argument", who);
  if (matter_check_common(who, 0, flags, weight, info)) return 1;
  if (pb != 4 && pb != 8) return pf_fail(0, "%s: products of %d bytes (4 or 8)", who, pb);
  if (n < 2 || n > 512) return pf_fail(0, "%s: a grid of %d (2 to 512)", who, n);
  const size_t ncell = (size_t)n * n * n;
  MatterBufs b;
  memset(&b, 0, sizeof(b));
  MatterGuard guard{&b};
  if (hipMalloc((void **)&b.win, ncell * 8) != hipSuccess || hipMalloc((void **)&b.words, MC_WORDS * 8) != hipSuccess || hipMalloc(&b.cols, 12 * ncell * pb) != hipSuccess) {
    (void)hipGetLastError();
    return pf_fail(0, "%s: cannot allocate %zu bytes on the device", who, ncell * 8 + MC_WORDS * 8 + 12 * ncell * pb);
  }
  MTHIP(0, who, hipMemcpy(b.cols, vel12_host, 12 * ncell * pb, hipMemcpyHostToDevice));
  MTHIP(0, who, hipMemsetAsync(b.words, 0, MC_WORDS * 8, nullptr));
  MatterTimer timer(nullptr);
  MatterCols cols;
  matter_cols(&cols, b.cols, ncell, n, n, 0, 12, weight);
  if (matter_deposit(who, 0, pb, cols, flags, b.win, b.words, nullptr)) return 1;
  return matter_tap_tail(who, 0, timer, b.win, ncell, n, b.words, grid_host, info, nullptr);
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
  if (!bad) bad = slab_check(who, sv, true, flags, weight, info);
  MatterBufs b;
  memset(&b, 0, sizeof(b));
  MatterGuard guard{&b};
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
  if (matter_grid(who, c, sv, cv.pb, cols, flags, true, sw, &b, &pl)) return 1;
  return matter_tap_tail(who, sv.rank, timer, b.win + (size_t)pl.own * cv.n * cv.n, cv.ncell, cv.n, b.words, grid_slab_host, info, sv.stream, sv.P > 1 ? c : nullptr,
                         b.words + sw.agree);
}

extern "C" int pf_debug_matter_shells(int field_bytes, int n, int y0, int nyl, const double *spec_m, const double *spec_lin, int flags, unsigned long long *nmodes,
                                      unsigned long long *k2sum, double *power, double *cross, pf_matter_info *info) {
  const char *who = "pf_debug_matter_shells";
  if (!spec_m || !nmodes || !k2sum || !power) return pf_fail(0, "%s: null argument", who);
  if (matter_check_common(who, 0, flags, nullptr, info)) return 1;
  if (cross && !spec_lin) return pf_fail(0, "%s: cross sums without a second spectrum", who);
  const bool two = spec_lin && cross;
  PfSpecStage d = {};
  if (pf_stage_spectra(who, field_bytes, n, y0, nyl, 2, spec_m, two ? spec_lin : nullptr, MC_WORDS + pf_matter_shells_words(n, 1), &d)) return 1;
  MTHIP(0, who, hipMemsetAsync(d.words, 0, MC_WORDS * 8, nullptr));
  MatterTimer timer(nullptr);
  PfShellSums g;
  if (pf_matter_shells_device(who, 0, field_bytes, d.spec[0], two ? d.spec[1] : nullptr, n, y0, nyl, d.nzp, flags, d.words + MC_WORDS, d.words, nullptr, &g, nullptr)) return 1;
  matter_last_scans = g.scans;
  timer.mark();
  const int phases[4] = {3, 3, 3, 3};
  timer.end(phases);
  return matter_fetch(who, 0, n, d.words, &g, (u64)nyl * n * n, nmodes, k2sum, power, cross, info, nullptr);
}
