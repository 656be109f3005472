// pf_peaks.hip -- count_peaks (src/fragment.c:605-706) on the device: the step of fragmentation that follows the selection of
// pf_select_sort.hip.  A cell is stored when Fmax >= Flast (update_distmap, src/distribute.c:695); a stored cell is a peak when
// its Fmax is strictly larger than that of every one of its six grid neighbours that is stored too (:637-686, the default,
// non-CLASSIC_FRAGMENTATION form: a neighbour that is not in the list vetoes nothing).  Peaks are the seeds of the halos.
//
// One kernel, k_peaks.  The pass is bound by HBM and reads the column about once:
//  * a thread owns a column of the slab -- TY consecutive rows (y) times V consecutive cells along z, V cells = one 16-byte load --
//    and marches along x with the planes x and x + 1 of its column in registers (rotating) and one bit per cell for what plane
//    x - 1 had to say: the x-neighbours and the y-neighbours inside the column cost no load at all;
//  * the two y-halo rows of the column are re-read once per plane: (TY + 2) / TY = 1.25 of the bytes for TY = 8;
//  * the z-neighbours of the first and last cell of a 16-byte piece come from the neighbouring lanes (ds_bpermute); only a lane whose
//    neighbour lies in another wavefront (lanes 0 and 63, the periodic wrap of a row) loads that one cell, from a line the
//    neighbouring wavefront of the same workgroup has just fetched;
//  * the march of a column is cut into chunks of x (blockIdx.y) to fill the device: 2 / chunk more bytes.
// A region (sub-box of the periodic box, src/fragment.c:630-635 and :691-694) only selects which cells are examined: a cell
// that is examined has all six neighbours inside the region, at the global coordinates +-1 (mod n).
// Counting: per-lane counters over the whole march, one 64-bit atomic per wavefront and counter at the end.  KEYS: the sort
// keys of pf_select_sort.hip appended with one atomic per wavefront and plane.
// MAP (pf_count_peaks_map): the stored set is a subset of the region's cells -- bit set in a resident map (pf_map.hip) of the region's
// box AND Fmax >= Flast.  Every value passes through the map as it is loaded: a cell whose bit is clear, or that lies outside the
// box, becomes NaN, which every comparison below already treats as "not stored, vetoes nothing".  The other instantiations do
// not see the map at all (their arguments are the plain PkArgs).
#include <hip/hip_runtime.h>

#include <math.h>

#include <type_traits>

#include "pf_internal.h"
#include "pf_keys.h"

#define PF_PEAK_BLOCK 256
#define PF_PEAK_TY 8

template <typename PR, int V>
struct alignas(sizeof(PR) * V) PkVec { PR v[V]; };

template <typename PR, int V>
__device__ __forceinline__ PkVec<PR, V> pk_load(const PR *p) { return *reinterpret_cast<const PkVec<PR, V> *>(p); }

struct PkArgs {
  const void *fmax, *halo_lo, *halo_hi;
  int n, nxl, x0, xchunk;
  int start[3], lo[3], hi[3], glo[3], ghi[3];
  unsigned long long *counters, *keys;
  unsigned long long key_cap;
};

struct PkMapArgs : PkArgs {
  const unsigned int *map;   // bit z + Lz (y + Ly x) of the box start[], mlen[]
  int mlen[3];
};

// bit i of the result: coordinate c0 + i (global, mod n) lies in [lo, hi) of the region's own coordinates
__device__ __forceinline__ unsigned int pk_range_mask(int c0, int count, int n, int start, int lo, int hi) {
  unsigned int m = 0;
  for (int i = 0; i < count; i++) {
    int l = (c0 + i) % n - start;
    if (l < 0) l += n;
    if (l >= lo && l < hi) m |= 1u << i;
  }
  return m;
}

template <typename PR, int V, bool KEYS, bool MAP = false>
__global__ void __launch_bounds__(PF_PEAK_BLOCK) k_peaks(typename std::conditional<MAP, PkMapArgs, PkArgs>::type a, PR thr) {
  constexpr int TY = PF_PEAK_TY;
  typedef PkVec<PR, V> Vec;
  const int n = a.n, nzv = n / V, nyg = (n + TY - 1) / TY;
  const long long ncols = (long long)nyg * nzv;
  const int lane = threadIdx.x & 63;
  const long long wave_first = (long long)blockIdx.x * blockDim.x + (threadIdx.x - lane);
  long long col = wave_first + lane;
  const bool valid = col < ncols;
  if (!valid) col = ncols - 1;  // (works on a copy of the last column and counts nothing: every lane of a wave runs the shuffles)
  const int yg = (int)(col / nzv), zq = (int)(col - (long long)yg * nzv);
  const int yb = yg * TY, z0 = zq * V;
  const int xa = blockIdx.y * a.xchunk, xb = min(a.nxl, xa + a.xchunk);

  // element offsets inside a plane
  unsigned int row[TY];  // (n <= 2048: a plane has at most 2^22 cells)
#pragma unroll
  for (int r = 0; r < TY; r++) row[r] = (unsigned int)((yb + r) % n) * n + z0;
  const unsigned int row_lo = (unsigned int)((yb + n - 1) % n) * n + z0, row_hi = (unsigned int)((yb + TY) % n) * n + z0;
  // z-neighbours across the 16-byte piece: the lane that holds them, or (outside this wavefront) their offset from z0
  const long long src_l = (long long)yg * nzv + (zq == 0 ? nzv - 1 : zq - 1) - wave_first;
  const long long src_r = (long long)yg * nzv + (zq == nzv - 1 ? 0 : zq + 1) - wave_first;
  const bool in_l = src_l >= 0 && src_l < 64, in_r = src_r >= 0 && src_r < 64;
  const int lane_l = in_l ? (int)src_l : lane, lane_r = in_r ? (int)src_r : lane;
  const long long off_l = (z0 == 0 ? n - 1 : z0 - 1) - z0, off_r = (z0 + V == n ? 0 : z0 + V) - z0;

  // the region: which of my cells are examined / well resolved (y, z fixed over the march)
  unsigned int ym = pk_range_mask(yb, TY, n, a.start[1], a.lo[1], a.hi[1]);
  unsigned int ymg = pk_range_mask(yb, TY, n, a.start[1], a.glo[1], a.ghi[1]);
#pragma unroll
  for (int r = 0; r < TY; r++) if (yb + r >= n) { ym &= ~(1u << r); ymg &= ~(1u << r); }  // (a last column of fewer than TY rows)
  if (!valid) ym = 0;
  const unsigned int zm = pk_range_mask(z0, V, n, a.start[2], a.lo[2], a.hi[2]);
  const unsigned int zmg = pk_range_mask(z0, V, n, a.start[2], a.glo[2], a.ghi[2]);

  const size_t plane = (size_t)n * n;
  const PR *slab = (const PR *)a.fmax;
  auto plane_of = [&](int xl) -> const PR * {
    return xl < 0 ? (const PR *)a.halo_lo : xl >= a.nxl ? (const PR *)a.halo_hi : slab + (size_t)xl * plane;
  };

  // MAP: the box coordinates of my rows (y-halo rows first and last) and cells (z-neighbours first and last), -1 outside the box
  int my[MAP ? TY + 2 : 1], mz[MAP ? V + 2 : 1];
  auto box_coord = [&](int g, int d) -> int {
    if constexpr (MAP) {
      int l = g % n - a.start[d];
      if (l < 0) l += n;
      return l < a.mlen[d] ? l : -1;
    } else return 0;
  };
  // the value of the cell (lx, ly, lz) of the box as the stored set sees it
  auto through = [&](PR f, int lx, int ly, int lz) -> PR {
    if constexpr (MAP) {
      if ((lx | ly | lz) < 0) return (PR)NAN;
      const unsigned int pos = ((unsigned int)lx * (unsigned int)a.mlen[1] + (unsigned int)ly) * (unsigned int)a.mlen[2] + (unsigned int)lz;   // (< 2^32 cells)
      return ((a.map[pos >> 5] >> (pos & 31u)) & 1u) ? f : (PR)NAN;
    } else return f;
  };
  auto through_vec = [&](Vec v, int lx, int ly) -> Vec {
    if constexpr (MAP) {
#pragma unroll
      for (int e = 0; e < V; e++) v.v[e] = through(v.v[e], lx, ly, mz[e + 1]);
    }
    return v;
  };
  auto plane_coord = [&](int xl) -> int { return box_coord(a.x0 + xl + n, 0); };
  if constexpr (MAP) {
    my[0] = box_coord(yb + n - 1, 1); my[TY + 1] = box_coord(yb + TY, 1);
#pragma unroll
    for (int r = 0; r < TY; r++) my[r + 1] = box_coord(yb + r, 1);
    mz[0] = box_coord(z0 == 0 ? n - 1 : z0 - 1, 2); mz[V + 1] = box_coord(z0 + V == n ? 0 : z0 + V, 2);
#pragma unroll
    for (int e = 0; e < V; e++) mz[e + 1] = box_coord(z0 + e, 2);
  }
  int lxc = 0, lxn = 0;   // box x of the planes in cur and nxt

  unsigned int cnt = 0, cntg = 0;
  // planes x and x + 1 of the column in registers; of plane x - 1 only what it says about plane x: bit r V + e of `below` is set when
  // its cell is no smaller than the cell (r, e) of the plane in `cur`
  Vec cur[TY], nxt[TY];
  unsigned int below = 0;
  if (xa < xb) {
    const PR *pp = plane_of(xa - 1), *pc = plane_of(xa);
    const int lxp = plane_coord(xa - 1);
    lxc = plane_coord(xa);
#pragma unroll
    for (int r = 0; r < TY; r++) {
      const Vec prv = through_vec(pk_load<PR, V>(pp + row[r]), lxp, my[MAP ? r + 1 : 0]);
      cur[r] = through_vec(pk_load<PR, V>(pc + row[r]), lxc, my[MAP ? r + 1 : 0]);
#pragma unroll
      for (int e = 0; e < V; e++) if (prv.v[e] >= cur[r].v[e]) below |= 1u << (r * V + e);
    }
  }
  for (int xl = xa; xl < xb; xl++) {
    const PR *pc = plane_of(xl), *pn = plane_of(xl + 1);
    lxn = plane_coord(xl + 1);
#pragma unroll
    for (int r = 0; r < TY; r++) nxt[r] = through_vec(pk_load<PR, V>(pn + row[r]), lxn, my[MAP ? r + 1 : 0]);
    const Vec hlo = through_vec(pk_load<PR, V>(pc + row_lo), lxc, my[0]), hhi = through_vec(pk_load<PR, V>(pc + row_hi), lxc, my[MAP ? TY + 1 : 0]);
    int gx = a.x0 + xl - a.start[0]; if (gx < 0) gx += n;
    const bool xok = gx >= a.lo[0] && gx < a.hi[0], xgood = gx >= a.glo[0] && gx < a.ghi[0];
    unsigned int pm = 0, gm = 0, below_next = 0;
#pragma unroll
    for (int r = 0; r < TY; r++) {
      // the shuffles run in every lane, whatever the region says
      PR left = __shfl(cur[r].v[V - 1], lane_l, 64), right = __shfl(cur[r].v[0], lane_r, 64);
      if (!in_l) left = through(pc[(long long)row[r] + off_l], lxc, my[MAP ? r + 1 : 0], mz[0]);
      if (!in_r) right = through(pc[(long long)row[r] + off_r], lxc, my[MAP ? r + 1 : 0], mz[MAP ? V + 1 : 0]);
      const Vec &up = r > 0 ? cur[r > 0 ? r - 1 : 0] : hlo;
      const Vec &dn = r < TY - 1 ? cur[r < TY - 1 ? r + 1 : 0] : hhi;
#pragma unroll
      for (int e = 0; e < V; e++) {
        const PR f = cur[r].v[e];
        const PR zl = e > 0 ? cur[r].v[e > 0 ? e - 1 : 0] : left;
        const PR zr = e < V - 1 ? cur[r].v[e < V - 1 ? e + 1 : 0] : right;
        // f stored, and no stored neighbour with Fn >= F (a neighbour with Fn >= F >= Flast is stored; NaN compares false)
        const bool peak = (f >= thr) && !((below >> (r * V + e)) & 1u) && !(nxt[r].v[e] >= f) && !(up.v[e] >= f) && !(dn.v[e] >= f) && !(zl >= f) && !(zr >= f);
        if (f >= nxt[r].v[e]) below_next |= 1u << (r * V + e);
        const bool ex = peak && xok && ((ym >> r) & 1u) && ((zm >> e) & 1u);
        if (ex) pm |= 1u << (r * V + e);
        if (ex && xgood && ((ymg >> r) & 1u) && ((zmg >> e) & 1u)) gm |= 1u << (r * V + e);
      }
    }
    cnt += __popc(pm); cntg += __popc(gm);
    if (KEYS) {
      // whole-box lists only: one cursor step per wavefront and plane
      unsigned int incl = __popc(pm);
      for (int o = 1; o < 64; o <<= 1) { const unsigned int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
      const unsigned int total = __shfl(incl, 63, 64);
      if (total) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(a.counters + 2, (unsigned long long)total);
        base = __shfl(base, 0, 64);
        unsigned long long pos = base + incl - __popc(pm);
#pragma unroll
        for (int r = 0; r < TY; r++)
#pragma unroll
          for (int e = 0; e < V; e++)
            if ((pm >> (r * V + e)) & 1u) {
              const unsigned int idx = (unsigned int)((size_t)xl * plane + row[r] + e);
              if (pos < a.key_cap) a.keys[pos] = ((unsigned long long)pf_desc_key((float)cur[r].v[e]) << 32) | idx;
              pos++;
            }
      }
    }
#pragma unroll
    for (int r = 0; r < TY; r++) cur[r] = nxt[r];
    below = below_next;
    lxc = lxn;
  }
  unsigned long long c0 = cnt, c1 = cntg;
  for (int o = 32; o > 0; o >>= 1) { c0 += __shfl_down(c0, o, 64); c1 += __shfl_down(c1, o, 64); }
  if (lane == 0) {
    if (c0) atomicAdd(a.counters, c0);
    if (c1) atomicAdd(a.counters + 1, c1);
  }
}

// the smallest value t of the product type with (double)t >= flast: F >= t is then "(double)F >= flast" (outputs.Flast is a double)
static float thr_of(double flast, float) {
  float t = (float)flast;
  if ((double)t < flast) t = nextafterf(t, INFINITY);
  return t;
}
static double thr_of(double flast, double) { return flast; }

// NULL = the whole periodic box; 0 ok, else the direction at fault in *bad and 1: len outside [1, n], 2: 2 safe > len or safe < 0
int pf_peak_region_setup(int n, const pf_peak_region *rg, PfPeakParams *p, int *bad) {
  for (int d = 0; d < 3; d++) {
    const int len = rg ? rg->len[d] : n, safe = rg ? rg->safe[d] : 0;
    *bad = d;
    if (len < 1 || len > n) return 1;
    if (safe < 0 || 2 * (long long)safe > len) return 2;
    int s = rg ? rg->start[d] % n : 0;
    if (s < 0) s += n;
    p->start[d] = s;
    const bool pbc = len == n;                    // subbox.pbc: the region spans the box in this direction
    p->lo[d] = pbc ? 0 : 1; p->hi[d] = pbc ? n : len - 1;    // "avoid borders", src/fragment.c:630-635
    p->glo[d] = safe; p->ghi[d] = len - safe;                // :691-694
  }
  return 0;
}

template <typename PR, int V, bool KEYS, bool MAP = false, typename Args = PkArgs>
static void launch_peaks(const Args &a, double flast, hipStream_t st) {
  const long long ncols = (long long)((a.n + PF_PEAK_TY - 1) / PF_PEAK_TY) * (a.n / V);
  const unsigned int gx = (unsigned int)((ncols + PF_PEAK_BLOCK - 1) / PF_PEAK_BLOCK);
  const unsigned int gy = (unsigned int)((a.nxl + a.xchunk - 1) / a.xchunk);
  hipLaunchKernelGGL((k_peaks<PR, V, KEYS, MAP>), dim3(gx, gy), dim3(PF_PEAK_BLOCK), 0, st, a, thr_of(flast, PR()));
}

// counters[0] += peaks of the region in this slab, counters[1] += the well resolved ones; keys != null: the sort keys of the
// peaks appended at counters[2] (fp32 products)
int pf_launch_peaks(int pb, const PfPeakParams &p, hipStream_t st) {
  if (p.n < 1 || p.n > 2048 || p.nxl < 1 || (p.keys && pb != 4) || (p.keys && p.map)) return 1;
  PkMapArgs a;   // (the instantiations without a map take its PkArgs part)
  a.map = p.map;
  for (int d = 0; d < 3; d++) a.mlen[d] = p.mlen[d];
  a.fmax = p.fmax; a.halo_lo = p.halo_lo; a.halo_hi = p.halo_hi;
  a.n = p.n; a.nxl = p.nxl; a.x0 = p.x0;
  for (int d = 0; d < 3; d++) { a.start[d] = p.start[d]; a.lo[d] = p.lo[d]; a.hi[d] = p.hi[d]; a.glo[d] = p.glo[d]; a.ghi[d] = p.ghi[d]; }
  a.counters = p.counters; a.keys = p.keys; a.key_cap = p.key_cap;
  // planes per march: enough workgroups to fill the device (about half a million threads: 64 planes per march at 1024^3, 2 / 64 more bytes), chunks of eight planes and more
  const int v = pb == 8 ? (p.n % 2 == 0 ? 2 : 1) : (p.n % 4 == 0 ? 4 : 1);
  const long long cols = (long long)((p.n + PF_PEAK_TY - 1) / PF_PEAK_TY) * (p.n / v);
  long long chunks = ((1ll << 19) + cols - 1) / cols;
  if (chunks > p.nxl / 8) chunks = p.nxl / 8;
  if (chunks < 1) chunks = 1;
  a.xchunk = (int)((p.nxl + chunks - 1) / chunks);
  if (p.map) {
    if (pb == 8) {
      if (v == 2) launch_peaks<double, 2, false, true>(a, p.flast, st);
      else launch_peaks<double, 1, false, true>(a, p.flast, st);
    } else {
      if (v == 4) launch_peaks<float, 4, false, true>(a, p.flast, st);
      else launch_peaks<float, 1, false, true>(a, p.flast, st);
    }
  } else if (pb == 8) {
    if (v == 2) launch_peaks<double, 2, false>(a, p.flast, st);
    else launch_peaks<double, 1, false>(a, p.flast, st);
  } else if (p.keys) {
    if (v == 4) launch_peaks<float, 4, true>(a, p.flast, st);
    else launch_peaks<float, 1, true>(a, p.flast, st);
  } else {
    if (v == 4) launch_peaks<float, 4, false>(a, p.flast, st);
    else launch_peaks<float, 1, false>(a, p.flast, st);
  }
  return hipGetLastError() != hipSuccess;
}

// the peaks of the slab in index_compare_F order: keys appended by k_peaks, sorted and unpacked by pf_select_sort.hip.
// npeaks: what a count pass with the same parameters has just found (sizes the key buffer); p.counters[2] is zero
int pf_select_peaks_device(PfPeakParams p, size_t npeaks, unsigned int **d_idx, float **d_f, hipStream_t st) {
  *d_idx = nullptr; *d_f = nullptr;
  if (!npeaks) return 0;
  unsigned long long *keys = nullptr;
  if (hipMalloc(&keys, npeaks * sizeof(unsigned long long)) != hipSuccess) { (void)hipGetLastError(); return 1; }
  p.keys = keys; p.key_cap = npeaks;
  if (pf_launch_peaks(4, p, st)) { hipFree(keys); return 1; }
  return pf_sort_keys_device(keys, npeaks, d_idx, d_f, st);  // takes the keys over
}
