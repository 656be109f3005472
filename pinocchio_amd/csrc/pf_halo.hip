// pf_halo.hip -- the power spectrum of a halo catalogue and its cross power with the linear field (include/pinfmax.h: pf_halo_power
// and its taps): a caller's list of points with integer masses, selected by mass into up to PF_HALO_MAX_BINS bins, each bin
// deposited into a grid of 64-bit integers, turned into a contrast with the bin's own mean in the scratch field of the transform
// taps, transformed by the context's forward transform and summed per shell with the resident delta(k).  The arithmetic of a halo
// is pf_halo_core.h's; the shell sums are pf_power.hip's (pf_matter_shells_device), exactly as pf_matter.hip uses them.  The
// reference has no counterpart.  pf_halo_multipoles is the same body (halo_spectra) with the list moved along one axis by its
// velocities (pf_halo_pos_rsd) and the multipole shell pass (pf_multipole_shells_device) in place of the plain one.
// pf_halo_correlation is the same body again up to the forward transform; behind it the form passes (pf_corr_form_device: delta_h(k)
// -> |delta_h|^2 / N^3 and Re(delta_h delta*) / N^3), the context's reverse transform (pf_ctx_matter_reverse) and the shell pass in
// separation space (pf_corr_shells_device), all three pf_power.hip's.  pf_halo_bispectrum is the same body once more up to the forward
// transform; behind it delta_h(k) is copied into a field of its own and handed to pf_bispec_device (pf_bispec.hip: per k-bin the mask
// pass, the context's reverse transform and the keep pass, then the triple pass), after the count fields of the call have gone the
// same way once.
//
//  k_halo_select    one halo per lane, every bin in one read of the list: the class of its position (ballots) and, per bin, the
//                   counts and the integer sums of W and of the high and low halves of W^2, reduced over the wave by shuffles; one
//                   integer atomic per wave and counter that has something to add, into one of PF_HALO_SLOTS copies.
//  k_halo_deposit   one halo per lane, one bin: up to eight 64-bit integer adds whose result is not used (relaxed, agent scope); a
//                   factor of zero adds nothing and is left out.  The list is sparse against the grid (about 1 % of the cells):
//                   the adds rarely meet, and there is no LDS-staged form (profiles/halo_notes.md).
//  k_halo_contrast  cell -> delta = cell / mean - 1 in double, rounded once to the field type, into the real rows of the scratch
//                   field; in the same pass the largest cell and the empty cells.
//
// Every index is in range by construction: a halo index is below count; a position of class 0 lies in [0, n] on every axis, so its
// rows and columns wrap into [0, n) (pf_halo_core.h), and its plane is deposited only where pf_halo_plane finds it among the nxl
// planes the grid was allocated with; a cell index of the contrast pass is below ncell = nxl n^2.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pf_internal.h"
#include "pf_halo_core.h"

#define HLHIP(task, who, call)                                                                                         \
  do {                                                                                                                 \
    hipError_t e__ = (call);                                                                                           \
    if (e__ != hipSuccess) return pf_fail(task, "%s: %s failed: %s", who, #call, hipGetErrorString(e__));             \
  } while (0)

#define PF_HALO_BLOCK 256
#define PF_HALO_FLAGS (PF_HALO_NGP | PF_HALO_DECONVOLVE | PF_HALO_MASS_WEIGHT)
#define PF_HALO_SLOTS 64   // copies of the selection counters: a workgroup adds to the copy of its index

typedef unsigned long long u64;

// the selection counters of a bin on the device
enum { HS_SELECTED = 0, HS_NONFINITE, HS_OUTSIDE, HS_WSUM, HS_W2HI, HS_W2LO, HS_COUNT };
#define HS_WORDS ((size_t)PF_HALO_SLOTS * PF_HALO_MAX_BINS * HS_COUNT)
#define MC_WORDS ((size_t)PF_MATTER_SLOTS * MC_COUNT)

// vlos: the velocity component along the line of sight, one per halo (null: real space, pf_halo_power's path); los: that axis
struct HaloList { const double *pos; const int *mass; size_t count; double scale; int n, mass_weight; const double *vlos; double vfac; int los; };
struct HaloBins { int nbins, lo[PF_HALO_MAX_BINS], hi[PF_HALO_MAX_BINS]; };

__device__ __forceinline__ void halo_add(u64 *p, u64 v) {
  if (v) (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void halo_max(u64 *p, u64 v) {
  if (v > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, v);
}
__device__ __forceinline__ void halo_count(bool flag, u64 *counter) {
  const u64 m = __ballot(flag);
  if (m && (threadIdx.x & (warpSize - 1)) == (unsigned int)(__ffsll((long long)m) - 1)) halo_add(counter, (u64)__popcll(m));
}
__device__ __forceinline__ u64 halo_wave_sum(u64 v) {
  for (int off = warpSize / 2; off; off >>= 1) v += __shfl_down(v, off);
  return v;
}
__device__ __forceinline__ u64 halo_wave_max(u64 v) {
  for (int off = warpSize / 2; off; off >>= 1) { const u64 o = __shfl_down(v, off); v = o > v ? o : v; }
  return v;
}

// the position and class of halo i (< count)
__device__ __forceinline__ int halo_position(const HaloList &h, size_t i, double p[3]) {
#pragma unroll
  for (int j = 0; j < 3; j++) p[j] = pf_halo_pos_rsd(h.pos[3 * i + j], (h.vlos && j == h.los) ? h.vlos + i : nullptr, h.vfac, h.scale, h.n);
  return pf_halo_class(p, h.n);
}

__global__ void __launch_bounds__(PF_HALO_BLOCK) k_halo_select(HaloList h, HaloBins bins, u64 *counters) {
  const size_t i = (size_t)blockIdx.x * PF_HALO_BLOCK + threadIdx.x;
  int cls = -1, m = 0;
  if (i < h.count) {
    double p[3];
    cls = halo_position(h, i, p);
    m = h.mass[i];
  }
  u64 *slot = counters + (size_t)(blockIdx.x % PF_HALO_SLOTS) * PF_HALO_MAX_BINS * HS_COUNT;
  for (int b = 0; b < bins.nbins; b++, slot += HS_COUNT) {
    const bool in = cls >= 0 && pf_halo_in_range(m, bins.lo[b], bins.hi[b]);
    if (!__ballot(in)) continue;
    const bool sel = in && cls == 0;
    halo_count(sel, slot + HS_SELECTED);
    halo_count(in && cls == 1, slot + HS_NONFINITE);
    halo_count(in && cls == 2, slot + HS_OUTSIDE);
    if (h.mass_weight && __ballot(sel)) {   // (without it W = 1: the three sums are the count)
      const u64 w = sel ? pf_halo_weight(m, true) : 0, w2 = w * w;
      const u64 s = halo_wave_sum(w), hi = halo_wave_sum(w2 >> 32), lo = halo_wave_sum(w2 & 0xffffffffull);
      if ((threadIdx.x & (warpSize - 1)) == 0) { halo_add(slot + HS_WSUM, s); halo_add(slot + HS_W2HI, hi); halo_add(slot + HS_W2LO, lo); }
    }
  }
}

// grid: the planes [x0, x0 + nxl) of the box, cleared by the caller
template <int NGP>
__global__ void __launch_bounds__(PF_HALO_BLOCK) k_halo_deposit(HaloList h, int lo, int hi, int x0, int nxl, u64 *grid) {
  const size_t i = (size_t)blockIdx.x * PF_HALO_BLOCK + threadIdx.x;
  if (i >= h.count) return;
  const int m = h.mass[i];
  if (!pf_halo_in_range(m, lo, hi)) return;
  double p[3];
  if (halo_position(h, i, p) != 0) return;
  const u64 W = pf_halo_weight(m, h.mass_weight != 0);
  const size_t n = (size_t)h.n;
  if (NGP) {
    const int lx = pf_halo_plane(pf_halo_ngp_axis(p[0], h.n), x0, nxl);
    if (lx >= 0) halo_add(grid + ((size_t)lx * n + (size_t)pf_halo_ngp_axis(p[1], h.n)) * n + (size_t)pf_halo_ngp_axis(p[2], h.n), W << PF_HALO_SHIFT);
    return;
  }
  int cell[3][2];
  uint32_t wt[3][2];
#pragma unroll
  for (int j = 0; j < 3; j++) pf_halo_cic_axis(p[j], h.n, cell[j], wt[j]);
#pragma unroll
  for (int a = 0; a < 2; a++) {
    const int lx = pf_halo_plane(cell[0][a], x0, nxl);
    if (lx < 0 || !wt[0][a]) continue;
#pragma unroll
    for (int b = 0; b < 2; b++) {
      const u64 wxy = W * ((u64)wt[0][a] * wt[1][b]);
      u64 *rowp = grid + ((size_t)lx * n + (size_t)cell[1][b]) * n;
      halo_add(rowp + cell[2][0], wxy * wt[2][0]);
      halo_add(rowp + cell[2][1], wxy * wt[2][1]);
    }
  }
}

// out null: the counters alone (pf_debug_halo_deposit).  counters: the MC_* words of pf_internal.h, of which MC_EMPTY and MC_MAX are filled
template <class F>
__global__ void __launch_bounds__(PF_HALO_BLOCK) k_halo_contrast(const u64 *grid, size_t ncell, int n, long long pitch, double mean, F *out, u64 *counters) {
  const size_t i = (size_t)blockIdx.x * PF_HALO_BLOCK + threadIdx.x;
  u64 cell = 0, empty = 0;
  if (i < ncell) {
    cell = grid[i];
    empty = cell == 0;
    if (out) {
      const size_t row = i / (unsigned int)n;
      out[row * (size_t)pitch + (i - row * (unsigned int)n)] = (F)pf_halo_contrast(cell, mean);
    }
  }
  const u64 mx = halo_wave_max(cell);
  empty = halo_wave_sum(empty);
  if ((threadIdx.x & (warpSize - 1)) == 0) {
    u64 *slot = counters + (size_t)(blockIdx.x % PF_MATTER_SLOTS) * MC_COUNT;
    halo_max(slot + MC_MAX, mx);
    halo_add(slot + MC_EMPTY, empty);
  }
}

// ------------------------------------------------------------------------------------------------------------ launches ----
// PF_HALO_TIMES=1: device ms of the phases of the calling thread's last pf_halo_power, summed over its bins
// (and of its last pf_halo_multipoles); PF_CORR_TIMES=1: of its last pf_halo_correlation, which has the form passes too and counts
// the reverse transforms with the forward ones
enum { HT_SELECT = 0, HT_DEPOSIT, HT_CONTRAST, HT_TRANSFORM, HT_SHELLS, HT_COUNT };
enum { CT_FORM = HT_SHELLS, CT_SHELLS, CT_COUNT };   // the phases of the correlation call: the first four as above
enum { BT_MASK = HT_SHELLS, BT_KEEP, BT_TRIPLES, BT_COUNT };   // ... and of the bispectrum call (PF_BISPEC_TIMES=1)
static thread_local double halo_last_ms[HT_COUNT] = {0.0, 0.0, 0.0, 0.0, 0.0};
static thread_local double corr_last_ms[CT_COUNT] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
static thread_local double bispec_last_ms[BT_COUNT] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
extern "C" int pf_debug_halo_times(double *ms) {
  if (!ms) return 1;
  for (int i = 0; i < HT_COUNT; i++) ms[i] = halo_last_ms[i];
  return 0;
}
extern "C" int pf_debug_corr_times(double *ms) {
  if (!ms) return 1;
  for (int i = 0; i < CT_COUNT; i++) ms[i] = corr_last_ms[i];
  return 0;
}
extern "C" int pf_debug_bispec_times(double *ms) {
  if (!ms) return 1;
  for (int i = 0; i < BT_COUNT; i++) ms[i] = bispec_last_ms[i];
  return 0;
}
struct HaloTimer {
  std::vector<hipEvent_t> ev; std::vector<int> phase; hipStream_t st; bool on; double *dst;
  // kind: 0 the power and multipole calls, 1 the correlation call, 2 the bispectrum call
  HaloTimer(hipStream_t st_, int kind) : st(st_), dst(kind == 2 ? bispec_last_ms : kind == 1 ? corr_last_ms : halo_last_ms) {
    const char *env = getenv(kind == 2 ? "PF_BISPEC_TIMES" : kind == 1 ? "PF_CORR_TIMES" : "PF_HALO_TIMES");
    on = env && atoi(env) != 0;
    for (int i = 0; i < (kind == 2 ? (int)BT_COUNT : kind == 1 ? (int)CT_COUNT : (int)HT_COUNT); i++) dst[i] = 0.0;
  }
  // what ran since the last mark belongs to `ph` (-1: to none)
  void mark(int ph) {
    if (!on) return;
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) { on = false; return; }
    ev.push_back(e); phase.push_back(ph);
    on = hipEventRecord(e, st) == hipSuccess;
  }
  void end() {
    if (on && !ev.empty() && hipEventSynchronize(ev.back()) == hipSuccess)
      for (size_t k = 1; k < ev.size(); k++) {
        float ms = 0.0f;
        if (phase[k] >= 0 && hipEventElapsedTime(&ms, ev[k - 1], ev[k]) == hipSuccess) dst[phase[k]] += ms;
      }
    on = false;
  }
  ~HaloTimer() { for (hipEvent_t e : ev) hipEventDestroy(e); }
};

// what a call holds on the device: the list, the selection counters, the grid of the slab and the words (counters and shell tables
// of every bin, then what the ranks agree on)
// extra: the cross spectrum of pf_halo_correlation, the copy of delta_h(k) of pf_halo_bispectrum; stores: the kept fields of the latter
struct HaloBufs { double *pos, *vlos; int *mass; u64 *sel, *grid, *words; void *extra, *stores; };
struct HaloGuard {
  HaloBufs *b;
  ~HaloGuard() {
    hipFree(b->pos); hipFree(b->vlos); hipFree(b->mass); hipFree(b->sel); hipFree(b->grid); hipFree(b->words); hipFree(b->extra); hipFree(b->stores);
    memset(b, 0, sizeof(*b));
  }
};

static bool halo_finite(double x) { return x - x == 0.0; }
// what a call checks of its list and ranges before anything is launched
static int halo_check_list(const char *who, int task, int flags, size_t count, const double *pos, double scale, const int *mass, int nbins, const int *range,
                           const pf_halo_info *info) {
  if (!pos || !mass || !range || !info) return pf_fail(task, "%s: null argument", who);
  if (flags & ~PF_HALO_FLAGS) return pf_fail(task, "%s: unknown flag bits 0x%x", who, (unsigned int)(flags & ~PF_HALO_FLAGS));
  if (nbins < 1 || nbins > PF_HALO_MAX_BINS) return pf_fail(task, "%s: %d bins (1 to %d)", who, nbins, PF_HALO_MAX_BINS);
  for (int b = 0; b < nbins; b++)
    if (range[2 * b] < 1 || range[2 * b + 1] < range[2 * b]) return pf_fail(task, "%s: bin %d takes the masses %d to %d (1 <= lo <= hi)", who, b, range[2 * b], range[2 * b + 1]);
  if (!halo_finite(scale) || !(scale > 0.0)) return pf_fail(task, "%s: a scale of %g (finite and above 0)", who, scale);
  if (count > ((size_t)1 << 31)) return pf_fail(task, "%s: %zu haloes are more than 2^31", who, count);
  return 0;
}
// ... and of the line of sight of a redshift-space call
static int halo_check_rsd(const char *who, int task, const double *vel, double vfac, int los) {
  if (los < 0 || los > 2) return pf_fail(task, "%s: a line of sight along axis %d (0, 1 or 2)", who, los);
  if (!halo_finite(vfac)) return pf_fail(task, "%s: a vfac of %g (finite)", who, vfac);
  if (vfac != 0.0 && !vel) return pf_fail(task, "%s: a vfac of %g without velocities", who, vfac);
  return 0;
}
// component los of vel[3 count] -> the device, through `pack`
static void halo_pack_vlos(size_t count, const double *vel, int los, std::vector<double> &pack) {
  pack.resize(count);
  for (size_t i = 0; i < count; i++) pack[i] = vel[3 * i + los];
}
static unsigned int halo_blocks(size_t count) { return (unsigned int)((count + PF_HALO_BLOCK - 1) / PF_HALO_BLOCK); }   // (count <= 2^31)

// the selection pass and its counters -> the list-derived part of info[0 .. nbins); synchronises the stream.  Returns 1 with the
// message set where a bin has no headroom
static int halo_select(const char *who, int task, const HaloList &h, const HaloBins &bins, u64 *sel, pf_halo_info *info, HaloTimer *timer, hipStream_t st) {
  HLHIP(task, who, hipMemsetAsync(sel, 0, HS_WORDS * 8, st));
  if (timer) timer->mark(-1);
  if (h.count) {
    hipLaunchKernelGGL(k_halo_select, dim3(halo_blocks(h.count)), dim3(PF_HALO_BLOCK), 0, st, h, bins, sel);
    if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  }
  if (timer) timer->mark(HT_SELECT);
  std::vector<u64> slots(HS_WORDS);
  HLHIP(task, who, hipMemcpyAsync(slots.data(), sel, HS_WORDS * 8, hipMemcpyDeviceToHost, st));
  HLHIP(task, who, hipStreamSynchronize(st));
  for (int b = 0; b < bins.nbins; b++) {
    u64 hc[HS_COUNT] = {0};
    for (int k = 0; k < PF_HALO_SLOTS; k++)
      for (int i = 0; i < HS_COUNT; i++) hc[i] += slots[((size_t)k * PF_HALO_MAX_BINS + b) * HS_COUNT + i];
    if (!h.mass_weight) { hc[HS_WSUM] = hc[HS_SELECTED]; hc[HS_W2HI] = 0; hc[HS_W2LO] = hc[HS_SELECTED]; }
    memset(&info[b], 0, sizeof(info[b]));
    info[b].selected = hc[HS_SELECTED]; info[b].nonfinite = hc[HS_NONFINITE]; info[b].outside = hc[HS_OUTSIDE]; info[b].weight_sum = hc[HS_WSUM];
    // sum W^2 = hi 2^32 + lo as 128 bits (each sum is below 2^63: at most 2^31 terms below 2^32)
    const u64 low = hc[HS_W2LO] + (hc[HS_W2HI] << 32);
    info[b].weight2_lo = low; info[b].weight2_hi = (hc[HS_W2HI] >> 32) + (low < hc[HS_W2LO] ? 1 : 0);
  }
  for (int b = 0; b < bins.nbins; b++)
    if (info[b].weight_sum >= PF_HALO_WEIGHT_LIMIT)
      return pf_fail(task, "%s: the weights of bin %d add up to %llu, 2^34 or more: a cell could overflow", who, b, info[b].weight_sum);
  return 0;
}

// grid (cleared here) += the haloes of [lo, hi] on the planes [x0, x0 + nxl)
static int halo_deposit(const char *who, int task, const HaloList &h, int flags, int lo, int hi, int x0, int nxl, u64 *grid, hipStream_t st) {
  HLHIP(task, who, hipMemsetAsync(grid, 0, (size_t)nxl * h.n * h.n * 8, st));
  if (!h.count) return 0;
  const dim3 gr(halo_blocks(h.count)), bl(PF_HALO_BLOCK);
  if (flags & PF_HALO_NGP) hipLaunchKernelGGL(k_halo_deposit<1>, gr, bl, 0, st, h, lo, hi, x0, nxl, grid);
  else hipLaunchKernelGGL(k_halo_deposit<0>, gr, bl, 0, st, h, lo, hi, x0, nxl, grid);
  if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  return 0;
}
// fb 0: no field, the counters alone
static int halo_contrast(const char *who, int task, int fb, const u64 *grid, size_t ncell, int n, long long pitch, double mean, void *field, u64 *counters, hipStream_t st) {
  const size_t nblk = (ncell + PF_HALO_BLOCK - 1) / PF_HALO_BLOCK;
  if (nblk > 0x7fffffffull) return pf_fail(task, "%s: %zu cells are more than one launch takes (internal error)", who, ncell);
  const dim3 gr((unsigned int)nblk), bl(PF_HALO_BLOCK);
  if (fb == 8) hipLaunchKernelGGL((k_halo_contrast<double>), gr, bl, 0, st, grid, ncell, n, pitch, mean, (double *)field, counters);
  else hipLaunchKernelGGL((k_halo_contrast<float>), gr, bl, 0, st, grid, ncell, n, pitch, mean, (float *)(fb ? field : nullptr), counters);
  if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  return 0;
}
// the copies of the counters of one bin (on the host) -> empty cells, largest cell, modes that are not finite
static void halo_reduce_slots(const u64 *slots, u64 *empty, u64 *mx, u64 *nonfin) {
  *empty = *mx = *nonfin = 0;
  for (int k = 0; k < PF_MATTER_SLOTS; k++) {
    const u64 *s = slots + (size_t)k * MC_COUNT;
    *empty += s[MC_EMPTY]; *nonfin += s[MC_NONFIN_MODES];
    if (s[MC_MAX] > *mx) *mx = s[MC_MAX];
  }
}

// a few words of the host summed over the ranks of the context, through `dev` (as many words on the device) on the context's stream
static int halo_agree(const char *who, int task, pf_ctx *c, u64 *dev, std::vector<u64> &a, hipStream_t st) {
  HLHIP(task, who, hipMemcpyAsync(dev, a.data(), a.size() * 8, hipMemcpyHostToDevice, st));
  HLHIP(task, who, hipStreamSynchronize(st));
  if (pf_ctx_allreduce(c, dev, a.size(), 1)) return 1;
  HLHIP(task, who, hipMemcpyAsync(a.data(), dev, a.size() * 8, hipMemcpyDeviceToHost, st));
  HLHIP(task, who, hipStreamSynchronize(st));
  return 0;
}
// what the ranks agree on before any deposit: a slot per rank -- count, nbins and flags, each bin's selected and weight_sum, the
// line of sight with whether there are velocities, the bits of vfac -- and behind the slots the flag of a rank that refuses
#define HA_SLOT (4 + 2 * PF_HALO_MAX_BINS)
static size_t halo_agree_words(int P) { return (size_t)P * HA_SLOT + 1; }
// a rank that refuses on its own (its message stands in pf_last_error) still meets the others in that all-reduce, with its flag
static int halo_refuse(const char *who, pf_ctx *c, const PfSpecView &sv) {
  if (sv.P == 1) return 1;
  u64 *dev = nullptr;
  const size_t cnt = halo_agree_words(sv.P);
  if (hipMalloc((void **)&dev, cnt * 8) != hipSuccess) { (void)hipGetLastError(); return 1; }
  std::vector<u64> a(cnt, 0);
  a[cnt - 1] = 1;
  (void)halo_agree(who, sv.rank, c, dev, a, sv.stream);   // (a successful all-reduce leaves the message as it is)
  hipFree(dev);
  return 1;
}

// the body of pf_halo_power (HM_POWER: vel null, vfac 0; power and cross [nbins][nb]), of pf_halo_multipoles (HM_MULTI: the list
// moved along axis los, the multipole shell pass, power and cross [nbins][3][nb]) and of pf_halo_correlation (HM_CORR: the list moved
// likewise; behind the forward transform the form passes, the reverse transforms and the shell pass in separation space; nmodes and
// k2sum are ncells and r2sum, power and cross xi and xi_cross [nbins][3][nb]; nonfinite_cells [nbins], null otherwise) and of
// pf_halo_bispectrum (HM_BISPEC: the list moved likewise; behind the forward transform pf_bispec_device on a copy of delta_h(k); bq:
// the k-bins and the outputs of that call; nmodes, k2sum and power are its kmodes, ntri and bsum, so that a null one is refused where
// every null is; cross null: no density is needed)
enum { HM_POWER = 0, HM_MULTI, HM_CORR, HM_BISPEC };
struct HaloBispec { int kmin, dk, nk; u64 *kmodes; double *ntri, *bsum, *psum; };
static void halo_bispec_mark(void *timer, int ph) {
  static const int of[4] = {HT_TRANSFORM, BT_MASK, BT_KEEP, BT_TRIPLES};   // PF_BISPEC_PH_* -> the phases of the timer
  ((HaloTimer *)timer)->mark(ph < 0 ? -1 : of[ph]);
}
static int halo_spectra(const char *who, int mode, pf_ctx *c, int flags, size_t count, const double *pos, const double *vel, double scale, double vfac, int los, const int *mass,
                        int nbins, const int *mass_range, unsigned long long *nmodes, unsigned long long *k2sum, double *power, double *cross, pf_halo_info *info, u64 *nonfinite_cells = nullptr,
                        const HaloBispec *bq = nullptr) {
  if (!c) return pf_fail(0, "%s: null argument", who);
  const bool multi = mode != HM_POWER, corr = mode == HM_CORR, bis = mode == HM_BISPEC;
  PfSpecView sv;
  pf_ctx_spec_geometry(c, &sv);
  if (sv.P > 1 && !pf_ctx_exchange_installed(c))
    return pf_fail(sv.rank, "%s: no exchange installed for %d ranks (pf_set_exchange and pf_set_allreduce / pf_init_rccl)", who, sv.P);
  PfCtxView cv;
  pf_ctx_view(c, &cv);
  PfMatterCtx mc;
  pf_ctx_matter_view(c, &mc);
  const int task = sv.rank, n = sv.n, P = sv.P;
  hipStream_t st = sv.stream;
  // every check a rank makes on its own; what it finds it tells the others before anything is launched
  int bad = 0;
  if (!nmodes || !k2sum || !power) bad = pf_fail(task, "%s: null argument", who);
  if (!bad) bad = halo_check_list(who, task, flags, count, pos, scale, mass, nbins, mass_range, info);
  if (!bad && bis && !bq->psum) bad = pf_fail(task, "%s: null argument", who);
  if (!bad && multi) bad = halo_check_rsd(who, task, vel, vfac, los);
  if (!bad && cross) bad = pf_ctx_spec_view(c, who, 0, &sv);   // "density not set" (which = 0: nothing is launched)
  if (!bad && bis) bad = pf_bispec_check_bins(who, task, bq->kmin, bq->dk, bq->nk, n);
  if (!bad && bis && n > 1024) bad = pf_fail(task, "%s: a grid of %d is above 1024: a limb counter takes n^3 terms below 2^32 and would pass 2^63", who, n);
  HaloBufs b;
  memset(&b, 0, sizeof(b));
  HaloGuard guard{&b};
  // (the correlation call: the tables of the auto field, then those of the cross field, each of corr_words)
  const size_t nb = (size_t)pf_power_nbins(n), corr_words = pf_corr_shells_words(n, P);
  const size_t shell_words = bis ? 0 : corr ? 2 * corr_words : multi ? pf_multipole_shells_words(n, P) : pf_matter_shells_words(n, P), bin_words = MC_WORDS + shell_words;
  const size_t orders = multi ? PF_MULTIPOLE_ORDERS : 1;
  const size_t fetch_words = (size_t)PF_HALO_MAX_BINS * (2 + (size_t)P);
  const size_t agree_words = halo_agree_words(P) > fetch_words ? halo_agree_words(P) : fetch_words;
  const size_t deconv_words = corr || bis ? (size_t)(n / 2 + 1) : 0;               // the deconvolution table of the form passes, behind everything
  const size_t bispec_words = bis && !bad ? pf_bispec_words(bq->kmin, bq->dk, bq->nk, P) : 0;   // ... and behind it the tables of pf_bispec_device
  const size_t words = bad ? 0 : (size_t)(nbins + 1) * bin_words + agree_words + deconv_words + bispec_words;   // (the bin behind the last: the tables of a call whose bins are all empty)
  size_t field_bytes = 0;
  void *rev = corr || bis ? pf_ctx_matter_reverse_field(c, &field_bytes) : nullptr;   // where the reverse transform works
  const size_t extra_bytes = (corr && cross) || bis ? field_bytes : 0;
  const size_t store_bytes = bis && !bad ? (size_t)bq->nk * cv.ncell * sv.fb : 0;      // the nk kept fields
  const size_t list = count ? count : 1, bytes = list * (vel ? 36 : 28) + HS_WORDS * 8 + cv.ncell * 8 + words * 8 + extra_bytes + store_bytes;
  if (!bad && (hipMalloc((void **)&b.pos, list * 24) != hipSuccess || (vel && hipMalloc((void **)&b.vlos, list * 8) != hipSuccess) || hipMalloc((void **)&b.mass, list * 4) != hipSuccess ||
               hipMalloc((void **)&b.sel, HS_WORDS * 8) != hipSuccess || hipMalloc((void **)&b.grid, cv.ncell * 8) != hipSuccess || hipMalloc((void **)&b.words, words * 8) != hipSuccess ||
               (extra_bytes && hipMalloc(&b.extra, extra_bytes) != hipSuccess) || (store_bytes && hipMalloc(&b.stores, store_bytes) != hipSuccess))) {
    (void)hipGetLastError();
    bad = pf_fail(task, "%s: cannot allocate %zu bytes of scratch on the device", who, bytes);
  }
  if (!bad && count && (pf_ctx_h2d(c, b.pos, pos, count * 24) || pf_ctx_h2d(c, b.mass, mass, count * 4))) bad = 1;
  // of the velocities only the component along the line of sight, packed on the way into the pinned pieces
  if (!bad && count && vel && pf_ctx_h2d_packed(c, b.vlos, vel + los, count, 8, 24, 0, nullptr)) bad = 1;
  if (bad) return halo_refuse(who, c, sv);
  u64 *agree = b.words + (size_t)(nbins + 1) * bin_words;
  HaloList h = {b.pos, b.mass, count, scale, n, (flags & PF_HALO_MASS_WEIGHT) != 0, vel ? b.vlos : nullptr, vfac, los};
  HaloBins bins;
  memset(&bins, 0, sizeof(bins));
  bins.nbins = nbins;
  for (int k = 0; k < nbins; k++) { bins.lo[k] = mass_range[2 * k]; bins.hi[k] = mass_range[2 * k + 1]; }
  HLHIP(task, who, hipMemsetAsync(b.words, 0, (size_t)(nbins + 1) * bin_words * 8, st));
  HaloTimer timer(st, bis ? 2 : corr ? 1 : 0);
  std::vector<pf_halo_info> hi(nbins);
  const int full = halo_select(who, task, h, bins, b.sel, hi.data(), &timer, st);
  if (P > 1) {   // the same list on every rank, and no rank that refuses
    std::vector<u64> a(halo_agree_words(P), 0);
    u64 *mine = a.data() + (size_t)sv.rank * HA_SLOT;
    if (full) a[a.size() - 1] = 1;
    else {
      mine[0] = (u64)count; mine[1] = ((u64)nbins << 8) | (u64)flags;
      if (bis) mine[1] |= ((u64)bq->nk << 16) | ((u64)bq->dk << 24) | ((u64)bq->kmin << 44);   // (dk and kmin are below 2^20: 3 kmax <= n)
      for (int k = 0; k < nbins; k++) { mine[2 + k] = hi[k].selected; mine[2 + PF_HALO_MAX_BINS + k] = hi[k].weight_sum; }
      mine[2 + 2 * PF_HALO_MAX_BINS] = ((u64)(vel != nullptr) << 8) | (u64)los;
      memcpy(&mine[3 + 2 * PF_HALO_MAX_BINS], &vfac, 8);
    }
    const std::vector<u64> own(mine, mine + HA_SLOT);
    if (halo_agree(who, task, c, agree, a, st)) return 1;
    if (full) return 1;
    if (a[a.size() - 1]) return pf_fail(task, "%s: refused on another rank of the context", who);
    for (int p = 0; p < P; p++)
      if (memcmp(a.data() + (size_t)p * HA_SLOT, own.data(), HA_SLOT * 8))
        return pf_fail(task, "%s: rank %d holds another list, other bins, other flags%s or another line of sight than rank %d (%llu haloes there, %zu here)", who, p,
                       bis ? ", other k-bins" : "", sv.rank, a[(size_t)p * HA_SLOT], count);
  } else if (full) return 1;
  // per bin: deposit, contrast, transform, shell sums; the tables stay on the device until every bin is through
  const u64 n3 = (u64)n * (u64)n * (u64)n;
  pf_ctx *coll = P > 1 ? c : nullptr;
  std::vector<PfShellSums> g(nbins + 1), gx(nbins + 1);   // gx: the cross field of the correlation call
  const double *Ctab = nullptr;
  if (corr || bis) {
    if (pf_corr_deconv_upload(who, task, flags & (PF_HALO_NGP | PF_HALO_DECONVOLVE), n, (double *)(agree + agree_words), &Ctab, st)) return 1;
    if (b.extra) HLHIP(task, who, hipMemsetAsync(b.extra, 0, extra_bytes, st));   // (the padding of its rows: the form pass writes the modes alone)
    timer.mark(-1);
  }
  // the bispectrum call: the geometry and the tables of pf_bispec_device; the count fields once, whatever the mass bins hold
  const PfBispecGeom bg = {n, sv.fb, sv.y0, sv.nyl, mc.x0, cv.nxl, sv.rank, P, sv.nzp, mc.rpitch};
  const PfBispecBins kb = {bis ? bq->kmin : 0, bis ? bq->dk : 0, bis ? bq->nk : 0};
  u64 *bwords = agree + agree_words + deconv_words;
  const int nt = bis ? pf_bispectrum_triangles(kb.kmin, kb.dk, kb.nk, nullptr) : 0;
  std::vector<double> bsum((size_t)nbins * nt, 0.0), psum((size_t)nbins * kb.nk, 0.0), ntri(nt, 0.0);
  std::vector<u64> kmodes(kb.nk, 0), bad_modes(nbins, 0), bad_cells(nbins, 0);
  if (bis) {
    PfBispecOut bo = {ntri.data(), nullptr, nullptr, nullptr, kmodes.data(), 0, 0};
    if (pf_bispec_device(who, task, c, bg, kb, nullptr, 1, nullptr, rev, b.stores, bwords, halo_bispec_mark, &timer, &bo, st)) return 1;
    const double dn3 = (double)n * (double)n * (double)n;
    for (int t = 0; t < nt; t++) ntri[t] = ntri[t] / dn3;
  }
  int first = -1;
  for (int k = 0; k < nbins; k++) {
    if (!hi[k].weight_sum) continue;
    u64 *counters = b.words + (size_t)k * bin_words;
    if (halo_deposit(who, task, h, flags, bins.lo[k], bins.hi[k], mc.x0, cv.nxl, b.grid, st)) return 1;
    timer.mark(HT_DEPOSIT);
    if (halo_contrast(who, task, sv.fb, b.grid, cv.ncell, n, mc.rpitch, pf_halo_mean(hi[k].weight_sum, n), mc.field, counters, st)) return 1;
    timer.mark(HT_CONTRAST);
    if (pf_ctx_matter_forward(c)) return 1;
    timer.mark(HT_TRANSFORM);
    const int sflags = flags & (PF_HALO_NGP | PF_HALO_DECONVOLVE);
    if (bis) {
      // delta_h(k) into the field of its own: the reverse transform overwrites the scratch spectrum with more than one rank, and with
      // one rank it works where the spectrum stands
      HLHIP(task, who, hipMemcpyAsync(b.extra, mc.field, (size_t)n * sv.nyl * sv.nzp * 2 * sv.fb, hipMemcpyDeviceToDevice, st));
      timer.mark(BT_MASK);
      PfBispecOut bo = {bsum.data() + (size_t)k * nt, nullptr, psum.data() + (size_t)k * kb.nk, nullptr, nullptr, 0, 0};
      if (pf_bispec_device(who, task, c, bg, kb, b.extra, 0, Ctab, rev, b.stores, bwords, halo_bispec_mark, &timer, &bo, st)) return 1;
      bad_modes[k] = bo.nonfinite_modes; bad_cells[k] = bo.nonfinite_cells;
      if (first < 0) first = k;
      continue;
    }
    if (corr) {
      // the cross spectrum first, into the field of its own; then the auto spectrum where the reverse transform works (with one
      // rank that is where delta_h(k) stands: in place).  The reverse transform overwrites mc.field with more than one rank: by
      // then both are formed
      u64 *tabs = counters + MC_WORDS;
      if (cross && pf_corr_form_device(who, task, sv.fb, mc.field, sv.spec, b.extra, n, sv.y0, sv.nyl, sv.nzp, Ctab, 1, counters, st)) return 1;
      if (pf_corr_form_device(who, task, sv.fb, mc.field, nullptr, rev, n, sv.y0, sv.nyl, sv.nzp, Ctab, 0, counters, st)) return 1;
      timer.mark(CT_FORM);
      if (pf_ctx_matter_reverse(c)) return 1;
      timer.mark(HT_TRANSFORM);
      if (pf_corr_shells_device(who, task, sv.fb, rev, n, mc.x0, cv.nxl, mc.rpitch, los, tabs, coll, &g[k], st)) return 1;
      timer.mark(CT_SHELLS);
      if (cross) {
        HLHIP(task, who, hipMemcpyAsync(rev, b.extra, field_bytes, hipMemcpyDeviceToDevice, st));
        if (pf_ctx_matter_reverse(c)) return 1;
        timer.mark(HT_TRANSFORM);
        if (pf_corr_shells_device(who, task, sv.fb, rev, n, mc.x0, cv.nxl, mc.rpitch, los, tabs + corr_words, coll, &gx[k], st)) return 1;
        timer.mark(CT_SHELLS);
      }
      if (first < 0) first = k;
      continue;
    }
    if (multi ? pf_multipole_shells_device(who, task, sv.fb, mc.field, cross ? sv.spec : nullptr, n, sv.y0, sv.nyl, sv.nzp, sflags, los, counters + MC_WORDS, counters, coll, &g[k], st)
              : pf_matter_shells_device(who, task, sv.fb, mc.field, cross ? sv.spec : nullptr, n, sv.y0, sv.nyl, sv.nzp, sflags, counters + MC_WORDS, counters, coll, &g[k], st))
      return 1;
    timer.mark(HT_SHELLS);
    if (first < 0) first = k;
  }
  if (first < 0 && !bis) {   // every bin is empty: nmodes and k2sum, which depend on the grid alone, from the shell pass over a spectrum of zeros
    first = nbins;
    u64 *counters = b.words + (size_t)nbins * bin_words;
    if (corr) {   // (ncells and r2sum from the separation-space pass over a field of zeros)
      HLHIP(task, who, hipMemsetAsync(rev, 0, field_bytes, st));
      if (pf_corr_shells_device(who, task, sv.fb, rev, n, mc.x0, cv.nxl, mc.rpitch, los, counters + MC_WORDS, coll, &g[nbins], st)) return 1;
    } else {
      HLHIP(task, who, hipMemsetAsync(mc.field, 0, (size_t)n * sv.nyl * sv.nzp * 2 * sv.fb, st));
      if (pf_matter_shells_device(who, task, sv.fb, mc.field, nullptr, n, sv.y0, sv.nyl, sv.nzp, 0, counters + MC_WORDS, counters, coll, &g[nbins], st)) return 1;
    }
    timer.mark(-1);
  }
  timer.end();
  // the fetch: the tables and the counters of every bin that ran
  std::vector<u64> hu(2 * nb), slots(MC_WORDS);
  const size_t per = orders * nb;                       // doubles of a bin in power and in cross; out holds power, then cross
  std::vector<double> hd(2 * per);
  if (!bis) {
    HLHIP(task, who, hipMemcpyAsync(hu.data(), g[first].nm, hu.size() * 8, hipMemcpyDeviceToHost, st));
    HLHIP(task, who, hipStreamSynchronize(st));
  }
  std::vector<u64> grid_words((size_t)nbins * (2 + (size_t)P), 0);   // per bin: empty cells, modes that are not finite, the largest cell of every rank
  for (int k = 0; k < nbins; k++) {
    hi[k].modes = n3;
    if (!hi[k].weight_sum) {
      hi[k].empty_cells = n3;
      if (corr || bis) nonfinite_cells[k] = 0;
      for (size_t s = 0; s < (bis ? 0 : per); s++) { power[(size_t)k * per + s] = 0.0; if (cross) cross[(size_t)k * per + s] = 0.0; }
      continue;
    }
    HLHIP(task, who, hipMemcpyAsync(slots.data(), b.words + (size_t)k * bin_words, MC_WORDS * 8, hipMemcpyDeviceToHost, st));
    if (bis) {   // the sums are on the host already, summed over the ranks; the counters of the contrast pass alone are fetched
      HLHIP(task, who, hipStreamSynchronize(st));
      nonfinite_cells[k] = bad_cells[k];
      u64 *w = grid_words.data() + (size_t)k * (2 + (size_t)P), unused;
      halo_reduce_slots(slots.data(), &w[0], &w[2 + sv.rank], &unused);
      continue;
    }
    u64 bad_cells[2] = {0, 0};
    if (corr) {   // xi of each field [3][nb] from the tables of its own; the cells that are not finite stand behind the limbs, summed over the ranks already
      HLHIP(task, who, hipMemcpyAsync(hd.data(), g[k].out, per * 8, hipMemcpyDeviceToHost, st));
      HLHIP(task, who, hipMemcpyAsync(&bad_cells[0], g[k].nm + 26 * nb, 8, hipMemcpyDeviceToHost, st));
      if (cross) {
        HLHIP(task, who, hipMemcpyAsync(hd.data() + per, gx[k].out, per * 8, hipMemcpyDeviceToHost, st));
        HLHIP(task, who, hipMemcpyAsync(&bad_cells[1], gx[k].nm + 26 * nb, 8, hipMemcpyDeviceToHost, st));
      }
    } else HLHIP(task, who, hipMemcpyAsync(hd.data(), g[k].out, hd.size() * 8, hipMemcpyDeviceToHost, st));
    HLHIP(task, who, hipStreamSynchronize(st));
    if (corr) nonfinite_cells[k] = bad_cells[0] + bad_cells[1];
    memcpy(power + (size_t)k * per, hd.data(), per * 8);
    if (cross) memcpy(cross + (size_t)k * per, hd.data() + per, per * 8);
    u64 *w = grid_words.data() + (size_t)k * (2 + (size_t)P);
    halo_reduce_slots(slots.data(), &w[0], &w[2 + sv.rank], &w[1]);
  }
  if (coll && halo_agree(who, task, c, agree, grid_words, st)) return 1;   // sums over the ranks, and the largest cell through a slot per rank
  for (int k = 0; k < nbins; k++) {
    if (!hi[k].weight_sum) continue;
    const u64 *w = grid_words.data() + (size_t)k * (2 + (size_t)P);
    hi[k].empty_cells = w[0]; hi[k].nonfinite_modes = bis ? bad_modes[k] : w[1];
    for (int p = 0; p < P; p++) hi[k].max_cell = w[2 + p] > hi[k].max_cell ? w[2 + p] : hi[k].max_cell;
  }
  if (bis) {
    memcpy(bq->kmodes, kmodes.data(), (size_t)kb.nk * 8); memcpy(bq->ntri, ntri.data(), (size_t)nt * 8);
    memcpy(bq->bsum, bsum.data(), bsum.size() * 8); memcpy(bq->psum, psum.data(), psum.size() * 8);
  } else { memcpy(nmodes, hu.data(), nb * 8); memcpy(k2sum, hu.data() + nb, nb * 8); }
  memcpy(info, hi.data(), (size_t)nbins * sizeof(pf_halo_info));
  return 0;
}

extern "C" int pf_halo_power(pf_ctx *c, int flags, size_t count, const double *pos, double scale, const int *mass, int nbins, const int *mass_range,
                             unsigned long long *nmodes, unsigned long long *k2sum, double *power, double *cross, pf_halo_info *info) {
  return halo_spectra("pf_halo_power", HM_POWER, c, flags, count, pos, nullptr, scale, 0.0, 0, mass, nbins, mass_range, nmodes, k2sum, power, cross, info);
}
extern "C" int pf_halo_multipoles(pf_ctx *c, int flags, size_t count, const double *pos, const double *vel, double scale, double vfac, int los, const int *mass, int nbins,
                                  const int *mass_range, unsigned long long *nmodes, unsigned long long *k2sum, double *power, double *cross, pf_halo_info *info) {
  return halo_spectra("pf_halo_multipoles", HM_MULTI, c, flags, count, pos, vel, scale, vfac, los, mass, nbins, mass_range, nmodes, k2sum, power, cross, info);
}
// info arrives as pf_corr_info: the body fills pf_halo_info of its own, so that a null info is refused where every refusal is (and told
// to the other ranks), and nothing of the caller's is written before the call has succeeded
extern "C" int pf_halo_correlation(pf_ctx *c, int flags, size_t count, const double *pos, const double *vel, double scale, double vfac, int los, const int *mass, int nbins,
                                   const int *mass_range, unsigned long long *ncells, unsigned long long *r2sum, double *xi, double *xi_cross, pf_corr_info *info) {
  pf_halo_info hinfo[PF_HALO_MAX_BINS];
  u64 bad_cells[PF_HALO_MAX_BINS];
  if (halo_spectra("pf_halo_correlation", HM_CORR, c, flags, count, pos, vel, scale, vfac, los, mass, nbins, mass_range, ncells, r2sum, xi, xi_cross, info ? hinfo : nullptr, bad_cells))
    return 1;
  for (int k = 0; k < nbins; k++) { info[k].halo = hinfo[k]; info[k].cells = hinfo[k].modes; info[k].nonfinite_cells = bad_cells[k]; }
  return 0;
}

// info arrives as pf_bispec_info, handled as pf_halo_correlation handles its own.  kmodes, ntri and bsum ride where the body checks
// for nulls; the body writes them through bq alone
extern "C" int pf_halo_bispectrum(pf_ctx *c, int flags, size_t count, const double *pos, const double *vel, double scale, double vfac, int los, const int *mass, int nbins,
                                  const int *mass_range, int kmin, int dk, int nk, unsigned long long *kmodes, double *ntri, double *bsum, double *psum, pf_bispec_info *info) {
  pf_halo_info hinfo[PF_HALO_MAX_BINS];
  u64 bad_cells[PF_HALO_MAX_BINS];
  const HaloBispec bq = {kmin, dk, nk, kmodes, ntri, bsum, psum};
  if (halo_spectra("pf_halo_bispectrum", HM_BISPEC, c, flags, count, pos, vel, scale, vfac, los, mass, nbins, mass_range, kmodes, (unsigned long long *)ntri, bsum, nullptr,
                   info ? hinfo : nullptr, bad_cells, &bq))
    return 1;
  for (int k = 0; k < nbins; k++) { info[k].halo = hinfo[k]; info[k].cells = hinfo[k].modes; info[k].nonfinite_cells = bad_cells[k]; }
  return 0;
}

// ------------------------------------------------------------------------------------------------------------ tap ----
// the body of pf_debug_halo_deposit (rsd false) and of pf_debug_halo_deposit_rsd
static int halo_deposit_tap(const char *who, bool rsd, int n, int x0, int nxl, int flags, size_t count, const double *pos, const double *vel, double scale, double vfac, int los,
                            const int *mass, int lo, int hi, unsigned long long *grid_host, pf_halo_info *info) {
  if (!grid_host) return pf_fail(0, "%s: null argument", who);
  const int range[2] = {lo, hi};
  if (halo_check_list(who, 0, flags, count, pos, scale, mass, 1, range, info)) return 1;
  if (rsd && halo_check_rsd(who, 0, vel, vfac, los)) return 1;
  if (n < 2 || n > 2048) return pf_fail(0, "%s: a grid of %d (2 to 2048)", who, n);
  if (x0 < 0 || nxl < 1 || x0 + nxl > n) return pf_fail(0, "%s: planes %d .. %d leave the grid of %d", who, x0, x0 + nxl - 1, n);
  const size_t ncell = (size_t)nxl * n * n, list = count ? count : 1;
  HaloBufs b;
  memset(&b, 0, sizeof(b));
  HaloGuard guard{&b};
  if (hipMalloc((void **)&b.pos, list * 24) != hipSuccess || (vel && hipMalloc((void **)&b.vlos, list * 8) != hipSuccess) || hipMalloc((void **)&b.mass, list * 4) != hipSuccess ||
      hipMalloc((void **)&b.sel, HS_WORDS * 8) != hipSuccess || hipMalloc((void **)&b.grid, ncell * 8) != hipSuccess || hipMalloc((void **)&b.words, MC_WORDS * 8) != hipSuccess) {
    (void)hipGetLastError();
    return pf_fail(0, "%s: cannot allocate %zu bytes on the device", who, list * (vel ? 36 : 28) + HS_WORDS * 8 + ncell * 8 + MC_WORDS * 8);
  }
  if (count) {
    HLHIP(0, who, hipMemcpy(b.pos, pos, count * 24, hipMemcpyHostToDevice));
    HLHIP(0, who, hipMemcpy(b.mass, mass, count * 4, hipMemcpyHostToDevice));
    if (vel) {
      std::vector<double> pack;
      halo_pack_vlos(count, vel, los, pack);
      HLHIP(0, who, hipMemcpy(b.vlos, pack.data(), count * 8, hipMemcpyHostToDevice));
    }
  }
  HLHIP(0, who, hipMemsetAsync(b.words, 0, MC_WORDS * 8, nullptr));
  const HaloList h = {b.pos, b.mass, count, scale, n, (flags & PF_HALO_MASS_WEIGHT) != 0, vel ? b.vlos : nullptr, vfac, los};
  HaloBins bins;
  memset(&bins, 0, sizeof(bins));
  bins.nbins = 1; bins.lo[0] = lo; bins.hi[0] = hi;
  pf_halo_info out;
  if (halo_select(who, 0, h, bins, b.sel, &out, nullptr, nullptr)) return 1;
  if (halo_deposit(who, 0, h, flags, lo, hi, x0, nxl, b.grid, nullptr)) return 1;
  if (halo_contrast(who, 0, 0, b.grid, ncell, n, n, 1.0, nullptr, b.words, nullptr)) return 1;
  std::vector<u64> slots(MC_WORDS);
  HLHIP(0, who, hipMemcpyAsync(slots.data(), b.words, MC_WORDS * 8, hipMemcpyDeviceToHost, nullptr));
  HLHIP(0, who, hipMemcpyAsync(grid_host, b.grid, ncell * 8, hipMemcpyDeviceToHost, nullptr));
  HLHIP(0, who, hipStreamSynchronize(nullptr));
  u64 nonfin;
  halo_reduce_slots(slots.data(), &out.empty_cells, &out.max_cell, &nonfin);
  *info = out;
  return 0;
}

extern "C" int pf_debug_halo_deposit(int n, int x0, int nxl, int flags, size_t count, const double *pos, double scale, const int *mass, int lo, int hi,
                                     unsigned long long *grid_host, pf_halo_info *info) {
  return halo_deposit_tap("pf_debug_halo_deposit", false, n, x0, nxl, flags, count, pos, nullptr, scale, 0.0, 0, mass, lo, hi, grid_host, info);
}
extern "C" int pf_debug_halo_deposit_rsd(int n, int x0, int nxl, int flags, size_t count, const double *pos, const double *vel, double scale, double vfac, int los, const int *mass,
                                         int lo, int hi, unsigned long long *grid_host, pf_halo_info *info) {
  return halo_deposit_tap("pf_debug_halo_deposit_rsd", true, n, x0, nxl, flags, count, pos, vel, scale, vfac, los, mass, lo, hi, grid_host, info);
}
