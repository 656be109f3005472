// pf_power.hip -- shell-averaged power and Gaussian-smoothed variances of a half-spectrum that lies on the device (include/pinfmax.h:
// pf_power_spectrum, pf_debug_power_spectrum): two streaming reads of the rows of this rank's ky-slab, [kx][ky_local] rows of `pitch`
// complex of which the first n/2 + 1 are modes; the padding behind them is never read.  The mode arithmetic is pf_power_core.h's.
//
// The walk of both kernels: workgroup g takes the rows [g rpw, (g + 1) rpw) one after the other; thread t owns the columns kz = t +
// 256 c < n/2 (c < CG, a template parameter: 1, 2 or 4 column groups), so consecutive lanes read consecutive modes of a row and
// everything that depends on kz alone -- kz^2, the weight, the window entries E_r[kz] -- stays in registers, while (kx, ky), their
// part of k2 and the window factor E_r[|kx|] E_r[|ky|] are the same for the whole workgroup and advance with the row.  The integer
// root of k2 that decides the shell is carried from row to row per column (pf_power_isqrt_near: k2 moves by one step of ky).  The
// Nyquist column kz = n/2 comes last, thread t taking the rows t, t + 256, ... of the workgroup.
//
//  k_power_scan   per mode: the shell, weight and k2 into the workgroup's LDS counters (nmodes, k2sum: integer adds; the largest
//                 finite term of the shell: an integer maximum of the bit pattern, which orders non-negative doubles), a mode whose
//                 term is not finite into the nonfinite count instead.  Per radius the largest windowed term, in a register.  The
//                 LDS tables and the register maxima leave as integer atomics on the tables in HBM.
//  k_power_acc    the same walk.  A term is added as the three limbs of its fixed-point form scaled to the maximum of ITS shell
//                 (pf_power_limbs), a windowed term scaled to the maximum of ITS radius -- so what the limbs drop is below 2^-95 of the
//                 largest term of the very sum, whatever the dynamic range of the spectrum.  Limb sums: 64-bit LDS counters per shell,
//                 64-bit registers per radius.  A workgroup carries its counters into each other before it adds them to HBM as four
//                 limbs, each then below 2^32 per workgroup.
//  k_power_final  one thread per shell and per radius: limbs -> double (pf_power_from_limbs), times 1 / N^6.
// Integer adds and maxima only: the result is the same bits for any grid, workgroup size or schedule.
// The window exp(-a k2) is factorised per axis: one table E_r[j] = exp(-a_r j^2), j <= n/2, per radius, built on the host (ns (n/2 +
// 1) exponentials) -- two multiplications per mode and radius in place of an exponential in each of the two passes.  Radii go in
// batches of PF_POWER_NR per pair of launches (their registers); the shells ride with the first batch.
//
// Every index is in range by construction: a mode is read only in the workgroup's own rows (< rows), at a column kz <= n/2 < pitch;
// a shell is below pf_power_nbins(n), which sized every table, since k2 <= 3 (n/2)^2; a radius index is below the batch's nr <=
// PF_POWER_NR inside a kernel and below ns in HBM; the window tables are read at |kx|, |ky|, kz <= n/2, their row length less one;
// the dynamic LDS is sized by nbins and PF_POWER_NR.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pf_internal.h"
#include "pf_power_core.h"

#define PWHIP(task, who, call)                                                                                         \
  do {                                                                                                                 \
    hipError_t e__ = (call);                                                                                           \
    if (e__ != hipSuccess) return pf_fail(task, "%s: %s failed: %s", who, #call, hipGetErrorString(e__));             \
  } while (0)

#define PF_POWER_BLOCK 256
#define PF_POWER_NR 12          // radii of one pair of launches at most
// workgroups at most.  Without radii many short ones: the CUs hold about 1800 at once, and with 2048 the last round ran nearly
// empty (1024^3, fp64: 3.6 ms against 3.1).  With radii few long ones: a workgroup loads its window entries and adds 36 register sums
// per thread to LDS at its end, and 8192 of them cost more than the last round saved (11.0 ms against 9.9).  The result does not
// depend on the choice (profiles/power_notes.md)
#define PF_POWER_MAXWG_SHELLS 8192
#define PF_POWER_MAXWG_RADII 2048
#define PF_POWER_LDS_MAX 65536  // bytes of LDS a workgroup may ask for without an attribute

typedef unsigned long long u64;

struct PowerView { const void *spec; int n, nzh, nyl, y0; long long pitch; unsigned int rows, rows_per_wg; };
// the radii of one pair of launches: nr of them, the first is radius r0 of the call; E: their window tables [nr][n/2 + 1] in HBM
struct PowerBatch { int nr, r0, shells; const double *E; };
// the tables in HBM, 64-bit words: one allocation, cleared before the scan
struct PowerTabs { u64 *smax, *vmax, *nm, *k2, *nonfin, *pl, *vl; double *out; };

template <class F> __device__ __forceinline__ double power_load(const PowerView &v, unsigned int row, unsigned int kz) {
  const F *e = (const F *)v.spec + 2 * ((long long)row * v.pitch + kz);
  if constexpr (sizeof(F) == 8) { const double2 x = *(const double2 *)e; return pf_power_term<double>(x.x, x.y); }
  else { const float2 x = *(const float2 *)e; return pf_power_term<float>(x.x, x.y); }
}

// the rows of this workgroup and the (kx, ky_local) of the first
__device__ __forceinline__ void power_rows(const PowerView &v, unsigned int &r0, unsigned int &r1, unsigned int &kx, unsigned int &yl) {
  r0 = blockIdx.x * v.rows_per_wg;
  r1 = r0 + v.rows_per_wg < v.rows ? r0 + v.rows_per_wg : v.rows;
  kx = r0 / (unsigned int)v.nyl; yl = r0 - kx * (unsigned int)v.nyl;
}
__device__ __forceinline__ unsigned int power_abs(int s) { return (unsigned int)(s < 0 ? -s : s); }

// one mode of the scan: counters and maxima
template <int NR>
__device__ __forceinline__ void scan_mode(double t, unsigned int k2, unsigned int root, unsigned int w, const PowerBatch &bt, u64 *smax, u64 *snm, u64 *sk2, u64 &nonfin,
                                          const double *exy, const double *ez, double *vmx) {
  const bool fin = pf_power_finite(t);
  if (bt.shells) {
    const int b = pf_power_shell_of_root(k2, root);
    atomicAdd(&snm[b], (u64)w);
    if (k2) atomicAdd(&sk2[b], (u64)w * k2);
    if (fin) {   // (a plain read first: a maximum only grows, so a term that is not above what the read saw needs no atomic)
      const u64 tb = (u64)__double_as_longlong(t);
      if (tb > smax[b]) atomicMax(&smax[b], tb);
    }
    else nonfin += (u64)w;
  }
  if (NR > 0 && fin && k2) {
#pragma unroll
    for (int r = 0; r < NR; r++) {
      const double x = t * (exy[r] * ez[r]);
      vmx[r] = x > vmx[r] ? x : vmx[r];
    }
  }
}

// one mode of the accumulation: limbs into the shell's LDS counters and the radii's registers
template <int NR>
__device__ __forceinline__ void acc_mode(double t, unsigned int k2, unsigned int root, unsigned int w, const PowerBatch &bt, u64 *sp, const int *se, const double *exy,
                                         const double *ez, const int *ve, u64 (*va)[3]) {
  if (!pf_power_finite(t) || !(t > 0.0)) return;
  const double wt = (double)w * t;
  uint32_t l[3];
  if (bt.shells) {
    const int b = pf_power_shell_of_root(k2, root);
    pf_power_limbs(wt, se[b], l);
#pragma unroll
    for (int i = 0; i < 3; i++)
      if (l[i]) atomicAdd(&sp[3 * b + i], (u64)l[i]);
  }
  if (NR > 0 && k2) {
#pragma unroll
    for (int r = 0; r < NR; r++) {
      const double x = wt * (exy[r] * ez[r]);   // (the weight is a power of two: the rounding of w (t (E E E)))
      if (x > 0.0) {
        pf_power_limbs(x, ve[r], l);
        va[r][0] += l[0]; va[r][1] += l[1]; va[r][2] += l[2];
      }
    }
  }
}

// what the two kernels share of the walk: the columns of this thread and their window entries
template <int CG, int NR> struct PowerCols {
  unsigned int kz[CG], kz2[CG], w[CG], root[CG];
  bool on[CG];
  double ez[CG][NR ? NR : 1], eny[NR ? NR : 1];   // E_r at the thread's columns and at the Nyquist column
  __device__ __forceinline__ void init(const PowerView &v, const PowerBatch &bt) {
    const unsigned int half = (unsigned int)v.n / 2;
#pragma unroll
    for (int c = 0; c < CG; c++) {
      kz[c] = threadIdx.x + PF_POWER_BLOCK * c;
      on[c] = kz[c] < half;
      kz2[c] = on[c] ? kz[c] * kz[c] : 0; w[c] = kz[c] ? 2 : 1; root[c] = 0;
#pragma unroll
      for (int r = 0; r < NR; r++) ez[c][r] = (on[c] && r < bt.nr) ? bt.E[(size_t)r * v.nzh + kz[c]] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < NR; r++) eny[r] = r < bt.nr ? bt.E[(size_t)r * v.nzh + half] : 0.0;
  }
};
// E_r[|kx|] E_r[|ky|] of a row: the same in every thread
template <int NR> __device__ __forceinline__ void power_exy(const PowerView &v, const PowerBatch &bt, unsigned int ax, unsigned int ay, double *exy) {
#pragma unroll
  for (int r = 0; r < NR; r++) exy[r] = r < bt.nr ? bt.E[(size_t)r * v.nzh + ax] * bt.E[(size_t)r * v.nzh + ay] : 0.0;
}

template <class F, int CG, int NR>
__global__ void __launch_bounds__(PF_POWER_BLOCK) k_power_scan(PowerView v, PowerBatch bt, int nb, PowerTabs g) {
  extern __shared__ u64 lds[];
  u64 *smax = lds, *snm = lds + nb, *sk2 = lds + 2 * nb, *svmax = lds + 3 * nb, *snf = lds + 3 * nb + PF_POWER_NR;
  for (int k = threadIdx.x; k < 3 * nb + PF_POWER_NR + 1; k += PF_POWER_BLOCK) lds[k] = 0;
  __syncthreads();
  unsigned int r0, r1, kx, yl;
  power_rows(v, r0, r1, kx, yl);
  PowerCols<CG, NR> pc;
  pc.init(v, bt);
  double vmx[NR ? NR : 1], exy[NR ? NR : 1];
#pragma unroll
  for (int r = 0; r < (NR ? NR : 1); r++) vmx[r] = 0.0;
  u64 nonfin = 0;
  const unsigned int half = (unsigned int)v.n / 2;
  for (unsigned int row = r0; row < r1; row++) {
    const int sx = pf_power_signed((int)kx, v.n), sy = pf_power_signed((int)yl + v.y0, v.n);
    const unsigned int kxy2 = (unsigned int)(sx * sx + sy * sy);
    power_exy<NR>(v, bt, power_abs(sx), power_abs(sy), exy);
#pragma unroll
    for (int c = 0; c < CG; c++)
      if (pc.on[c]) {
        const double t = power_load<F>(v, row, pc.kz[c]);
        const unsigned int k2 = kxy2 + pc.kz2[c];
        if (bt.shells) pc.root[c] = row == r0 ? pf_power_isqrt(k2) : pf_power_isqrt_near(k2, pc.root[c]);
        scan_mode<NR>(t, k2, pc.root[c], pc.w[c], bt, smax, snm, sk2, nonfin, exy, pc.ez[c], vmx);
      }
    if (++yl == (unsigned int)v.nyl) { yl = 0; kx++; }
  }
  for (unsigned int row = r0 + threadIdx.x; row < r1; row += PF_POWER_BLOCK) {   // the Nyquist column
    const unsigned int x = row / (unsigned int)v.nyl, y = row - x * (unsigned int)v.nyl;
    const int sx = pf_power_signed((int)x, v.n), sy = pf_power_signed((int)y + v.y0, v.n);
    const unsigned int k2 = (unsigned int)(sx * sx + sy * sy) + half * half;
    power_exy<NR>(v, bt, power_abs(sx), power_abs(sy), exy);
    scan_mode<NR>(power_load<F>(v, row, half), k2, bt.shells ? pf_power_isqrt(k2) : 0, 1, bt, smax, snm, sk2, nonfin, exy, pc.eny, vmx);
  }
#pragma unroll
  for (int r = 0; r < NR; r++)
    if (vmx[r] > 0.0) atomicMax(&svmax[r], (u64)__double_as_longlong(vmx[r]));
  if (nonfin) atomicAdd(snf, nonfin);
  __syncthreads();
  if (bt.shells)
    for (int b = threadIdx.x; b < nb; b += PF_POWER_BLOCK) {
      if (snm[b]) { atomicAdd(&g.nm[b], snm[b]); atomicAdd(&g.k2[b], sk2[b]); }
      if (smax[b]) atomicMax(&g.smax[b], smax[b]);
    }
  for (int r = threadIdx.x; r < bt.nr; r += PF_POWER_BLOCK)
    if (svmax[r]) atomicMax(&g.vmax[bt.r0 + r], svmax[r]);
  if (threadIdx.x == 0 && snf[0]) atomicAdd(g.nonfin, snf[0]);
}

// three counters of a workgroup (weights 2^0, 2^32, 2^64) -> four limbs below 2^32 each, added to the four counters in HBM
__device__ __forceinline__ void power_flush(const u64 *s, u64 *gl) {
  u64 c0 = s[0], c1 = s[1], c2 = s[2];
  if (!(c0 | c1 | c2)) return;
  c1 += c0 >> 32; c2 += c1 >> 32;
  const u64 l0 = c0 & 0xffffffffull, l1 = c1 & 0xffffffffull, l2 = c2 & 0xffffffffull, l3 = c2 >> 32;
  if (l0) atomicAdd(&gl[0], l0);
  if (l1) atomicAdd(&gl[1], l1);
  if (l2) atomicAdd(&gl[2], l2);
  if (l3) atomicAdd(&gl[3], l3);
}

template <class F, int CG, int NR>
__global__ void __launch_bounds__(PF_POWER_BLOCK) k_power_acc(PowerView v, PowerBatch bt, int nb, PowerTabs g) {
  extern __shared__ u64 lds[];
  u64 *sp = lds, *sv = lds + 3 * nb;
  int *se = (int *)(lds + 3 * nb + 3 * PF_POWER_NR);
  for (int k = threadIdx.x; k < 3 * nb + 3 * PF_POWER_NR; k += PF_POWER_BLOCK) lds[k] = 0;
  for (int b = threadIdx.x; b < nb; b += PF_POWER_BLOCK) se[b] = g.smax[b] ? pf_power_exponent(__longlong_as_double((long long)g.smax[b])) : 0;
  __syncthreads();
  unsigned int r0, r1, kx, yl;
  power_rows(v, r0, r1, kx, yl);
  PowerCols<CG, NR> pc;
  pc.init(v, bt);
  double exy[NR ? NR : 1];
  int ve[NR ? NR : 1];
  u64 va[NR ? NR : 1][3];
#pragma unroll
  for (int r = 0; r < (NR ? NR : 1); r++) {
    const u64 m = (r < bt.nr) ? g.vmax[bt.r0 + r] : 0;
    ve[r] = m ? pf_power_exponent(__longlong_as_double((long long)m)) : 0;   // (no maximum: no positive term, nothing is added)
    va[r][0] = va[r][1] = va[r][2] = 0;
  }
  const unsigned int half = (unsigned int)v.n / 2;
  for (unsigned int row = r0; row < r1; row++) {
    const int sx = pf_power_signed((int)kx, v.n), sy = pf_power_signed((int)yl + v.y0, v.n);
    const unsigned int kxy2 = (unsigned int)(sx * sx + sy * sy);
    power_exy<NR>(v, bt, power_abs(sx), power_abs(sy), exy);
#pragma unroll
    for (int c = 0; c < CG; c++)
      if (pc.on[c]) {
        const double t = power_load<F>(v, row, pc.kz[c]);
        const unsigned int k2 = kxy2 + pc.kz2[c];
        if (bt.shells) pc.root[c] = row == r0 ? pf_power_isqrt(k2) : pf_power_isqrt_near(k2, pc.root[c]);
        acc_mode<NR>(t, k2, pc.root[c], pc.w[c], bt, sp, se, exy, pc.ez[c], ve, va);
      }
    if (++yl == (unsigned int)v.nyl) { yl = 0; kx++; }
  }
  for (unsigned int row = r0 + threadIdx.x; row < r1; row += PF_POWER_BLOCK) {   // the Nyquist column
    const unsigned int x = row / (unsigned int)v.nyl, y = row - x * (unsigned int)v.nyl;
    const int sx = pf_power_signed((int)x, v.n), sy = pf_power_signed((int)y + v.y0, v.n);
    const unsigned int k2 = (unsigned int)(sx * sx + sy * sy) + half * half;
    power_exy<NR>(v, bt, power_abs(sx), power_abs(sy), exy);
    acc_mode<NR>(power_load<F>(v, row, half), k2, bt.shells ? pf_power_isqrt(k2) : 0, 1, bt, sp, se, exy, pc.eny, ve, va);
  }
#pragma unroll
  for (int r = 0; r < NR; r++)
#pragma unroll
    for (int i = 0; i < 3; i++)
      if (va[r][i]) atomicAdd(&sv[3 * r + i], va[r][i]);
  __syncthreads();
  if (bt.shells)
    for (int b = threadIdx.x; b < nb; b += PF_POWER_BLOCK) power_flush(sp + 3 * b, g.pl + 4 * b);
  for (int r = threadIdx.x; r < bt.nr; r += PF_POWER_BLOCK) power_flush(sv + 3 * r, g.vl + 4 * (size_t)(bt.r0 + r));
}

__global__ void __launch_bounds__(PF_POWER_BLOCK) k_power_final(int nb, int ns, double n6, PowerTabs g) {
  const int i = blockIdx.x * PF_POWER_BLOCK + threadIdx.x;
  if (i >= nb + ns) return;
  const u64 mx = i < nb ? g.smax[i] : g.vmax[i - nb];
  const u64 *l = i < nb ? g.pl + 4 * i : g.vl + 4 * (i - nb);
  g.out[i] = mx ? pf_power_from_limbs(l, 4, pf_power_exponent(__longlong_as_double((long long)mx))) / n6 : 0.0;
}

// ------------------------------------------------------------------------------------------------------------ launches ----
// PF_POWER_TIMES=1: device ms of the last call, from the clearing of the tables (the upload of the window tables included) to the finishing kernel (profiles/tools/power_time.py)
static double power_last_ms = 0.0;
extern "C" int pf_debug_power_times(double *ms) {
  if (!ms) return 1;
  ms[0] = power_last_ms;
  return 0;
}
static bool power_times_on() {
  const char *env = getenv("PF_POWER_TIMES");
  return env && atoi(env) != 0;
}
struct PowerTimer {
  hipEvent_t a, b; hipStream_t st; bool on;
  PowerTimer(bool on_, hipStream_t st_) : a(nullptr), b(nullptr), st(st_), on(on_) {
    power_last_ms = 0.0;
    if (on) on = hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess && hipEventRecord(a, st) == hipSuccess;
  }
  void end() {
    float ms = 0.0f;
    if (on && hipEventRecord(b, st) == hipSuccess && hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&ms, a, b) == hipSuccess) power_last_ms = ms;
    on = false;
  }
  ~PowerTimer() { end(); if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); }
};

extern "C" int pf_power_bins(int n) { return n > 0 ? pf_power_nbins(n) : 0; }

// what every entry point refuses before anything else (no device is touched)
static int power_check_args(const char *who, int task, int ns, const double *radius_cells, const u64 *nmodes, const u64 *k2sum, const double *power, const double *variance,
                            const pf_power_info *info) {
  if (!nmodes || !k2sum || !power || !info) return pf_fail(task, "%s: null argument", who);
  if (ns < 0 || ns > PF_MAX_SMOOTH) return pf_fail(task, "%s: %d radii not in [0, %d]", who, ns, PF_MAX_SMOOTH);
  if (ns > 0 && (!radius_cells || !variance)) return pf_fail(task, "%s: %d radii with a null radius_cells or variance", who, ns);
  for (int i = 0; i < ns; i++)
    if (!(radius_cells[i] >= 0.0) || !pf_power_finite(radius_cells[i])) return pf_fail(task, "%s: radius %d (%g cells) is negative or not finite", who, i, radius_cells[i]);
  return 0;
}

struct PowerScratch { u64 *words; };
struct PowerGuard { PowerScratch *s; ~PowerGuard() { hipFree(s->words); s->words = nullptr; } };

struct PowerLaunch { PowerView v; int nb; unsigned int nwg; size_t lds_scan, lds_acc; PowerTabs g; hipStream_t st; };
// the scan and the accumulation of one batch of radii: the instantiation without radii, with up to four, or with up to PF_POWER_NR
template <class F, int CG, int NR> static int power_pair(const PowerLaunch &L, const PowerBatch &bt) {
  hipLaunchKernelGGL((k_power_scan<F, CG, NR>), dim3(L.nwg), dim3(PF_POWER_BLOCK), L.lds_scan, L.st, L.v, bt, L.nb, L.g);
  if (hipGetLastError() != hipSuccess) return 1;
  hipLaunchKernelGGL((k_power_acc<F, CG, NR>), dim3(L.nwg), dim3(PF_POWER_BLOCK), L.lds_acc, L.st, L.v, bt, L.nb, L.g);
  return hipGetLastError() != hipSuccess;
}
template <class F, int CG> static int power_batch(const PowerLaunch &L, const PowerBatch &bt) {
  return bt.nr == 0 ? power_pair<F, CG, 0>(L, bt) : bt.nr <= 4 ? power_pair<F, CG, 4>(L, bt) : power_pair<F, CG, PF_POWER_NR>(L, bt);
}

// the rows y0 .. y0 + nyl - 1 of a spectrum on the device -> this slab's sums on the device: g->nm (nb nmodes, nb k2sum and the
// nonfinite count, contiguous) and g->out (nb power, ns variance).  Nothing is synchronised
static int power_device(const char *who, int task, int fb, const void *spec, int n, int y0, int nyl, long long pitch, int ns, const double *radius_cells,
                        PowerScratch *s, PowerTabs *g, hipStream_t st) {
  const int nb = pf_power_nbins(n);
  PowerView v;
  v.spec = spec; v.n = n; v.nzh = n / 2 + 1; v.nyl = nyl; v.y0 = y0; v.pitch = pitch;
  v.rows = (unsigned int)n * (unsigned int)nyl;
  const unsigned int maxwg = ns ? PF_POWER_MAXWG_RADII : PF_POWER_MAXWG_SHELLS;
  v.rows_per_wg = (v.rows + maxwg - 1) / maxwg;
  const unsigned int nwg = (v.rows + v.rows_per_wg - 1) / v.rows_per_wg;
  if (n > 8 * PF_POWER_BLOCK) return pf_fail(task, "%s: a grid of %d has more than %d columns (internal error)", who, n, 4 * PF_POWER_BLOCK);
  const size_t lds_scan = (size_t)(3 * nb + PF_POWER_NR + 1) * 8, lds_acc = (size_t)(3 * nb + 3 * PF_POWER_NR) * 8 + (size_t)nb * 4;
  if (lds_scan > PF_POWER_LDS_MAX || lds_acc > PF_POWER_LDS_MAX) return pf_fail(task, "%s: the %d shells of a grid of %d do not fit the LDS tables", who, nb, n);
  if ((uintptr_t)spec & 15) return pf_fail(task, "%s: the spectrum is not 16-byte aligned (internal error)", who);
  // the window tables, one per radius: E_r[j] = exp(-(a_r j^2)), a_r = (2 pi / n)^2 R_r^2
  const double kf = 2.0 * 3.14159265358979323846 / (double)n;
  std::vector<double> E((size_t)ns * v.nzh);
  for (int r = 0; r < ns; r++) {
    const double a = (kf * kf) * (radius_cells[r] * radius_cells[r]);
    for (int j = 0; j < v.nzh; j++) E[(size_t)r * v.nzh + j] = pf_power_window_entry(a, j);
  }
  const size_t nwords = (size_t)7 * nb + 5 * (size_t)ns + 1, nout = (size_t)nb + ns;
  if (hipMalloc((void **)&s->words, (nwords + nout + E.size()) * 8) != hipSuccess) {
    (void)hipGetLastError(); s->words = nullptr;
    return pf_fail(task, "%s: cannot allocate %zu bytes of scratch on the device", who, (nwords + nout + E.size()) * 8);
  }
  PWHIP(task, who, hipMemsetAsync(s->words, 0, (nwords + nout) * 8, st));
  g->smax = s->words; g->vmax = g->smax + nb; g->nm = g->vmax + ns; g->k2 = g->nm + nb; g->nonfin = g->k2 + nb; g->pl = g->nonfin + 1; g->vl = g->pl + 4 * (size_t)nb;
  g->out = (double *)(g->vl + 4 * (size_t)ns);
  double *Edev = g->out + nout;
  if (ns) {   // (pageable memory: the copy has left E when the call returns)
    PWHIP(task, who, hipMemcpyAsync(Edev, E.data(), E.size() * 8, hipMemcpyHostToDevice, st));
    PWHIP(task, who, hipStreamSynchronize(st));
  }
  const PowerLaunch L = {v, nb, nwg, lds_scan, lds_acc, *g, st};
  const int cg = n / 2 <= PF_POWER_BLOCK ? 1 : n / 2 <= 2 * PF_POWER_BLOCK ? 2 : 4;
  for (int r0 = 0; r0 == 0 || r0 < ns; r0 += PF_POWER_NR) {
    PowerBatch bt;
    bt.r0 = r0; bt.nr = ns - r0 < PF_POWER_NR ? ns - r0 : PF_POWER_NR; bt.shells = r0 == 0; bt.E = Edev + (size_t)r0 * v.nzh;
    int rc;
    if (fb == 8) rc = cg == 1 ? power_batch<double, 1>(L, bt) : cg == 2 ? power_batch<double, 2>(L, bt) : power_batch<double, 4>(L, bt);
    else rc = cg == 1 ? power_batch<float, 1>(L, bt) : cg == 2 ? power_batch<float, 2>(L, bt) : power_batch<float, 4>(L, bt);
    if (rc) return pf_fail(task, "%s: launch failed", who);
  }
  const double n3 = (double)n * (double)n * (double)n;
  hipLaunchKernelGGL(k_power_final, dim3((unsigned int)((nout + PF_POWER_BLOCK - 1) / PF_POWER_BLOCK)), dim3(PF_POWER_BLOCK), 0, st, nb, ns, n3 * n3, *g);
  if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  return 0;
}

// the sums on the device -> the caller's arrays
static int power_fetch(const char *who, int task, int n, int ns, const PowerTabs &g, u64 total_modes, u64 *nmodes, u64 *k2sum, double *power, double *variance,
                       pf_power_info *info, hipStream_t st) {
  const int nb = pf_power_nbins(n);
  std::vector<u64> hu(2 * (size_t)nb + 1);
  std::vector<double> hd((size_t)nb + ns);
  PWHIP(task, who, hipMemcpyAsync(hu.data(), g.nm, hu.size() * 8, hipMemcpyDeviceToHost, st));
  PWHIP(task, who, hipMemcpyAsync(hd.data(), g.out, hd.size() * 8, hipMemcpyDeviceToHost, st));
  PWHIP(task, who, hipStreamSynchronize(st));
  memcpy(nmodes, hu.data(), (size_t)nb * 8);
  memcpy(k2sum, hu.data() + nb, (size_t)nb * 8);
  memcpy(power, hd.data(), (size_t)nb * 8);
  if (ns) memcpy(variance, hd.data() + nb, (size_t)ns * 8);
  info->modes = total_modes; info->nonfinite = hu[2 * (size_t)nb];
  return 0;
}

extern "C" int pf_power_spectrum(pf_ctx *c, int which, int ns, const double *radius_cells, unsigned long long *nmodes, unsigned long long *k2sum, double *power,
                                 double *variance, pf_power_info *info) {
  const char *who = "pf_power_spectrum";
  if (!c) return pf_fail(0, "%s: null argument", who);
  PfSpecView sv;
  pf_ctx_spec_geometry(c, &sv);
  if (power_check_args(who, sv.rank, ns, radius_cells, nmodes, k2sum, power, variance, info)) return 1;
  if (which < 0 || which > 3) return pf_fail(sv.rank, "%s: spectrum %d not in 0..3", who, which);
  if (pf_ctx_spec_view(c, who, which, &sv)) return 1;
  PowerScratch s = {nullptr};
  PowerGuard guard{&s};
  PowerTabs g;
  PowerTimer timer(power_times_on(), sv.stream);
  if (power_device(who, sv.rank, sv.fb, sv.spec, sv.n, sv.y0, sv.nyl, sv.nzp, ns, radius_cells, &s, &g, sv.stream)) return 1;
  timer.end();
  // the box's numbers on every rank: nmodes, k2sum and the nonfinite count as integers, power and variance as doubles
  const size_t nb = (size_t)pf_power_nbins(sv.n);
  if (pf_ctx_allreduce(c, g.nm, 2 * nb + 1, 1) || pf_ctx_allreduce(c, g.out, nb + ns, 0)) return 1;
  return power_fetch(who, sv.rank, sv.n, ns, g, (u64)sv.n * sv.n * sv.n, nmodes, k2sum, power, variance, info, sv.stream);
}

extern "C" int pf_debug_power_spectrum(int field_bytes, int n, int y0, int nyl, const double *spec_host, int ns, const double *radius_cells, unsigned long long *nmodes,
                                       unsigned long long *k2sum, double *power, double *variance, pf_power_info *info) {
  const char *who = "pf_debug_power_spectrum";
  if (!spec_host) return pf_fail(0, "%s: null argument", who);
  if (power_check_args(who, 0, ns, radius_cells, nmodes, k2sum, power, variance, info)) return 1;
  if (field_bytes != 4 && field_bytes != 8) return pf_fail(0, "%s: fields of %d bytes (4 or 8)", who, field_bytes);
  if (n < 2 || n > 2048 || (n & 1)) return pf_fail(0, "%s: a grid of %d (even, 2 to 2048)", who, n);
  if (y0 < 0 || nyl < 1 || y0 + nyl > n) return pf_fail(0, "%s: rows %d .. %d leave the grid of %d", who, y0, y0 + nyl - 1, n);
  // the production layout: rows of whole 128-byte lines, and NaN patterns in the padding that no sum may see
  const int nzh = n / 2 + 1, nzp = n / 2 + 64 / field_bytes;
  const long long nrows = (long long)nyl * n;
  const size_t in_bytes = (size_t)nrows * nzh * 16, field = (size_t)nrows * nzp * 2 * field_bytes;
  struct Bufs { void *in, *spec; ~Bufs() { hipFree(in); hipFree(spec); } } d = {nullptr, nullptr};
  if (hipMalloc(&d.in, in_bytes) != hipSuccess || hipMalloc(&d.spec, field) != hipSuccess) {
    (void)hipGetLastError();
    return pf_fail(0, "%s: cannot allocate %zu bytes on the device", who, in_bytes + field);
  }
  PWHIP(0, who, hipMemcpy(d.in, spec_host, in_bytes, hipMemcpyHostToDevice));
  PWHIP(0, who, hipMemset(d.spec, 0xff, field));
  // [ky_local][kx][kz] of the caller -> [kx][ky_local][kz] rows of nzp
  if (pf_launch_spec_import_t(field_bytes, (const double *)d.in, d.spec, n, nyl, nzh, nzp, nullptr)) return pf_fail(0, "%s: launch failed", who);
  PowerScratch s = {nullptr};
  PowerGuard guard{&s};
  PowerTabs g;
  PowerTimer timer(power_times_on(), nullptr);
  if (power_device(who, 0, field_bytes, d.spec, n, y0, nyl, nzp, ns, radius_cells, &s, &g, nullptr)) return 1;
  timer.end();
  return power_fetch(who, 0, n, ns, g, (u64)nyl * n * n, nmodes, k2sum, power, variance, info, nullptr);
}
