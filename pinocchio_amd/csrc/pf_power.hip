// pf_power.hip -- every shell sum over spectra that lie on the device.  First the shell-averaged power and Gaussian-smoothed variances
// of one half-spectrum (include/pinfmax.h: pf_power_spectrum, pf_debug_power_spectrum): two streaming reads of the rows of this rank's ky-slab, [kx][ky_local] rows of `pitch`
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
// Then the sums of two spectra, |m|^2 and Re(m conj lin) per shell, for pf_matter.hip (pf_matter_shells_device; the mode arithmetic is
// pf_matter_core.h's) -- the same two passes and the same fixed point on the same helpers, with a walk of their own (matter_walk: a
// thread at the columns kz = t, t + 256, ..., the root of every mode anew), not merged with the one above:
//  k_matter_scan  three positive sums per shell (0 |m|^2, 1 the positive cross terms, 2 the negative ones): ONE scan takes the largest
//                 term of every shell for all three, with nmodes, k2sum and the modes whose terms are not finite (five LDS tables;
//                 where they do not fit, n above about 1800, a scan per sum).
//  k_matter_acc   an accumulation per sum adds every term as three 32-bit limbs scaled to that maximum (LDS holds one sum's
//                 counters, so every grid up to 2048 fits).  Four passes over the two spectra (profiles/matter_notes.md).
//  k_matter_final limbs -> double, times 1 / N^6; cross = positive - negative, formed once.
//  k_matter_slot_max  with more than one rank: the maxima of the scans over the ranks, before any limb is formed.
// And their multipoles for pf_halo.hip (pf_multipole_shells_device; pf_multipole_core.h): on the same walk every term times the
// Legendre weights L2, L4 of the mode's angle to one axis, eleven positive sums per shell:
//  k_multipole_scan / k_multipole_acc  the sums [first, first + ns) of the eleven, as many as the launcher found LDS for; a signed term
//                 goes to the one sum its sign selects.  k_multipole_final: power and cross of l = 0, 2, 4 and the eleven sums.
//
// Every index is in range by construction: a mode is read only in the workgroup's own rows (< rows), at a column kz <= n/2 < pitch;
// a shell is below pf_power_nbins(n), which sized every table, since k2 <= 3 (n/2)^2; a radius index is below the batch's nr <=
// PF_POWER_NR inside a kernel and below ns in HBM; the window tables are read at |kx|, |ky|, kz <= n/2, their row length less one;
// the dynamic LDS is sized by nbins and PF_POWER_NR; the deconvolution table of the two-spectrum passes is read at |kx|, |ky|, kz <=
// n/2, its length less one, and a counter slot is blockIdx.x mod PF_MATTER_SLOTS of the MC_COUNT words each the caller allocated.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pf_internal.h"
#include "pf_corr_core.h"        // one cell of the separation-space pass; it includes pf_multipole_core.h (the Legendre weights of a mode), which includes
                                 // pf_matter_core.h (the two terms of a mode of two spectra) and pf_power_core.h

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

// one complex element of a spectrum, widened to double (exact), and its term
template <class F> __device__ __forceinline__ void power_load(const void *spec, long long pitch, unsigned int row, unsigned int kz, double &re, double &im) {
  const F *e = (const F *)spec + 2 * ((long long)row * pitch + kz);
  if constexpr (sizeof(F) == 8) { const double2 x = *(const double2 *)e; re = x.x; im = x.y; }
  else { const float2 x = *(const float2 *)e; re = (double)x.x; im = (double)x.y; }
}
template <class F> __device__ __forceinline__ double power_term_at(const PowerView &v, unsigned int row, unsigned int kz) {
  double re, im;
  power_load<F>(v.spec, v.pitch, row, kz, re, im);
  return pf_power_term<double>(re, im);
}

// the rows of this workgroup and the (kx, ky_local) of the first
__device__ __forceinline__ void power_rows(const PowerView &v, unsigned int &r0, unsigned int &r1, unsigned int &kx, unsigned int &yl) {
  r0 = blockIdx.x * v.rows_per_wg;
  r1 = r0 + v.rows_per_wg < v.rows ? r0 + v.rows_per_wg : v.rows;
  kx = r0 / (unsigned int)v.nyl; yl = r0 - kx * (unsigned int)v.nyl;
}
__device__ __forceinline__ unsigned int power_abs(int s) { return (unsigned int)(s < 0 ? -s : s); }
// a maximum in LDS only grows: a term that is not above what a relaxed read saw needs no atomic
__device__ __forceinline__ void power_max_lds(u64 *p, u64 v) {
  if (v > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) atomicMax(p, v);
}
// the scale exponent of a stored maximum, the bit pattern of a double (none: no positive term, nothing is added under it)
__device__ __forceinline__ int power_exponent_of(u64 m) { return m ? pf_power_exponent(__longlong_as_double((long long)m)) : 0; }

// one mode of the scan: counters and maxima
template <int NR>
__device__ __forceinline__ void scan_mode(double t, unsigned int k2, unsigned int root, unsigned int w, const PowerBatch &bt, u64 *smax, u64 *snm, u64 *sk2, u64 &nonfin,
                                          const double *exy, const double *ez, double *vmx) {
  const bool fin = pf_power_finite(t);
  if (bt.shells) {
    const int b = pf_power_shell_of_root(k2, root);
    atomicAdd(&snm[b], (u64)w);
    if (k2) atomicAdd(&sk2[b], (u64)w * k2);
    if (fin) power_max_lds(&smax[b], (u64)__double_as_longlong(t));
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
        const double t = power_term_at<F>(v, row, pc.kz[c]);
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
    scan_mode<NR>(power_term_at<F>(v, row, half), k2, bt.shells ? pf_power_isqrt(k2) : 0, 1, bt, smax, snm, sk2, nonfin, exy, pc.eny, vmx);
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
  for (int b = threadIdx.x; b < nb; b += PF_POWER_BLOCK) se[b] = power_exponent_of(g.smax[b]);
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
    ve[r] = power_exponent_of((r < bt.nr) ? g.vmax[bt.r0 + r] : 0);
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
        const double t = power_term_at<F>(v, row, pc.kz[c]);
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
    acc_mode<NR>(power_term_at<F>(v, row, half), k2, bt.shells ? pf_power_isqrt(k2) : 0, 1, bt, sp, se, exy, pc.eny, ve, va);
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
  g.out[i] = mx ? pf_power_from_limbs(l, 4, power_exponent_of(mx)) / n6 : 0.0;
}

// ------------------------------------------------------------------------------------------------------------ two spectra ----
// the rows of both spectra (spec: the matter's); lin null: no cross sums; C null: no deconvolution
struct MatterView : PowerView { const void *lin; const double *C; int los; };   // los: the axis of the line of sight (the multipole passes)
// the tables in HBM, 64-bit words: one allocation, cleared before the first scan.  smax / pl: [3][nb] and [3][4 nb] by `which`
struct MatterTabs { u64 *smax, *nm, *k2, *pl; double *out; };

__device__ __forceinline__ u64 power_wave_sum(u64 v) {
  for (int off = warpSize / 2; off; off >>= 1) v += __shfl_down(v, off);
  return v;
}

// the auto and the cross term of mode (row, kz); fin: both are finite (a mode with a term that is not is in no sum)
template <class F> __device__ __forceinline__ void matter_terms(const MatterView &v, unsigned int row, unsigned int kz, double cxy, double &ta, double &tc, bool &fin) {
  double a, b, p = 0.0, q = 0.0;
  power_load<F>(v.spec, v.pitch, row, kz, a, b);
  const double c = v.C ? pf_matter_deconv(cxy, 1.0, v.C[kz]) : -1.0;
  ta = pf_matter_auto(a, b, c);
  tc = 0.0;
  if (v.lin) { power_load<F>(v.lin, v.pitch, row, kz, p, q); tc = pf_matter_cross(a, b, p, q, c); }
  fin = pf_power_finite(ta) && pf_power_finite(tc);
}

// what both passes share: the rows of this workgroup one after the other, thread t at the columns kz = t, t + 256, ... <= n/2; op also
// gets a, the squared wavenumber along axis v.los (the multipole passes; the others ignore it)
template <class F, class OP> __device__ __forceinline__ void matter_walk(const MatterView &v, OP op) {
  const unsigned int r0 = blockIdx.x * v.rows_per_wg, r1 = r0 + v.rows_per_wg < v.rows ? r0 + v.rows_per_wg : v.rows;
  const unsigned int half = (unsigned int)v.n / 2;
  for (unsigned int row = r0; row < r1; row++) {
    const unsigned int kx = row / (unsigned int)v.nyl, yl = row - kx * (unsigned int)v.nyl;
    const int sx = pf_power_signed((int)kx, v.n), sy = pf_power_signed((int)yl + v.y0, v.n);
    const unsigned int kxy2 = (unsigned int)(sx * sx + sy * sy);
    const double cxy = v.C ? v.C[power_abs(sx)] * v.C[power_abs(sy)] : 1.0;
    for (unsigned int kz = threadIdx.x; kz <= half; kz += PF_POWER_BLOCK) {
      const unsigned int k2 = kxy2 + kz * kz, w = (kz > 0 && kz < half) ? 2u : 1u;
      bool fin;
      double ta, tc;
      matter_terms<F>(v, row, kz, cxy, ta, tc, fin);
      op(pf_power_shell(k2), k2, pf_multipole_a(v.los, sx, sy, kz), w, ta, tc, fin);
    }
  }
}

// ALL: the maxima of the three sums in one pass (LDS: five tables of nb words, the launch says whether they fit); else that of `which`
// alone (three tables).  nmodes, k2sum and the modes that are not finite are counted by the pass that takes the maximum of sum 0;
// the last into the caller's counters, the copy of this workgroup's slot (pf_internal.h)
template <class F, bool ALL>
__global__ void __launch_bounds__(PF_POWER_BLOCK) k_matter_scan(MatterView v, int which, int nb, MatterTabs g, u64 *counters) {
  extern __shared__ u64 lds[];
  constexpr int NS = ALL ? 3 : 1;
  u64 *smax = lds, *snm = lds + NS * nb, *sk2 = lds + (NS + 1) * nb;
  for (int k = threadIdx.x; k < (NS + 2) * nb; k += PF_POWER_BLOCK) lds[k] = 0;
  __syncthreads();
  const bool count = ALL || which == 0;
  u64 nonfin = 0;
  matter_walk<F>(v, [&](int b, unsigned int k2, unsigned int, unsigned int w, double ta, double tc, bool fin) {
    if (count) {
      atomicAdd(&snm[b], (u64)w);
      if (k2) atomicAdd(&sk2[b], (u64)w * k2);
      if (!fin) nonfin += (u64)w;
    }
    if (!fin) return;
#pragma unroll
    for (int s = 0; s < NS; s++) {
      const double t = pf_matter_part(ALL ? s : which, ta, tc);
      if (t > 0.0) power_max_lds(&smax[s * nb + b], (u64)__double_as_longlong(t));
    }
  });
  nonfin = power_wave_sum(nonfin);
  if (nonfin && (threadIdx.x & (warpSize - 1)) == 0) atomicAdd(counters + (size_t)(blockIdx.x % PF_MATTER_SLOTS) * MC_COUNT + MC_NONFIN_MODES, nonfin);
  __syncthreads();
  for (int b = threadIdx.x; b < nb; b += PF_POWER_BLOCK) {
    if (count && snm[b]) { atomicAdd(&g.nm[b], snm[b]); atomicAdd(&g.k2[b], sk2[b]); }
#pragma unroll
    for (int s = 0; s < NS; s++)
      if (smax[s * nb + b]) atomicMax(&g.smax[(size_t)(ALL ? s : which) * nb + b], smax[s * nb + b]);
  }
}

template <class F>
__global__ void __launch_bounds__(PF_POWER_BLOCK) k_matter_acc(MatterView v, int which, int nb, MatterTabs g) {
  extern __shared__ u64 lds[];
  u64 *sp = lds;
  int *se = (int *)(lds + 3 * nb);
  for (int k = threadIdx.x; k < 3 * nb; k += PF_POWER_BLOCK) lds[k] = 0;
  for (int b = threadIdx.x; b < nb; b += PF_POWER_BLOCK) se[b] = power_exponent_of(g.smax[(size_t)which * nb + b]);
  __syncthreads();
  matter_walk<F>(v, [&](int b, unsigned int, unsigned int, unsigned int w, double ta, double tc, bool fin) {
    const double t = pf_matter_part(which, ta, tc);
    if (!fin || !(t > 0.0)) return;
    uint32_t l[3];
    pf_power_limbs((double)w * t, se[b], l);
#pragma unroll
    for (int i = 0; i < 3; i++)
      if (l[i]) atomicAdd(&sp[3 * b + i], (u64)l[i]);
  });
  __syncthreads();
  for (int b = threadIdx.x; b < nb; b += PF_POWER_BLOCK) power_flush(sp + 3 * b, g.pl + 4 * ((size_t)which * nb + b));
}

// out: [nb] power, [nb] cross = positive - negative, formed once
__global__ void __launch_bounds__(PF_POWER_BLOCK) k_matter_final(int nb, double n6, MatterTabs g) {
  const int b = blockIdx.x * PF_POWER_BLOCK + threadIdx.x;
  if (b >= nb) return;
  double s[3];
  for (int which = 0; which < 3; which++) {
    const u64 mx = g.smax[(size_t)which * nb + b];
    s[which] = mx ? pf_power_from_limbs(g.pl + 4 * ((size_t)which * nb + b), 4, power_exponent_of(mx)) : 0.0;
  }
  g.out[b] = s[0] / n6;
  g.out[nb + b] = (s[1] - s[2]) / n6;
}

// ---- the multipoles of the same two spectra (pf_multipole_core.h): eleven positive sums per shell, the terms of a mode times the
// Legendre weights of its angle to axis v.los.  The same two passes on the same walk; a launch carries the sums [first, first + ns),
// as many as the launcher found room for in LDS.  The tables of MatterTabs are [11][nb] (smax) and [11][4 nb] (pl) here
template <class F>
__global__ void __launch_bounds__(PF_POWER_BLOCK) k_multipole_scan(MatterView v, int first, int ns, int nb, MatterTabs g, u64 *counters) {
  extern __shared__ u64 lds[];
  u64 *smax = lds, *snm = lds + (size_t)ns * nb, *sk2 = snm + nb;
  for (int k = threadIdx.x; k < (ns + 2) * nb; k += PF_POWER_BLOCK) lds[k] = 0;
  __syncthreads();
  const bool count = first == 0;   // nmodes, k2sum and the modes that are not finite: by the launch that carries sum 0
  u64 nonfin = 0;
  matter_walk<F>(v, [&](int b, unsigned int k2, unsigned int a, unsigned int w, double ta, double tc, bool fin) {
    if (count) {
      atomicAdd(&snm[b], (u64)w);
      if (k2) atomicAdd(&sk2[b], (u64)w * k2);
      if (!fin) nonfin += (u64)w;
    }
    if (!fin) return;
    double L2, L4;
    pf_multipole_weights(a, k2, &L2, &L4);
    double x[6];
    pf_multipole_terms(ta, tc, L2, L4, x);
#pragma unroll
    for (int k = 0; k < 6; k++) {   // (a term has one sum, by its sign: at most six maxima per mode, whatever the launch carries)
      const double t = fabs(x[k]);
      const int s = pf_multipole_sum_of(k, x[k]) - first;
      if (t > 0.0 && s >= 0 && s < ns) power_max_lds(&smax[s * nb + b], (u64)__double_as_longlong(t));
    }
  });
  nonfin = power_wave_sum(nonfin);
  if (nonfin && (threadIdx.x & (warpSize - 1)) == 0) atomicAdd(counters + (size_t)(blockIdx.x % PF_MATTER_SLOTS) * MC_COUNT + MC_NONFIN_MODES, nonfin);
  __syncthreads();
  for (int b = threadIdx.x; b < nb; b += PF_POWER_BLOCK) {
    if (count && snm[b]) { atomicAdd(&g.nm[b], snm[b]); atomicAdd(&g.k2[b], sk2[b]); }
    for (int s = 0; s < ns; s++)
      if (smax[s * nb + b]) atomicMax(&g.smax[(size_t)(first + s) * nb + b], smax[s * nb + b]);
  }
}

template <class F>
__global__ void __launch_bounds__(PF_POWER_BLOCK) k_multipole_acc(MatterView v, int first, int ns, int nb, MatterTabs g) {
  extern __shared__ u64 lds[];
  u64 *sp = lds;
  int *se = (int *)(lds + (size_t)3 * ns * nb);
  for (int k = threadIdx.x; k < 3 * ns * nb; k += PF_POWER_BLOCK) lds[k] = 0;
  for (int k = threadIdx.x; k < ns * nb; k += PF_POWER_BLOCK) se[k] = power_exponent_of(g.smax[(size_t)first * nb + k]);
  __syncthreads();
  matter_walk<F>(v, [&](int b, unsigned int k2, unsigned int a, unsigned int w, double ta, double tc, bool fin) {
    if (!fin) return;
    double L2, L4;
    pf_multipole_weights(a, k2, &L2, &L4);
    double x[6];
    pf_multipole_terms(ta, tc, L2, L4, x);
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const double t = fabs(x[k]);
      const int s = pf_multipole_sum_of(k, x[k]) - first;
      if (!(t > 0.0) || s < 0 || s >= ns) continue;
      uint32_t l[3];
      pf_power_limbs((double)w * t, se[s * nb + b], l);
#pragma unroll
      for (int i = 0; i < 3; i++)
        if (l[i]) atomicAdd(&sp[3 * (s * nb + b) + i], (u64)l[i]);
    }
  });
  __syncthreads();
  for (int k = threadIdx.x; k < ns * nb; k += PF_POWER_BLOCK) power_flush(sp + 3 * k, g.pl + 4 * ((size_t)first * nb + k));
}

// out: [3][nb] power and [3][nb] cross (l = 0, 2, 4: positive - negative, formed once), then [11][nb] the positive sums themselves
__global__ void __launch_bounds__(PF_POWER_BLOCK) k_multipole_final(int nb, double n6, MatterTabs g) {
  const int b = blockIdx.x * PF_POWER_BLOCK + threadIdx.x;
  if (b >= nb) return;
  double s[PF_MULTIPOLE_NSUMS];
  double *parts = g.out + 6 * (size_t)nb;
#pragma unroll
  for (int which = 0; which < PF_MULTIPOLE_NSUMS; which++) {
    const u64 mx = g.smax[(size_t)which * nb + b];
    s[which] = mx ? pf_power_from_limbs(g.pl + 4 * ((size_t)which * nb + b), 4, power_exponent_of(mx)) : 0.0;
    parts[(size_t)which * nb + b] = s[which] / n6;
  }
  g.out[b] = s[0] / n6;
  g.out[nb + b] = (s[1] - s[2]) / n6;
  g.out[2 * nb + b] = (s[3] - s[4]) / n6;
#pragma unroll
  for (int l = 0; l < 3; l++) g.out[(size_t)(3 + l) * nb + b] = (s[5 + 2 * l] - s[6 + 2 * l]) / n6;
}

// out[i] = the largest of slots[p][i], p < P: the maximum over the ranks of `count` words, after the sum over the ranks of vectors in
// which every rank filled its own slot alone
__global__ void __launch_bounds__(PF_POWER_BLOCK) k_matter_slot_max(const u64 *slots, int P, int count, u64 *out) {
  const int i = blockIdx.x * PF_POWER_BLOCK + threadIdx.x;
  if (i >= count) return;
  u64 m = 0;
  for (int p = 0; p < P; p++) { const u64 v = slots[(size_t)p * count + i]; m = v > m ? v : m; }
  out[i] = m;
}

// ---- the two passes of pf_halo_correlation (pf_corr_core.h).  The form pass: on the rows of matter_walk every stored mode of spec
// becomes ((F)(t / N^3), 0), t its auto term (which 0) or its cross term with v.lin (which 1), where it stood or in another field of
// the same layout: a mode is read and written by the one lane that owns it.  A term that is not finite is written as zero and
// counted with its weight; the k = 0 mode is written as zero
template <class F>
__global__ void __launch_bounds__(PF_POWER_BLOCK) k_corr_form(MatterView v, void *out, int which, double n3, u64 *counters) {
  const unsigned int r0 = blockIdx.x * v.rows_per_wg, r1 = r0 + v.rows_per_wg < v.rows ? r0 + v.rows_per_wg : v.rows;
  const unsigned int half = (unsigned int)v.n / 2;
  u64 nonfin = 0;
  for (unsigned int row = r0; row < r1; row++) {
    const unsigned int kx = row / (unsigned int)v.nyl, yl = row - kx * (unsigned int)v.nyl;
    const int sx = pf_power_signed((int)kx, v.n), sy = pf_power_signed((int)yl + v.y0, v.n);
    const unsigned int kxy2 = (unsigned int)(sx * sx + sy * sy);
    const double cxy = v.C ? v.C[power_abs(sx)] * v.C[power_abs(sy)] : 1.0;
    for (unsigned int kz = threadIdx.x; kz <= half; kz += PF_POWER_BLOCK) {
      bool fin, bad;
      double ta, tc;
      matter_terms<F>(v, row, kz, cxy, ta, tc, fin);
      const double q = pf_corr_form(which ? tc : ta, kxy2 + kz * kz, n3, &bad);
      if (bad) nonfin += (kz > 0 && kz < half) ? 2u : 1u;
      F *e = (F *)out + 2 * ((long long)row * v.pitch + kz);
      if constexpr (sizeof(F) == 8) *(double2 *)e = make_double2(q, 0.0);
      else *(float2 *)e = make_float2((float)q, 0.0f);
    }
  }
  nonfin = power_wave_sum(nonfin);
  if (nonfin && (threadIdx.x & (warpSize - 1)) == 0) atomicAdd(counters + (size_t)(blockIdx.x % PF_MATTER_SLOTS) * MC_COUNT + MC_NONFIN_MODES, nonfin);
}

// The shell pass in separation space: a real field, the planes [x0, x0 + nxl) of the box in rows (x_local, y) of `pitch` reals of which
// the first n are cells.  The same two passes and the same fixed point as above on a walk of its own (corr_walk: workgroup g takes
// the rows [g rpw, (g + 1) rpw), thread t the cells z = t, t + 256, ... < n); six positive sums per shell, a launch carries the sums
// [first, first + ns).  Tables: smax [6][nb], nm [nb], k2 [nb], pl [6][4 nb], nonfin [1]
struct CorrView { const void *real; int n, nxl, x0, los; long long pitch; unsigned int rows, rows_per_wg; };
struct CorrTabs { u64 *smax, *nm, *k2, *pl, *nonfin; double *out; };

template <class F, class OP> __device__ __forceinline__ void corr_walk(const CorrView &v, OP op) {
  const unsigned int r0 = blockIdx.x * v.rows_per_wg, r1 = r0 + v.rows_per_wg < v.rows ? r0 + v.rows_per_wg : v.rows;
  for (unsigned int row = r0; row < r1; row++) {
    const unsigned int xl = row / (unsigned int)v.n, y = row - xl * (unsigned int)v.n;
    const int sx = pf_power_signed((int)xl + v.x0, v.n), sy = pf_power_signed((int)y, v.n);
    const F *line = (const F *)v.real + (long long)row * v.pitch;
    for (unsigned int z = threadIdx.x; z < (unsigned int)v.n; z += PF_POWER_BLOCK) {
      const int sz = pf_power_signed((int)z, v.n);
      const unsigned int r2 = pf_corr_r2(sx, sy, sz);
      op(pf_power_shell(r2), r2, pf_corr_a(v.los, sx, sy, sz), (double)line[z]);
    }
  }
}

// ncells, r2sum and the cells that are not finite are counted by the launch that carries sum 0
template <class F>
__global__ void __launch_bounds__(PF_POWER_BLOCK) k_corr_scan(CorrView v, int first, int ns, int nb, CorrTabs g) {
  extern __shared__ u64 lds[];
  u64 *smax = lds, *snm = lds + (size_t)ns * nb, *sk2 = snm + nb;
  for (int k = threadIdx.x; k < (ns + 2) * nb; k += PF_POWER_BLOCK) lds[k] = 0;
  __syncthreads();
  const bool count = first == 0;
  u64 nonfin = 0;
  corr_walk<F>(v, [&](int b, unsigned int r2, unsigned int a, double val) {
    const bool fin = pf_power_finite(val);
    if (count) {
      atomicAdd(&snm[b], (u64)1);
      if (r2) atomicAdd(&sk2[b], (u64)r2);
      if (!fin) nonfin++;
    }
    if (!fin) return;
    double L2, L4, x[PF_CORR_NORDERS];
    pf_multipole_weights(a, r2, &L2, &L4);
    pf_corr_terms(val, L2, L4, x);
#pragma unroll
    for (int k = 0; k < PF_CORR_NORDERS; k++) {
      const double t = fabs(x[k]);
      const int s = pf_corr_sum_of(k, x[k]) - first;
      if (t > 0.0 && s >= 0 && s < ns) power_max_lds(&smax[s * nb + b], (u64)__double_as_longlong(t));
    }
  });
  nonfin = power_wave_sum(nonfin);
  if (nonfin && (threadIdx.x & (warpSize - 1)) == 0) atomicAdd(g.nonfin, nonfin);
  __syncthreads();
  for (int b = threadIdx.x; b < nb; b += PF_POWER_BLOCK) {
    if (count && snm[b]) { atomicAdd(&g.nm[b], snm[b]); atomicAdd(&g.k2[b], sk2[b]); }
    for (int s = 0; s < ns; s++)
      if (smax[s * nb + b]) atomicMax(&g.smax[(size_t)(first + s) * nb + b], smax[s * nb + b]);
  }
}

template <class F>
__global__ void __launch_bounds__(PF_POWER_BLOCK) k_corr_acc(CorrView v, int first, int ns, int nb, CorrTabs g) {
  extern __shared__ u64 lds[];
  u64 *sp = lds;
  int *se = (int *)(lds + (size_t)3 * ns * nb);
  for (int k = threadIdx.x; k < 3 * ns * nb; k += PF_POWER_BLOCK) lds[k] = 0;
  for (int k = threadIdx.x; k < ns * nb; k += PF_POWER_BLOCK) se[k] = power_exponent_of(g.smax[(size_t)first * nb + k]);
  __syncthreads();
  corr_walk<F>(v, [&](int b, unsigned int r2, unsigned int a, double val) {
    if (!pf_power_finite(val)) return;
    double L2, L4, x[PF_CORR_NORDERS];
    pf_multipole_weights(a, r2, &L2, &L4);
    pf_corr_terms(val, L2, L4, x);
#pragma unroll
    for (int k = 0; k < PF_CORR_NORDERS; k++) {
      const double t = fabs(x[k]);
      const int s = pf_corr_sum_of(k, x[k]) - first;
      if (!(t > 0.0) || s < 0 || s >= ns) continue;
      uint32_t l[3];
      pf_power_limbs(t, se[s * nb + b], l);
#pragma unroll
      for (int i = 0; i < 3; i++)
        if (l[i]) atomicAdd(&sp[3 * (s * nb + b) + i], (u64)l[i]);
    }
  });
  __syncthreads();
  for (int k = threadIdx.x; k < ns * nb; k += PF_POWER_BLOCK) power_flush(sp + 3 * k, g.pl + 4 * ((size_t)first * nb + k));
}

// out: [3][nb] xi (l = 0, 2, 4: positive - negative, formed once), then [6][nb] the positive sums themselves
__global__ void __launch_bounds__(PF_POWER_BLOCK) k_corr_final(int nb, CorrTabs g) {
  const int b = blockIdx.x * PF_POWER_BLOCK + threadIdx.x;
  if (b >= nb) return;
  double s[PF_CORR_NSUMS];
  double *parts = g.out + PF_CORR_NORDERS * (size_t)nb;
#pragma unroll
  for (int which = 0; which < PF_CORR_NSUMS; which++) {
    const u64 mx = g.smax[(size_t)which * nb + b];
    s[which] = mx ? pf_power_from_limbs(g.pl + 4 * ((size_t)which * nb + b), 4, power_exponent_of(mx)) : 0.0;
    parts[(size_t)which * nb + b] = s[which];
  }
#pragma unroll
  for (int l = 0; l < PF_CORR_NORDERS; l++) g.out[(size_t)l * nb + b] = s[2 * l] - s[2 * l + 1];
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

// what every shell pass begins with: the rows of a ky-slab over at most maxwg workgroups, and the two refusals -- LDS tables (`lds`
// bytes, the largest of the passes) beyond what a workgroup may ask for, a spectrum (the one, or a of two) off the 16 bytes of a load
static int power_view(const char *who, int task, const char *article, const void *spec, const void *lin, int n, int y0, int nyl, long long pitch, unsigned int maxwg,
                      size_t lds, PowerView *v, unsigned int *nwg) {
  v->spec = spec; v->n = n; v->nzh = n / 2 + 1; v->nyl = nyl; v->y0 = y0; v->pitch = pitch;
  v->rows = (unsigned int)n * (unsigned int)nyl;
  v->rows_per_wg = (v->rows + maxwg - 1) / maxwg;
  *nwg = (v->rows + v->rows_per_wg - 1) / v->rows_per_wg;
  if (lds > PF_POWER_LDS_MAX) return pf_fail(task, "%s: the %d shells of a grid of %d do not fit the LDS tables", who, pf_power_nbins(n), n);
  if (((uintptr_t)spec | (uintptr_t)lin) & 15) return pf_fail(task, "%s: %s spectrum is not 16-byte aligned (internal error)", who, article);
  return 0;
}
// a table of the host -> the device, behind the out array of a call's words (pageable memory: the copy has left the table on return)
static int power_upload(const char *who, int task, double *dev, const std::vector<double> &tab, hipStream_t st) {
  PWHIP(task, who, hipMemcpyAsync(dev, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, st));
  PWHIP(task, who, hipStreamSynchronize(st));
  return 0;
}

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
  if (n > 8 * PF_POWER_BLOCK) return pf_fail(task, "%s: a grid of %d has more than %d columns (internal error)", who, n, 4 * PF_POWER_BLOCK);
  const size_t lds_scan = (size_t)(3 * nb + PF_POWER_NR + 1) * 8, lds_acc = (size_t)(3 * nb + 3 * PF_POWER_NR) * 8 + (size_t)nb * 4;
  PowerView v;
  unsigned int nwg;
  if (power_view(who, task, "the", spec, nullptr, n, y0, nyl, pitch, ns ? PF_POWER_MAXWG_RADII : PF_POWER_MAXWG_SHELLS, lds_scan > lds_acc ? lds_scan : lds_acc, &v, &nwg)) return 1;
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
  if (ns && power_upload(who, task, Edev, E, st)) return 1;
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

// what the two-spectrum passes share of their launches.  The deconvolution table of `flags` -> Cdev and *C (left as it is without
// PF_MATTER_DECONVOLVE)
static int matter_deconv_upload(const char *who, int task, int flags, int n, double *Cdev, const double **C, hipStream_t st) {
  if (!(flags & PF_MATTER_DECONVOLVE)) return 0;
  std::vector<double> tab(n / 2 + 1);
  for (int j = 0; j < n / 2 + 1; j++) tab[j] = pf_matter_deconv_entry(j, n, (flags & PF_MATTER_NGP) ? 1 : 2);
  if (power_upload(who, task, Cdev, tab, st)) return 1;
  *C = Cdev;
  return 0;
}
// smax[cnt], the maxima of this rank's scans -> those of the box: over the ranks through the slots [P][cnt], in which every rank
// fills its own alone.  Every all-reduce runs on the context's stream, which is st
static int matter_box_max(const char *who, int task, pf_ctx *coll, u64 *smax, size_t cnt, u64 *slots, hipStream_t st) {
  PfSpecView sv;
  pf_ctx_spec_geometry(coll, &sv);
  PWHIP(task, who, hipMemsetAsync(slots, 0, (size_t)sv.P * cnt * 8, st));
  PWHIP(task, who, hipMemcpyAsync(slots + (size_t)sv.rank * cnt, smax, cnt * 8, hipMemcpyDeviceToDevice, st));
  if (pf_ctx_allreduce(coll, slots, (size_t)sv.P * cnt, 1)) return 1;
  hipLaunchKernelGGL(k_matter_slot_max, dim3((unsigned int)((cnt + PF_POWER_BLOCK - 1) / PF_POWER_BLOCK)), dim3(PF_POWER_BLOCK), 0, st, slots, sv.P, (int)cnt, smax);
  if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  return 0;
}

// ---- the sums of two spectra (pf_internal.h; pf_matter.hip calls them).  Three positive sums per shell (0 |m|^2, 1 the positive
// cross terms, 2 the negative ones).  Words: smax [3 nb], nm [nb], k2 [nb], pl [12 nb]; then out [2 nb] doubles and the deconvolution
// table [n/2 + 1]; with P ranks the slots of the scans' maxima behind them, [P][3 nb]
size_t pf_matter_shells_words(int n, int P) {
  const size_t nb = (size_t)pf_power_nbins(n);
  return 19 * nb + (size_t)(n / 2 + 1) + (P > 1 ? (size_t)P * 3 * nb : 0);
}
int pf_matter_shells_device(const char *who, int task, int fb, const void *spec_m, const void *spec_lin, int n, int y0, int nyl, long long pitch, int flags, u64 *words,
                            u64 *counters, pf_ctx *coll, PfShellSums *sums, hipStream_t st) {
  const int nb = pf_power_nbins(n), nzh = n / 2 + 1;
  const size_t lds = (size_t)3 * nb * 8 + (size_t)nb * 4;
  MatterView v;
  unsigned int nwg;
  if (power_view(who, task, "a", spec_m, spec_lin, n, y0, nyl, pitch, PF_POWER_MAXWG_SHELLS, lds, &v, &nwg)) return 1;
  v.lin = spec_lin; v.C = nullptr; v.los = 0;
  PWHIP(task, who, hipMemsetAsync(words, 0, (size_t)19 * nb * 8, st));
  MatterTabs g;
  g.smax = words; g.nm = g.smax + 3 * (size_t)nb; g.k2 = g.nm + nb; g.pl = g.k2 + nb; g.out = (double *)(g.pl + 12 * (size_t)nb);
  if (matter_deconv_upload(who, task, flags, n, g.out + 2 * (size_t)nb, &v.C, st)) return 1;
  // with a second spectrum one scan takes the three maxima where its five tables fit (n up to about 1800); PF_MATTER_SCAN_EACH=1
  // (tests only) takes the way of the larger grids: a scan per sum
  const size_t lds_all = (size_t)5 * nb * 8;
  const char *each = getenv("PF_MATTER_SCAN_EACH");
  const bool fused = spec_lin && lds_all <= PF_POWER_LDS_MAX && !(each && atoi(each) != 0);
  const dim3 gr(nwg), bl(PF_POWER_BLOCK);
  if (fused) hipLaunchKernelGGL((fb == 8 ? k_matter_scan<double, true> : k_matter_scan<float, true>), gr, bl, lds_all, st, v, 0, nb, g, counters);
  // more than one rank: every scan first, then the maxima of the box (matter_box_max), so that every limb of every rank is formed
  // under the box's exponent
  for (int pass = coll ? 0 : 1; pass < 2; pass++) {
    for (int which = 0; which < (spec_lin ? 3 : 1); which++) {
      if (!fused && (!coll || pass == 0)) hipLaunchKernelGGL((fb == 8 ? k_matter_scan<double, false> : k_matter_scan<float, false>), gr, bl, lds, st, v, which, nb, g, counters);
      if (pass == 1) hipLaunchKernelGGL(fb == 8 ? k_matter_acc<double> : k_matter_acc<float>, gr, bl, lds, st, v, which, nb, g);
      if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
    }
    if (coll && pass == 0 && matter_box_max(who, task, coll, g.smax, (size_t)3 * nb, words + 19 * (size_t)nb + nzh, st)) return 1;
  }
  if (coll && pf_ctx_allreduce(coll, g.nm, (size_t)14 * nb, 1)) return 1;   // nm, k2 and the limbs pl lie one behind the other
  const double n3 = (double)n * (double)n * (double)n;
  hipLaunchKernelGGL(k_matter_final, dim3((unsigned int)((nb + PF_POWER_BLOCK - 1) / PF_POWER_BLOCK)), bl, 0, st, nb, n3 * n3, g);
  if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  sums->nm = g.nm; sums->out = g.out; sums->scans = fused ? 1 : spec_lin ? 3 : 1;
  return 0;
}

// ---- the multipoles of two spectra (pf_internal.h; pf_halo.hip calls them).  Eleven positive sums per shell (pf_multipole_core.h),
// five without a second spectrum.  Words: smax [11 nb], nm [nb], k2 [nb], pl [44 nb]; then out [17 nb] doubles (3 nb power, 3 nb cross,
// 11 nb the positive sums) and the deconvolution table [n/2 + 1]; with P ranks the slots of the scans' maxima behind them, [P][11 nb].
// A launch carries as many sums as PF_MULTIPOLE_LDS_SCAN / _ACC bytes of LDS hold (a scan: a table of 8 bytes per shell and sum and two more; an
// accumulation: 28 bytes per shell and sum), the sums spread evenly over the launches; every grid up to 2048 has room for one.  The
// sums are integers under the exponents of the scans' maxima: how they are grouped changes no bit.  PF_MULTIPOLE_SCAN_EACH=1 (tests
// only): one sum per launch
#ifndef PF_MULTIPOLE_LDS_SCAN
#define PF_MULTIPOLE_LDS_SCAN PF_POWER_LDS_MAX
#endif
#ifndef PF_MULTIPOLE_LDS_ACC
#define PF_MULTIPOLE_LDS_ACC PF_POWER_LDS_MAX
#endif
static_assert(PF_MULTIPOLE_NSUMS == PF_MULTIPOLE_SUMS, "pf_multipole_core.h and pinfmax.h disagree");
static thread_local int multipole_last_form[2] = {0, 0};   // scans and accumulations launched by the last call
extern "C" int pf_debug_multipole_form(int *form) {
  if (!form) return 1;
  form[0] = multipole_last_form[0]; form[1] = multipole_last_form[1];
  return 0;
}
// `total` sums in launches of at most `room` (at least one) each, spread evenly.  The two sums of a signed term, 2k - 1 and 2k, should
// ride together -- a mode adds to one of them, so the second costs a launch nothing --: the launches cut the indices -1 .. total - 1
// into runs of *per, so that an even *per splits no pair; the run [-1, 0) of *per = 1 is empty and is not launched
static void multipole_groups(int total, size_t room, int *per) {
  const int slots = total + 1, g = room < 1 ? 1 : room > (size_t)slots ? slots : (int)room, launches = (slots + g - 1) / g;
  *per = (slots + launches - 1) / launches;
}
size_t pf_multipole_shells_words(int n, int P) {
  const size_t nb = (size_t)pf_power_nbins(n);
  return 74 * nb + (size_t)(n / 2 + 1) + (P > 1 ? (size_t)P * PF_MULTIPOLE_NSUMS * nb : 0);
}
int pf_multipole_shells_device(const char *who, int task, int fb, const void *spec_m, const void *spec_lin, int n, int y0, int nyl, long long pitch, int flags, int los, u64 *words,
                               u64 *counters, pf_ctx *coll, PfShellSums *sums, hipStream_t st) {
  const int nb = pf_power_nbins(n), nzh = n / 2 + 1, total = spec_lin ? PF_MULTIPOLE_NSUMS : PF_MULTIPOLE_NSUMS_AUTO;
  const char *each = getenv("PF_MULTIPOLE_SCAN_EACH");
  const bool one = each && atoi(each) != 0;
  const size_t table = (size_t)nb * 8, acc1 = (size_t)nb * 28;
  int per_scan, per_acc;
  multipole_groups(total, one ? 1 : PF_MULTIPOLE_LDS_SCAN / table < 3 ? 1 : PF_MULTIPOLE_LDS_SCAN / table - 2, &per_scan);
  multipole_groups(total, one ? 1 : PF_MULTIPOLE_LDS_ACC / acc1, &per_acc);
  const size_t lds_scan = (size_t)((per_scan < total ? per_scan : total) + 2) * table, lds_acc = (size_t)(per_acc < total ? per_acc : total) * acc1;
  MatterView v;
  unsigned int nwg;
  if (power_view(who, task, "a", spec_m, spec_lin, n, y0, nyl, pitch, PF_POWER_MAXWG_SHELLS, lds_scan > lds_acc ? lds_scan : lds_acc, &v, &nwg)) return 1;
  if (los < 0 || los > 2) return pf_fail(task, "%s: a line of sight along axis %d (0, 1 or 2)", who, los);
  v.lin = spec_lin; v.C = nullptr; v.los = los;
  PWHIP(task, who, hipMemsetAsync(words, 0, (size_t)74 * nb * 8, st));
  MatterTabs g;
  g.smax = words; g.nm = g.smax + PF_MULTIPOLE_NSUMS * (size_t)nb; g.k2 = g.nm + nb; g.pl = g.k2 + nb; g.out = (double *)(g.pl + 4 * PF_MULTIPOLE_NSUMS * (size_t)nb);
  if (matter_deconv_upload(who, task, flags, n, g.out + 17 * (size_t)nb, &v.C, st)) return 1;
  const dim3 gr(nwg), bl(PF_POWER_BLOCK);
  int scans = 0, accs = 0;
  for (int v0 = -1; v0 < total; v0 += per_scan) {
    const int first = v0 < 0 ? 0 : v0, ns = (v0 + per_scan < total ? v0 + per_scan : total) - first;
    if (ns <= 0) continue;
    scans++;
    hipLaunchKernelGGL(fb == 8 ? k_multipole_scan<double> : k_multipole_scan<float>, gr, bl, lds_scan, st, v, first, ns, nb, g, counters);
    if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  }
  // more than one rank: the maxima of the box before any limb is formed, as in pf_matter_shells_device
  if (coll && matter_box_max(who, task, coll, g.smax, (size_t)PF_MULTIPOLE_NSUMS * nb, words + 74 * (size_t)nb + nzh, st)) return 1;
  for (int v0 = -1; v0 < total; v0 += per_acc) {
    const int first = v0 < 0 ? 0 : v0, ns = (v0 + per_acc < total ? v0 + per_acc : total) - first;
    if (ns <= 0) continue;
    accs++;
    hipLaunchKernelGGL(fb == 8 ? k_multipole_acc<double> : k_multipole_acc<float>, gr, bl, lds_acc, st, v, first, ns, nb, g);
    if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  }
  if (coll && pf_ctx_allreduce(coll, g.nm, (size_t)(2 + 4 * PF_MULTIPOLE_NSUMS) * nb, 1)) return 1;   // nm, k2 and the limbs pl lie one behind the other
  const double n3 = (double)n * (double)n * (double)n;
  hipLaunchKernelGGL(k_multipole_final, dim3((unsigned int)((nb + PF_POWER_BLOCK - 1) / PF_POWER_BLOCK)), bl, 0, st, nb, n3 * n3, g);
  if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  sums->nm = g.nm; sums->out = g.out; sums->scans = scans;
  multipole_last_form[0] = scans; multipole_last_form[1] = accs;
  return 0;
}

extern "C" int pf_debug_multipole_shells(int field_bytes, int n, int y0, int nyl, const double *spec_m, const double *spec_lin, int flags, int los, unsigned long long *nmodes,
                                         unsigned long long *k2sum, double *power, double *cross, double *parts, pf_matter_info *info) {
  const char *who = "pf_debug_multipole_shells";
  if (!spec_m || !nmodes || !k2sum || !power || !info) return pf_fail(0, "%s: null argument", who);
  if (flags & ~(PF_MATTER_NGP | PF_MATTER_DECONVOLVE)) return pf_fail(0, "%s: unknown flag bits 0x%x", who, (unsigned int)(flags & ~(PF_MATTER_NGP | PF_MATTER_DECONVOLVE)));
  if (los < 0 || los > 2) return pf_fail(0, "%s: a line of sight along axis %d (0, 1 or 2)", who, los);
  if (cross && !spec_lin) return pf_fail(0, "%s: cross sums without a second spectrum", who);
  const bool two = spec_lin && cross;
  const size_t slot_words = (size_t)PF_MATTER_SLOTS * MC_COUNT;
  PfSpecStage d = {};
  if (pf_stage_spectra(who, field_bytes, n, y0, nyl, 2, spec_m, two ? spec_lin : nullptr, slot_words + pf_multipole_shells_words(n, 1), &d)) return 1;
  PWHIP(0, who, hipMemsetAsync(d.words, 0, slot_words * 8, nullptr));
  PfShellSums g;
  if (pf_multipole_shells_device(who, 0, field_bytes, d.spec[0], two ? d.spec[1] : nullptr, n, y0, nyl, d.nzp, flags, los, d.words + slot_words, d.words, nullptr, &g, nullptr)) return 1;
  const size_t nb = (size_t)pf_power_nbins(n);
  std::vector<u64> hu(2 * nb), slots(slot_words);
  std::vector<double> hd(17 * nb);
  PWHIP(0, who, hipMemcpyAsync(hu.data(), g.nm, hu.size() * 8, hipMemcpyDeviceToHost, nullptr));
  PWHIP(0, who, hipMemcpyAsync(hd.data(), g.out, hd.size() * 8, hipMemcpyDeviceToHost, nullptr));
  PWHIP(0, who, hipMemcpyAsync(slots.data(), d.words, slot_words * 8, hipMemcpyDeviceToHost, nullptr));
  PWHIP(0, who, hipStreamSynchronize(nullptr));
  memcpy(nmodes, hu.data(), nb * 8);
  memcpy(k2sum, hu.data() + nb, nb * 8);
  memcpy(power, hd.data(), 3 * nb * 8);
  if (cross) memcpy(cross, hd.data() + 3 * nb, 3 * nb * 8);
  if (parts) memcpy(parts, hd.data() + 6 * nb, PF_MULTIPOLE_NSUMS * nb * 8);
  memset(info, 0, sizeof(*info));
  info->modes = (u64)nyl * n * n;
  for (int k = 0; k < PF_MATTER_SLOTS; k++) info->nonfinite_modes += slots[(size_t)k * MC_COUNT + MC_NONFIN_MODES];
  return 0;
}

// ---- the passes of pf_halo_correlation (pf_internal.h; pf_halo.hip calls them) ----
static_assert(PF_CORR_NORDERS == PF_CORR_ORDERS && 2 * PF_CORR_NSUMS == PF_CORR_SUMS, "pf_corr_core.h and pinfmax.h disagree");
int pf_corr_deconv_upload(const char *who, int task, int flags, int n, double *Cdev, const double **C, hipStream_t st) {
  return matter_deconv_upload(who, task, flags, n, Cdev, C, st);
}
int pf_corr_form_device(const char *who, int task, int fb, const void *spec_m, const void *spec_lin, void *out, int n, int y0, int nyl, long long pitch, const double *C,
                        int which, u64 *counters, hipStream_t st) {
  MatterView v;
  unsigned int nwg;
  if (which < 0 || which > 1) return pf_fail(task, "%s: form %d (0 auto, 1 cross)", who, which);
  if (which && !spec_lin) return pf_fail(task, "%s: the cross form without a second spectrum", who);
  if (power_view(who, task, "a", spec_m, which ? spec_lin : nullptr, n, y0, nyl, pitch, PF_POWER_MAXWG_SHELLS, 0, &v, &nwg)) return 1;
  if ((uintptr_t)out & 15) return pf_fail(task, "%s: the formed spectrum is not 16-byte aligned (internal error)", who);
  v.lin = which ? spec_lin : nullptr; v.C = C; v.los = 0;
  const double n3 = (double)n * (double)n * (double)n;
  hipLaunchKernelGGL(fb == 8 ? k_corr_form<double> : k_corr_form<float>, dim3(nwg), dim3(PF_POWER_BLOCK), 0, st, v, out, which, n3, counters);
  if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  return 0;
}

// Six positive sums per shell.  Words: smax [6 nb], nm [nb], k2 [nb], pl [24 nb], nonfin [1]; then out [9 nb] doubles (3 nb xi, 6 nb
// the positive sums); with P ranks the slots of the scans' maxima behind them, [P][6 nb].  A launch carries as many sums as
// PF_CORR_LDS_SCAN / _ACC bytes of LDS hold, as the multipole passes do, in runs of an even length where there is room for two, so
// that the two sums of a term's signs ride together.  PF_CORR_SCAN_EACH=1 (tests only): one sum per launch.  What was launched is kept
// for pf_debug_corr_passes
#ifndef PF_CORR_LDS_SCAN
#define PF_CORR_LDS_SCAN PF_POWER_LDS_MAX
#endif
#ifndef PF_CORR_LDS_ACC
#define PF_CORR_LDS_ACC PF_POWER_LDS_MAX
#endif
static thread_local int corr_last_passes[2] = {0, 0};   // scans and accumulations launched by the last call
extern "C" int pf_debug_corr_passes(int *passes) {
  if (!passes) return 1;
  passes[0] = corr_last_passes[0]; passes[1] = corr_last_passes[1];
  return 0;
}
static int corr_group(size_t room) {
  int g = room < 1 ? 1 : room > (size_t)PF_CORR_NSUMS ? PF_CORR_NSUMS : (int)room;
  if (g > 1) g &= ~1;
  const int launches = (PF_CORR_NSUMS + g - 1) / g;
  int per = (PF_CORR_NSUMS + launches - 1) / launches;
  if (per > 1 && (per & 1)) per++;   // (still at most g, which is even)
  return per;
}
size_t pf_corr_shells_words(int n, int P) {
  const size_t nb = (size_t)pf_power_nbins(n);
  return 41 * nb + 1 + (P > 1 ? (size_t)P * PF_CORR_NSUMS * nb : 0);
}
int pf_corr_shells_device(const char *who, int task, int fb, const void *real, int n, int x0, int nxl, long long pitch, int los, u64 *words, pf_ctx *coll, PfShellSums *sums,
                          hipStream_t st) {
  const int nb = pf_power_nbins(n);
  const char *each = getenv("PF_CORR_SCAN_EACH");
  const bool one = each && atoi(each) != 0;
  const size_t table = (size_t)nb * 8, acc1 = (size_t)nb * 28;
  const int per_scan = corr_group(one ? 1 : PF_CORR_LDS_SCAN / table < 3 ? 1 : PF_CORR_LDS_SCAN / table - 2), per_acc = corr_group(one ? 1 : PF_CORR_LDS_ACC / acc1);
  const size_t lds_scan = (size_t)(per_scan + 2) * table, lds_acc = (size_t)per_acc * acc1;
  if (lds_scan > PF_POWER_LDS_MAX || lds_acc > PF_POWER_LDS_MAX) return pf_fail(task, "%s: the %d shells of a grid of %d do not fit the LDS tables", who, nb, n);
  if (los < 0 || los > 2) return pf_fail(task, "%s: a line of sight along axis %d (0, 1 or 2)", who, los);
  if (n < 2 || n > 2048 || x0 < 0 || nxl < 1 || x0 + nxl > n || pitch < n) return pf_fail(task, "%s: planes %d .. %d of a grid of %d in rows of %lld (internal error)", who, x0, x0 + nxl - 1, n, pitch);
  CorrView v;
  v.real = real; v.n = n; v.nxl = nxl; v.x0 = x0; v.los = los; v.pitch = pitch;
  v.rows = (unsigned int)nxl * (unsigned int)n;
  v.rows_per_wg = (v.rows + PF_POWER_MAXWG_SHELLS - 1) / PF_POWER_MAXWG_SHELLS;
  const unsigned int nwg = (v.rows + v.rows_per_wg - 1) / v.rows_per_wg;
  PWHIP(task, who, hipMemsetAsync(words, 0, (41 * (size_t)nb + 1) * 8, st));
  CorrTabs g;
  g.smax = words; g.nm = g.smax + PF_CORR_NSUMS * (size_t)nb; g.k2 = g.nm + nb; g.pl = g.k2 + nb; g.nonfin = g.pl + 4 * PF_CORR_NSUMS * (size_t)nb;
  g.out = (double *)(g.nonfin + 1);
  const dim3 gr(nwg), bl(PF_POWER_BLOCK);
  int scans = 0, accs = 0;
  for (int first = 0; first < PF_CORR_NSUMS; first += per_scan, scans++) {
    const int ns = first + per_scan < PF_CORR_NSUMS ? per_scan : PF_CORR_NSUMS - first;
    hipLaunchKernelGGL(fb == 8 ? k_corr_scan<double> : k_corr_scan<float>, gr, bl, lds_scan, st, v, first, ns, nb, g);
    if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  }
  // more than one rank: the maxima of the box before any limb is formed, as in pf_matter_shells_device
  if (coll && matter_box_max(who, task, coll, g.smax, (size_t)PF_CORR_NSUMS * nb, words + 41 * (size_t)nb + 1, st)) return 1;
  for (int first = 0; first < PF_CORR_NSUMS; first += per_acc, accs++) {
    const int ns = first + per_acc < PF_CORR_NSUMS ? per_acc : PF_CORR_NSUMS - first;
    hipLaunchKernelGGL(fb == 8 ? k_corr_acc<double> : k_corr_acc<float>, gr, bl, lds_acc, st, v, first, ns, nb, g);
    if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  }
  if (coll && pf_ctx_allreduce(coll, g.nm, (size_t)(2 + 4 * PF_CORR_NSUMS) * nb + 1, 1)) return 1;   // nm, k2, the limbs pl and nonfin lie one behind the other
  hipLaunchKernelGGL(k_corr_final, dim3((unsigned int)((nb + PF_POWER_BLOCK - 1) / PF_POWER_BLOCK)), bl, 0, st, nb, g);
  if (hipGetLastError() != hipSuccess) return pf_fail(task, "%s: launch failed", who);
  sums->nm = g.nm; sums->out = g.out; sums->scans = scans;
  corr_last_passes[0] = scans; corr_last_passes[1] = accs;
  return 0;
}

extern "C" int pf_debug_corr_form(int field_bytes, int n, int y0, int nyl, const double *spec_m, const double *spec_lin, int flags, int which, double *spec_out,
                                  pf_matter_info *info) {
  const char *who = "pf_debug_corr_form";
  if (!spec_m || !spec_out || !info) return pf_fail(0, "%s: null argument", who);
  if (flags & ~(PF_MATTER_NGP | PF_MATTER_DECONVOLVE)) return pf_fail(0, "%s: unknown flag bits 0x%x", who, (unsigned int)(flags & ~(PF_MATTER_NGP | PF_MATTER_DECONVOLVE)));
  if (which < 0 || which > 1) return pf_fail(0, "%s: form %d (0 auto, 1 cross)", who, which);
  if (which && !spec_lin) return pf_fail(0, "%s: the cross form without a second spectrum", who);
  const size_t slot_words = (size_t)PF_MATTER_SLOTS * MC_COUNT;
  PfSpecStage d = {};
  if (pf_stage_spectra(who, field_bytes, n, y0, nyl, 2, spec_m, which ? spec_lin : nullptr, slot_words + (size_t)(n / 2 + 1), &d)) return 1;
  PWHIP(0, who, hipMemsetAsync(d.words, 0, slot_words * 8, nullptr));
  const double *Ctab = nullptr;
  if (matter_deconv_upload(who, 0, flags, n, (double *)(d.words + slot_words), &Ctab, nullptr)) return 1;
  if (pf_corr_form_device(who, 0, field_bytes, d.spec[0], which ? d.spec[1] : nullptr, d.spec[0], n, y0, nyl, d.nzp, Ctab, which, d.words, nullptr)) return 1;
  const int nzh = n / 2 + 1;
  if (pf_launch_spec_export_t(field_bytes, d.spec[0], (double *)d.in, n, nyl, nzh, d.nzp, nullptr)) return pf_fail(0, "%s: launch failed", who);
  std::vector<u64> slots(slot_words);
  PWHIP(0, who, hipMemcpyAsync(spec_out, d.in, (size_t)nyl * n * nzh * 16, hipMemcpyDeviceToHost, nullptr));
  PWHIP(0, who, hipMemcpyAsync(slots.data(), d.words, slot_words * 8, hipMemcpyDeviceToHost, nullptr));
  PWHIP(0, who, hipStreamSynchronize(nullptr));
  memset(info, 0, sizeof(*info));
  info->modes = (u64)nyl * n * n;
  for (int k = 0; k < PF_MATTER_SLOTS; k++) info->nonfinite_modes += slots[(size_t)k * MC_COUNT + MC_NONFIN_MODES];
  return 0;
}

struct CorrStage { void *in, *field; u64 *words; ~CorrStage() { hipFree(in); hipFree(field); hipFree(words); } };
extern "C" int pf_debug_corr_shells(int field_bytes, int n, int x0, int nxl, const double *real_host, int los, unsigned long long *ncells, unsigned long long *r2sum, double *xi,
                                    double *parts, unsigned long long *nonfinite_cells) {
  const char *who = "pf_debug_corr_shells";
  if (!real_host || !ncells || !r2sum || !xi || !nonfinite_cells) return pf_fail(0, "%s: null argument", who);
  if (field_bytes != 4 && field_bytes != 8) return pf_fail(0, "%s: fields of %d bytes (4 or 8)", who, field_bytes);
  if (n < 2 || n > 2048 || (n & 1)) return pf_fail(0, "%s: a grid of %d (even, 2 to 2048)", who, n);
  if (x0 < 0 || nxl < 1 || x0 + nxl > n) return pf_fail(0, "%s: planes %d .. %d leave the grid of %d", who, x0, x0 + nxl - 1, n);
  if (los < 0 || los > 2) return pf_fail(0, "%s: a line of sight along axis %d (0, 1 or 2)", who, los);
  // the production layout of a real field: rows of 2 (n/2 + 64 / field_bytes) reals, NaN patterns in the padding that no sum may see
  const long long pitch = 2 * ((long long)n / 2 + 64 / field_bytes), nrows = (long long)nxl * n;
  const size_t in_bytes = (size_t)nrows * n * 8, field = (size_t)nrows * pitch * field_bytes, words = pf_corr_shells_words(n, 1);
  CorrStage d = {nullptr, nullptr, nullptr};
  if (hipMalloc(&d.in, in_bytes) != hipSuccess || hipMalloc(&d.field, field) != hipSuccess || hipMalloc((void **)&d.words, words * 8) != hipSuccess) {
    (void)hipGetLastError();
    return pf_fail(0, "%s: cannot allocate %zu bytes on the device", who, in_bytes + field + words * 8);
  }
  PWHIP(0, who, hipMemset(d.field, 0xff, field));
  PWHIP(0, who, hipMemcpy(d.in, real_host, in_bytes, hipMemcpyHostToDevice));
  if (pf_launch_real_import(field_bytes, (const double *)d.in, d.field, nrows, n, pitch, nullptr)) return pf_fail(0, "%s: launch failed", who);
  PfShellSums g;
  if (pf_corr_shells_device(who, 0, field_bytes, d.field, n, x0, nxl, pitch, los, d.words, nullptr, &g, nullptr)) return 1;
  const size_t nb = (size_t)pf_power_nbins(n);
  std::vector<u64> hu(26 * nb + 1);
  std::vector<double> hd(9 * nb);
  PWHIP(0, who, hipMemcpyAsync(hu.data(), g.nm, hu.size() * 8, hipMemcpyDeviceToHost, nullptr));
  PWHIP(0, who, hipMemcpyAsync(hd.data(), g.out, hd.size() * 8, hipMemcpyDeviceToHost, nullptr));
  PWHIP(0, who, hipStreamSynchronize(nullptr));
  memcpy(ncells, hu.data(), nb * 8);
  memcpy(r2sum, hu.data() + nb, nb * 8);
  memcpy(xi, hd.data(), 3 * nb * 8);
  if (parts) memcpy(parts, hd.data() + 3 * nb, PF_CORR_NSUMS * nb * 8);
  *nonfinite_cells = hu[26 * nb];
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

// what the taps on a caller's spectra begin with (pf_internal.h): the refusals of a layout, then the production layout on the device
// -- rows of whole 128-byte lines, and NaN patterns in the padding that no sum may see -- filled from a and, where given, b
int pf_stage_spectra(const char *who, int field_bytes, int n, int y0, int nyl, int fields, const double *a, const double *b, size_t words, PfSpecStage *d) {
  if (field_bytes != 4 && field_bytes != 8) return pf_fail(0, "%s: fields of %d bytes (4 or 8)", who, field_bytes);
  if (n < 2 || n > 2048 || (n & 1)) return pf_fail(0, "%s: a grid of %d (even, 2 to 2048)", who, n);
  if (y0 < 0 || nyl < 1 || y0 + nyl > n) return pf_fail(0, "%s: rows %d .. %d leave the grid of %d", who, y0, y0 + nyl - 1, n);
  const int nzh = n / 2 + 1;
  d->nzp = n / 2 + 64 / field_bytes;
  const long long nrows = (long long)nyl * n;
  const size_t in_bytes = (size_t)nrows * nzh * 16, field = (size_t)nrows * d->nzp * 2 * field_bytes;
  if (hipMalloc(&d->in, in_bytes) != hipSuccess || hipMalloc(&d->spec[0], fields * field) != hipSuccess || (words && hipMalloc((void **)&d->words, words * 8) != hipSuccess)) {
    (void)hipGetLastError();
    return pf_fail(0, "%s: cannot allocate %zu bytes on the device", who, in_bytes + fields * field + words * 8);
  }
  d->spec[1] = (char *)d->spec[0] + field;
  PWHIP(0, who, hipMemset(d->spec[0], 0xff, fields * field));
  const double *host[2] = {a, b};
  for (int k = 0; k < 2 && host[k]; k++) {
    if (k) PWHIP(0, who, hipDeviceSynchronize());   // (the first import has read `in`)
    PWHIP(0, who, hipMemcpy(d->in, host[k], in_bytes, hipMemcpyHostToDevice));
    // [ky_local][kx][kz] of the caller -> [kx][ky_local][kz] rows of nzp
    if (pf_launch_spec_import_t(field_bytes, (const double *)d->in, d->spec[k], n, nyl, nzh, d->nzp, nullptr)) return pf_fail(0, "%s: launch failed", who);
  }
  return 0;
}

extern "C" int pf_debug_power_spectrum(int field_bytes, int n, int y0, int nyl, const double *spec_host, int ns, const double *radius_cells, unsigned long long *nmodes,
                                       unsigned long long *k2sum, double *power, double *variance, pf_power_info *info) {
  const char *who = "pf_debug_power_spectrum";
  if (!spec_host) return pf_fail(0, "%s: null argument", who);
  if (power_check_args(who, 0, ns, radius_cells, nmodes, k2sum, power, variance, info)) return 1;
  PfSpecStage d = {};
  if (pf_stage_spectra(who, field_bytes, n, y0, nyl, 1, spec_host, nullptr, 0, &d)) return 1;
  PowerScratch s = {nullptr};
  PowerGuard guard{&s};
  PowerTabs g;
  PowerTimer timer(power_times_on(), nullptr);
  if (power_device(who, 0, field_bytes, d.spec[0], n, y0, nyl, d.nzp, ns, radius_cells, &s, &g, nullptr)) return 1;
  timer.end();
  return power_fetch(who, 0, n, ns, g, (u64)nyl * n * n, nmodes, k2sum, power, variance, info, nullptr);
}
