// pf_power_core.h -- one mode of the power-spectrum pass (include/pinfmax.h: pf_power_spectrum): its signed wavenumber, k2, shell,
// weight and term, and the fixed-point form in which the terms are added.  Plain C++ for host and device: the kernels of
// pf_power.hip call it, and a CPU test compiles it on its own (tests/cpu_emul/power_emul.cpp) against the numpy restatement
// (tests/np_power.py).
//
//   signed wavenumber  i > n/2 -> i - n, n/2 stays positive (compute_derivative, src/fmax-pfft.c:312-334)
//   k2                 ix^2 + iy^2 + iz^2 of the signed wavenumbers: an integer, at most 3 (n/2)^2
//   shell b            (2b - 1)^2 <= 4 k2 < (2b + 1)^2: the nearest integer to |k|, found by an integer square root of k2 and one
//                      comparison -- r = isqrt(k2), then b = r + (k2 > r^2 + r), since (2r + 1)^2 <= 4 k2 <=> k2 >= r^2 + r + 1/4
//   weight             2 for 0 < iz < n/2, 1 on the planes iz = 0 and iz = n/2
//   term               re^2 + im^2 in double: two products and one sum, each rounded once (the file that includes this is compiled
//                      without contraction)
//   window             exp(-a k2), a = (2 pi / n)^2 R^2, as the product of three entries of ONE table per radius, E[j] = exp(-(a j^2)) for
//                      j = 0 .. n/2 at |ix|, |iy| and iz: the term is wt ((E[|ix|] E[|iy|]) E[iz]), five roundings more than the plain form
//   fixed point        a term t <= M, 2^(e-1) <= M < 2^e, is added as the integer floor(w t 2^(95 - e)) < 2^96 in three 32-bit limbs,
//                      each limb into a 64-bit counter: integer sums, so any order gives the same bits.  What is dropped lies below
//                      2^-95 of the scale per term.  pf_power_from_limbs carries the counters into each other and rounds three times.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PF_POWER_HD __host__ __device__ __forceinline__
#else
#define PF_POWER_HD static inline
#endif

PF_POWER_HD int pf_power_signed(int i, int n) { return i > n / 2 ? i - n : i; }

PF_POWER_HD unsigned long long pf_power_k2(int ix, int iy, int iz, int n) {
  const long long sx = pf_power_signed(ix, n), sy = pf_power_signed(iy, n), sz = pf_power_signed(iz, n);
  return (unsigned long long)(sx * sx + sy * sy + sz * sz);
}

// k2 < 2^24 (n <= 2048: k2 <= 3 * 1024^2 < 2^22), so r < 2^12 and every product below fits 32 bits
PF_POWER_HD unsigned int pf_power_isqrt(unsigned int x) {
  unsigned int r = 0;
  for (unsigned int bit = 1u << 11; bit; bit >>= 1) {   // integer square root, bit by bit: r^2 <= x < (r + 1)^2
    const unsigned int t = r | bit;
    if (t * t <= x) r = t;
  }
  return r;
}
// the same root from a guess (the root of a neighbouring mode): steps of one, usually none or one
PF_POWER_HD unsigned int pf_power_isqrt_near(unsigned int x, unsigned int r) {
  while (r * r > x) r--;
  while ((r + 1) * (r + 1) <= x) r++;
  return r;
}
PF_POWER_HD int pf_power_shell_of_root(unsigned int k2, unsigned int r) { return (int)(r + (k2 > r * r + r ? 1u : 0u)); }
PF_POWER_HD int pf_power_shell(unsigned long long k2) { return pf_power_shell_of_root((unsigned int)k2, pf_power_isqrt((unsigned int)k2)); }

PF_POWER_HD int pf_power_weight(int iz, int n) { return (iz > 0 && iz < n / 2) ? 2 : 1; }

// number of shells of a grid of n points per side: 1 + the largest b with (2b - 1)^2 <= 3 n^2
PF_POWER_HD int pf_power_nbins(int n) {
  const unsigned long long lim = 3ull * (unsigned long long)n * (unsigned long long)n;
  unsigned long long b = 0;
  while ((2 * (b + 1) - 1) * (2 * (b + 1) - 1) <= lim) b++;
  return (int)(b + 1);
}

template <class F> PF_POWER_HD double pf_power_term(F re, F im) {
  const double a = (double)re, b = (double)im;
  const double aa = a * a, bb = b * b;
  return aa + bb;
}

PF_POWER_HD bool pf_power_finite(double t) { return t - t == 0.0; }   // false for NaN and infinities

// the exponent e of a scale M > 0: 2^(e-1) <= M < 2^e (subnormal M included)
PF_POWER_HD int pf_power_exponent(double m) { return ilogb(m) + 1; }

// wt = w t with 0 <= t < 2^e: the three limbs of floor(wt 2^(95 - e)), least significant first
PF_POWER_HD void pf_power_limbs(double wt, int e, uint32_t l[3]) {
  const double f = ldexp(wt, 95 - e);                   // < 2^96, exact: a power of two times wt, no underflow below 2^-1074 matters
  const double hi = floor(ldexp(f, -32));               // < 2^64
  const unsigned long long h = (unsigned long long)hi;
  const double lo = f - ldexp(hi, 32);                  // exact, in [0, 2^32)
  l[0] = (uint32_t)lo; l[1] = (uint32_t)(h & 0xffffffffull); l[2] = (uint32_t)(h >> 32);
}

PF_POWER_HD double pf_power_window_entry(double a, int j) { return exp(-(a * (double)(j * j))); }   // (host: the tables are built there)
PF_POWER_HD double pf_power_windowed(double wt, double ex, double ey, double ez) { return wt * ((ex * ey) * ez); }

// counters c[0..nl-1] (limb sums, weights 2^0, 2^32, ...; each below 2^63) of scale exponent e -> the sum as a double
PF_POWER_HD double pf_power_from_limbs(const unsigned long long *c, int nl, int e) {
  unsigned long long carry = 0;
  double v[5];
  for (int i = 0; i < nl; i++) {
    const unsigned long long s = c[i] + carry;
    if (i + 1 < nl) { v[i] = (double)(s & 0xffffffffull); carry = s >> 32; }
    else v[i] = (double)s;
  }
  double d = v[nl - 1];
  for (int i = nl - 2; i >= 0; i--) d = d * 4294967296.0 + v[i];
  return ldexp(d, e - 95);
}
