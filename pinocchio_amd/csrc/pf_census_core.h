// pf_census_core.h -- the per-cell classification of the flavour census (include/pinfmax.h: pf_flavour_census): how far the Fmax
// of the fast flavour of the collapse solve lies from the Fmax of the exact one, in units of the last place of the product
// precision, and into which bin of the census that distance falls.  Plain C++ for host and device: the kernels of pf_census.hip
// call it, and a CPU test compiles it on its own (tests/cpu_emul/census_emul.cpp) against the numpy restatement
// (tests/np_census.py).  T is PRODFLOAT.  A pure function of the two values, the two Rmax and the precision.
//
//   d   = |fast - exact|, formed in double (exact for float products; one rounding, and +inf where it overflows, for double ones)
//   ulp = the spacing of max(|exact|, 1) in T: 2^(E - mantissa bits), E its unbiased exponent, read from the exponent field
//   u   = d / ulp, formed as ldexp(d, -(E - mantissa bits)): exact, subnormal results included (|exact| < 1 with double products)
//   bin   0: u == 0;  1: 0 < u <= 1;  k >= 2: 2^(k-2) < u <= 2^(k-1);  the last one (PF_CENSUS_NBIN - 1) is open at the top --
//         from u's own exponent and mantissa fields: u = 2^e (1 + m) lies in bin e + 1 when m == 0 and in bin e + 2 otherwise
// Identical bit patterns are bin 0 with d = u = 0 whatever the value (NaN against the same NaN included).  Different bit patterns
// with a NaN or an infinity on either side are `nonfinite`: bin -1, outside the histogram and the maxima.  +0 against -0: different
// bits, d = 0, bin 0.  No logarithm, no division, no comparison of floating-point values beyond d > 0.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PF_CENSUS_HD __host__ __device__ __forceinline__
#else
#define PF_CENSUS_HD static inline
#endif

#define PF_CENSUS_NBIN 64   // PF_CENSUS_BINS of the interface

template <class T> struct PfCensusFmt;
template <> struct PfCensusFmt<float> { typedef uint32_t U; enum { MANT = 23, BIAS = 127, EMAX = 255 }; };
template <> struct PfCensusFmt<double> { typedef uint64_t U; enum { MANT = 52, BIAS = 1023, EMAX = 2047 }; };

struct PfCensusCell {
  int bin;          // 0 .. PF_CENSUS_NBIN - 1, or -1: nonfinite
  bool differ;      // the Fmax bit patterns differ
  bool rdiffer;     // the Rmax differ
  bool outlier;     // bin >= 3 (d > 2 ulp) or nonfinite: the cell has a record
  double d, u;      // 0 for a nonfinite cell
};

template <class T> PF_CENSUS_HD typename PfCensusFmt<T>::U pf_census_bits(T v) {
  typename PfCensusFmt<T>::U b;
  __builtin_memcpy(&b, &v, sizeof(b));
  return b;
}

// the bin of u >= 0 (+inf: the last bin)
PF_CENSUS_HD int pf_census_bin(double u) {
  if (!(u > 0.0)) return 0;
  const uint64_t b = pf_census_bits<double>(u);
  const int e = (int)(b >> 52) - 1023;
  const bool pow2 = (b & 0xFFFFFFFFFFFFFull) == 0;
  if (e < 0 || (e == 0 && pow2)) return 1;   // u <= 1 (subnormal u: the exponent field is 0, e = -1023)
  const int k = pow2 ? e + 1 : e + 2;
  return k < PF_CENSUS_NBIN - 1 ? k : PF_CENSUS_NBIN - 1;
}

template <class T> PF_CENSUS_HD PfCensusCell pf_census_classify(T fast, T exact, int rmax_fast, int rmax_exact) {
  typedef PfCensusFmt<T> F;
  typedef typename F::U U;
  PfCensusCell c;
  c.rdiffer = rmax_fast != rmax_exact;
  c.d = 0.0; c.u = 0.0; c.bin = 0; c.outlier = false;
  const U bf = pf_census_bits<T>(fast), be = pf_census_bits<T>(exact);
  c.differ = bf != be;
  if (!c.differ) return c;
  const U absmask = ~(U)0 >> 1;
  const int ef = (int)((bf & absmask) >> F::MANT), ee = (int)((be & absmask) >> F::MANT);
  if (ef == F::EMAX || ee == F::EMAX) { c.bin = -1; c.outlier = true; return c; }
  c.d = fabs((double)fast - (double)exact);
  const int e1 = ee < F::BIAS ? (int)F::BIAS : ee;   // the exponent field of max(|exact|, 1)
  c.u = ldexp(c.d, -(e1 - (int)F::BIAS - (int)F::MANT));
  c.bin = pf_census_bin(c.u);
  c.outlier = c.bin >= 3;
  return c;
}
