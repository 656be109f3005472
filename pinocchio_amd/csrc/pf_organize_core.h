// pf_organize_core.h -- the sort keys of sort_and_organize() (src/fragment.c:484-520) on the device (pf_organize.hip): a key of the
// BITS of Fmax whose ascending unsigned order is index_compare_F order (:118-126, descending Fmax).  32 bits for float products, 64
// for PRODFLOAT double.  A stable sort of (key, input index) pairs then leaves equal Fmax in input order -- the tie rule of
// pf_keys.h -- with no index bits in the key.  Two rules make "equal" mean equal as floating-point values and give every input a
// place:
//   -0.0 is keyed as +0.0 (they compare equal, so they tie);
//   NaN of either sign and any payload gets the largest key: after -inf, all NaN tied (pf_distribute never stores one; a caller
//   of pf_organize may hold some).
// Integer arithmetic on the bit patterns only, no device dependence: a CPU test compiles this header on its own
// (tests/cpu_emul/organize_emul.cpp).
#pragma once

#if defined(__HIPCC__)
#define PF_ORG_HD __host__ __device__ __forceinline__
#else
#define PF_ORG_HD static inline
#endif

PF_ORG_HD unsigned int pf_org_key32(unsigned int u) {
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;   // NaN (no number maps here: that would take u = 0xFFFFFFFF, a NaN)
  if (!(u << 1)) u = 0u;                                      // -0.0
  u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;                 // ascending-orderable
  return ~u;                                                  // descending
}

PF_ORG_HD unsigned long long pf_org_key64(unsigned long long u) {
  if ((u & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return 0xFFFFFFFFFFFFFFFFull;
  if (!(u << 1)) u = 0ull;
  u ^= (u >> 63) ? 0xFFFFFFFFFFFFFFFFull : 0x8000000000000000ull;
  return ~u;
}
