// pf_keys.h -- the 64-bit sort key of the fragmentation hand-off (pf_select_sort.hip, pf_peaks.hip):
// (descending-orderable Fmax bits) << 32 | cell index, so that an ascending radix sort gives index_compare_F order
// (src/fragment.c:118-126) with ties by ascending cell index
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned int pf_desc_key(float f) {
  unsigned int u = __float_as_uint(f);
  u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;  // ascending-orderable
  return ~u;                                   // descending
}
__device__ __forceinline__ float pf_key_to_float(unsigned int k) {
  unsigned int u = ~k;
  u ^= (u >> 31) ? 0x80000000u : 0xFFFFFFFFu;
  return __uint_as_float(u);
}
