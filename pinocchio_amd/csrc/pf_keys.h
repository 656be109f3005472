// pf_keys.h -- the 64-bit sort key of the fragmentation hand-off (pf_select_sort.hip, pf_peaks.hip):
// (descending-orderable Fmax bits) << 32 | cell index, so that an ascending radix sort gives index_compare_F order
// (src/fragment.c:118-126) with ties by ascending cell index
//
// sort_and_organize on the device (pf_organize.hip) sorts (key, input index) PAIRS with a stable sort instead, so its keys carry no
// index; they come in a float and a double form and place -0.0 and NaN: pf_org_key32 / pf_org_key64 of pf_organize_core.h
#pragma once
#include <hip/hip_runtime.h>

#include "pf_organize_core.h"

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
