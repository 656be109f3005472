// the sort keys of sort_and_organize on the device (pinocchio_amd/csrc/pf_organize_core.h) compiled for the host: the keys of arrays
// of fp32 / fp64 bit patterns, for tests/test_organize_cpu.py
#include <stddef.h>

#include "../../pinocchio_amd/csrc/pf_organize_core.h"

extern "C" void emul_keys32(size_t count, const unsigned int *bits, unsigned int *keys) {
  for (size_t i = 0; i < count; i++) keys[i] = pf_org_key32(bits[i]);
}
extern "C" void emul_keys64(size_t count, const unsigned long long *bits, unsigned long long *keys) {
  for (size_t i = 0; i < count; i++) keys[i] = pf_org_key64(bits[i]);
}
