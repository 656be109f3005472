// Host-side unit-test driver for the two per-cell functions of pinocchio_amd/csrc/pf_collapse_core.h that the contracting z-pass
// (k_c2r_invariants / k_mixed_c2r_invariants, MODE 1 and 2) calls: pf_lpt3b_accumulate and the src32 of pf_lpt_sources_cell, with
// the kernels' conversions from and to the field type around them.  TEST ONLY -- not a CPU path of the library.
// Built as a shared object (-DZF_EMUL_LIB) for tests/test_zpass_forms_cpu.py, and as a program of its own under the sanitizers:
//   zpass_forms_emul_san IN OUT   IN: int64 fb, int64 count, then s0[count], d[6][count], h[6][count] doubles
//                                 OUT: acc[count], start[count] doubles
#include "../../pinocchio_amd/csrc/pf_collapse_core.h"
#include <cstdio>
#include <vector>

static double to_field(double v, int fb) { return fb == 4 ? (double)(float)v : v; }

// s0, d[c], h[c] hold values of the field type (fp32 fields: floats widened), as the kernel loads them
extern "C" int zf_emul_acc(int fb, long count, const double *s0, const double *d, const double *h, double *out) {
  if ((fb != 4 && fb != 8) || count < 0) return 1;
  for (long i = 0; i < count; i++) {
    double dd[6], hh[6];
    for (int c = 0; c < 6; c++) { dd[c] = d[c * count + i]; hh[c] = h[c * count + i]; }
    out[i] = to_field(pf_lpt3b_accumulate(s0[i], dd, hh), fb);
  }
  return 0;
}
extern "C" int zf_emul_start(int fb, long count, const double *h, double *out) {
  if ((fb != 4 && fb != 8) || count < 0) return 1;
  for (long i = 0; i < count; i++) {
    double hh[6], s2, s31, s32;
    for (int c = 0; c < 6; c++) hh[c] = h[c * count + i];
    pf_lpt_sources_cell(hh, s2, s31, s32);
    out[i] = to_field(s32, fb);
  }
  return 0;
}

#ifndef ZF_EMUL_LIB
int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
  FILE *fi = fopen(argv[1], "rb");
  if (!fi) { perror(argv[1]); return 2; }
  long long head[2];
  if (fread(head, sizeof(long long), 2, fi) != 2 || head[1] < 0 || head[1] > (1 << 24)) { fclose(fi); fprintf(stderr, "bad header\n"); return 2; }
  const int fb = (int)head[0];
  const long count = (long)head[1];
  std::vector<double> s0(count), d(6 * count), h(6 * count), acc(count), start(count);
  const bool ok = fread(s0.data(), 8, count, fi) == (size_t)count && fread(d.data(), 8, 6 * count, fi) == (size_t)(6 * count) &&
                  fread(h.data(), 8, 6 * count, fi) == (size_t)(6 * count);
  fclose(fi);
  if (!ok) { fprintf(stderr, "short input\n"); return 2; }
  if (zf_emul_acc(fb, count, s0.data(), d.data(), h.data(), acc.data()) || zf_emul_start(fb, count, h.data(), start.data())) return 1;
  FILE *fo = fopen(argv[2], "wb");
  if (!fo) { perror(argv[2]); return 2; }
  const bool wrote = fwrite(acc.data(), 8, count, fo) == (size_t)count && fwrite(start.data(), 8, count, fo) == (size_t)count;
  if (fclose(fo) || !wrote) return 2;
  printf("cells %ld\n", count);
  return 0;
}
#endif
