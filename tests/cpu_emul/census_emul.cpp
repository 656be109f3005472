// census_emul.cpp -- pinocchio_amd/csrc/pf_census_core.h compiled for the host and run cell by cell on one thread: the census that
// pf_census.hip forms by waves and workgroups, as one loop.  As a library (-DCENSUS_EMUL_LIB) tests/test_census_cpu.py holds it
// against tests/np_census.py; as a program it reads the cases that test wrote and runs them under -fsanitize=address,undefined.
//
// A case in the file: int64 pb, first_cell, count, capacity; then fmax_fast[count], fmax_exact[count] (pb bytes each),
// rmax_fast[count], rmax_exact[count] (int32), each array padded to a multiple of 8 bytes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/pinfmax.h"
#include "../../pinocchio_amd/csrc/pf_census_core.h"

static_assert(PF_CENSUS_NBIN == PF_CENSUS_BINS, "the bins of the core header are those of the interface");

template <class T>
static void run(unsigned long long first_cell, size_t count, const T *ff, const int *rf, const T *fe, const int *re, pf_census *out, size_t cap, pf_census_cell *cells) {
  memset(out, 0, sizeof(*out));
  out->cells = count;
  out->max_abs_cell = ~0ull;
  bool any = false;
  for (size_t i = 0; i < count; i++) {
    const PfCensusCell q = pf_census_classify<T>(ff[i], fe[i], rf[i], re[i]);
    out->differing_bits += q.differ; out->rmax_differing += q.rdiffer;
    if (q.bin < 0) out->nonfinite++;
    else {
      out->hist[q.bin]++;
      if (q.bin >= 3) out->beyond_2ulp++;
      if (!any || q.d > out->max_abs) { out->max_abs = q.d; out->max_abs_cell = first_cell + i; }
      if (!any || q.u > out->max_ulps) out->max_ulps = q.u;
      any = true;
    }
    if (q.outlier) {
      if (out->outliers < cap) {
        pf_census_cell &r = cells[out->outliers];
        r.cell = first_cell + i; r.fast = (double)ff[i]; r.exact = (double)fe[i]; r.rmax_fast = rf[i]; r.rmax_exact = re[i];
      }
      out->outliers++;
    }
  }
}

extern "C" int census_emul_run(int pb, unsigned long long first_cell, size_t count, const void *ff, const int *rf, const void *fe, const int *re, pf_census *out,
                               size_t cap, pf_census_cell *cells) {
  if (pb == 8) run<double>(first_cell, count, (const double *)ff, rf, (const double *)fe, re, out, cap, cells);
  else if (pb == 4) run<float>(first_cell, count, (const float *)ff, rf, (const float *)fe, re, out, cap, cells);
  else return 1;
  return 0;
}
extern "C" int census_emul_sizes(size_t *s) {   // what the ABI test holds against ctypes
  s[0] = sizeof(pf_census); s[1] = sizeof(pf_census_cell);
  s[2] = offsetof(pf_census, hist); s[3] = offsetof(pf_census, beyond_2ulp); s[4] = offsetof(pf_census, max_abs); s[5] = offsetof(pf_census, max_abs_cell);
  s[6] = offsetof(pf_census_cell, fast); s[7] = offsetof(pf_census_cell, rmax_fast); s[8] = offsetof(pf_census_cell, rmax_exact);
  return 9;
}

#ifndef CENSUS_EMUL_LIB
static size_t pad8(size_t b) { return (b + 7) & ~(size_t)7; }
// census_emul_san FILE
int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  long long head[4];
  int ncase = 0;
  while (fread(head, 8, 4, f) == 4) {
    const int pb = (int)head[0];
    const size_t count = (size_t)head[2], cap = (size_t)head[3];
    if ((pb != 4 && pb != 8) || head[2] < 0 || head[3] < 0 || head[2] > (1ll << 28)) { fprintf(stderr, "bad case header\n"); return 2; }
    std::vector<char> ff(pad8(count * pb)), fe(pad8(count * pb)), rf(pad8(count * 4)), re(pad8(count * 4));
    bool ok = true;
    for (std::vector<char> *a : {&ff, &fe, &rf, &re}) ok = ok && (a->empty() || fread(a->data(), 1, a->size(), f) == a->size());
    if (!ok) { fprintf(stderr, "short case\n"); return 2; }
    pf_census out;
    std::vector<pf_census_cell> cells(cap);   // exactly the capacity: a record written beyond it is the sanitizer's to find
    if (census_emul_run(pb, (unsigned long long)head[1], count, ff.data(), (const int *)rf.data(), fe.data(), (const int *)re.data(), &out, cap, cells.data())) return 2;
    unsigned long long hs = 0, cs = 0;
    for (int k = 0; k < PF_CENSUS_BINS; k++) hs += out.hist[k];
    const size_t m = out.outliers < cap ? (size_t)out.outliers : cap;
    for (size_t k = 0; k < m; k++) cs += cells[k].cell;
    printf("case %d: outliers %llu beyond %llu differing %llu nonfinite %llu histsum %llu maxcell %llu cellsum %llu\n", ncase++, out.outliers, out.beyond_2ulp,
           out.differing_bits, out.nonfinite, hs, out.max_abs_cell, cs);
  }
  fclose(f);
  return 0;
}
#endif
