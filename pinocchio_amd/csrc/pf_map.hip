// pf_map.hip -- the fragmentation maps on the device: frag_map and frag_map_update of fragment() (src/fragment.c:193-346) as one
// resident object, pf_map.  The reference keeps two bit arrays of subbox.maplength words over the sub-box with its boundary layer:
// create_map() (:708-751) fills the well resolved box plus one layer into frag_map_update, update_map()
// (src/build_groups.c:2246-2318) rasterises one sphere per halo of the quick catalogue into it, and "frag_map = frag_map_update"
// (turn 0) / "frag_map |= frag_map_update" (turn 1) (:304-309) make it current.  The distribute and count_peaks entry points read
// the arrays where they lie (pf_distribute_map, pf_distribute_sorted_map, pf_count_peaks_map).
//
//  k_map_box      create_map: along z the bits of a row are consecutive, so a lane takes one WORD of one row: a word that lies
//                 wholly inside the row is a plain store, the (at most two) words a row shares with its neighbours an atomicOr.
//  k_map_spheres  update_map, the hot kernel.  The work per group goes as size^3 and sizes span 1 .. ~100, so a group is never given
//                 to a fixed unit: the unit is a ROW -- one (group, i1, j1), 2 size cells consecutive in k1 and, but for the single
//                 wrap, consecutive bits -- and a wavefront takes an item of pf_map_core.h: one long row in rounds of 64 lanes, or as
//                 many short rows of one group as fill 64 lanes.  The host forms the exclusive prefix of the items over the groups;
//                 a wavefront finds the group of its item by bisection (uniform loads).  A lane takes one cell: wrap / out-of-range
//                 flag, the CURRENT bit, rr <= size^2; the wavefront ballots and the first lane of every run of consecutive bits
//                 inside one word ORs the run in -- one atomic per touched word, not per bit.  Counts per lane, one 64-bit atomic
//                 per wavefront and counter at the end, as k_peaks.  OR commutes and no count depends on what an atomic returns:
//                 words and counts are bitwise reproducible whatever the schedule.  The per-bit form (one atomicOr per set cell)
//                 is kept for the A/B: PF_MAP_WORDS=0, read when a map is created.  PF_MAP_STATS=1 (read there too)
//                 selects instantiations that also count the atomics they issue, for the measurement tool; the default ones do not.
//  k_map_commit, k_map_popcount, k_map_trim   streaming helpers.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pf_internal.h"
#include "pf_map_core.h"

#define PF_MAP_BLOCK 256
#define PF_MAP_MAX_SIZE 16384   // rr = 3 size^2 stays an int (the reference's own overflows beyond 26754)

struct pf_map {
  pf_ctx *ctx;                      // null: context-free (current device, default stream)
  int rank, n;                      // n = 0 without a context
  pf_peak_region box;
  PfMapBox mb;
  unsigned long long cells;
  size_t words;
  unsigned int *bits[2];            // PF_MAP_CURRENT, PF_MAP_UPDATE
  unsigned long long *counters;     // device [3]: nadd[0], nadd[1], atomics of the last update
  unsigned long long atomics;
  bool words_form;                  // PF_MAP_WORDS
  bool stats;                       // PF_MAP_STATS: the kernel counts its atomics
  PfMapGroup *dgroups;              // device copies of the groups and of the prefix of their items, kept between updates
  unsigned long long *dprefix;
  size_t dcap;                      // groups they hold
};

struct PfMapRange { int lo[3], hi[3]; };

// ---------------------------------------------------------------------------------------------------------- kernels ----
__global__ void __launch_bounds__(PF_MAP_BLOCK) k_map_box(PfMapBox b, PfMapRange rg, unsigned long long nrows, unsigned int wpr, unsigned int *__restrict__ upd) {
  const unsigned long long total = nrows * wpr;
  for (unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long r = t / wpr, q = t - r * wpr;
    unsigned long long first; unsigned int length;
    pf_map_box_row(b, rg.lo, rg.hi, r, &first, &length);
    const unsigned long long word = (first >> 5) + q;
    if (word > ((first + length - 1) >> 5)) continue;
    const unsigned int mask = pf_map_word_mask(first, length, word);
    if (mask == 0xFFFFFFFFu) upd[word] = mask;   // the word belongs to this row alone
    else atomicOr(&upd[word], mask);
  }
}

template <bool WORDS, bool STATS>
__global__ void __launch_bounds__(PF_MAP_BLOCK) k_map_spheres(PfMapBox b, const PfMapGroup *__restrict__ groups, const unsigned long long *__restrict__ prefix,
                                                              unsigned int ngroups, unsigned long long nitems, const unsigned int *__restrict__ cur,
                                                              unsigned int *__restrict__ upd, unsigned long long *__restrict__ nadd) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned long long nwaves = (unsigned long long)gridDim.x * (PF_MAP_BLOCK / 64);
  unsigned long long c0 = 0, c1 = 0;
  unsigned int c2 = 0;   // STATS: atomics issued (measurement: PF_MAP_STATS=1, pf_debug_map_atomics)
  for (unsigned long long item = (unsigned long long)blockIdx.x * (PF_MAP_BLOCK / 64) + wave; item < nitems; item += nwaves) {
    unsigned int lo = 0, hi = ngroups;   // prefix[lo] <= item < prefix[hi]
    while (hi - lo > 1) {
      const unsigned int mid = lo + ((hi - lo) >> 1);
      if (prefix[mid] <= item) lo = mid; else hi = mid;
    }
    const PfMapGroup g = groups[lo];
    const unsigned long long local = item - prefix[lo];
    const int nch = pf_map_chunks(g.size);
    for (int ch = 0; ch < nch; ch++) {
      const PfMapCell cell = pf_map_cell(b, g, local, ch, lane);
      const bool live = cell.valid && !cell.out;
      bool set = false;
      if (live && cell.inside) set = !((cur[cell.pos >> 5] >> (cell.pos & 31u)) & 1u);   // get_map_bit_coord reads frag_map, not frag_map_update
      c0 += set ? 1u : 0u;
      c1 += (cell.valid && cell.out) ? 1u : 0u;
      if (WORDS) {
        const unsigned long long flags = __ballot(set);
        if (flags) {
          const unsigned int pos_prev = __shfl_up(cell.pos, 1, 64);
          const bool live_prev = __shfl_up((int)live, 1, 64) != 0;
          const bool head = pf_map_run_head(lane, live, live_prev, cell.pos, pos_prev);
          const unsigned long long heads = __ballot(head);
          if (head && live) {
            const unsigned int mask = pf_map_run_mask(heads, flags, lane, cell.pos);
            if (mask) { atomicOr(&upd[cell.pos >> 5], mask); if (STATS) c2++; }
          }
        }
      } else if (set) {
        atomicOr(&upd[cell.pos >> 5], 1u << (cell.pos & 31u));
        if (STATS) c2++;
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) { c0 += __shfl_down(c0, o, 64); c1 += __shfl_down(c1, o, 64); }
  if (lane == 0) {
    if (c0) atomicAdd(nadd, c0);
    if (c1) atomicAdd(nadd + 1, c1);
  }
  if (STATS) {
    unsigned long long c2l = c2;
    for (int o = 32; o > 0; o >>= 1) c2l += __shfl_down(c2l, o, 64);
    if (lane == 0 && c2l) atomicAdd(nadd + 2, c2l);
  }
}

__global__ void __launch_bounds__(PF_MAP_BLOCK) k_map_commit(size_t words, int merge, unsigned int *__restrict__ cur, const unsigned int *__restrict__ upd) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) cur[i] = merge ? (cur[i] | upd[i]) : upd[i];
}

__global__ void __launch_bounds__(PF_MAP_BLOCK) k_map_popcount(size_t words, const unsigned int *__restrict__ w, unsigned long long *__restrict__ out) {
  unsigned long long c = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) c += (unsigned int)__popc(w[i]);
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}

// the unused bits of the last word stay zero whatever the caller of pf_map_set passes
__global__ void k_map_trim(unsigned int *last, unsigned int keep) { *last &= keep; }

// ------------------------------------------------------------------------------------------------------------ helpers ----
#define MAPHIP(m, who, call)                                                                                           \
  do {                                                                                                                 \
    hipError_t e__ = (call);                                                                                           \
    if (e__ != hipSuccess) return pf_fail((m)->rank, "%s: %s failed: %s", who, #call, hipGetErrorString(e__));        \
  } while (0)

static hipStream_t map_stream(const pf_map *m) {
  if (!m->ctx) return nullptr;
  PfCtxView v;
  pf_ctx_view(m->ctx, &v);
  return v.stream;
}
// the timers of a context ("distribute" kernel class: phase 0, mem_transf: phase 1); nothing without one
struct MapTimer {
  void *t; int phase;
  MapTimer(pf_ctx *c, int phase_, double bytes = 0) : t(c ? pf_ctx_timer_begin(c, phase_, bytes, nullptr) : nullptr), phase(phase_) {}
  ~MapTimer() { if (t) pf_ctx_timer_end(t, phase); }
};
static int map_grid(unsigned long long threads) {
  unsigned long long b = (threads + PF_MAP_BLOCK - 1) / PF_MAP_BLOCK;
  if (b < 1) b = 1;
  if (b > 8192) b = 8192;
  return (int)b;
}
static int map_which(const pf_map *m, const char *who, int which) {
  if (which != PF_MAP_CURRENT && which != PF_MAP_UPDATE)
    return pf_fail(m->rank, "%s: which = %d is neither PF_MAP_CURRENT (%d) nor PF_MAP_UPDATE (%d)", who, which, PF_MAP_CURRENT, PF_MAP_UPDATE);
  return 0;
}

int pf_map_view(const char *who, pf_ctx *c, int rank, pf_map *m, int which, PfMapView *v) {
  if (!m) return pf_fail(rank, "%s: null map", who);
  if (m->ctx != c) return pf_fail(rank, "%s: the map was not created with this context (pf_map_create)", who);
  if (map_which(m, who, which)) return 1;
  for (int d = 0; d < 3; d++) { v->start[d] = m->box.start[d]; v->len[d] = m->box.len[d]; v->safe[d] = m->box.safe[d]; }
  v->bits = m->bits[which]; v->words = m->words;
  return 0;
}

// the box of a map, and of the neighbour table (pf_neighbours.hip): n = 0 without a context
int pf_map_box_check(const char *who, int rank, int n, const pf_peak_region *box, PfMapBox *out, unsigned long long *ncells) {
  const int nmax = n ? n : 2048;
  unsigned long long cells = 1;
  PfMapBox mb;
  for (int d = 0; d < 3; d++) {
    const int len = box->len[d], safe = box->safe[d];
    if (len < 1 || len > nmax) return pf_fail(rank, "%s: box does not fit: len[%d] = %d outside [1, %d]", who, d, len, nmax);
    const int pbc = n ? len == n : safe == 0;    // subbox.pbc; without a context: a direction without safety layer
    if (pbc && safe != 0) return pf_fail(rank, "%s: safe[%d] = %d in a periodic direction (len[%d] = %d spans the box): must be 0", who, d, safe, d, len);
    if (!pbc && safe < 1)
      return pf_fail(rank, "%s: safe[%d] = %d in a direction that is not periodic (len[%d] = %d): create_map() starts at safe - 1", who, d, safe, d, len);
    if (!pbc && 2 * (long long)safe > len) return pf_fail(rank, "%s: safe[%d] = %d, 2 * safe > len[%d] = %d", who, d, safe, d, len);
    mb.len[d] = len; mb.pbc[d] = pbc;
    cells *= (unsigned long long)len;
  }
  if (cells > (1ull << 32)) return pf_fail(rank, "%s: a sub-box of more than 2^32 cells (bit positions are 32-bit as in the reference)", who);
  *out = mb; *ncells = cells;
  return 0;
}

// -------------------------------------------------------------------------------------------------------- entry points ----
extern "C" int pf_map_create(pf_ctx *c, const pf_peak_region *box, pf_map **out) {
  const char *who = "pf_map_create";
  int rank = 0, n = 0;
  if (c) { PfCtxView v; pf_ctx_view(c, &v); rank = v.rank; n = v.n; }
  if (!box || !out) return pf_fail(rank, "%s: null argument", who);
  *out = nullptr;
  unsigned long long cells = 1;
  PfMapBox mb;
  if (pf_map_box_check(who, rank, n, box, &mb, &cells)) return 1;
  pf_map *m = new pf_map();
  m->ctx = c; m->rank = rank; m->n = n; m->box = *box; m->mb = mb; m->cells = cells; m->words = (size_t)((cells + 31) / 32);
  m->bits[0] = m->bits[1] = nullptr; m->counters = nullptr; m->atomics = 0; m->dgroups = nullptr; m->dprefix = nullptr; m->dcap = 0;
  const char *e = getenv("PF_MAP_WORDS");
  m->words_form = !(e && atoi(e) == 0);
  e = getenv("PF_MAP_STATS");
  m->stats = e && atoi(e) != 0;
  const hipStream_t st = map_stream(m);
  const size_t bytes = m->words * sizeof(unsigned int);
  if (hipMalloc((void **)&m->bits[0], bytes) != hipSuccess || hipMalloc((void **)&m->bits[1], bytes) != hipSuccess ||
      hipMalloc((void **)&m->counters, 3 * sizeof(unsigned long long)) != hipSuccess ||
      hipMemsetAsync(m->bits[0], 0, bytes, st) != hipSuccess || hipMemsetAsync(m->bits[1], 0, bytes, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    (void)hipGetLastError();
    pf_map_destroy(m);
    return pf_fail(rank, "%s: cannot allocate two maps of %zu bytes on the device", who, bytes);
  }
  *out = m;
  return 0;
}

extern "C" void pf_map_destroy(pf_map *m) {
  if (!m) return;
  hipStreamSynchronize(map_stream(m));
  hipFree(m->bits[0]); hipFree(m->bits[1]); hipFree(m->counters); hipFree(m->dgroups); hipFree(m->dprefix);
  delete m;
}

extern "C" size_t pf_map_length(const pf_map *m) { return m ? m->words : 0; }

extern "C" int pf_map_fill_box(pf_map *m) {
  const char *who = "pf_map_fill_box";
  if (!m) return pf_fail(0, "%s: null map", who);
  const hipStream_t st = map_stream(m);
  PfMapRange rg;
  for (int d = 0; d < 3; d++) pf_map_box_range(m->box.len[d], m->box.safe[d], m->mb.pbc[d], &rg.lo[d], &rg.hi[d]);
  const unsigned long long nrows = (unsigned long long)(rg.hi[0] - rg.lo[0]) * (unsigned long long)(rg.hi[1] - rg.lo[1]);
  const unsigned int wpr = (unsigned int)(rg.hi[2] - rg.lo[2] + 30) / 32 + 1;   // words a row can touch
  MapTimer kt(m->ctx, 0, 2.0 * (double)m->words * sizeof(unsigned int));
  MAPHIP(m, who, hipMemsetAsync(m->bits[PF_MAP_UPDATE], 0, m->words * sizeof(unsigned int), st));   // the reference's memset
  hipLaunchKernelGGL(k_map_box, dim3(map_grid(nrows * wpr)), dim3(PF_MAP_BLOCK), 0, st, m->mb, rg, nrows, wpr, m->bits[PF_MAP_UPDATE]);
  MAPHIP(m, who, hipGetLastError());
  return 0;
}

extern "C" int pf_map_update(pf_map *m, size_t ngroups, const double *pos, const int *mass, double boundary_layer_factor, unsigned long long nadd[2]) {
  const char *who = "pf_map_update";
  if (!m) return pf_fail(0, "%s: null map", who);
  if (!nadd || (ngroups && (!pos || !mass))) return pf_fail(m->rank, "%s: null argument", who);
  if (ngroups > 0x7FFFFFFFull) return pf_fail(m->rank, "%s: %zu groups: ngroups is int in the reference", who, ngroups);
  // centre and size of every group with the reference's own expressions and libm calls (:2255-2258): the edge of a sphere never
  // depends on a device pow
  std::vector<PfMapGroup> groups(ngroups);
  std::vector<unsigned long long> prefix(ngroups + 1);
  unsigned long long items = 0, visits = 0;
  for (size_t g = 0; g < ngroups; g++) {
    const double s = boundary_layer_factor * pow((double)mass[g] / 4.188790205, 0.333333333333333) + 0.5;
    if (!(s > -1.0 && s < (double)PF_MAP_MAX_SIZE + 1.0))
      return pf_fail(m->rank, "%s: group %zu of mass %d: size %g outside [0, %d]", who, g, mass[g], s, PF_MAP_MAX_SIZE);
    const int size = (int)s;
    int c[3];
    for (int d = 0; d < 3; d++) {
      const double p = pos[3 * g + d] + 0.5;
      if (!(p > -1073741824.0 && p < 1073741824.0)) return pf_fail(m->rank, "%s: group %zu: position[%d] = %g", who, g, d, pos[3 * g + d]);
      c[d] = (int)p;
      if (m->mb.pbc[d]) {
        // the reference wraps once: beyond these its index leaves the map
        if (size > m->box.len[d])
          return pf_fail(m->rank, "%s: group %zu: size %d > len[%d] = %d in a periodic direction (one wrap does not bring the cube back)", who, g, size, d, m->box.len[d]);
        if (c[d] < 0 || c[d] > m->box.len[d])
          return pf_fail(m->rank, "%s: group %zu: centre[%d] = %d outside [0, %d] in a periodic direction", who, g, d, c[d], m->box.len[d]);
      }
    }
    groups[g] = PfMapGroup{c[0], c[1], c[2], size};
    prefix[g] = items;
    items += pf_map_items(size);
    visits += 8ull * (unsigned long long)size * (unsigned long long)size * (unsigned long long)size;
  }
  prefix[ngroups] = items;
  const hipStream_t st = map_stream(m);
  MapTimer pt(m->ctx, 1);
  MAPHIP(m, who, hipMemsetAsync(m->bits[PF_MAP_UPDATE], 0, m->words * sizeof(unsigned int), st));
  MAPHIP(m, who, hipMemsetAsync(m->counters, 0, 3 * sizeof(unsigned long long), st));
  if (items) {
    if (ngroups > m->dcap) {   // (the buffers of the last update are idle: every update ends with a synchronised stream)
      hipFree(m->dgroups); hipFree(m->dprefix);
      m->dgroups = nullptr; m->dprefix = nullptr; m->dcap = 0;
      MAPHIP(m, who, hipMalloc((void **)&m->dgroups, ngroups * sizeof(PfMapGroup)));
      MAPHIP(m, who, hipMalloc((void **)&m->dprefix, (ngroups + 1) * sizeof(unsigned long long)));
      m->dcap = ngroups;
    }
    PfMapGroup *dg = m->dgroups;
    unsigned long long *dp = m->dprefix;
    MAPHIP(m, who, hipMemcpyAsync(dg, groups.data(), ngroups * sizeof(PfMapGroup), hipMemcpyHostToDevice, st));
    MAPHIP(m, who, hipMemcpyAsync(dp, prefix.data(), (ngroups + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    MapTimer kt(m->ctx, 0, (double)visits * 0.25 + (double)ngroups * 24.0);
    const dim3 grid(map_grid(items * 64ull)), block(PF_MAP_BLOCK);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, block, 0, st, m->mb, dg, dp, (unsigned int)ngroups, items, m->bits[PF_MAP_CURRENT], m->bits[PF_MAP_UPDATE], m->counters);
    };
    if (m->words_form) { if (m->stats) launch(k_map_spheres<true, true>); else launch(k_map_spheres<true, false>); }
    else { if (m->stats) launch(k_map_spheres<false, true>); else launch(k_map_spheres<false, false>); }
    MAPHIP(m, who, hipGetLastError());
  }
  unsigned long long h[3] = {0, 0, 0};
  MAPHIP(m, who, hipMemcpyAsync(h, m->counters, sizeof(h), hipMemcpyDeviceToHost, st));
  MAPHIP(m, who, hipStreamSynchronize(st));
  nadd[0] = h[0]; nadd[1] = h[1]; m->atomics = h[2];
  return 0;
}

extern "C" int pf_debug_map_atomics(const pf_map *m, unsigned long long *atomics) {
  if (!m || !atomics) return pf_fail(0, "pf_debug_map_atomics: null argument");
  if (!m->stats) return pf_fail(m->rank, "pf_debug_map_atomics: the map was created without PF_MAP_STATS=1");
  *atomics = m->atomics;
  return 0;
}

extern "C" int pf_map_commit(pf_map *m, int merge) {
  const char *who = "pf_map_commit";
  if (!m) return pf_fail(0, "%s: null map", who);
  const hipStream_t st = map_stream(m);
  MapTimer kt(m->ctx, 0, (merge ? 3.0 : 2.0) * (double)m->words * sizeof(unsigned int));
  hipLaunchKernelGGL(k_map_commit, dim3(map_grid(m->words)), dim3(PF_MAP_BLOCK), 0, st, m->words, merge, m->bits[PF_MAP_CURRENT], m->bits[PF_MAP_UPDATE]);
  MAPHIP(m, who, hipGetLastError());
  return 0;
}

extern "C" int pf_map_get(pf_map *m, int which, unsigned int *words) {
  const char *who = "pf_map_get";
  if (!m) return pf_fail(0, "%s: null map", who);
  if (map_which(m, who, which)) return 1;
  if (!words) return pf_fail(m->rank, "%s: null argument", who);
  const size_t bytes = m->words * sizeof(unsigned int);
  if (m->ctx) {
    MapTimer pt(m->ctx, 1);
    return pf_ctx_d2h(m->ctx, words, m->bits[which], bytes);   // the hand-off pieces; starts behind the compute stream
  }
  MAPHIP(m, who, hipMemcpy(words, m->bits[which], bytes, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int pf_map_set(pf_map *m, int which, const unsigned int *words) {
  const char *who = "pf_map_set";
  if (!m) return pf_fail(0, "%s: null map", who);
  if (map_which(m, who, which)) return 1;
  if (!words) return pf_fail(m->rank, "%s: null argument", who);
  const size_t bytes = m->words * sizeof(unsigned int);
  const hipStream_t st = map_stream(m);
  if (m->ctx) {
    MapTimer pt(m->ctx, 1);
    if (pf_ctx_h2d(m->ctx, m->bits[which], words, bytes)) return 1;
  } else {
    MAPHIP(m, who, hipMemcpy(m->bits[which], words, bytes, hipMemcpyHostToDevice));
  }
  if (m->cells & 31ull) {
    hipLaunchKernelGGL(k_map_trim, dim3(1), dim3(1), 0, st, m->bits[which] + (m->words - 1), (1u << (unsigned int)(m->cells & 31ull)) - 1u);
    MAPHIP(m, who, hipGetLastError());
  }
  return 0;
}

extern "C" int pf_map_count(pf_map *m, int which, unsigned long long *bits) {
  const char *who = "pf_map_count";
  if (!m) return pf_fail(0, "%s: null map", who);
  if (map_which(m, who, which)) return 1;
  if (!bits) return pf_fail(m->rank, "%s: null argument", who);
  const hipStream_t st = map_stream(m);
  MAPHIP(m, who, hipMemsetAsync(m->counters, 0, sizeof(unsigned long long), st));
  {
    MapTimer kt(m->ctx, 0, (double)m->words * sizeof(unsigned int));
    hipLaunchKernelGGL(k_map_popcount, dim3(map_grid(m->words)), dim3(PF_MAP_BLOCK), 0, st, m->words, m->bits[which], m->counters);
    MAPHIP(m, who, hipGetLastError());
  }
  MAPHIP(m, who, hipMemcpyAsync(bits, m->counters, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  MAPHIP(m, who, hipStreamSynchronize(st));
  return 0;
}
