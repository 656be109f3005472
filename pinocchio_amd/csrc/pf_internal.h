// pf_internal.h -- launch interface between the translation units of libpinfmax_hip.so
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/pinfmax.h"

#define PF_MAX_JOBS 6
#define PF_MAX_DEVICES 64

// run-time switches, read from the environment once per context in pf_create (pf_api.hip: read_tuning);
// launch paths see only this struct
struct PfTuning {
  int zpass_persist;        // PF_ZPASS_PERSIST: workgroups per CU of the persistent z-pass, 0 = one-shot workgroups
  int zpass_inv_wg_per_cu;  // PF_ZPASS_INV_WG_PER_CU
  int collapse_wg_per_cu;   // PF_COLLAPSE_WG_PER_CU
  bool spline_lut, exchange_rows, general, pipeline, exact_libm;
  int invariants, lpt_fuse;  // PF_INVARIANTS / PF_LPT_FUSE: 0 off, 1 where the invariant z-pass is the faster way (pf_c2r_invariants_preferred), 2 wherever it exists
  int replicate;  // PF_REPLICATE_DK: -1 by rank count, 0 off, 1 on
  double prune_eps;
  int debug_fault;          // PF_DEBUG_PIPELINE_FAULT (tests only): 1 / 2 = one wait of the exchange pipeline left out
  int solve_beside_z;       // PF_SOLVE_BESIDE_Z: the solve of sweep radius i runs on its own stream beside the z-pass of radius i + 1 (1), every
                            // kernel in line (0), or -- the default, -1 -- beside with fp32 fields and in line with fp64 fields (pf_sweep)
  int handoff_chunk_mb, handoff_threads;  // PF_HANDOFF_CHUNK_MB, PF_HANDOFF_THREADS: pieces and host threads of the hand-off (pf_api.hip PfHandoff)
  bool host_register;       // PF_HOST_REGISTER: register the caller's product array with the driver, DMA straight into it
  bool preflight;           // PF_PREFLIGHT: pf_create holds the plan's bytes against the device's free memory before it allocates
  bool distribute_lds;      // PF_DISTRIBUTE_LDS: pf_distribute stages the records of a round in LDS (1, default) or writes one lane per record (0)
  bool gtab;                // PF_GTAB: the inverse growing mode of the fast flavour from the polynomial table (pf_gtab.h)
  bool lpt3b_start;         // PF_LPT3B_START: 1 = the solve of the sweep's last radius stores the 3LPT(b) start value and the contracting z-pass reads it (0: that z-pass forms it)
  bool lpt_xfuse;           // PF_LPT_XFUSE: one rank, the forward x-pass of an LPT source runs inside the inverse x-passes that read it (k_strided with PF_DIR_XF)
};

// multiplier applied along the transformed axis before the 1-D transform
// (k = 2 pi s / N, s the signed wavenumber of src/fmax-pfft.c:306-339)
enum { PF_MUL_ONE = 0, PF_MUL_K = 1, PF_MUL_K2 = 2, PF_MUL_IK = 3 };

// element address of (outer, e, col) in a strided pass:
//   outer*os + (e >> el_shift)*ehs + (e & (el-1))*els + col      (units: complex elements)
// (e / el, e % el) lets the y-pass read the P received all-to-all blocks in place.
struct PfAddr {
  long long os;
  int el_shift;  // el = 1 << el_shift (slab thickness; a power of two where n and P are: what the power-of-two kernels split by)
  long long ehs, els;
  int el_len;    // the slab thickness itself (n, n / P): what the mixed-radix kernels split by (multiply-high), any length
};

struct PfStridedJob {
  const void *in;
  void *out;
  int mul;
};

struct PfStridedParams {
  int njobs;
  PfStridedJob job[PF_MAX_JOBS];
  PfAddr ain, aout;
  int ncols;         // valid columns (n/2+1)
  int nouter;        // lines of tiles along the non-transformed slow axis
  int pre;           // 1: multiply by exp(-k^2 rs^2/2) * growth / k^2 (0 at k = 0) on load
  int outer_offset;  // global index of outer = 0 (k-space y-slab start)
  double rs, growth;
  // pre: the Gaussian window is separable, exp(-k^2 rs^2/2) = E(k_e) * exp(-(k_o^2 + k_c^2) rs^2/2): etab[e] = E of the
  // transformed axis (n doubles, pf_launch_exp_table) leaves one exp per thread instead of eight; rs == 0 needs none
  const double *etab;
  const void *tw;    // exp(+2 pi i j / n), n entries of complex F
  // pruned transform of a band-limited (Gaussian-smoothed) spectrum: wavenumbers |s| > band carry a
  // weight below 2^-60 and are treated as exact zeros.  band_e masks the loads along the transformed
  // axis, band_outer skips whole workgroups; columns are pruned by ncols.  band >= n/2 disables.
  int band_e, band_outer;
  int dev;           // device the launch goes to (the LDS-size attribute of an instantiation is raised once per device)
  // out_ne > 0: only the outputs e in [out_e0, out_e0 + out_ne) are stored (a rank that holds the whole spectrum and
  // transforms every line, but keeps its own slab of the transformed axis: no exchange afterwards)
  int out_e0, out_ne;
};

// one x- or y-pass: for every job, out = FFT_e[ in * pre * mul ]  (dir = +1 inverse, -1 forward)
int pf_launch_strided(int field_bytes, int n, int dir, const PfStridedParams &p, hipStream_t st);
// dir = +1 with the forward transform of the (single) input along the same axis done first, in the same workgroup (k_strided with PF_DIR_XF)
bool pf_strided_xfuse_supported(int field_bytes, int n);
int pf_launch_strided_xfuse(int field_bytes, int n, const PfStridedParams &p, hipStream_t st);
int pf_launch_exp_table(double *etab, int n, double rs, hipStream_t st);
// 2048-point fp32 lines, sixteen points per thread (pf_fft16_kernels.hip); -1: not a case of that kernel
int pf_launch_strided16(int field_bytes, int n, int dir, const PfStridedParams &p, hipStream_t st);

struct PfC2RJob {
  const void *in;   // complex rows
  void *out;        // real rows (type F, pitch out_pitch); out_f32 == 1: float rows of pitch n; == 2: rows of type F, pitch n
  int mul;          // multiplier in kz
  int out_f32;
};

struct PfC2RParams {
  int njobs;
  PfC2RJob job[PF_MAX_JOBS];
  long long nlines;     // rows = nx_local * n
  long long in_pitch;   // complex elements per input row
  long long out_pitch;  // real elements per output row (F outputs)
  double norm;          // 1/N^3 applied to the result (src/fmax-pfft.c:220-225)
  const double *dc;     // device scalar added after normalisation (DC mode of 2nd derivatives), or null
  const void *tw;       // exp(+2 pi i j / n)
  int band_k;           // input columns kz > band_k are zero (pruned), not read
  void *acc;            // k_c2r_invariants MODE 1: the real field updated in place (3LPT(b) source); job[c].out = first-order Hessian
  double *flag;         // k_c2r_invariants MODE 0: set to 1 when a cell has q == 0 without being exactly isotropic (pf_sweep repeats)
  int ncu, dev;         // CUs of the device, device index
  int persist_per_cu;   // workgroups per CU of the persistent z-pass (0: one-shot kernel)
  int inv_per_cu;       // workgroups per CU of the invariant z-pass
  double *inv_out[3];   // k_c2r_invariants<float> MODE 0: the fp64 invariant rows (pitch inv_pitch) -- fp32 rows cannot hold them
  long long inv_pitch;
};
int pf_launch_c2r(int field_bytes, int n, const PfC2RParams &p, hipStream_t st);
// six components (njobs == 6) -> the three invariants of the tensor: fp64 fields into job[0..2].out, fp32 fields into inv_out
// mode 1: nothing stored, p.acc -= 2 phi2_ab h_ab with h_ab read from job[c].out (the 3LPT(b) source, src/LPT.c:134-137)
int pf_launch_c2r_invariants(int field_bytes, int n, const PfC2RParams &p, hipStream_t st, int mode = 0);

struct PfR2CParams {
  const void *in;       // real rows, pitch in_pitch reals
  void *out;            // complex rows, pitch out_pitch complex (may alias in)
  long long nlines, in_pitch, out_pitch;
  const void *tw;
};
int pf_launch_r2c(int field_bytes, int n, const PfR2CParams &p, hipStream_t st);

// ---- grid sizes that are not a power of two (pf_mixed_kernels.hip): the same three passes with a run-time stage plan ----
#define PF_MIXED_MAX_STAGES 12
struct PfMixedPlan { int n, nstages; int radix[PF_MIXED_MAX_STAGES]; unsigned magic[PF_MIXED_MAX_STAGES]; unsigned magic_in, magic_out; /* ceil(2^32 / el_len) of the launch's input and output layouts (strided passes) */ };
bool pf_mixed_plan(int n, bool allow4, PfMixedPlan *pl);
bool pf_mixed_supported(int n);   // n = 8 m with m = 2^a 3^b 5^c, up to 2048: strided passes on n, z-passes on n / 2
int pf_launch_mixed_strided(int field_bytes, int n, int dir, const PfStridedParams &p, hipStream_t st);
int pf_launch_mixed_c2r(int field_bytes, int n, const PfC2RParams &p, hipStream_t st);
int pf_launch_mixed_r2c(int field_bytes, int n, const PfR2CParams &p, hipStream_t st);
bool pf_mixed_invariants_supported(int field_bytes, int n);  // six lines of a row fit one workgroup
int pf_launch_mixed_c2r_invariants(int field_bytes, int n, const PfC2RParams &p, hipStream_t st, int mode);
bool pf_c2r_invariants_preferred(int field_bytes, int n);   // ... and the sweep uses it (pf_fft_kernels.hip)
bool pf_mixed_plan_compiled_in(int n);                       // n is one of PF_MIXED_CT_SIZES (pf_mixed_kernels.hip)
bool pf_c2r_invariants_supported(int field_bytes, int n);    // pf_launch_c2r_invariants takes rows of n points (either kind of plan)

// ---- per-cell kernels (pf_cell_kernels.hip) ----
#define PF_KNOT_CAP 512  // knots per spline at most; the five arrays of a spline lie PF_KNOT_CAP doubles apart (y = x + PF_KNOT_CAP ...: spline_for)
struct PfSplineDev {
  const double *x, *y, *c, *b, *d;  // knots, GSL cspline c_i, and the per-interval b_i, d_i (pf_spline_bd)
  int n;
  // pf_gtab.h: header + records of the polynomial table of this spline and its start table; null: none (table refused or PF_GTAB=0)
  const double *gt;
  const unsigned short *gt_lut;
};
// TABULATED_CT table of one radius on the device (pf_collapse_core.h pf_ct_view)
struct PfCtDev {
  double *delta, *y, *b, *c, *d;   // [100], 4 x [50*50*100]
  const double *alpha, *gamma;     // [98] factors of the shared tridiagonal system
  double ampl;
  int model;                       // what fills the table: 0 ell_classic + InverseGrowingMode, 1 ell_sng (pf_sng_core.h)
  int flavour;                     // how the solve reads it: 0 BILINEAR_SPLINE, 1 TRILINEAR, 2 ALL_SPLINE (pf_collapse_core.h)
  double sng_cosmo[7], sng_Din;    // ELL_SNG: Omega0, OmegaLambda, OmegaRad, OmegaK, FR0, H_over_c, size; GrowingMode at a = 1e-5 for this radius
};
struct PfCollapseParams {
  const void *h[6];     // Hessian fields, type F, rows of pitch reals
  long long pitch;
  long long nrows;      // nx_local * n
  int n;                // row length
  void *fmax;           // products.Fmax: float, or double when prod_f64 (-DDOUBLE_PRECISION_PRODUCTS, fp64 fields only)
  int prod_f64;
  int *rmax;
  int ismooth;
  PfSplineDev spline;
  double *partials;     // [2*nblocks]: sum delta, sum delta^2 per block
  int nblocks;
  int fast;             // 1: sincos/cbrt/exp10 forms of the transcendental hot spots (pf_collapse_core.h)
  int no_lut;           // 1: plain bisection in the spline lookup (PF_SPLINE_LUT=0)
  int invariants;       // 1: h[0..2] hold mu1, mu2, mu3 (k_c2r_invariants), h[3..5] unused
  int tabulated;        // 1: F from the collapse-time table `ct` (TABULATED_CT build) instead of the direct solve
  int sng;              // 1: ELL_SNG without a table -- one RKF45 integration per cell, cosmology and D_in in ct.sng_*
  // sources: the same pass also forms the 2LPT / 3LPT sources of the cell from the six components it holds (what
  // k_lpt_sources computes, src/LPT.c:64-93) -- fields of type F in src[0..2], per-block sums of S2 in src_partials
  int sources;
  void *src[3];
  double *src_partials;
  PfCtDev ct;
};
int pf_launch_ct_build(const PfSplineDev &sp, const PfCtDev &ct, int fast, int compute_table, hipStream_t st);
int pf_launch_collapse(int field_bytes, const PfCollapseParams &p, hipStream_t st);
int pf_launch_final_sum(const double *partials, int nblocks, double *out2, hipStream_t st);
int pf_launch_collapse_cells(const double *d, size_t count, PfSplineDev s, double *F, int fast, hipStream_t st);

struct PfLptSrcParams {
  const void *h[6];
  void *s2, *s3a, *s3b;  // real rows, same pitch
  long long pitch, nrows;
  int n;
  double *partials;      // per-block sum of s2 (its spectrum's DC), [nblocks]
  int nblocks;
};
int pf_launch_lpt_sources(int field_bytes, const PfLptSrcParams &p, hipStream_t st);

struct PfLptAccParams {
  const void *h[6], *phi2[6];
  void *s3b;
  long long pitch, nrows;
  int n;
};
int pf_launch_lpt_accum(int field_bytes, const PfLptAccParams &p, hipStream_t st);

int pf_launch_sum1(const double *partials, int nblocks, double scale, double *out, hipStream_t st);
// pb: bytes of a PRODFLOAT (4, or 8 for -DDOUBLE_PRECISION_PRODUCTS): the type of fmax[] and of the twelve vel12 columns
int pf_launch_fill_products(void *fmax, int *rmax, void *vel12, size_t ncell, int pb, hipStream_t st);
int pf_launch_apply_growth(int fb, const void *in, void *out, int n, int nyl, int nzh, int nzp, int y0, const double *T, int nk,
                           double logkmin, double dlogk, double sign, hipStream_t st);
int pf_launch_pack_products(int pb, const void *fmax, const int *rmax, const void *vel12, size_t ncell_total,
                            size_t first, size_t count, char *aos, size_t stride, int off_rmax, int off_fmax,
                            const int off_vel[4], hipStream_t st);
int pf_launch_fmax_pdf(const void *fmax, size_t ncell, unsigned long long *hist, int pb, hipStream_t st);
// copy + pitch/precision conversion of a half-spectrum between the boundary layout
// (fp64, rows of nzh complex) and the internal one (F, rows of nzp complex)
int pf_launch_spec_import(int field_bytes, const double *src, void *dst, long long nrows, int nzh, int nzp, hipStream_t st);
int pf_launch_spec_export(int field_bytes, const void *src, double *dst, long long nrows, int nzh, int nzp, hipStream_t st);
int pf_launch_spec_import_t(int fb, const double *src, void *dst, int n, int nyl, int nzh, int nzp, hipStream_t st);
int pf_launch_spec_export_t(int fb, const void *src, double *dst, int n, int nyl, int nzh, int nzp, hipStream_t st);
int pf_launch_real_import(int field_bytes, const double *src, void *dst, long long nrows, int n, long long pitch, hipStream_t st);
int pf_launch_real_export(int field_bytes, const void *src, double *dst, long long nrows, int n, long long pitch, hipStream_t st);
// general grid sizes (library-FFT path)
int pf_launch_gen_filter(const void *in, void *out, int n, int a, int b, double rs, double growth, const double *T, int nk, double logkmin,
                         double dlogk, double sign, double norm, hipStream_t st);
int pf_launch_real_to_col(const double *src, void *dst, size_t ncell, int pb, hipStream_t st);
int pf_launch_scale_real(double *f, size_t ncell, double s, hipStream_t st);
// pf_gfft.hip: chirp-z (Bluestein) 3-D transforms for any even n (double precision, natural layouts: spectrum [n][n][n/2+1], real [n][n][n])
int pf_gfft_create(int n, hipStream_t st, void **c2r, void **r2c);
int pf_gfft_c2r(void *plan, void *spec, void *real);   // unnormalised, out of place; may destroy spec
int pf_gfft_r2c(void *plan, void *real, void *spec);   // unnormalised, out of place
void pf_gfft_destroy(void *plan);
int pf_launch_debug_math(int which, const double *a, const double *b, size_t count, double *out, hipStream_t st);
// pf_select_sort.hip
int pf_select_sort_device(const float *fmax, size_t ncell, float flast, unsigned int **d_idx, float **d_f, size_t *count, hipStream_t st);
int pf_sort_keys_device(unsigned long long *keys_in, size_t count, unsigned int **d_idx, float **d_f, hipStream_t st);  // takes keys_in over
// pf_peaks.hip: count_peaks (src/fragment.c:605-706) on a slab
struct PfPeakParams {
  const void *fmax;               // this rank's slab [nxl][n][n] of PRODFLOAT
  const void *halo_lo, *halo_hi;  // the planes x - 1 of the first and x + 1 of the last local plane, [n][n]
  int n, nxl, x0;                 // x0: global x of the first local plane
  double flast;
  int start[3], lo[3], hi[3], glo[3], ghi[3];  // pf_peak_region_setup: examined and well resolved ranges in the region's own coordinates
  unsigned long long *counters;   // device: [0] peaks, [1] well resolved peaks, [2] key cursor
  unsigned long long *keys;       // null: count only
  size_t key_cap;
  const unsigned int *map;        // non-null (device): the stored set is (bit of the map's box set) && Fmax >= flast; the region is that box
  int mlen[3];                    // ... whose Lgwbl this is (its start is start[])
};
int pf_peak_region_setup(int n, const pf_peak_region *rg, PfPeakParams *p, int *bad);
int pf_launch_peaks(int pb, const PfPeakParams &p, hipStream_t st);
int pf_select_peaks_device(PfPeakParams p, size_t npeaks, unsigned int **d_idx, float **d_f, hipStream_t st);
// pf_distribute.hip: distribute() (src/distribute.c:58-175) for one target sub-box -- order-preserving selection and packing
#include "pf_distribute_boxes.h"  // PfDistTable, PF_DIST_GROUP_WAVES: the box table (plain C++, also compiled by a CPU test)
#define PF_DIST_MAX_WORDS 56     // 4-byte words of a record the LDS-staged pack holds (records up to 224 bytes: 56 KB of LDS per workgroup)
struct PfDistScratch {                   // device memory of one call (pf_dist_release)
  unsigned int *map;                     // the caller's map, null: every bit set
  unsigned long long *masks;             // [ngroups * PF_DIST_GROUP_WAVES] ballots
  unsigned int *counts;                  // [ngroups]
  unsigned long long *offs;              // [ngroups + 1] exclusive scan; the last one is the total
};
// the record as 4-byte words: src[j] = -1 zero, 0 Rmax, 1 + h word h of Fmax, 4 + 2 k + h word h of displacement column k (0..11)
// (src[] is filled for records of up to PF_DIST_MAX_WORDS words; the named words alone, in named_off / named_src, for any stride)
struct PfDistRecord { int nwords, nnamed; int named_off[28]; signed char named_src[28]; signed char src[PF_DIST_MAX_WORDS]; };
// 0 ok; 1: len[*bad] outside [1, n]; 2: more than 2^32 cells
int pf_dist_table(int n, int x0, int nxl, const pf_subbox *sub, PfDistTable *t, int *bad);
// 0 ok; 1: stride or an offset is not a multiple of four, or a field leaves the record; 2: fields overlap
int pf_dist_record(int pb, const pf_product_layout *l, PfDistRecord *r);
// flag pass + scan: *count = cells taken.  Synchronises the stream (the count sizes what follows)
// map_dev (with map_host null): a map that lies on the device already is read in place, nothing is uploaded and *s does not own it
int pf_dist_select(const PfDistTable &t, int pb, const void *fmax, double flast, const unsigned int *map_host, const unsigned int *map_dev,
                   PfDistScratch *s, hipStream_t st, unsigned long long *count);
// records [first, first + cnt) of the selection: aos (null: none; cnt records of `stride` bytes), frag_pos and cell_index (null: none).
// lds: records staged in LDS and written as contiguous words (needs r.nwords <= PF_DIST_MAX_WORDS); else one lane per record into a
// cleared aos
int pf_dist_pack(const PfDistTable &t, const PfDistScratch &s, int pb, const void *fmax, const int *rmax, const void *vel12,
                 size_t ncell_total, const PfDistRecord &r, size_t stride, unsigned long long first, unsigned long long cnt, char *aos,
                 unsigned int *frag_pos, unsigned int *cell_index, bool lds, hipStream_t st);
void pf_dist_release(PfDistScratch *s);
// ---- pf_organize.hip: sort_and_organize() (src/fragment.c:484-520); it holds its own extern "C" entry points and sees a context
// through these (pf_api.hip) ----
int pf_fail(int task, const char *fmt, ...);   // sets pf_last_error, prints "ERROR on task %d: ...", returns 1
int pf_dist_table_checked(int task, const char *who, int n, int x0, int nxl, const pf_subbox *sub, PfDistTable *t);  // pf_dist_table + message
struct PfCtxView {
  int rank, n, nxl, pb;
  bool products_init, distribute_lds;
  const void *fmax, *vel12; const int *rmax;
  size_t ncell;           // cells of the slab
  hipStream_t stream;
};
void pf_ctx_view(pf_ctx *c, PfCtxView *v);
int pf_ctx_velocities_ready(pf_ctx *c);
// the hand-off machinery (pf_api.hip PfHandoff): two streams that start behind the compute stream, a pinned buffer and a staging
// field of the device for each, `chunk` bytes long
struct PfHandoffView { hipStream_t st[2]; char *pin[2], *dev[2]; size_t chunk; };
int pf_ctx_handoff_begin(pf_ctx *c, PfHandoffView *v);
void pf_ctx_host_copy(pf_ctx *c, void *dst, const void *src, size_t bytes);          // by the host threads of the hand-off
int pf_ctx_d2h(pf_ctx *c, void *host, const void *src_dev, size_t bytes);             // device array -> pageable memory, in pieces
int pf_ctx_h2d(pf_ctx *c, void *dst_dev, const void *host, size_t bytes);
// a kernel timer of the "distribute" class (phase 0) or the memory-transfer phase timer (phase 1) around a scope
void *pf_ctx_timer_begin(pf_ctx *c, int phase, double bytes, hipStream_t st);
void pf_ctx_timer_end(void *t, int phase);
struct PfScopedTimer {
  void *t; int phase;
  PfScopedTimer(pf_ctx *c, int phase_, double bytes = 0, hipStream_t st = nullptr) : t(pf_ctx_timer_begin(c, phase_, bytes, st)), phase(phase_) {}
  ~PfScopedTimer() { pf_ctx_timer_end(t, phase); }
};
// ---- pf_map.hip: the resident fragmentation maps; what the distribute and count_peaks entry points see of one ----
struct PfMapView { int start[3], len[3], safe[3]; const unsigned int *bits; size_t words; };
// refuses (message of `who`) a null map, a map of another context and a `which` that names no array
int pf_map_view(const char *who, pf_ctx *c, int rank, pf_map *m, int which, PfMapView *v);
// the box check of pf_map_create (len, safe, periodic directions, 2^32 cells; n = 0 without a context), shared with pf_neighbours
struct PfMapBox;
int pf_map_box_check(const char *who, int rank, int n, const pf_peak_region *box, PfMapBox *mb, unsigned long long *cells);
// ---- pf_neighbours.hip: the neighbour table of the stored particles ----
// what the fused call asks of pf_distribute_sorted_impl beside its own outputs (host pointers, each may be null)
struct PfNeighOut { int len[3], pbc[3], safe[3]; bool rows; int *neigh; unsigned char *flags; unsigned long long *peaks; };
// the table of the first m records of the sorted order from the position index that lies on the device; Fmax of record i is element
// cell[perm[i]] of the column fmax (pb bytes each).  Results through the hand-off pieces of the context
int pf_neigh_from_index(pf_ctx *c, const PfCtxView &v, const char *who, const PfNeighOut &nb, size_t m, const unsigned int *sorted_pos,
                        const unsigned int *indices, const unsigned int *perm, const unsigned int *cell, const void *fmax);
// the position sort of pf_organize.hip on its own: m positions in k0 -> *sorted_pos / *indices (each one of the four buffers of m
// words); *tmp is rocPRIM's, the caller's to free once the stream has drained
int pf_org_position_sort(unsigned int *k0, unsigned int *k1, unsigned int *v0, unsigned int *v1, size_t m, unsigned int pos_bits, void **tmp,
                         hipStream_t st, unsigned int **sorted_pos, unsigned int **indices);
// `count` elements of `elem` bytes that lie `stride` bytes apart in the caller's memory, packed by the host threads while they fill
// the pinned pieces, to dst_dev.  limit != 0: the elements are 32-bit positions, and one that is not below limit ends the upload:
// 2 is returned (no message) and *bad is the index of one such element
int pf_ctx_h2d_packed(pf_ctx *c, void *dst_dev, const void *host, size_t count, size_t elem, size_t stride, unsigned long long limit, size_t *bad);
// pf_distribute_sorted with the map on the host or (map_host null) on the device (pf_organize.hip); nb: the neighbour table too
int pf_distribute_sorted_impl(const char *who, pf_ctx *c, double flast, const pf_subbox *sub, const unsigned int *map_host, const unsigned int *map_dev,
                              const pf_product_layout *l, size_t capacity, void *frag, unsigned int *frag_pos, unsigned int *sorted_pos, int *indices,
                              size_t *count, const PfNeighOut *nb = nullptr);
// ---- pf_back.hip: distribute_back() (src/distribute.c:703-946) into the zacc / group_ID columns of the slab ----
// zacc := -1 (pb bytes each), group_ID := 0 (src/allocations.c:519-524)
int pf_launch_back_fill(int pb, void *zacc, int *group, size_t ncell, hipStream_t st);
// the two columns of the context (pf_api.hip).  They come into being at the first call -- allocated, counted into pf_device_bytes and
// set to -1 / 0 on the context's stream; *fresh says that this call did it --, and a failure (message of `who` with the bytes it needs)
// leaves the context without them, as it was
int pf_ctx_back_columns(pf_ctx *c, const char *who, void **zacc, int **group, bool *fresh);
// ---- pf_refresh.hip: the velocities of the stored particles of a sub-box gathered from the columns (src/fragment.c:398-430) ----
// the Vel*_prev columns of the context (pf_api.hip: pf_shift_displacements), twelve laid out as vel12 -- null while there are none --,
// the shifts that filled them and the LPT order whose columns are computed (pf_set_lpt_order)
void pf_ctx_prev_view(pf_ctx *c, const void **prev, int *shifts, int *lpt_order);
// f(user, a, b) on disjoint ranges that cover [0, count), by the host threads of the hand-off (after pf_ctx_handoff_begin)
void pf_ctx_host_run(pf_ctx *c, size_t count, void (*f)(void *user, size_t a, size_t b), void *user);
// what pf_groupvel.hip shares with it.  The columns as 4-byte words: cur / prev = twelve columns of ncell PRODFLOATs each (prev null:
// its slots read zero); columns kmax .. 11 of either set read zero (the LPT orders the context does not compute)
struct PfRefreshCols { const unsigned int *cur, *prev; size_t ncell; int kmax; };
// what a call holds on the device beside the columns: masks / counts / offs are the ballots, block counts and their scan of whatever
// flag pass filled them (k_refresh_flag: found; k_groupvel_flag: found and loose)
struct PfRefreshScratch { unsigned int *pos; int *order; unsigned long long *masks, *offs; unsigned int *counts; unsigned int *index; void *vel; };
struct PfRefreshFields { int nf; int off[8], slot[8]; };
struct PfBackBox;
void pf_refresh_release(PfRefreshScratch *s);
size_t pf_refresh_blocks(size_t count);
size_t pf_refresh_in_bytes(size_t count, bool with_order);
int pf_refresh_alloc_in(PfRefreshScratch *s, size_t count, bool with_order);
int pf_refresh_alloc_out(PfRefreshScratch *s, size_t m, int pb, bool want_index, bool want_vel);
int pf_refresh_scan(const unsigned int *counts, size_t nblocks, unsigned long long *offs, hipStream_t st);   // k_refresh_scan
// k_refresh_flag + k_refresh_scan behind positions that lie on the device (pf_points.hip); synchronises the stream: *found sizes what follows
int pf_refresh_select(const char *who, int task, const PfBackBox &b, size_t count, const PfRefreshScratch &s, hipStream_t st, unsigned long long *found);
int pf_refresh_gather(int pb, const PfBackBox &b, size_t count, const PfRefreshScratch &s, const PfRefreshCols &cols, unsigned long long cap, hipStream_t st);
int pf_refresh_box(const char *who, int rank, int n, int x0, int nxl, const pf_peak_region *box, PfBackBox *b, unsigned long long *cells);
size_t pf_refresh_first_bad(const unsigned int *a, size_t upto, unsigned long long limit);
int pf_refresh_fields(const char *who, int rank, int pb, int shifts, const pf_product_layout *l, const pf_prev_layout *p, PfRefreshFields *f);
int pf_refresh_to_records(pf_ctx *c, const PfCtxView &v, const char *who, const PfRefreshScratch &s, size_t m, size_t count, void *frag, size_t stride,
                          const PfRefreshFields &f);
// ---- pf_plc.hip: the past-light-cone test of build_groups(); the context keeps one pointer for it and frees it in pf_destroy ----
void **pf_ctx_plc_slot(pf_ctx *c);
void pf_plc_release(void *state);
// ---- pf_catalog.hip: the halo catalogue and the mass function of an output; it reads the tables the light-cone state keeps ----
struct PfPlcTab;
bool pf_plc_tables(pf_ctx *c, PfPlcTab *tab, int *tab_doubles);   // false: no cosmology set
// ---- pf_census.hip: the census of the Fmax / Rmax columns of the two flavours of the solve (pf_flavour_census in pf_api.hip runs the sweeps) ----
// four columns of `count` cells on the device (pb bytes per Fmax) -> *out and the first min(outliers, capacity) records, both on the host
int pf_census_device(const char *who, int task, int pb, unsigned long long first_cell, size_t count, const void *fmax_fast, const int *rmax_fast,
                     const void *fmax_exact, const int *rmax_exact, pf_census *out, size_t capacity, pf_census_cell *cells, hipStream_t st);
// ---- pf_power.hip: power and smoothed variances of a resident spectrum; what it sees of a context (pf_api.hip) ----
// this rank's ky-slab of a spectrum: rows [kx][ky_local] of nzp complex (nzp = nzh on the general path), ky = y0 + ky_local
struct PfSpecView { const void *spec; int n, nzh, nzp, nyl, y0, fb, rank, P; hipStream_t stream; };
void pf_ctx_spec_geometry(pf_ctx *c, PfSpecView *v);   // everything but `spec`
// which: 0 delta(k), 1..3 the LPT source spectra, under the conditions of pf_get_density / pf_get_kvector (a pending x-transform of a
// source is finished first, as that export does); refuses with the message of `who`
int pf_ctx_spec_view(pf_ctx *c, const char *who, int which, PfSpecView *v);
int pf_ctx_allreduce(pf_ctx *c, void *buf_dev, size_t count, int is_u64);   // the installed pf_allreduce_fn on the context's stream
// the installed pf_alltoall_fn on the context's stream: block q of send_dev goes to rank q, block p of recv_dev comes from rank p
int pf_ctx_alltoall(pf_ctx *c, const void *send_dev, void *recv_dev, size_t bytes_per_peer);
int pf_ctx_exchange_installed(pf_ctx *c);   // one rank, or both an all-to-all and an all-reduce are installed
// the staging of the taps on a caller's spectra (pf_debug_power_spectrum, pf_debug_matter_shells): after the refusals of field_bytes,
// n, y0 and nyl, one or two ky-slabs [ky_local][kx][kz] of the host (b may be null) into `fields` fields in the production layout,
// rows of nzp complex, and `words` 64-bit words of scratch beside them (0: none); *d starts zeroed and frees what it holds
struct PfSpecStage { void *in, *spec[2]; unsigned long long *words; int nzp; ~PfSpecStage() { hipFree(in); hipFree(spec[0]); hipFree(words); } };
int pf_stage_spectra(const char *who, int field_bytes, int n, int y0, int nyl, int fields, const double *a, const double *b, size_t words, PfSpecStage *d);
// the shell sums of two resident spectra, |m|^2 and Re(m conj lin) (lin null: the first alone), of the rows y0 .. y0 + nyl - 1 ->
// this slab's sums on the device, or with coll (collective) the box's on every rank: nm ([nb] nmodes, [nb] k2sum) and out ([nb]
// power, [nb] cross).  words: pf_matter_shells_words(n, ranks of coll) of them, not yet cleared.  Nothing is synchronised
struct PfShellSums { const unsigned long long *nm; const double *out; int scans; };   // scans: the scan launches (pf_debug_matter_form)
size_t pf_matter_shells_words(int n, int P);
int pf_matter_shells_device(const char *who, int task, int fb, const void *spec_m, const void *spec_lin, int n, int y0, int nyl, long long pitch, int flags,
                            unsigned long long *words, unsigned long long *counters, pf_ctx *coll, PfShellSums *sums, hipStream_t st);
// the same sums weighted by the Legendre polynomials of the angle to axis `los` (pf_multipole_core.h), eleven positive sums per shell
// (five without lin), under the same collective scheme: nm as above, out ([3][nb] power, [3][nb] cross, [11][nb] the positive sums,
// each over N^6).  words: pf_multipole_shells_words(n, ranks of coll); scans: the scan launches.  What was launched is also kept for
// pf_debug_multipole_form
size_t pf_multipole_shells_words(int n, int P);
int pf_multipole_shells_device(const char *who, int task, int fb, const void *spec_m, const void *spec_lin, int n, int y0, int nyl, long long pitch, int flags, int los,
                               unsigned long long *words, unsigned long long *counters, pf_ctx *coll, PfShellSums *sums, hipStream_t st);
// ---- the two passes of pf_halo_correlation (pf_power.hip; pf_halo.hip calls them; pf_corr_core.h) ----
// the form pass on the rows y0 .. y0 + nyl - 1 of spec_m: out = ((F)(t / N^3), 0) per stored mode, t the auto term of matter_terms
// (which 0; spec_lin is not read) or its cross term with spec_lin (which 1), deconvolved by the table C (null: not; on the device,
// n/2 + 1 doubles: pf_corr_deconv_upload).  out may be spec_m: a mode is read and written by one lane.  The k = 0 mode is written as
// zero; so is a term that is not finite, which adds its weight to MC_NONFIN_MODES of `counters`.  Nothing is synchronised
int pf_corr_deconv_upload(const char *who, int task, int flags, int n, double *Cdev, const double **C, hipStream_t st);
int pf_corr_form_device(const char *who, int task, int fb, const void *spec_m, const void *spec_lin, void *out, int n, int y0, int nyl, long long pitch, const double *C,
                        int which, unsigned long long *counters, hipStream_t st);
// the shell sums of a real field in separation space, the planes x0 .. x0 + nxl - 1 of the box in rows of `pitch` reals: six positive
// sums per shell (pf_corr_core.h) -> this slab's sums on the device, or with coll (collective) the box's on every rank: nm ([nb]
// ncells, [nb] r2sum, then the limbs, then at nm[26 nb] the cells that are not finite) and out ([3][nb] xi = positive - negative,
// [6][nb] the positive sums).  words: pf_corr_shells_words(n, ranks of coll), not yet cleared.  Nothing is synchronised.  What was
// launched is also kept for pf_debug_corr_passes
size_t pf_corr_shells_words(int n, int P);
int pf_corr_shells_device(const char *who, int task, int fb, const void *real, int n, int x0, int nxl, long long pitch, int los, unsigned long long *words, pf_ctx *coll,
                          PfShellSums *sums, hipStream_t st);
// ---- pf_bispec.hip: the bispectrum of a spectrum on the device (pf_halo.hip calls it; pf_bispec_core.h) ----
#define PF_BISPEC_SLOTS 8   // copies of every counter of the passes: a workgroup adds to the copy of its index, one atomic per wave
enum { PF_BISPEC_PH_TRANSFORM = 0, PF_BISPEC_PH_MASK, PF_BISPEC_PH_KEEP, PF_BISPEC_PH_TRIPLES };   // what `mark` is told has just run
// this rank's ky-slab of the spectrum (rows of nzp complex) and x-slab of the real field (rows of rpitch reals)
struct PfBispecGeom { int n, fb, y0, nyl, x0, nxl, rank, P; long long nzp, rpitch; };
struct PfBispecBins { int kmin, dk, nk; };
// on the host: sums [nt] = positive - negative; parts [2][nt] the positive sums, pair [nk], maxima [nk], kmodes [nk] (each may be null)
struct PfBispecOut { double *sums, *parts, *pair, *maxima; unsigned long long *kmodes; unsigned long long nonfinite_modes, nonfinite_cells; };
int pf_bispec_check_bins(const char *who, int task, int kmin, int dk, int nk, int n);   // the refusals of the k-bins (n 0: not 3 kmax > n)
size_t pf_bispec_words(int kmin, int dk, int nk, int P);                                 // 64-bit words of tables a call needs
// the mask pass of k-bin `bin` on the rows y0 .. y0 + nyl - 1: spec -> out (another field of the same layout), kind 0 the data field,
// 1 the count field (spec null: nothing is read); counters: PF_BISPEC_SLOTS copies of (kmodes, modes that are not finite), cleared
int pf_bispec_mask_device(const char *who, int task, int fb, const void *spec, void *out, int n, int y0, int nyl, long long pitch, const double *C, int kind, int kmin, int dk,
                          int bin, unsigned long long *counters, hipStream_t st);
// the whole estimator on a spectrum that stands in a field of its own (spec; null with kind 1: the count fields): per k-bin the mask
// pass into `work` (the field of pf_ctx_matter_reverse_field), the context's reverse transform and the keep pass into store i of
// `stores` (nk times nxl n^2 elements of the field type); then the triple pass (the pair pass with out->pair) and the sums on the
// host, over the ranks of the context where it has several (collective).  words: pf_bispec_words of them.  Synchronises the stream
int pf_bispec_device(const char *who, int task, pf_ctx *c, const PfBispecGeom &g, const PfBispecBins &kb, const void *spec, int kind, const double *C, void *work, void *stores,
                     unsigned long long *words, void (*mark)(void *, int), void *user, PfBispecOut *out, hipStream_t st);
// counters of a pf_matter call on the device: PF_MATTER_SLOTS copies of each, a workgroup adds to the copy of its index -- one counter for all
// wavefronts of a 1024^3 call is 1.7e7 atomics on one address: the contrast pass took 778 ms that way and takes 8 (profiles/matter_notes.md);
// the copies are summed (MC_MAX: reduced) on the host.  The scans of pf_matter_shells_device add to MC_NONFIN_MODES of `counters`
#define PF_MATTER_SLOTS 1024
enum { MC_DEPOSITED = 0, MC_NONFINITE, MC_OUTSIDE, MC_EMPTY, MC_MAX, MC_SUMHI, MC_SUMLO, MC_NONFIN_MODES, MC_COUNT };
// ---- pf_matter.hip: the density of the displaced particles and its spectra; what it sees of a context beside the views above ----
// field: the scratch field of the transform taps (real rows of rpitch reals, then its spectrum in the layout of PfSpecView; with more
// than one rank that is receive field 0, the field pf_forward_transform uses there); x0: global x
// of the first local plane; lpt_order: the LPT order whose columns are computed (the others read zero)
struct PfMatterCtx { void *field; long long rpitch; int x0, lpt_order; };
void pf_ctx_matter_view(pf_ctx *c, PfMatterCtx *m);
int pf_ctx_matter_forward(pf_ctx *c);                 // the context's forward transform of that field, in place
int pf_ctx_matter_export(pf_ctx *c, double *host);    // its real rows -> [nxl][n][n] fp64 on the host (through the staging fields)
// the field the context's reverse transform works on in place (the field of pf_reverse_transform: A[0]; with one rank that is
// `field` above) and its bytes; the transform itself, spectrum -> real rows of rpitch reals times 1 / N^3.  With more than one rank
// it receives into receive field 0: `field` above is overwritten
void *pf_ctx_matter_reverse_field(pf_ctx *c, size_t *bytes);
int pf_ctx_matter_reverse(pf_ctx *c);
int pf_launch_block_vec3(const float *vel12, size_t ncell, int o, size_t first, size_t count, float *out, hipStream_t st);
int pf_launch_block_id(int id_bytes, unsigned long long global_first, size_t count, void *out, hipStream_t st);
int pf_launch_to_blocks(int field_bytes, const void *src, void *dst, int nxl, int n, int nyl, int nzp, int back, hipStream_t st);
int pf_launch_extract_dc(int field_bytes, const void *spec, double scale, double *out, hipStream_t st);

// ---- synthetic density (pf_synth.hip) ----
int pf_launch_white(int field_bytes, void *real, long long nrows, long long row0, int n, long long pitch,
                    uint64_t seed, hipStream_t st);
struct PfShapeParams {
  void *spec;            // internal layout, rows (x, y_local) of nzp complex
  int n, nzp, nyl, y0;   // y-slab
  double slope, scale;   // amplitude k^(slope/2) * scale ; scale applied only when apply != 0
  double *partials;      // per-block weighted sum |dk|^2
  int nblocks;
  int mode;              // 0: apply shape + accumulate power; 1: multiply by *dscale
  const double *dscale;
};
int pf_launch_shape(int field_bytes, const PfShapeParams &p, hipStream_t st);
int pf_launch_stream(int kind, const void *src, void *dst, size_t bytes, float *sink, hipStream_t st);  // 0 read, 1 write, 2 copy
int pf_launch_sigma_scale(const double *power_sum, double sigma0, double n3, double *dscale, hipStream_t st);

// ---- GenIC on the device (pf_genic.hip) ----
int pf_genic_launch(int field_bytes, void *dk, int n, int nzp, int nyl, int y0, const pf_genic_params *p, hipStream_t st,
                    unsigned int **seed_dev_out);
