/*
 * pinfmax.h -- C ABI of libpinfmax_hip.so, the MI355X (gfx950) implementation
 * of PINOCCHIO's collapse-time hot path (Fmax sweep + 2LPT/3LPT displacements).
 *
 * Plain C, plain pointers and sizes.  One context = one MPI rank = one GPU =
 * one x-slab of the grid, exactly the reference's 1-D PFFT decomposition
 * (src/initialization.c:1317-1325).  Every entry point names the reference
 * interface it replaces (file:line relative to the reference tree).  The
 * reference-side adapter that maps PINOCCHIO's globals onto these calls is
 * pinocchio_amd/host/pf_compat.c; INTEGRATION.md shows the link line.
 *
 * Conventions (src/pinocchio.c:259-263, src/fmax.c): every function returns
 * int, 0 = ok, non-zero = error after printing "ERROR on task %d: ..." on
 * stdout; the caller aborts (MPI_Abort).  All ranks call every function
 * collectively and in the same order (PFFT plans and reductions are collective
 * in the reference too).  Not thread-safe per context (MPI_THREAD_FUNNELED).
 * There is NO CPU fallback: without a HIP device pf_create fails.
 */
#ifndef PINFMAX_H
#define PINFMAX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PF_NBINS 210     /* NBINS, src/pinocchio.h:65 (spline knots, Fmax PDF bins) */
#define PF_MAX_SMOOTH 64 /* upper bound on Smoothing.Nsmooth accepted by pf_sweep */

typedef struct pf_ctx pf_ctx;

/* grid_data / FFT decomposition (src/pinocchio.h:295-308, src/fmax-pfft.c:80-134) */
typedef struct {
  int64_t n;        /* GSglobal[_x_] = [_y_] = [_z_] : cubic grid (the reference accepts any GridSize: src/fmax-pfft.c:139-188).
                       Power of two in 16..2048: the hand-written transform passes (any nranks, fp64 or fp32 fields).
                       n = 8 m, m = 2^a 3^b 5^c, up to 2048 (24, 40, 200, 384, 768, 1000, 1536 ...): the hand-written passes on
                       stage plans of radices 8, 5, 4, 3, 2 -- built into the kernels for 200, 384, 400, 640, 768, 800, 1000, 1280,
                       1536, 1600 and 2000 (the fast way: 768^3 runs at 0.84 of the per-cell rate of 1024^3), a run-time table for the
                       others -- any nranks (a power of two), fp64 or fp32 fields.  Any other even size in 4..2048: hand-written
                       chirp-z (Bluestein) transforms on the power-of-two stages, one per component, one rank and fp64 fields only
                       (csrc/pf_gfft.hip; no library transform anywhere).  pf_transform_path() says which */
  int     rank;     /* ThisTask */
  int     nranks;   /* NTasks; x-slabs, nranks must divide n (src/fmax-pfft.c:95-111 without the ragged last slab).  A power of two for n = 2^k; any
                       divisor that leaves slabs of two planes and more for n = 8 m that is not a power of two (96^3 on 3, 120^3 on 6, 200^3 on 5 ...) */
  int     device;   /* HIP device ordinal of this rank */
  int     field_bytes; /* 8: fp64 density/derivative fields (reference); 4: fp32 fields, fp64 collapse solve */
  int     flags;    /* PF_FLAG_* */
} pf_config;

#define PF_FLAG_TIMING 1  /* record per-kernel HIP-event timings (pf_kernel_stats) */
/* Environment, read once per context in pf_create (DESIGN.md section 6 has the whole table).  One of them changes what is computed:
   PF_EXACT_LIBM=1 makes the collapse solve call the reference's own libm functions (cos x3, acos, pow, pow, log10, exp, IEEE / and sqrt)
   instead of the series / table / hardware-seeded forms of the default arithmetic.  It is a DIAGNOSTIC mode -- the flavour in which
   the oracle's solver fed with the device's Hessian reproduces the device's Fmax bit for bit (tests) -- not a supported speed: 1.6x the
   step time, kernels with scratch, never tuned or profiled. */
/* a -DDOUBLE_PRECISION_PRODUCTS build (src/Makefile:68, src/pinocchio.h:219-225: PRODFLOAT double): Fmax and the Vel*
   fields of product_data are doubles.  Fmax is then kept and compared in fp64 (no rounding of the running maximum to fp32
   between radii, cf. src/collapse_times.c:587-590) and the displacements leave the z-pass as the doubles it computes.
   fp64 fields only.  pf_get_products / pf_update_products write doubles at the layout's offsets; pf_select_sorted and
   pf_get_block (fp32 by definition) refuse. */
#define PF_FLAG_DOUBLE_PRODUCTS 2

/* layout of the caller's product_data record (src/pinocchio.h:233-259).
   Offsets in bytes; a negative offset means "field absent".  pf_layout_3lpt()
   fills the -DTWO_LPT -DTHREE_LPT float layout (56 B). */
typedef struct {
  size_t stride;     /* sizeof(product_data) */
  int    off_Rmax, off_Fmax, off_Vel, off_Vel_2LPT, off_Vel_3LPT_1, off_Vel_3LPT_2;
} pf_product_layout;
void pf_layout_3lpt(pf_product_layout *l);

/* cputime_data (src/pinocchio.h:368-378), seconds, device time by HIP events.  fmax, deriv, coll, lpt are spans between events
   on the streams the phases run on.  In a sweep whose collapse passes ran beside the z-passes of the following radii (the
   default, pf_solve_ran_beside_zpass) `coll` is what they add to the sweep beyond the derivative passes, so that
   deriv + coll <= fmax as in the reference's report (src/fmax.c:160-170); with every kernel in line (PF_SOLVE_BESIDE_Z=0)
   both are the plain spans. */
typedef struct {
  double fmax, deriv, fft, coll, lpt, mem_transf;
} pf_cputime;

/* Device memory a context of this configuration holds, in bytes: *at_create by pf_create itself, *peak once a sweep and the LPT part
   have run (the second field set is allocated at first use).  pf_create compares *peak with the free memory of the device
   (hipMemGetInfo) BEFORE allocating anything and fails in the usual format when it does not fit (PF_PREFLIGHT=0: no check).  The
   host's counterpart of the memory report of src/allocations.c:60-160.  Needs no device.  Not in the plan: the columns that come
   into being at first use -- zacc / group_ID of the back calls, and the twelve Vel*_prev columns of pf_shift_displacements, 48
   bytes per cell (96 with double products) until pf_drop_prev. */
int pf_plan_bytes(const pf_config *cfg, size_t *at_create, size_t *peak);

/* --- life cycle: replaces set_one_grid + compute_fft_plans + the FFT-buffer
       part of allocate_main_memory (src/fmax-pfft.c:80-188, src/allocations.c:382) --- */
int  pf_create(pf_ctx **out, const pf_config *cfg);
/* finalize_fft (src/fmax-pfft.c:231-252) + release of all device memory */
int  pf_destroy(pf_ctx *ctx);
const char *pf_last_error(void);

/* --- multi-GPU exchange (replaces the MPI_Alltoall inside pfft_execute,
       src/fmax-pfft.c:197,211).  One all-to-all per 3-D FFT: every rank sends
       bytes_per_peer bytes from sendbuf + q*bytes_per_peer to rank q and
       receives into recvbuf + p*bytes_per_peer from rank p, ordered on `stream`
       (a hipStream_t).  Install either a callback or the built-in RCCL
       exchange (grouped ncclSend/ncclRecv) created from a broadcast
       ncclUniqueId (128 bytes).  Not needed when nranks == 1. --- */
typedef int (*pf_alltoall_fn)(void *user, const void *sendbuf, void *recvbuf,
                              size_t bytes_per_peer, void *stream);
int pf_set_exchange(pf_ctx *ctx, pf_alltoall_fn fn, void *user);
/* Optional companion for band-limited spectra (smoothing radii whose Gaussian window is below 2^-60 beyond |k| = band):
   of each of the P blocks only one row range carries data.  Rank r sends send_bytes bytes from
   sendbuf + q*block_bytes + send_off to every rank q (nothing when send_bytes == 0) and receives recv_bytes[p] bytes into
   recvbuf + p*block_bytes + recv_off[p] from every rank p.  Without it the full blocks go through pf_alltoall_fn. */
typedef int (*pf_alltoallv_fn)(void *user, const void *sendbuf, void *recvbuf, size_t block_bytes, size_t send_off,
                               size_t send_bytes, const size_t *recv_off, const size_t *recv_bytes, void *stream);
int pf_set_exchange_rows(pf_ctx *ctx, pf_alltoallv_fn fn, void *user);
int pf_rccl_available(void);                        /* 1 when librccl can be bound in this process (host side only: no
                                                       communicator, no collective -- what the ranks vote on before any of them
                                                       enters ncclCommInitRank) */
#define PF_RCCL_ID_BYTES 128                         /* sizeof(ncclUniqueId); checked at build time against rccl.h */
int pf_rccl_unique_id(void *id128);                 /* rank 0: ncclGetUniqueId */
int pf_init_rccl(pf_ctx *ctx, const void *id128);   /* all ranks: ncclCommInitRank; the context owns the communicator */
/* version code of the RCCL bound at run time (0: none bound); *build_code: NCCL_VERSION_CODE of the header the library was built
   against.  Binding refuses a run-time library of another major version (types and enumerators come from that header). */
int pf_rccl_version(int *build_code);
int pf_release_rccl(pf_ctx *ctx);                   /* ncclCommDestroy + callbacks cleared (also done by pf_destroy) */
int pf_rccl_comm_count(pf_ctx *ctx);                /* ncclCommCount of the built-in exchange's communicator: the number of ranks
                                                       RCCL itself sees (the MPI_Comm_size of FFT_Comm, src/initialization.c:1317);
                                                       0 when the built-in exchange is not installed, -1 on error */
/* small reductions (MPI_Reduce/MPI_Bcast at src/collapse_times.c:656-667,
   src/fmax.c:527): sum `count` doubles / uint64 in place over all ranks */
typedef int (*pf_allreduce_fn)(void *user, void *buf, size_t count, int is_u64, void *stream);
int pf_set_allreduce(pf_ctx *ctx, pf_allreduce_fn fn, void *user);
/* in-process fabric: P contexts (ranks 0..P-1) driven by P host threads on ONE GPU meet in the
   exchange through device-to-device copies.  Bring-up/test transport for the slab code path on a
   single-GPU box; multi-GPU runs use pf_init_rccl. */
typedef struct pf_fabric pf_fabric;
pf_fabric *pf_fabric_create(int nranks);
void pf_fabric_destroy(pf_fabric *f);
int pf_fabric_attach(pf_fabric *f, pf_ctx *ctx);
/* test knob: every all-to-all first idles its stream for that long, so that the copies land late and anything the
   pipelined exchange fails to wait for reads stale data */
int pf_fabric_set_delay(pf_fabric *f, int microseconds);
/* self-test of the installed exchange (pattern through the all-to-all and the all-reduce), any nranks >= 1 */
int pf_debug_exchange(pf_ctx *ctx, size_t bytes_per_peer);
/* Measurement aid: ONE rank of an nranks-rank decomposition on its own.  The all-to-all hands this rank's own blocks back to it
   (copied for the first `copies` calls, so that the receive buffers hold finite, field-like numbers; afterwards nothing moves) and
   the all-reduce leaves the rank's contribution.  The kernels then run on the rank's slab of the full-size box with the launch
   geometry of the real run; the results are NOT those of the box.  Used by `bench.py --slab-of P` to time the compute side of a
   configuration whose box does not fit one GPU (BASELINE config 5: 2048^3 with fp32 fields on eight GPUs). */
int pf_set_loopback_exchange(pf_ctx *ctx, int copies);   /* refused when a real exchange (RCCL, callbacks, fabric) is installed */
/* ... with ONE exception, which is how a configuration that fits no single GPU is CHECKED rank by rank on one (BASELINE config 5,
   tests/test_gpu_config5.py): a context that keeps the whole spectrum (PF_REPLICATE_DK=1) and whose density came from
   pf_genic_density -- a function of (seed, cosmology) alone -- generates every rank's slab of delta(k) itself; the sweep of such a
   context exchanges nothing, so its Fmax / Rmax / variance contributions / histogram ARE those of this rank's slab of the box.
   (The LPT part still transposes the source spectra: its displacements behind a loopback are no box's.) */
int pf_loopback_active(pf_ctx *ctx);                      /* 1 when the loopback stands in for the exchange (results are no box's) */
/* device pointers + size (bytes) of the exchange buffers, so that a host
   harness can wrap them (e.g. torch tensors for torch.distributed) */
int pf_exchange_buffers(pf_ctx *ctx, void **sendbuf, void **recvbuf, size_t *bytes);
/* stream the work is enqueued on (hipStream_t); pf_set_stream adopts a caller stream.  Two internal streams run beside it, ordered
   against it by events and joined before an entry point returns: the communication stream of a pipelined multi-rank run and the
   solve stream of a sweep (the collapse solve of radius i beside the z-pass of radius i + 1: the default with fp32 fields, PF_SOLVE_BESIDE_Z=1
   with fp64 fields, where it gains nothing since round 5; PF_SOLVE_BESIDE_Z=0: every kernel in line).  What
   follows an entry point on this stream sees all of its results. */
int pf_set_stream(pf_ctx *ctx, void *stream);
void *pf_get_stream(pf_ctx *ctx);

/* --- inputs --- */
/* kdensity[0] (src/fmax-pfft.c:366): this rank's x-slab of the half-spectrum,
   fp64 [n/nranks][n][n/2+1][2], pre-multiplied by N^3 (src/GenIC.c:430-445).
   host pointer; uploaded (and converted to fp32 when field_bytes == 4). */
int pf_set_density(pf_ctx *ctx, const double *kdensity_slab);
/* params.use_transposed_fft (PFFT_TRANSPOSED_OUT on slabs, src/fmax-pfft.c:92, 271-281): with on != 0 every spectrum that
   crosses this interface -- pf_set_density, pf_get_density, pf_get_kvector, pf_forward_transform (out),
   pf_reverse_transform / pf_derivative (in) -- is this rank's KY-slab in the memory order [ky_local][kx][kz][2]
   (ky_local = n/nranks rows starting at rank * n/nranks) instead of the kx-slab [kx_local][ky][kz][2].  The device
   layout is a ky-slab anyway, so the regrouping all-to-all of the non-transposed boundary disappears.  Call it right
   after pf_create; results do not depend on it. */
int pf_set_transposed_spectra(pf_ctx *ctx, int on);
/* 1 if this context (nranks > 1) keeps the whole delta(k) on every rank, so that the second derivatives of the sweep and
   the Zel'dovich displacements need no all-to-all (each rank transforms every x-line and stores its own slab): chosen at
   pf_create -- up to four ranks, or PF_REPLICATE_DK=0|1.  Results do not depend on it. */
int pf_replicated_spectrum(pf_ctx *ctx);
/* synthetic delta(k) generated in HBM (bench / large property tests):
   Philox-4x32 white noise, P(k) ~ k^slope inside the Nyquist sphere, DC and
   Nyquist planes zero, sigma(R=0) = sigma0.  numpy mirror:
   pinocchio_amd/synth.py philox_density. */
int pf_synth_density(pf_ctx *ctx, uint64_t seed, double sigma0, double slope);
/* GenIC_large (src/GenIC.c:73-460) on the device: PINOCCHIO's own Gaussian initial conditions generated straight
   into HBM -- one gsl_rng_ranlxd1 stream per (kx,ky) column seeded from the MT19937 seed plane along the spiral
   (src/GenIC.c:840-990), Eisenstein & Hu P(k) (src/cosmo.c:1443-1497) times PkNorm, Hermitian kz = 0 plane, Nyquist
   planes and DC zero, final factor N^3.  Replaces GenIC + pf_set_density (no host array, no 8.6 GB upload at 1024^3);
   every rank generates its own k-space slab.  BoxSize in true Mpc (params.BoxSize_htrue), PkNorm as printed by
   normalize_PowerSpectrum (src/cosmo.c:1058-1075) or from pf_pk_norm (sigma8^2 / top-hat variance at 8/h Mpc). */
typedef struct {
  double Omega0, OmegaBaryon, Hubble100, PrimordialIndex;
  double BoxSize_true_Mpc;
  double PkNorm;
  unsigned int RandomSeed;
  int FixedIC;    /* params.FixedIC: "non-random modules of the Fourier modes", no Rayleigh factor -log(ampl) (src/GenIC.c:375) */
  int PairedIC;   /* params.PairedIC: every phase shifted by pi (src/GenIC.c:371) */
  /* pk_n > 0: a tabulated spectrum instead of Eisenstein & Hu (FileWithInputSpectrum <file> or CAMBTable: WhichSpectrum 2 / 5) --
     P(k) = PkNorm 10^my_spline_eval(SPLINE[SP_PK], log10 k) / k^3 (PowerSpec_Tabulated, src/cosmo.c:1432-1435) with the knots of
     SPLINE[SP_PK]: pk_logk[i] = log10 k [true 1/Mpc], pk_logk3p[i] = log10(k^3 P) (read_Pk_from_file :1099-1170,
     read_Pk_table_from_CAMB :1290-1330); host arrays, copied.  The cosmology fields are then unused. */
  int pk_n;
  const double *pk_logk, *pk_logk3p;
  /* the other forms of PowerSpectrum() (src/cosmo.c:953-1007).  spectrum: 0 = by pk_n as above (Eisenstein & Hu or the table);
     3 = the Efstathiou fit (FileWithInputSpectrum "Efstathiou": PowerSpec_Efstathiou :1437-1440, Gamma = SHAPE_EFST = 0.21);
     4 = a power law k^PrimordialIndex ("PowerLaw", :1442-1445).  WDM_PartMass_in_kev > 0: every form is multiplied by the
     warm-dark-matter cut-off Tf^2 of Bode, Ostriker & Turok (:987-1005; needs Omega0, OmegaBaryon, Hubble100);
     UnitLength_in_cm: the reference's global of that name (0 = its default 3.085678e24, i.e. Mpc) */
  int spectrum;
  double WDM_PartMass_in_kev, UnitLength_in_cm;
} pf_genic_params;
int pf_pk_norm(const pf_genic_params *p, double sigma8, double *pknorm);
int pf_genic_density(pf_ctx *ctx, const pf_genic_params *p);
/* SPLINE[SP_INVGROW] knots (src/cosmo.c:401): x = log10 D, y = log10 a, n knots
   (natural cubic spline coefficients are computed on the host, GSL cspline).
   ismooth = -1: one spline for every radius (non SCALE_DEPENDENT build);
   ismooth >= 0: SPLINE_INVGROW[ismooth] (src/initialization.c:1704-1708). */
int pf_set_invgrow(pf_ctx *ctx, int ismooth, const double *x, const double *y, int n);
/* growth multipliers applied by compute_derivative when ScaleDep.order = 1..4
   (src/fmax-pfft.c:344-364): g[0]=GrowingMode, g[1]=GrowingMode_2LPT,
   g[2]=GrowingMode_3LPT_1 (carrying its minus sign, src/cosmo.c:1810),
   g[3]=GrowingMode_3LPT_2, all at the target redshift, scale-independent. */
int pf_set_growth(pf_ctx *ctx, const double g[4]);
/* SCALE_DEPENDENT build: the multiplier of ScaleDep.order = order (1..4) depends on |k| --
   GrowingMode*(z, k_module) = sign * pow(10., InterpolateGrowth(z, k, SP_GROW*)) (src/cosmo.c:1728-1755, 1789-1819),
   log-linear between nk k-bins at 10^(logkmin + j dlogk) (NkBINS = 10, LOGKMIN = -3, DELTALOGK = 0.5,
   src/def_splines.h:40-42).  log10_growth[j] = my_spline_eval(SPLINE[SP_GROW* + j], -log10(1+z)) evaluated by the
   caller at the target redshift; sign = -1 for order 3 (src/cosmo.c:1810).  |k| is taken in rad/cell exactly as
   compute_derivative passes it (src/fmax-pfft.c:315-359).  nk = 0 returns to the scalar of pf_set_growth. */
int pf_set_growth_table(pf_ctx *ctx, int order, const double *log10_growth, int nk, double logkmin, double dlogk, double sign);

/* TABULATED_CT build (src/collapse_times.c:780-1231, the BILINEAR_SPLINE interpolation of :40): per smoothing radius
   a table of ell() on 100 x 50 x 50 nodes in (delta, x, y) = (l1+l2+l3, l1-l2, l2-l3) / sqrt(Smoothing.Variance[ismooth])
   and one natural cubic spline in delta per (x, y) node; the per-cell pass then interpolates instead of solving.
   pf_set_tabulated_ct(ns, Smoothing.Variance): pf_sweep builds the table of each radius right before its
   collapse-time pass (src/fmax.c:103-106); ns = 0 returns to the direct solve.
   pf_ct_build = initialize_collapse_times(ismooth, .) alone: the table is computed on the device (with the
   inverse-growth spline of that radius) and, if table_host is not NULL, copied out as CT_table
   [iy][ix][id] (100*50*50 doubles, what the reference writes to its CTtable file);
   pf_ct_load installs a table read from such a file (params.CTtableFile) instead of computing it.
   A following pf_collapse_times(ismooth) uses the table in place. */
int pf_set_tabulated_ct(pf_ctx *ctx, int nsmooth, const double *variance);
/* How the collapse pass reads the table (interpolate_collapse_time, src/collapse_times.c:1139-1231): 0 = BILINEAR_SPLINE, the
   source's own define (default); 1 = a build with -DTRILINEAR (eight table entries, no splines); 2 = -DALL_SPLINE (sixteen
   node splines, then gsl_spline2d's bicubic on the 4 x 4 grid around the cell) -- the three options of
   tests/Readme_Pinocchio_tests_V5_1.txt.  The table and its file are the same for all three. */
int pf_set_ct_interpolation(pf_ctx *ctx, int flavour);
/* What fills the table: model 0 = ELL_CLASSIC (ell_classic + InverseGrowingMode, src/collapse_times.c:114-221, 404-415);
   model 1 = ELL_SNG (src/collapse_times.c:222-400, 416-426): per node one adaptive RKF45 integration of the
   nine-equation system of Nadkarni-Ghosh & Singhal (2016) -- the step, error control and accept/reject logic of
   gsl_odeiv2_step_rkf45 / control_standard_new(1e-6, 1e-6, 1, 1) / evolve_apply -- with
   cosmo = {Omega0, OmegaLambda, OmegaRad, OmegaK} for OmegaMatter(z) / OmegaLambda(z) (src/cosmo.c:1675-1718) and
   D_in[ismooth] = GrowingMode(1/1e-5 - 1, k of the radius) (:353-361).  With pf_set_tabulated_ct the model fills the
   table (250 000 integrations per radius); without it -- a reference build with -DELL_SNG and no -DTABULATED_CT -- every
   cell integrates its own ellipsoid in the collapse pass (k_collapse_sng: correct, and ~10^3 times the work of the table
   at 1024^3).  pf_set_modified_gravity adds the MOD_GRAV_FR force modification. */
int pf_set_collapse_model(pf_ctx *ctx, int model, const double cosmo[4], int nsmooth, const double *D_in);
/* -DMOD_GRAV_FR on top of ELL_SNG: the force in the velocity equations is enhanced by 1 + ForceModification(size, a, delta)
   (src/collapse_times.c:271-273, 295-312), Hu-Sawicki f(R) with |f_R0| = fr0 (the FR0 of the build; 0 switches it off),
   h_over_c = 100 / c[km/s] (src/cosmo.c:109), size[ismooth] = the ODE parameter of that radius: Smoothing.Radius[ismooth],
   and Smoothing.Radius[ismooth-1] for the last one (:378-388). */
int pf_set_modified_gravity(pf_ctx *ctx, double fr0, double h_over_c, int nsmooth, const double *size);
int pf_ct_build(pf_ctx *ctx, int ismooth, double variance, double *table_host);
int pf_ct_load(pf_ctx *ctx, int ismooth, double variance, const double *table_host);

/* --- the path --- */
/* compute_fmax's radius loop (src/fmax.c:66-150): for each radius (CELL units,
   Rsmooth = Radius/CellSize, src/fmax.c:233) second derivatives + collapse
   times; Smoothing.TrueVariance[0..ns-1] out (src/collapse_times.c:670). */
int pf_sweep(pf_ctx *ctx, int ns, const double *radius_cells, double *true_variance);
/* The reference chooses the order of the displacements at compile time (src/Makefile: -DTWO_LPT, -DTHREE_LPT;
   src/fmax.c:300-336, src/LPT.c:30, 78, 113, 214).  order 3 (default): both; 2: -DTWO_LPT alone -- the 2LPT source and its
   displacement, no 3LPT sources, no Hessian of the 2LPT potential; 1: neither -- Zel'dovich displacements only, no second
   derivatives on re-entry.  Columns of orders that are not computed are zero (their fields do not exist in such a build's
   product_data: give them negative offsets in pf_product_layout). */
int pf_set_lpt_order(pf_ctx *ctx, int order);
/* compute_fmax goes straight from the last radius to compute_displacements(1, 0, z) (src/fmax.c:150-163): with on != 0 the
   collapse pass of the last radius of every following pf_sweep also writes the 2LPT / 3LPT sources of src/LPT.c:64-93
   from the six components it holds, and the next pf_displacements(1, 0) starts from them instead of reading the six
   fields again (same arithmetic, same sums: results do not change).  Off by default: a sweep that is not followed by
   the displacements would write three fields for nothing. */
int pf_set_sources_in_sweep(pf_ctx *ctx, int on);
/* compute_second_derivatives (src/fmax.c:225-258): six Hessian fields at one radius */
int pf_second_derivatives(pf_ctx *ctx, double radius_cells);
/* compute_collapse_times (src/collapse_times.c:431-673) on the resident Hessian */
int pf_collapse_times(pf_ctx *ctx, int ismooth, double *true_variance);
/* compute_displacements(compute_sources, recompute_sd, z) (src/fmax.c:292-367):
   2LPT/3LPT sources + 12 displacement fields; growth from pf_set_growth.
   With compute_sources = 0 the resident LPT spectra are reused
   (RECOMPUTE_DISPLACEMENTS re-entry, src/fragment.c:398-410). */
int pf_displacements(pf_ctx *ctx, int compute_sources, int recompute_sd);
/* Fmax_PDF (src/fmax.c:509-550): 210-bin histogram of (int)(Fmax*10), summed over ranks */
int pf_fmax_pdf(pf_ctx *ctx, unsigned long long hist[PF_NBINS]);

/* --- outputs --- */
/* products[] of this rank's slab into the caller's AoS (host), index
   i = z + n*(y + n*x_local) (src/pinocchio.h:84-85) */
int pf_get_products(pf_ctx *ctx, void *products_host, const pf_product_layout *layout);
/* the same columns merged into records the caller already holds: bytes of the record not named by a
   non-negative offset keep their host value (Fmax/Rmax, the *_prev copies of a RECOMPUTE_DISPLACEMENTS
   build filled by shift_all_displacements, src/fragment.c:832-850).  Used after a re-entrant
   compute_displacements(0, 0, z) (src/fragment.c:398-410), which rewrites only the Vel* fields. */
int pf_update_products(pf_ctx *ctx, void *products_host, const pf_product_layout *layout);
/* First stage of fragmentation on the device: the cells of this rank's slab with Fmax >= flast (update_distmap,
   src/distribute.c:695) in order of descending Fmax (sort_and_organize, src/fragment.c:484-503; index_compare_F
   :118-126; equal keys, which qsort leaves unspecified, by ascending index).  cell_index = z + n*(y + n*x_local)
   (src/pinocchio.h:84-85).  *count receives the number selected; the first min(*count, capacity) entries are
   copied (either array may be NULL). */
int pf_select_sorted(pf_ctx *ctx, float flast, size_t capacity, unsigned int *cell_index, float *fmax, size_t *count);
/* The next step of fragmentation on the device: count_peaks (src/fragment.c:605-706, default non-CLASSIC_FRAGMENTATION form).
   A cell is stored when Fmax >= flast (a double, as outputs.Flast; src/distribute.c:695); a stored cell is a peak when its
   Fmax is strictly larger than that of each of its six grid neighbours that is stored too (two equal neighbours are both no
   peak; NaN is never stored and vetoes nothing).  Region: a sub-box start[3], len[3] in global grid coordinates (x, y, z;
   wrapping around the periodic box) with the safety layer safe[3] of the reference's subbox.  A direction with len == n is
   periodic (subbox.pbc); in any other the two border layers are skipped (:630-635).  Well resolved: safe[d] <= i_d <
   len[d] - safe[d] in the region's own coordinates (:691-694). */
typedef struct { int start[3], len[3], safe[3]; } pf_peak_region;   /* NULL = the whole periodic box */
/* peaks[0] = all peaks of the region, peaks[1] = those in its well resolved part, summed over ranks (the reference logs
   "Task %d found %d peaks, %d in the well resolved region").  Slabs: the planes next to the slab come from the neighbouring
   ranks through the installed pf_alltoall_fn (a block of two planes per peer), the sums through pf_allreduce_fn.
   Collective: every rank passes the same flast and region.
   Products of either precision. */
int pf_count_peaks(pf_ctx *ctx, double flast, const pf_peak_region *region, unsigned long long peaks[2]);
/* this rank's peaks of the whole box in index_compare_F order (the order in which fragmentation opens the groups);
   conventions of pf_select_sorted (local cell index, *count, capacity); fp32 products only */
int pf_select_peaks(pf_ctx *ctx, double flast, size_t capacity, unsigned int *cell_index, float *fmax, size_t *count);
/* test tap without a context: the same kernel on a caller's n^3 fp32 field (host, index z + n*(y + n*x)) */
int pf_debug_peaks(int n, const float *fmax_host, double flast, const pf_peak_region *region, unsigned long long peaks[2]);
/* The step between the two on the device: distribute() (src/distribute.c:58-175), which moves the product records from the FFT
   slabs to the fragmentation sub-boxes.  pf_distribute gives THIS RANK'S CONTRIBUTION TO ONE TARGET SUB-BOX: what keep_data()
   (:547-600) stores when the target is the rank itself and what send_data() (:300-416) puts on the wire otherwise.
   sub = subbox.stabl (may be negative; any start is reduced to the periodic box) and subbox.Lgwbl of the TARGET.
   Region and order: the cells of intersection(my_fft_box, sub) (:178-297; the x-slab spans y and z) -- up to eight boxes when the
   sub-box wraps, in the order intersection() emits them, and within a box by ascending i of INDEX_TO_COORD(i, ., ., ., box + 3)
   (src/pinocchio.h:84, z fastest).
   Selection: a cell is taken when the bit subbox_space_index(i, box) (:627-645) of `map` is set (host; UINTLEN = 32 bits per
   word, bit p % 32 of word p / 32, prod(len) bits: frag_map_update / frag_map through build_distmap, :670-682; NULL = every bit
   set) and (double)Fmax >= flast (update_distmap, :685-698).  NaN is never taken.
   Output: every taken cell appends one record in the caller's layout to `frag` -- the conventions of pf_get_products; bytes no
   non-negative offset names are zero (the *_prev fields of a RECOMPUTE_DISPLACEMENTS build among them: pf_refresh_velocities
   fills those); stride and offsets are
   multiples of four -- and its sub-box-space index to `frag_pos`.  *count receives the number taken; the first
   min(*count, capacity) entries are copied, counting goes on beyond capacity as frag_offset does (:586-592).  frag and frag_pos
   may each be NULL (both: a count-only call).  A sub-box that misses the slab gives *count = 0.
   Needs the products of a sweep.  NOT collective and nothing goes through the exchange callbacks: the caller owns the transport
   that carries a contribution to the sub-box's owner, and concatenates the contributions in distribute()'s order -- its own
   first, then those of the hypercube loop (:109-148) -- to get the reference's frag[] / frag_pos[].  INTEGRATION.md has the loop. */
typedef struct { int start[3], len[3]; } pf_subbox;
int pf_distribute(pf_ctx *ctx, double flast, const pf_subbox *sub, const unsigned int *map, const pf_product_layout *layout,
                  size_t capacity, void *frag, unsigned int *frag_pos, size_t *count);
/* test tap without a context: the selection and ordering kernels on a caller's slab of an fp32 field -- planes x0 .. x0 + nxl - 1
   of an n^3 box, host, index z + n*(y + n*x_local); returns frag_pos and the local cell index of each taken cell.  n <= 2048; the
   sub-box has at most 2^32 cells (frag_pos is 32-bit) and so has the slab: cell_index is 32-bit and holds the indices 0 .. 2^32 - 1,
   the limit pf_group_velocity_sums sets for its keys (a slab of exactly 2^32 cells is accepted by both, one of 2^32 + 1 by neither) */
int pf_debug_distribute(int n, int x0, int nxl, const float *fmax_host, double flast, const pf_subbox *sub, const unsigned int *map,
                        size_t capacity, unsigned int *frag_pos, unsigned int *cell_index, size_t *count);
/* The call of fragment() (src/fragment.c:193-346) that follows distribute(): sort_and_organize() (:484-520).  The reference sorts
   an index array by descending Fmax (index_compare_F, :118-126), moves frag[] and frag_pos[] into that order (reorder, :533-564),
   sorts again by frag_pos (index_compare_P, :128-136) and leaves sorted_pos[] / indices[] for find_location() (:592-603).  State
   after it over N records: frag[i].Fmax non-increasing; sorted_pos[p] = frag_pos[indices[p]] strictly ascending (frag_pos is
   unique within a sub-box; equal positions, which only a caller of pf_organize can supply, keep their order).  qsort leaves the
   order of equal Fmax unspecified: here, as in pf_select_sorted, ties keep the order of the input (distribute()'s), -0.0 ties
   with +0.0, and NaN -- which pf_distribute never stores -- goes last, after -inf.
   pf_distribute_sorted = distribute() + sort_and_organize() for this rank's contribution to one target sub-box, straight from the
   columns: selection, map, layout, zero-fill and *count / capacity as pf_distribute; frag / frag_pos receive the first
   min(*count, capacity) records of the SORTED order and sorted_pos / indices describe exactly those records.  Any output may be
   NULL.  When this rank is the only contributor (one rank; or a sub-box inside its own slab) the four arrays are the
   reference's state after sort_and_organize().  2^31 records or more are refused: indices is int as in the reference. */
int pf_distribute_sorted(pf_ctx *ctx, double flast, const pf_subbox *sub, const unsigned int *map, const pf_product_layout *layout,
                         size_t capacity, void *frag, unsigned int *frag_pos, unsigned int *sorted_pos, int *indices, size_t *count);
/* sort_and_organize() (src/fragment.c:484-520) on arrays the caller already holds -- the contributions of several ranks to one
   sub-box, concatenated in distribute()'s order: frag (records of layout->stride bytes, Fmax of the context's precision at
   layout->off_Fmax >= 0) and frag_pos are reordered in place; sorted_pos / indices (each may be NULL) as above.  The records
   travel to one device buffer of count * stride bytes and back in the hand-off pieces; when that buffer and the sort's scratch
   cannot be allocated the call fails, says how many bytes it needs and has touched nothing. */
int pf_organize(pf_ctx *ctx, const pf_product_layout *layout, size_t count, void *frag, unsigned int *frag_pos,
                unsigned int *sorted_pos, int *indices);
/* test tap without a context: the ordering alone (index_compare_F then index_compare_P, src/fragment.c:118-136) on a caller's fp32
   Fmax and frag_pos; order[i] = input index of record i of the sorted order */
int pf_debug_organize(size_t count, const float *fmax, const unsigned int *frag_pos,
                      unsigned int *order /* new -> old */, unsigned int *sorted_pos, int *indices);
/* The maps of fragment() (src/fragment.c:193-346) on the device: frag_map and frag_map_update as ONE resident object, so that the
   two-turn loop of the default (non-CLASSIC_FRAGMENTATION) build uploads no map and builds none on the host.  A pf_map holds two
   bit arrays of pf_map_length() = subbox.maplength = ceil(Lx Ly Lz / 32) words over box->len = subbox.Lgwbl: CURRENT (frag_map)
   and UPDATE (frag_map_update), both zero after pf_map_create.  Bit pos = z + Lz (y + Ly x) (COORD_TO_INDEX, UINTLEN = 32) is
   bit pos & 31 of word pos >> 5; the unused bits of the last word stay zero through every call.
   pf_map_create: box = subbox.stabl, subbox.Lgwbl, subbox.safe.  With a context a direction is periodic (subbox.pbc) when
   len[d] == n, the map lives on the context's device and every call is ordered on the context's stream; ctx may be NULL
   (context-free: current device, default stream; such a map serves the pf_map_* calls only) and a direction is then periodic
   when safe[d] == 0.  Refused: len[d] outside [1, n] (2048 without a context); more than 2^32 cells; safe[d] < 1 (or 2 safe >
   len) in a direction that is not periodic -- create_map() would start at safe - 1 = -1 --; safe[d] != 0 in a periodic one.
   pf_map_fill_box = create_map() (:708-751): UPDATE := zero, then per direction the range [safe - 1, Lgrid + safe + 1) with
   Lgrid = len - 2 safe, [0, len) when periodic: the well resolved region plus one layer.
   pf_map_update = update_map() (src/build_groups.c:2246-2318) over the groups the caller passes (FILAMENT + 1 .. ngroups - 1 of
   the quick catalogue): pos[3 g ..] = groups[].Pos in sub-box coordinates, mass[g] = groups[].Mass.  UPDATE := zero; for every
   group c = (int)(pos + 0.5) and size = (int)(boundary_layer_factor * pow((double)mass / 4.188790205, 0.333333333333333) + 0.5)
   are computed on the HOST with the reference's own libm calls, and the cube [c - size, c + size)^3 is visited: a coordinate
   outside [0, len) wraps ONCE in a periodic direction, otherwise the cell counts into nadd[1] and is skipped -- before the sphere
   test, so nadd[1] counts cells of the cube, not of the sphere; a cell whose CURRENT bit is clear and whose unwrapped offset has
   rr <= size^2 gets its UPDATE bit and counts into nadd[0].  nadd[0] counts WITH MULTIPLICITY: a cell that two spheres cover
   counts twice, because the test reads frag_map and not frag_map_update.  (The log lines "Requesting %Ld particles from the
   boundary layer" / "... lie beyond the boundary layer".)  The counts are 64-bit; the reference's unsigned int nadd[] wraps at
   2^32.  ngroups = 0 is valid.  Refused, with nothing changed: in a periodic direction a group with size > len[d] or c outside
   [0, len[d]] (the reference indexes out of bounds after its single wrap); a size beyond 16384; a position that is no number.
   Words and counts do not depend on the schedule (bitwise reproducible).  PF_MAP_WORDS=0, read by pf_map_create, selects the
   one-atomic-per-bit form of the kernel for that map (A/B; same results).
   pf_map_commit: CURRENT = UPDATE (merge 0: "frag_map = frag_map_update", turn 0, :304-306) or CURRENT |= UPDATE (merge != 0,
   turn 1, :307-309).  pf_map_get / pf_map_set move the pf_map_length() words of one array to / from the host (through the
   context's hand-off pieces): how the map of a target sub-box reaches the device of a rank that sends to it -- get on the
   target, the caller's transport, create + set on the sender.  pf_map_count: the number of set bits, an upper bound of what a
   distribute call with that array stores. */
typedef struct pf_map pf_map;
#define PF_MAP_CURRENT 0   /* frag_map */
#define PF_MAP_UPDATE 1    /* frag_map_update */
int pf_map_create(pf_ctx *ctx, const pf_peak_region *box, pf_map **m);
void pf_map_destroy(pf_map *m);                  /* before pf_destroy of its context */
size_t pf_map_length(const pf_map *m);
int pf_map_fill_box(pf_map *m);
int pf_map_update(pf_map *m, size_t ngroups, const double *pos /* [3 * ngroups] */, const int *mass, double boundary_layer_factor,
                  unsigned long long nadd[2]);
int pf_map_commit(pf_map *m, int merge);
int pf_map_get(pf_map *m, int which, unsigned int *words);
int pf_map_set(pf_map *m, int which, const unsigned int *words);
int pf_map_count(pf_map *m, int which, unsigned long long *bits);
/* measurement aid (profiles/tools/map_time.py): the atomicOr the last pf_map_update of this map issued -- one per touched word of a
   row, or with PF_MAP_WORDS=0 one per requested cell (= nadd[0]).  Only for a map created under PF_MAP_STATS=1, which selects
   kernel instantiations that count; the default ones carry no counter and the call refuses */
int pf_debug_map_atomics(const pf_map *m, unsigned long long *atomics);
/* pf_distribute / pf_distribute_sorted with sub = (box.start, box.len) of the map and the named array (PF_MAP_CURRENT /
   PF_MAP_UPDATE) read where it lies: nothing is uploaded.  The map must have been created with this context.  Results are those of
   the host-map calls given the same words. */
int pf_distribute_map(pf_ctx *ctx, double flast, pf_map *m, int which, const pf_product_layout *layout, size_t capacity, void *frag,
                      unsigned int *frag_pos, size_t *count);
int pf_distribute_sorted_map(pf_ctx *ctx, double flast, pf_map *m, int which, const pf_product_layout *layout, size_t capacity,
                             void *frag, unsigned int *frag_pos, unsigned int *sorted_pos, int *indices, size_t *count);
/* count_peaks() over the STORED set of the map's box: a cell is stored when its bit is set AND Fmax >= flast, and a neighbour
   that is not stored vetoes nothing (:678-682) -- pf_count_peaks with a region takes every cell of the region with Fmax >= flast
   for stored.  Region (= the map's box), border skipping, well resolved test, slab halos and sums as pf_count_peaks; collective,
   every rank holding the same words.  peaks[0] is the reference's Npeaks ("found %d peaks") of either turn. */
int pf_count_peaks_map(pf_ctx *ctx, double flast, pf_map *m, int which, unsigned long long peaks[2]);
/* The neighbour table of the stored particles: every find_location() (src/fragment.c:592-603) that the loops of count_peaks()
   (:605-706), quick_build_groups() (src/build_groups.c:1916-2004) and build_groups() (:245-343) issue -- six per particle, each a
   bsearch over all stored positions followed by indices[pos] and an Fmax comparison -- answered for every particle in one call,
   with the per-particle flags the loops derive beside them.  None of it depends on the group state; the order-dependent group
   construction stays on the host and reads the table.
   The particles are in the order after sort_and_organize(); box = subbox.stabl, subbox.Lgwbl, subbox.safe; positions are
   pos = z + Lz (y + Ly x) (COORD_TO_INDEX, src/pinocchio.h:84-85).  For particle iz: (i, j, k) = INDEX_TO_COORD(frag_pos[iz]);
   PF_NEIGH_SKIP when a coordinate is 0 or len - 1 in a direction that is not periodic (src/build_groups.c:251-254); PF_NEIGH_GOOD
   when safe[d] <= coord < len[d] - safe[d] in all three (good_particle, :262-264); neigh[6 iz + nn], nn = 0..5 = x-, x+, y-, y+,
   z-, z+ with the single wrap of the switch at :274-306, is the index IN THE SAME ORDER of the particle stored at the neighbour's
   position -- the reference's indices[find_location(i1, j1, k1)] -- or -1 when none is stored there; all six are -1 for a skipped
   particle, which the reference never looks up.  PF_NEIGH_PEAK: not skipped and Fmax[iz] > Fmax[neigh] for every neighbour that
   is present (:322), the C comparison in the product precision: a NaN on either side clears it; a periodic direction of length 1
   makes a particle its own neighbour and never a peak, one of length 2 gives the same index twice.  peaks[0] counts the PEAK
   particles (the reference's Npeaks), peaks[1] those that are GOOD too (Ngood); 64-bit, independent of the schedule.
   pf_neighbours: on arrays the caller holds (the contributions of several ranks after pf_organize).  fmax points at the first
   particle's Fmax and fmax_stride is the byte distance to the next -- (char *)frag + off_Fmax and sizeof(product_data) --, float,
   or double for a context with PF_FLAG_DOUBLE_PRODUCTS; the host packs the values while it stages the upload, so 8 (12) bytes per
   particle go up and nothing else of the records.  The position index is built on the device by the call itself; equal positions
   give one of the duplicates.  ctx may be NULL (current device, default stream, float Fmax, a direction periodic when
   safe[d] == 0); with a context a direction is periodic when len[d] == n.  The box is checked as pf_map_create checks it.  neigh
   and flags may each be NULL (both: a count).  count = 0 gives peaks = {0, 0}.  Not collective.
   pf_distribute_sorted_neighbours_map = pf_distribute_sorted_map plus the table of exactly the records it returns -- the first
   min(*count, capacity) of the sorted order; a neighbour beyond the capacity is absent -- without a second trip: box and safe are
   the map's, the first four arrays and *count are byte for byte those of pf_distribute_sorted_map, every output may be NULL.
   Refused, with nothing written and no kernel launched: 2^31 records or more (the table is int like indices[]); a frag_pos entry
   that is not below Lx Ly Lz (checked on the host while staging: every index on the device is then in range whatever the caller
   passes); a stride that is no multiple of the element size; a map of another context.  When the scratch cannot be allocated the
   call says how many bytes it needs.  Results leave through the hand-off pieces (PF_HANDOFF_CHUNK_MB).  PF_NEIGH_ROWS=0, read
   per call, selects the plain form of the kernel (one search of the whole of sorted_pos per neighbour; A/B, same results). */
#define PF_NEIGH_SKIP 1
#define PF_NEIGH_GOOD 2
#define PF_NEIGH_PEAK 4
int pf_neighbours(pf_ctx *ctx, const pf_peak_region *box, size_t count, const unsigned int *frag_pos, const void *fmax,
                  size_t fmax_stride, int *neigh /* [6 * count] */, unsigned char *flags /* [count] */, unsigned long long peaks[2]);
int pf_distribute_sorted_neighbours_map(pf_ctx *ctx, double flast, pf_map *m, int which, const pf_product_layout *layout,
                                        size_t capacity, void *frag, unsigned int *frag_pos, unsigned int *sorted_pos, int *indices,
                                        int *neigh, unsigned char *flags, unsigned long long peaks[2], size_t *count);
/* measurement aid (profiles/tools/neigh_time.py): device time in ms of the position sort and of the table kernels (Fmax gather, row
   starts, lookups) of the calling thread's last context-free pf_neighbours that ran under PF_NEIGH_STATS=1 (read per call: such a
   call brackets the two parts with HIP events; the default records nothing and the call refuses) */
int pf_debug_neigh_ms(double *sort_ms, double *table_ms);
/* distribute_back() (src/distribute.c:703-946): the one data-parallel step BEHIND the group construction.  build_groups() leaves
   frag[].zacc and frag[].group_ID for the stored particles of every sub-box; the reference scatters those of the good particles
   into products[] of the FFT slabs, where write_timeless_snapshot() (src/write_snapshot.c:859-905) reads them for its ZACC and
   GRUP blocks.  Here they go into two per-cell columns of this rank's slab in HBM -- zacc of the product precision (float, or
   double with PF_FLAG_DOUBLE_PRODUCTS), group_ID int; index z + n*(y + n*x_local) as every product column; zacc = -1 and
   group_ID = 0 before anything is written (src/allocations.c:519-524).  The columns do not exist until one of these calls, or a
   ZACC / GRUP request to pf_get_block, needs them: 8 bytes per cell (12 with double products), counted into pf_device_bytes from
   then on and freed by pf_destroy; when they cannot be allocated the call says how many bytes it needs and the context stays as it
   was.  They depend on no sweep -- none of these calls needs computed products -- and no sweep touches them.  Every call is
   ordered on the context's stream: a block read after a back call sees it.
   pf_back_reset: zacc := -1, group_ID := 0.
   pf_distribute_back: keep_data_back() (:799-837), which is also the loop of send_data_back() (:859-896), with THIS rank's slab as
   the receiving fft box.  box = subbox.stabl, subbox.Lgwbl, subbox.safe of the sub-box the arrays belong to, checked as
   pf_map_create checks its box; a direction is periodic when len[d] == n.  frag_pos[iz] is the sub-box-space index
   z + Lz (y + Ly x) of particle iz; frag_pos == NULL is the CLASSIC_FRAGMENTATION form, particle iz at position iz (:808-809).
   zacc points at the first particle's value and zacc_stride is the byte distance to the next -- a packed array, or
   (char *)frag + off_zacc and sizeof(product_data) --, float, or double for a double-products context; group_id / group_stride
   likewise.  Particle iz is taken when it is a good particle, safe[d] <= c[d] < len[d] - safe[d] in all three directions with
   c = INDEX_TO_COORD(frag_pos[iz]) (:815-817), and its global cell (c[d] + start[d]) mod n -- the start first reduced to the
   periodic box, as pf_distribute does -- lies in this rank's x-slab (:824-827); both columns are then written at
   z + n*(y + n*(x - x0)) (:830-832).  *stored (may be NULL) is the number written on this rank, 64-bit and independent of the
   schedule.  Not collective and without an exchange: the owner of the sub-box, or whoever carries its arrays, calls it on every
   rank whose slab the sub-box meets; a box that misses the slab stores nothing; count = 0 is valid.  Positions are unique within
   a sub-box and the good regions of different sub-boxes are disjoint; of duplicates passed anyway one is kept, which is
   unspecified.
   pf_back_apply: recv_data_back() (:911-946) -- entries whose position in THIS rank's fft box the sender has computed already
   (back_data of the reference's unmodified send_data_back: pos, zacc, group_ID, each with its stride).
   Refused, with nothing written to the columns and no scatter launched (everything is validated on the host while it is staged,
   before the first launch): a frag_pos entry that is not below Lx Ly Lz (or, with frag_pos NULL, count above it); a pos entry of
   pf_back_apply that is not below the cells of the slab; more than 2^32 entries; a stride that is no multiple of the element
   size; a bad box; null arrays with count > 0.  The three arrays go up through the hand-off pieces (PF_HANDOFF_CHUNK_MB),
   packed by the host threads -- 12 bytes per particle (16 with double products) and nothing else of the records -- and one
   kernel scatters them.
   pf_update_back: the two columns merged into host records the caller holds (products[i].zacc / .group_ID of a -DSNAPSHOT
   build), as pf_update_products merges the others: stride and offsets are multiples of four, a negative offset skips that
   field, every other byte of a record keeps its value; only the 8 (12) bytes per cell cross the link.
   pf_debug_distribute_back: test tap without a context -- the same kernel on the slab planes x0 .. x0 + nxl - 1 of an n^3 box,
   float zacc, columns that start at -1 / 0 and are returned whole. */
int pf_back_reset(pf_ctx *ctx);
int pf_distribute_back(pf_ctx *ctx, const pf_peak_region *box, size_t count, const unsigned int *frag_pos, const void *zacc,
                       size_t zacc_stride, const int *group_id, size_t group_stride, size_t *stored);
int pf_back_apply(pf_ctx *ctx, size_t count, const unsigned int *pos, size_t pos_stride, const void *zacc, size_t zacc_stride,
                  const int *group_id, size_t group_stride);
int pf_update_back(pf_ctx *ctx, void *products_host, size_t stride, long off_zacc, long off_group_ID);
int pf_debug_distribute_back(int n, int x0, int nxl, const pf_peak_region *box, size_t count, const unsigned int *frag_pos,
                             const float *zacc, const int *group_id, float *zacc_out, int *group_out, size_t *stored);
/* The redshift segments of a RECOMPUTE_DISPLACEMENTS build (the reference's default; src/fragment.c:398-430): for every segment
   after the first, shift_all_displacements() (:832-850) copies Vel* to Vel*_prev, compute_displacements(0, 0, z) rewrites Vel*,
   and a whole second distribute() + sort_and_organize() brings both sets into frag[] for recompute_group_velocities().  The
   stored set and its order cannot change between segments (Fmax and the map are the same): only 24 numbers per stored particle
   are new, and the caller holds frag_pos[].  So here the step is a gather by position from the columns.
   pf_shift_displacements: vel12_prev := vel12, twelve more per-cell columns of PRODFLOAT laid out as the displacement columns
   -- 48 bytes per cell, 96 with PF_FLAG_DOUBLE_PRODUCTS.  They come into being at the first shift, count into pf_device_bytes from
   then on and are freed by pf_drop_prev or pf_destroy; when they cannot be allocated the call says how many bytes it needs and the
   context stays as it was.  A copy on the context's stream, not an exchange of pointers: until the next pf_displacements
   Vel == Vel_prev as in the reference, and pf_get_block / pf_distribute* may be called in between.  Refused unless
   pf_displacements has run since the products were last reset.  pf_distribute* and pf_update_products do not know the columns.
   pf_drop_prev: frees them (after the last segment, before the zacc / group_ID columns come into being); without columns it
   does nothing.  pf_prev_shifts: the shifts since creation or since the last drop; 0 = there are no columns.
   pf_gather_velocities: box = subbox.stabl, subbox.Lgwbl, subbox.safe of the sub-box the particles belong to, checked as
   pf_map_create checks its box; a direction is periodic when len[d] == n.  Particle i lies at the sub-box position frag_pos[i] =
   z + Lz (y + Ly x) (as pf_distribute returns it); its cell is that coordinate plus start, the start first reduced to the periodic
   box, modulo n (src/distribute.c:806-830 WITHOUT the good_particle test of :815-817: every stored particle has velocities, the
   boundary layer included).  It is FOUND when the x-plane of the cell lies in this rank's slab.  The found particles come back in
   ascending i: index[j] = i, and vel24[24 j ..] = the current columns 0..11 (Vel, Vel_2LPT, Vel_3LPT_1, Vel_3LPT_2, three
   components each) then the prev columns 0..11, as PRODFLOAT.  The slots of LPT orders the context does not compute
   (pf_set_lpt_order) are zero, and so are the prev slots while there are no prev columns.  *found counts beyond capacity, as *count
   of pf_distribute does; the first min(*found, capacity) entries are written; index and vel24 may each be NULL.  Duplicates in
   frag_pos are legal.  Needs products (a sweep or pf_displacements).  NOT collective: on P ranks each rank's call finds its own
   particles, the hit sets are disjoint and together they are all of count -- the owner of a sub-box sends frag_pos[] (4 bytes per
   particle) to every contributor, each calls this on its own context and sends index / vel24 back.
   order: NULL, or the caller's indices[] of sort_and_organize() / pf_distribute_sorted -- a permutation of 0 .. count - 1 in
   ascending position.  It changes which thread serves which particle and nothing else: with it consecutive threads serve
   z-neighbours and the column reads of a wavefront fall into few lines, while each particle's 96 bytes are written on their own;
   without it the reads are scattered and the output leaves as contiguous words.  Output order and contents are identical either
   way.  An order that is no permutation omits particles: their entries come back as index 0xFFFFFFFF with zero values, and
   pf_refresh_velocities leaves their records as they are.
   pf_refresh_velocities: the gather plus the scatter into the caller's records, done by the hand-off threads while they drain the
   pinned pieces: frag[i] of every found particle gets the fields named by a non-negative offset in layout (the four off_Vel*;
   off_Rmax / off_Fmax are ignored) and in prev (NULL: none -- a plain Vel* refresh; always allowed).  Every other byte of every
   record keeps its host value, records of particles that were not found keep theirs whole.  Stride and offsets follow the rules
   of pf_distribute's layout (multiples of four, inside the record, no overlap -- between layout and prev fields too).
   Refused, before anything is launched: a frag_pos entry that is not below Lx Ly Lz and an order entry that is not below count
   (checked on the host while staging; the message names the first offender); 2^31 particles or more; a bad box; a bad layout; a
   prev that names a field before any shift ("no pf_shift_displacements yet"); no products.  When the scratch -- 4 (8 with order)
   bytes per particle going up, 4 + 24 PRODFLOATs per found particle coming back -- cannot be allocated the call says how many
   bytes it needs.  Transfers go through the hand-off pieces (PF_HANDOFF_CHUNK_MB).
   pf_debug_gather_velocities: test tap without a context -- the same kernels on a caller's columns (host): planes x0 ..
   x0 + nxl - 1 of an n^3 box, 24 columns of nxl n n values of pb = 4 or 8 bytes (current 0..11, prev 0..11); index and vel24 have
   room for count entries. */
typedef struct { int off_Vel_prev, off_Vel_2LPT_prev, off_Vel_3LPT_1_prev, off_Vel_3LPT_2_prev; } pf_prev_layout;  /* bytes, negative = absent */
int pf_shift_displacements(pf_ctx *ctx);
int pf_drop_prev(pf_ctx *ctx);
int pf_prev_shifts(pf_ctx *ctx);
int pf_gather_velocities(pf_ctx *ctx, const pf_peak_region *box, size_t count, const unsigned int *frag_pos, const int *order,
                         size_t capacity, unsigned int *index, void *vel24, size_t *found);
int pf_refresh_velocities(pf_ctx *ctx, const pf_peak_region *box, size_t count, const unsigned int *frag_pos, const int *order,
                          void *frag, const pf_product_layout *layout, const pf_prev_layout *prev, size_t *found);
int pf_debug_gather_velocities(int n, int x0, int nxl, int pb, const void *cols24, const pf_peak_region *box, size_t count,
                               const unsigned int *frag_pos, const int *order, unsigned int *index, void *vel24, size_t *found);
/* The group velocities of a segment on the device: recompute_group_velocities() (src/fragment.c:852-909), the line behind the
   re-distribution, is a segmented sum of the same 24 columns over the particles of every group, and the only consumer of most of
   what pf_refresh_velocities brings back -- once a particle has joined a group the reference reads its frag[].Vel* no more
   (INTEGRATION.md has the argument).  So a segment needs the frag[] fields of the particles that are still loose and the group
   means; the grouped particles' 96 bytes need not cross the link.
   Which particles count: box, frag_pos and FOUND mean exactly what they mean for pf_gather_velocities (the cell of the position
   lies in this rank's slab; no good_particle test; duplicates are legal and count twice).  group_id points at the first
   particle's int, group_stride is the byte distance to the next (the reference's packed group_ID[]: 4; or a field of a record).
   Particle i is COUNTED when it is found and group_id[i] >= first_group -- the caller passes FILAMENT + 1 = 2 --, and LOOSE when it
   is found and group_id[i] < first_group.
   pf_group_velocity_sums: the groups with at least one counted particle on this rank in ascending group ID: group[j] the ID,
   npart[j] the number of counted particles, sum24[24 j + k] the fp64 sum of column k over them -- columns 0..11 current, 12..23
   prev, in the order of vel24; a column is zero where the LPT order or the prev columns are absent; with PF_FLAG_DOUBLE_PRODUCTS
   the columns are fp64 already.  The sums are deterministic: they depend on the set of (group, cell, value) alone, not on the order
   of the particles nor on the schedule (sorted keys, a fixed tree of additions, no floating-point atomics); the error of a sum is
   within npart 2^-53 sum|v|.  *groups_found counts beyond capacity, as *found does elsewhere; the first min(*groups_found,
   capacity) entries are written; *particles_found = the counted particles; each output pointer may be NULL.  NOT collective, like
   pf_gather_velocities: with several contributors the owner adds npart and sum24 of equal IDs and divides.  Refused before any
   launch, the first offender named: a negative group_id; a frag_pos entry not below Lx Ly Lz; 2^31 particles or more; a stride
   that is no multiple of 4; a bad box; no products; a slab of more than 2^32 cells.  Scratch that cannot be allocated is reported
   with its size: 8 bytes per particle going up, then per counted particle 16 bytes of keys plus the sort's own, and 200 bytes per
   group.
   pf_refresh_segment: the whole step of fragment.c:416-427 for ONE contributor that keeps frag[] and groups[].  The loose
   particles get their frag[] fields exactly as pf_refresh_velocities writes them (layout, prev, order as there); every other byte,
   and every record of a grouped or not-found particle, keeps its value.  Every group g in [first_group, ngroups] with npart > 0
   gets (PRODFLOAT)(sum / npart) in the fields gl names, in record g of groups (ngroups + 1 records of gl->stride bytes, as the
   reference's groups[0 .. ngroups]); groups without particles keep their bytes, and so does every byte gl does not name.  Where
   gl->off_Mass >= 0, *mass_mismatch counts the groups whose int at that offset differs from npart: reported, not refused -- the
   caller decides.  A group ID above ngroups is refused (named, before any launch).  frag == NULL skips the loose half, groups ==
   NULL the group half.  *loose / *grouped: the particles of either class.  The layouts follow the rules of pf_distribute's layout
   (multiples of four, inside the record, no overlap).  The means are plain means: the reference zeroes Vel_prev twice and
   Vel_2LPT_prev never (src/fragment.c:863), so ITS Vel_2LPT_prev is (old value + sum) / Mass; a caller who wants that literally
   has the sums of pf_group_velocity_sums.
   pf_debug_group_velocity_sums: test tap without a context -- the same kernels on a caller's columns (host), as
   pf_debug_gather_velocities; group, npart and sum24 have room for count entries.
   pf_debug_groupvel_times: with PF_GROUPVEL_TIMES=1 in the environment every call above measures its stages between events on its
   stream (one more synchronisation per call); ms3 = the device ms of the last call's keys + sort, head flags + scan, and
   reduce + fold.  Zeros otherwise.  For profiles/tools/groupvel_time.py. */
typedef struct { size_t stride; long off_Mass, off_Vel, off_Vel_2LPT, off_Vel_3LPT_1, off_Vel_3LPT_2,
                 off_Vel_prev, off_Vel_2LPT_prev, off_Vel_3LPT_1_prev, off_Vel_3LPT_2_prev; } pf_group_layout;  /* bytes, negative = absent */
int pf_group_velocity_sums(pf_ctx *ctx, const pf_peak_region *box, size_t count, const unsigned int *frag_pos,
                           const int *group_id, size_t group_stride, int first_group,
                           size_t capacity, int *group, unsigned int *npart, double *sum24,
                           size_t *groups_found, size_t *particles_found);
int pf_refresh_segment(pf_ctx *ctx, const pf_peak_region *box, size_t count, const unsigned int *frag_pos, const int *order,
                       const int *group_id, size_t group_stride, int first_group,
                       void *frag, const pf_product_layout *layout, const pf_prev_layout *prev,
                       void *groups, size_t ngroups, const pf_group_layout *gl,
                       size_t *loose, size_t *grouped, size_t *mass_mismatch);
int pf_debug_group_velocity_sums(int n, int x0, int nxl, int pb, const void *cols24, const pf_peak_region *box, size_t count,
                                 const unsigned int *frag_pos, const int *group_id, int first_group,
                                 int *group, unsigned int *npart, double *sum24, size_t *groups_found, size_t *particles_found);
int pf_debug_groupvel_times(double *ms3);
/* --- the past-light-cone test of build_groups() on the device (src/build_groups.c:356-448 and :783-868, a -DPLC build) ---
   For every good, massive group and every replication of the box the reference asks whether the group crossed the observer's
   light cone between a lower F and its Flast, finds the crossing F with a root finder and stores a plcgroup_data record.  Here
   the position of a group and the comoving distance at the two ends of its interval are computed once per group and serve every
   replication; only the crossing pairs reach the root finder (INTEGRATION.md has the two call sites).
   pf_plc_set_cosmology: the reference's splines the test reads, all on the abscissa x = -log10(1 + z) (n knots, increasing, 3 to
   512), evaluated as my_spline_eval does (src/cosmo.c:2016-2027): GSL's natural cubic spline inside, linear extrapolation outside.
   comvdist = SP_COMVDIST; grow[f] / fomega[f], f = 0..3 for the orders 1, 2, 31, 32: nk tables of n values each, the growth
   tables as log10 (SP_GROW31 positive: the minus sign of cosmo.c:1810 is applied here).  nk = 1 is the scale-independent build
   and reads k_for_GM; nk > 1 (at most 32) is -DSCALE_DEPENDENT with the bins log10 k = logkmin + j deltalogk, interpolated as
   InterpolateGrowth does (cosmo.c:1728-1755), and reads Smoothing.Rad_GM[0], Nsmooth >= 2 and k_GM_displ[Nsmooth], from which
   set_obj takes a group's own k (:1361-1375).  hubble: Hubble(z) at the same knots -- set_obj_vel's factor (:1449) reads this
   table where the reference calls its closed form.
   pf_plc_set_geometry: plc.center, the three versors, PLCAperture (degrees), Fstop, InterPartDist, GSglobal, the replications
   (src/pinocchio.h:412-416; F1, F2 are PRODFLOATs there and are rounded to PRODFLOAT here), and LastzForPLC, delta_z, nzbins of
   the n(z) histogram.  Both calls work on a context that has run no sweep, replace what an earlier call set, and refuse null
   pointers, knots that do not increase, nk or nsmooth out of range and zero replications.  What they keep on the device (the tables,
   32 bytes per replication) is freed by pf_destroy and is not counted in pf_device_bytes.
   pf_plc_cross: `ncand` records of `gl->stride` bytes at `groups`, each a group state: Mass (int), Pos (PRODFLOAT[3]), name
   (unsigned long long), Flast (PRODFLOAT), good and point (int), and the velocities of pf_group_layout; a negative offset = absent
   (velocities read zero; an absent good or point passes; Mass, Pos and Flast must be there).  The host threads pack what goes up:
   29 PRODFLOATs, Mass and one byte -- 121 bytes per candidate (237 with PF_FLAG_DOUBLE_PRODUCTS).  A candidate is tested when point >= 0 && good && Mass >= min_mass.
   seg: myseg, z_seg = ScaleDep.z[myseg], z_prev = ScaleDep.z[myseg - 1] (read when myseg >= 1): the weights of set_weight
   (:1411-1444); use_v31 = 0 reproduces src/build_groups.c:1588 as written (w31 times v32), 1 the line as meant.  box->start is
   subbox.stabl; periodic wrapping is off, as the reference switches it off around the test.  The displacement order is
   ORDER_FOR_CATALOG = 3, capped by pf_set_lpt_order.
   mode PF_PLC_LAST_CHECK: the lower end of every interval is Fstop (f_lo ignored), replication r is tried when Flast > F2 (:819).
   mode PF_PLC_EVENTS: the lower end of candidate i is the PRODFLOAT at f_lo + i f_lo_stride, r is tried when !(F_lo > F1 ||
   Flast < F2) (:394-395) -- for a host that logs (group state, Flast, F) at every touch and flushes the log in batches.
   A tried pair with bb = condition_PLC(F_lo) == 0 is stored at F_lo; with bb > 0 and condition_PLC(Flast) < 0 at the root in
   between: a PRODFLOAT F in [F_lo, Flast] with |condition_PLC(F)| < 1e-2 InterPartDist, the stopping rule of find_brent (:1865),
   found by a bracketing method of our own within 100 iterations.  A pair that does not get there counts in *unconverged and is
   not stored.  Storing is store_PLC (:1764-1822): the aperture test, then z = F - 1, Mass, name, x[3], v[3] into the fields `ol`
   names (negative = absent) of record j of plcgroups.
   Records come in ascending (candidate, replication) order and are the same from run to run (flags, scans, compactions; no atomic
   decides an order).  *count is the number found; the first min(*count, capacity) are written.  cand_of / rep_of (optional) name
   the pair of every written record.  nz (optional, nzbins doubles) gets +1.0 per written record in bin (int)((z - LastzForPLC) /
   delta_z), the top edge folded in (:1813-1816); a bin outside the histogram is skipped.
   pf_debug_plc_times: with PF_PLC_TIMES=1 in the environment pf_plc_cross measures its device part between two events (one more
   synchronisation); ms2 = the device ms of the last call's candidate passes and of its root + store passes.  Zeros otherwise. */
#define PF_PLC_LAST_CHECK 0
#define PF_PLC_EVENTS 1
typedef struct { int n; const double *x, *comvdist, *hubble; int nk; const double *grow[4], *fomega[4];
                 double logkmin, deltalogk, k_for_GM, rad_gm0; int nsmooth; const double *k_gm_displ; } pf_plc_cosmology;
typedef struct { int i, j, k; double F1, F2; } pf_plc_replication;
typedef struct { double center[3], xvers[3], yvers[3], zvers[3], aperture, Fstop, InterPartDist; long long GSglobal[3];
                 size_t nrep; const pf_plc_replication *repls; double LastzForPLC, delta_z; int nzbins; } pf_plc_geometry;
typedef struct { int myseg, use_v31; double z_seg, z_prev; } pf_plc_segment;
typedef struct { size_t stride; long off_Mass, off_Pos, off_name, off_Flast, off_good, off_point, off_Vel, off_Vel_2LPT, off_Vel_3LPT_1, off_Vel_3LPT_2,
                 off_Vel_prev, off_Vel_2LPT_prev, off_Vel_3LPT_1_prev, off_Vel_3LPT_2_prev; } pf_plc_group_layout;  /* bytes, negative = absent */
typedef struct { size_t stride; long off_Mass, off_name, off_z, off_x, off_v; } pf_plc_out_layout;
int pf_plc_set_cosmology(pf_ctx *ctx, const pf_plc_cosmology *cosmo);
int pf_plc_set_geometry(pf_ctx *ctx, const pf_plc_geometry *geom);
int pf_plc_cross(pf_ctx *ctx, int mode, const pf_plc_segment *seg, const pf_peak_region *box,
                 size_t ncand, const void *groups, const pf_plc_group_layout *gl,
                 const void *f_lo, size_t f_lo_stride, int min_mass,
                 size_t capacity, void *plcgroups, const pf_plc_out_layout *ol,
                 unsigned int *cand_of, int *rep_of, double *nz,
                 size_t *count, size_t *unconverged);
int pf_debug_plc_times(double *ms2);
/* --- the halo catalogue and the mass function of an output on the device (src/build_groups.c:899-905) ---
   At every output redshift build_groups() runs write_catalog() (src/write_halos.c:227-318) and compute_mf() (:35-65): one loop
   over groups[] that, for every group with point >= 0 && good && Mass >= MinHaloMass, evaluates set_obj, set_weight, set_obj_vel,
   q2x and vel (src/build_groups.c:1354-1460, :1554-1643) at F = outputs.F[iout] and fills a catalog_data record
   (src/pinocchio.h:515-524), and a second one that bins the same groups by log10(Mass * ParticleMass).  pf_catalog is both loops
   (write_halos.c:268-318 and :46-65) for a host that keeps groups[]; the file, its headers, the MPI_Reduce of the histogram, the
   analytic mass function and write_histories stay with the host (INTEGRATION.md has the call site).
   It reads the splines of pf_plc_set_cosmology -- which must have been called; pf_plc_set_geometry need not -- and works on a
   context that has run no sweep.
   groups: `ngroups` records of `gl->stride` bytes, the first one the reference's loop visits (groups + FILAMENT + 1), read through
   the layout of pf_plc_cross: Mass (int), Pos (PRODFLOAT[3]), name, good, point and the eight velocities; a negative offset =
   absent (velocities read zero, an absent good or point passes, an absent name reads zero; Mass and Pos must be there; Flast is
   not read and need not be named).  The host threads pack what goes up: 27 PRODFLOATs, Mass and one byte -- 113 bytes per group
   (221 with PF_FLAG_DOUBLE_PRODUCTS); name stays on the host.  What comes down is 10 PRODFLOATs and the batch index per record.
   seg: as in pf_plc_cross (myseg, z_seg, z_prev for set_weight; use_v31 = 0 reproduces build_groups.c:1588 as written).
   box->start is subbox.stabl and box->len is subbox.Lgwbl (safe is not read).
   par: F = outputs.F[iout] (rounded to PRODFLOAT as set_obj's argument is; z = F - 1), InterPartDist, ParticleMass, hfactor
   (params.Hubble100 with OutputInH100, else 1: write_halos.c:262-265), GSglobal, pbc = subbox.pbc, min_mass = MinHaloMass.
   Record of a passing group (write_halos.c:289-315), every expression rounded where the reference's C rounds it:
     name = the group's, n = Mass, M = Mass * ParticleMass * hfactor
     q[j] = Pos[j] + stabl[j]; if (q < 0) q += GSglobal[j]; if (q >= GSglobal[j]) q -= GSglobal[j]; q *= InterPartDist * hfactor
     x[j] = q2x at order ORDER_FOR_CATALOG = 3 (capped by pf_set_lpt_order), wrapped into [0, len[j]) where pbc[j] is set
            (:1595-1600: >= Box first, then < 0), + stabl[j], then the same two wraps and the same factor as q
     v[j] = vel(j) with set_obj_vel's factors at z (Hubble(z) from the table of pf_plc_set_cosmology)
   Records come in ascending batch index, the same from run to run: a flag pass, a scan, a record pass; no atomic decides an order.
   *count is the number of passing groups; the first min(*count, capacity) are written into the fields `ol` names of record j of
   `catalog` (name 8 bytes, M, x[3], v[3], q[3] PRODFLOATs, n an int; negative = absent).  Bytes of a record that the layout does
   not name -- pad, n under LIGHT_OUTPUT -- and records beyond those written are left as the caller had them.  group_of (optional)
   gets the batch index of every written record.
   bins (NULL: no mass function): ninbin and massinbin, nbin entries each, are SET to the mf.ninbin_local / mf.massinbin_local of
   these groups -- all passing groups, whatever the capacity; the MPI_Reduce stays the caller's.  The bin of a group is
   (int)((log10(Mass * ParticleMass) - mmin) / deltam), skipped outside [0, nbin) (write_halos.c:59-62), with mmin as
   src/initialization.c:1122 forms it and deltam = DELTAM.  The device evaluates no log10: the call turns the bins into nbin + 1
   integer thresholds -- the smallest Mass >= 1 of every bin, by bisection over Mass with the host libm's log10 -- and the device
   bins by binary search, which is the reference's binning to the last bit wherever log10(Mass * ParticleMass) does not decrease
   with Mass.  A group with Mass < 1 is never binned.  The sums are integers on the device (a count and a 64-bit sum of Mass per
   bin); massinbin[b] = (double)sumMass[b] * ParticleMass, within (n_b + 1) 2^-53 relative of the reference's running sum of
   doubles and independent of the order of groups[].
   Refused (return 1, pf_last_error, *count = 0): null arguments, no cosmology set, myseg < 0, F not finite or <= 0, InterPartDist
   or hfactor <= 0, ParticleMass or deltam <= 0 with bins, nbin outside 0..2^20, len or GSglobal <= 0, a layout field that leaves
   its record, more than 2^31 - 1 groups.
   pf_debug_catalog_times: with PF_CATALOG_TIMES=1 in the environment pf_catalog measures its device part between two events; ms2 =
   the device ms of the last call's flag + scan passes and of its record + histogram passes.  Zeros otherwise.
   pf_debug_catalog_parts: the host's wall ms of the last call's four parts -- pack, upload, device (allocations and waits
   included), download + records -- for profiles/tools/catalog_time.py. */
typedef struct { double F, InterPartDist, ParticleMass, hfactor; long long GSglobal[3]; int pbc[3]; int min_mass; } pf_catalog_params;
typedef struct { size_t stride; long off_name, off_M, off_x, off_v, off_q, off_n; } pf_catalog_out_layout;   /* bytes, negative = absent */
typedef struct { int nbin; double mmin, deltam; } pf_mf_bins;
int pf_catalog(pf_ctx *ctx, const pf_plc_segment *seg, const pf_peak_region *box, const pf_catalog_params *par,
               size_t ngroups, const void *groups, const pf_plc_group_layout *gl,
               size_t capacity, void *catalog, const pf_catalog_out_layout *ol, unsigned int *group_of,
               const pf_mf_bins *bins, int *ninbin, double *massinbin, size_t *count);
int pf_debug_catalog_times(double *ms2);
int pf_debug_catalog_parts(double *ms4);
/* --- the state of every stored particle at its own collapse time (src/build_groups.c:1286-1317 and what it calls) ---
   condition_for_accretion() evaluates, for the particle iz the loop of build_groups() works on, virial(Mass, F, flag) (:1023-1051),
   set_point(i, j, k, ind, F, ...) (:1464-1520) with its set_weight() (:1411-1444) and, through distance() (:1646-1664), q2x()
   (:1554-1603) of the point -- all at F = frag[iz].Fmax, once per neighbouring group and once more per filament particle.  What of
   this depends on F, the particle's cell and its velocities alone -- not on the sequential group state -- is computed here for a
   whole batch of stored particles from the columns in HBM; the host loop then reads a table.
   box, frag_pos, order, capacity, index and found follow the contract of pf_gather_velocities to the letter: the cell of a
   particle, FOUND by slab, ascending i, *found counting beyond capacity, periodic when len[d] == n, duplicates legal, an order
   that is no permutation omits particles (index 0xFFFFFFFF, zero values), NOT collective.  `order` is the access hint of that
   call; it has nothing to do with par->order.
   seg: as in pf_plc_cross (myseg, z_seg = ScaleDep.z[myseg], z_prev = ScaleDep.z[myseg - 1] read when myseg >= 1; use_v31 = 0
   reproduces :1588 as written).
   par: sigma0 = sqrt(Smoothing.TrueVariance[Nsmooth - 1]); k_sigma = Smoothing.k_GM_dens[Nsmooth - 1] in a -DSCALE_DEPENDENT build,
   else params.k_for_GM (:1040-1045); k_point = Smoothing.k_GM_displ[Nsmooth - 1], else params.k_for_GM (:1470-1475); order =
   ORDER_FOR_GROUPS (2), 1 to 3; the order q2x uses is min(order, the order of pf_set_lpt_order).
   states: 8 PRODFLOATs per found particle, entry j beside index[j].  With F the PRODFLOAT in the Fmax column of the particle's
   cell and z = (double)F - 1.0:
     [0..3]  w, w2, w31, w32 of set_weight() for myk = k_point -- the branch of myseg == 0 or of myseg >= 1 --, each rounded to
             PRODFLOAT where the reference's assignment rounds; GrowingMode_3LPT_1 keeps its minus sign (cosmo.c:1810); the slots
             of LPT orders the context does not compute (pf_set_lpt_order) are zero
     [4]     sigmaD of virial(): (PRODFLOAT)(sigma0 * GrowingMode(z, k_sigma))
     [5..7]  q2x(d, point, pbc[d], (double)Lgwbl[d], order) for d = 0..2 with q[d] = the sub-box coordinate + SHIFT (0.5), the
             velocities from the current columns and, for myseg >= 1, from the prev columns; the two periodic wraps in the
             reference's order (>= Box first, then < 0)
   It reads the growth tables of pf_plc_set_cosmology (pf_plc_set_geometry need not have been called).  With nk == 1 there is one
   table per family and the two k values are not read; with nk > 1 each goes through the three branches of InterpolateGrowth
   (cosmo.c:1737-1749).  Only the tables the call reads are staged on the CU: with nk > 1 the two bins around k_point of the four
   growth families and those around k_sigma of the first.  The growing modes at the segment's redshifts are computed once per call.
   Deterministic: no floating-point atomics; output identical from run to run and with or without `order`.
   4 bytes go up per particle, 8 with order; 4 + 8 PRODFLOATs come down per found particle.  When the scratch cannot be allocated
   the call says how many bytes it needs.
   Refused (return 1, pf_last_error, *found = 0) before anything is launched: null arguments; no cosmology set; no products;
   myseg >= 1 without prev columns; myseg < 0; par->order outside 1..3; sigma0, k_sigma or k_point not finite or <= 0; a bad box; a
   frag_pos entry not below Lx Ly Lz or an order entry not below count (the first offender named); 2^31 particles or more.
   pf_debug_point_states: test tap on a caller's host columns: planes x0 .. x0 + nxl - 1 of an n^3 box, pb = 4 or 8; fmax_col =
   nxl n n values, cols24 as for pf_debug_gather_velocities; tables_ctx supplies the cosmology tables and nothing else; the LPT
   order of the columns counts as 3; index and states have room for count entries.
   pf_debug_point_times: with PF_POINT_TIMES=1 in the environment a call measures its device part between events; ms2 = the device
   ms of the last call's select + scan passes and of its state pass.  Zeros otherwise.  For profiles/tools/points_time.py. */
typedef struct { double sigma0, k_sigma, k_point; int order; } pf_point_params;
int pf_point_states(pf_ctx *ctx, const pf_plc_segment *seg, const pf_peak_region *box, const pf_point_params *par,
                    size_t count, const unsigned int *frag_pos, const int *order,
                    size_t capacity, unsigned int *index, void *states, size_t *found);
int pf_debug_point_states(int n, int x0, int nxl, int pb, const void *fmax_col, const void *cols24,
                          pf_ctx *tables_ctx, const pf_plc_segment *seg, const pf_peak_region *box, const pf_point_params *par,
                          size_t count, const unsigned int *frag_pos, const int *order,
                          unsigned int *index, void *states, size_t *found);
int pf_debug_point_times(double *ms2);
/* Per-particle payload of one block of the "timeless snapshot" (write_timeless_snapshot, src/write_snapshot.c:207-342)
   for this rank's slab, from the SoA columns in HBM: name = "ID  " (1 + global index as MYIDTYPE of id_bytes = 4 or 8,
   :648-664), "FMAX" float, "RMAX" int, "ZEL " / "2LPT" / "31PT" / "32PT" float[3] per particle (:700-855), and the last
   two blocks of the file, "ZACC" float and "GRUP" int per particle (:859-905), from the columns of the back calls above --
   these two need no computed products and read -1 / 0 where nothing was distributed back. */
int pf_get_block(pf_ctx *ctx, const char *name, int id_bytes, void *host);
/* debug / test taps (host copies, fp64): second_derivatives[0][i] of the last
   pf_second_derivatives (i = 0..5 <-> 11,22,33,12,13,23; src/LPT.c:36-44),
   compact [n/nranks][n][n]; LPT source spectra kvector_2LPT/3LPT_1/3LPT_2
   (which = 0,1,2) regrouped to the boundary layout [n/nranks][n][n/2+1][2]
   (one all-to-all when nranks > 1; collective). */
int pf_get_second_derivative(pf_ctx *ctx, int i, double *host);
int pf_get_kvector(pf_ctx *ctx, int which, double *host);
int pf_get_density(pf_ctx *ctx, double *host);  /* resident delta(k), boundary layout */
/* test tap: rows kx0 .. kx0 + nkx - 1 of the replicated spectrum (pf_replicated_spectrum) as this rank transforms it,
   [nkx][n (ky)][n/2+1] complex fp64, natural order (gathered -- or, behind the loopback exchange, generated -- first) */
int pf_debug_replicated_rows(pf_ctx *ctx, int kx0, int nkx, double *host);
/* The FFT-module seam of the reference (src/pinocchio.h:551-562), host in and host out in the boundary layouts
   (this rank's x-slab: real [n/nranks][n][n], spectrum [n/nranks][n][n/2+1][2]); collective over the ranks.
   forward_transform / reverse_transform (src/fmax-pfft.c:191-228): unnormalised r2c, and c2r followed by the
   1/N^3 normalisation.  Callers outside the hot path: the density writer (src/pinocchio.c:146-150) and
   ReadWhiteNoise.c:161-222. */
int pf_forward_transform(pf_ctx *ctx, const double *real_host, double *spec_host);
int pf_reverse_transform(pf_ctx *ctx, const double *spec_host, double *real_host);
/* compute_derivative(ThisGrid, first_derivative, second_derivative) (src/fmax-pfft.c:255-441) on a caller-held
   spectrum: real = c2r[ spec * G * exp(-k^2 rs^2/2) * growth(order) ] / N^3, with G = k_a k_b / k^2 (a, b in 1..3),
   i k_a / k^2 (one of them 0), -1/k^2 (both 0) (greens_function :444-456, the re/im swap :379-384); the k = 0 mode
   is left as it is.  rs in cells (Rsmooth); order = ScaleDep.order: 0 no growth, 1..4 the multiplier of
   pf_set_growth / pf_set_growth_table.  The spectrum on the host is not modified (the reference filters
   cvector_fft in place; nothing reads it afterwards). */
int pf_derivative(pf_ctx *ctx, const double *spec_host, int first_derivative, int second_derivative, double rs_cells,
                  int order, double *real_host);
/* test tap: the elementary functions the solver's default arithmetic uses on the device, which =
   0 a/b, 1 sqrt(a), 2 acos(a), 3 log10(a), 4 sin (b != 0) or cos (b == 0) of a in [0, pi/3], 5 a^0.333333333333333, 6 a/9,
   7 exp(a), 8 10^a, 9 / 10 the raw hardware seeds v_rcp_f64(a) / v_rsq_f64(a) */
int pf_debug_math(pf_ctx *ctx, int which, const double *a, const double *b, size_t count, double *out);
/* measurement aid (bench.py): GB/s of a kernel that only reads (kind 0), only writes (1) or copies (2) one spectrum-sized field of this
   context, `reps` launches between two events -- the streaming rates of this memory system, beside which the transform passes are
   reported.  No counterpart in the reference. */
int pf_debug_stream_rate(pf_ctx *ctx, int kind, int reps, double *gbps);
/* test tap without a context: ONE pass kernel on a batch of lines, host in / host out in fp64 (converted to field_bytes on
   the way); every instantiation of the hand-written transforms -- N = 2048 of BASELINE config 5 included, whose box does
   not fit one GPU -- can so be compared line by line with an independent transform (tests/test_gpu_lines.py).
   pass 0 / 1: the strided x / y pass, inverse / forward, complex [nouter][n][ncols] in and out, with the k-space factor
   `mul` (0 one, 1 k, 2 k^2, 3 i k) along the transformed axis, loads beyond |wavenumber| > band treated as zeros, and with
   pre != 0 the first-pass filter exp(-k^2 rs^2 / 2) growth / k^2 of compute_derivative (src/fmax-pfft.c:366-373);
   pass 2: z-pass c2r, complex [nouter][n/2+1] -> real [nouter][n], unnormalised (reverse_transform without its 1/N^3);
   pass 3: z-pass r2c, real [nouter][n] -> complex [nouter][n/2+1] (forward_transform);
   pass 4: the six-rows-to-three-invariants z-pass of the sweep, complex [6][nouter][n/2+1] -> real [3][nouter][n], followed by
           one more double: 1.0 when a cell raised the q == 0 flag (see pf_debug_invariant_reruns). */
int pf_debug_lines(int field_bytes, int n, int pass, int mul, int band, int nouter, int ncols, int pre, double rs,
                   double growth, int outer_offset, const double *in, double *out);
/* test tap without a context: one operation of the packed (re, im) fp32 algebra the sixteen-point strided pass is written in
   (csrc/pf_fft16.h) on `count` pairs: which = 0 / 1 a +- i b, 2 / 3 +- i a, 4 / 5 a * b, a * conj(b), 6 / 7 the same with b[0] in scalar
   registers, 8 / 9 a * (c +- i s) for a constant, 10 a - i b */
int pf_debug_pk(int which, const float *a, const float *b, float *out, int count);
/* test tap without a context: the chirp-z 3-D transforms of the general path (csrc/pf_gfft.hip: any even n in 4..2048, no library) on
   host arrays in the natural layouts; dir > 0: spectrum [n][n][n/2+1] complex -> real [n][n][n] (unnormalised), dir < 0: real -> spectrum */
int pf_debug_gfft(int n, int dir, const double *in, double *out);
/* ... and ONE chirp-z pass on a few lines of n points (any even n in 4..2048, so that the convolution lengths 1024, 2048 and 4096 --
   whose n^3 boxes no test can afford -- are run too).  mode 0: complex lines laid out [n][nlines] as the x- and y-passes meet them,
   dir > 0 inverse / < 0 forward; mode 1: Hermitian rows [nlines][n/2+1] -> real rows [nlines][n]; mode 2: real rows -> Hermitian rows */
int pf_debug_gfft_lines(int n, int mode, int dir, int nlines, const double *in, double *out);
/* test tap without a context: ONE strided (inverse) launch with several jobs as the passes of the sweep issue them: job j transforms
   input field in_of[j] (of `nin` complex fields [nouter][n][ncols], fp64 on the host) with the factor mul[j] (0 one, 1 k, 2 k^2, 3 i k)
   along the transformed axis into out[j] ([njobs][nouter][n][ncols]); jobs on the same input must be adjacent.  n a power of two. */
int pf_debug_strided_jobs(int field_bytes, int n, int njobs, int nin, const int *in_of, const int *mul, int nouter, int ncols,
                          const double *in, double *out);
/* ... and the same launch the way the passes of a pruned (band-limited) radius issue it: loads with |wavenumber| > band_e along the
   transformed axis are zeros, outer lines with |signed index of (outer + outer_offset)| > band_outer leave early (a band >= n / 2
   switches either off), pre / rs / growth are the first-pass filter of pf_debug_lines, and the device rows of the inputs / outputs are
   in_pitch / out_pitch complex columns long (each whole 128-byte lines -- a multiple of 8 with fp64, of 16 with fp32 fields -- and
   >= ncols; they may differ: the x-pass of a pruned radius writes the compact pitch of its band).  The input rows' padding beyond ncols holds junk, not zeros.  Behind every output field lies a
   guard region filled with a fixed byte pattern: *guard_ok = 1 when all of them came back intact.  in: [nin][nouter][n][ncols],
   out: [njobs][nouter][n][ncols] (the columns below ncols of the device rows); lines that left early come back as zeros. */
int pf_debug_strided_band(int field_bytes, int n, int njobs, int nin, const int *in_of, const int *mul, int nouter, int ncols,
                          int in_pitch, int out_pitch, int band_e, int band_outer, int outer_offset, int pre, double rs, double growth,
                          const double *in, double *out, int *guard_ok);
/* test tap without a context: the z-pass c2r in the forms the library itself launches it (tests/test_gpu_zpass_forms.py) -- several jobs in
   one launch, float / packed product rows, the fields' padded row pitches (spectra: n/2 + 64/field_bytes complex; real rows: twice that),
   norm, a DC constant (dc: host pointer or NULL), in place or not, and the 3LPT(b) contraction inside the six-row z-pass.
   form 0: njobs (1..6) jobs, job j with the kz factor mul[j] (0 one, 1 k, 2 k^2, 3 i k) and out_f32[j] (0: field-type rows at the fields'
           pitch; 1: float rows of pitch n; 2: field-type rows of pitch n, fp64 fields only); in_place != 0 (every out_f32 == 0): each job's
           result overwrites its own spectrum rows, as the Hessian z-pass does; otherwise every job has a buffer of its own.
           spec [njobs][nrows][n/2+1] complex -> out [njobs][nrows][n]
   form 1: the six jobs of the Hessian z-pass (kz factors one, one, k^2, one, k, k), nothing stored: acc -= 2 sum_ab phi2_ab hess_ab per cell,
           hess [6][nrows][n] the first-order Hessian, acc [nrows][n] -> out [nrows][n]; form 2: the same with acc formed, not read, from
           hess first (2 (h11 + h22 + h33) S2(h)); n a power of two.  mul, out_f32, njobs and in_place are ignored.
   band: columns kz > band are not read (>= n/2: none); ncu: compute units the launch is sized for (0: the device's).
   A size without such a kernel is an error (nothing is launched).  Every row's padding and a guard region behind every packed buffer
   hold a byte pattern; *sentinel_ok = 1 when all of it -- and with form 1 / 2 the six hess fields as a whole -- came back unchanged. */
int pf_debug_zpass_jobs(int field_bytes, int n, int form, int njobs, const int *mul, const int *out_f32, int in_place, int nrows, int band,
                        double norm, const double *dc, int ncu, const double *spec, const double *hess, const double *acc, double *out,
                        int *sentinel_ok);
/* test tap without a context: the inverse x-pass that does the pending forward x-transform of its single input first (one rank, LPT
   source spectra) into out_fused, and the two launches it replaces -- forward pass, then the plain inverse pass with the same jobs --
   into out_plain.  in [nouter][n][ncols] complex, out_* [njobs][nouter][n][ncols]; mul, pre, rs, growth, outer_offset as in pf_debug_lines.
   n a power of two up to 2048 (fp32 fields: below 1024). */
int pf_debug_strided_xfuse(int field_bytes, int n, int njobs, const int *mul, int nouter, int ncols, int pre, double rs, double growth,
                           int outer_offset, const double *in, double *out_fused, double *out_plain);
/* how many sweeps of this context were repeated with six components per cell because the invariant z-pass met a tensor
   with q == 0 that is not exactly isotropic (the reference's "already diagonal" branch, src/collapse_times.c:722-727) */
int pf_debug_invariant_reruns(pf_ctx *ctx);
/* 1 when the last sweep of this context ran the collapse solve of its invariant radii on the solve stream, beside the z-pass of
   the radius that follows (PF_SOLVE_BESIDE_Z): HIP-event spans then overlap (the solve trails into the passes after
   that z-pass too) -- per-kernel times of pf_kernel_stats are spans, not kernel times or shares of the step; 0 when every kernel ran in line */
int pf_solve_ran_beside_zpass(pf_ctx *ctx);
/* which transforms serve the context's grid size (the reference plans any GridSize, src/fmax-pfft.c:139-188): 0 the hand-written
   power-of-two passes, 1 the hand-written passes with mixed-radix stage plans (n = 8 m, m = 2^a 3^b 5^c; any number of ranks that divides n),
   2 chirp-z transforms, one 3-D transform per component (any other even n on one rank, or PF_GENERAL=1) */
int pf_transform_path(pf_ctx *ctx);
/* 1: in the default (fast) arithmetic the inverse growing mode of radius `ismooth` (-1: the shared spline) comes from the
   polynomial table built from its knots by pf_set_invgrow (csrc/pf_gtab.h; *max_rel_err: its largest relative error against
   the composite 10^(-S(log10 D)) in long double; NaN when the build was refused before it got to check one: meaningful with
   status 1, or with status 0 of a table refused for its error); 0: the series forms are used (table refused, PF_GTAB=0, PF_EXACT_LIBM=1) */
int pf_invgrow_table_status(pf_ctx *ctx, int ismooth, double *max_rel_err);
/* per-cell solver on a list of Hessians d[6*count] -> F[count] (tests of
   inverse_collapse_time, src/collapse_times.c:679-776), ismooth selects the spline */
int pf_collapse_cells(pf_ctx *ctx, int ismooth, const double *d, size_t count, double *F);
/* The arithmetic of the collapse solve as a run-time setting of the context.  PF_ARITH_FAST: the series, table and hardware-seeded
   forms of cos, acos, pow, log10, exp, / and sqrt, the default; PF_ARITH_EXACT: the reference's own calls.
   The initial value is what PF_EXACT_LIBM says when pf_create runs.  pf_set_arithmetic holds for every solve that follows --
   pf_sweep, pf_collapse_times, pf_collapse_cells, pf_ct_build -- and a context computes after it, bit for bit, what a context
   created under the matching environment value computes: both solve kernels are compiled in and chosen at launch, the
   polynomial tables of pf_set_invgrow are built whatever the flavour and read by the fast one alone (pf_invgrow_table_status
   follows the setting), and neither the spline look-up, the solve queue's use nor the solve-beside-z-pass choice is decided by
   anything kept from the flavour before.  A collapse-time table that pf_ct_build or a sweep built on the device belongs to the
   flavour that built it: a change of flavour marks it as not in place, so that the next pf_collapse_times (or sweep) of its
   radius rebuilds it from the variance it was built with.  A table installed by pf_ct_load is data and stays.
   pf_set_arithmetic: 1 (pf_last_error) for a null context or a flavour that is neither; pf_get_arithmetic: -1 for a null context. */
enum { PF_ARITH_FAST = 0, PF_ARITH_EXACT = 1 };
int pf_set_arithmetic(pf_ctx *ctx, int flavour);
int pf_get_arithmetic(pf_ctx *ctx);
/* The census of a sweep: Fmax and Rmax of both flavours on the same resident delta(k), compared on the device.
   A DIAGNOSTIC call: it costs two sweeps and one streaming pass over four columns.  It runs pf_sweep once in the other flavour,
   keeps that sweep's Fmax / Rmax as shadow columns (product bytes + 4 per cell of the slab, allocated for the call and freed
   before it returns, not counted in pf_device_bytes; when they do not fit the call fails before the first sweep and the
   context is untouched), then pf_sweep in the context's own flavour, then the census kernel (csrc/pf_census.hip).  On return the
   context is in exactly the state a plain pf_sweep(ctx, ns, radius_cells, true_variance) in its own flavour leaves: products,
   true_variance, the sources of pf_set_sources_in_sweep, every flag, pf_device_bytes and the arithmetic setting.  Collective
   exactly as pf_sweep is; it adds no communication: the numbers are this rank's, over its slab (summing counts and taking
   maxima over ranks is the caller's).  pf_kernel_stats / pf_get_cputime show both sweeps.  It compares the two device flavours
   on the device's own Hessian; it is no comparison with the reference's transforms.
   Per cell, the same for float and double products: d = |fast - exact| formed in double; ulp = the spacing of
   max(|exact|, 1) in the product precision, from its exponent bits; u = d / ulp.  hist[0]: u == 0 (identical bits, whatever
   the value, and +0 against -0); hist[1]: 0 < u <= 1; hist[k], k >= 2: 2^(k-2) < u <= 2^(k-1); the last bin is open at the
   top.  A cell whose bit patterns differ and where either side is NaN or infinite counts in `nonfinite` and nowhere in the
   histogram or the maxima.  sum(hist) + nonfinite == cells.  max_abs / max_ulps: the largest d / u; max_abs_cell: the lowest
   cell index that attains max_abs (all ones when every cell is nonfinite).  Cell index: z + n (y + n x_local).
   The outlier records -- cells with d > 2 ulp or counted in nonfinite -- come in ascending cell index, the same from run to
   run; the first min(outliers, capacity) are written.  cells may be NULL with capacity 0.  `fast` / `exact` always mean those
   flavours, whichever ran last.  Integer sums and per-workgroup partials throughout: no floating-point atomics, the result
   does not depend on the schedule.
   Refused (1, pf_last_error) with the context untouched: null ctx / radius_cells / out, cells NULL with capacity > 0, ns
   outside [1, PF_MAX_SMOOTH], no density set, no room for the shadow columns.
   pf_debug_census: test tap without a context, the production kernels on a caller's host columns of `count` cells
   (product_bytes 4: float, 8: double); the cell indices start at first_cell. */
#define PF_CENSUS_BINS 64
typedef struct {
  unsigned long long cells;            /* cells of this rank's slab */
  unsigned long long differing_bits;   /* Fmax bit patterns differ (+0 against -0 counts here and in bin 0) */
  unsigned long long hist[PF_CENSUS_BINS];
  unsigned long long beyond_2ulp;      /* = sum of hist[3..]: d > 2 ulp */
  unsigned long long rmax_differing;
  unsigned long long nonfinite;        /* either Fmax is NaN or infinite, and the bit patterns differ */
  unsigned long long outliers;         /* beyond_2ulp + nonfinite: how many records exist, whatever the capacity */
  double max_abs, max_ulps;            /* over the finite cells */
  unsigned long long max_abs_cell;     /* lowest cell index that attains max_abs */
} pf_census;
typedef struct { unsigned long long cell; double fast, exact; int rmax_fast, rmax_exact; } pf_census_cell;   /* 32 bytes */
int pf_flavour_census(pf_ctx *ctx, int ns, const double *radius_cells, double *true_variance,
                      pf_census *out, size_t capacity, pf_census_cell *cells);
int pf_debug_census(int product_bytes, unsigned long long first_cell, size_t count,
                    const void *fmax_fast, const int *rmax_fast, const void *fmax_exact, const int *rmax_exact,
                    pf_census *out, size_t capacity, pf_census_cell *cells);

/* --- power spectrum and smoothed variances of a resident spectrum ---
   What the reference plots as P(k) (tests/pk_and_HMF_tests) and logs per radius as "computed sigma" (src/fmax.c:142-146), from
   the spectrum in HBM: two streaming reads of this rank's ky-slab, nothing else of size.
   which: 0 the resident delta(k); 1, 2, 3 kvector_2LPT, kvector_3LPT_1, kvector_3LPT_2 -- the spectra pf_get_kvector(which - 1)
     exports, refused under the same conditions as that export.
   Wavenumbers: signed integers as in compute_derivative (src/fmax-pfft.c:312-334): i > n/2 -> i - n, n/2 stays positive;
     k2 = ix^2 + iy^2 + iz^2, an integer.
   Shell b of a mode: (2b - 1)^2 <= 4 k2 < (2b + 1)^2, the nearest integer to |k|, decided in integers (no tie: 4 k2 is even).
     pf_power_bins(n) = 1 + the largest b with (2b - 1)^2 <= 3 n^2 (15 for n = 16); shell 0 holds only the k = 0 mode.
   Weight w: 2 for 0 < iz < n/2, 1 on the planes iz = 0 and iz = n/2 -- the half-spectrum stands for the full sphere.
   nmodes[b] = sum of w and k2sum[b] = sum of w k2 over ALL modes of the shell (exact integers; the nmodes add up to info->modes
     = n^3 over all ranks).
   power[b] = sum of w (re^2 + im^2) / N^6, N^6 = (n^3)^2, re and im widened to double first; P(k) of the shell is
     power[b] / nmodes[b] * Box^3 at k_eff = (2 pi / Box) sqrt(k2sum[b] / nmodes[b]).
   variance[i], i < ns = sum over k != 0 of w (re^2 + im^2) exp(-(2 pi / n)^2 k2 radius_cells[i]^2) / N^6: the window of
     src/fmax-pfft.c:366-373 squared, so by Parseval the TrueVariance[i] that pf_sweep reports for that radius.  ns from 0 to
     PF_MAX_SMOOTH; variance and radius_cells may be NULL when ns = 0.
   info->nonfinite: the modes (counted with w) whose re^2 + im^2 is not finite -- a NaN or infinite part, or parts whose squares
     overflow; they are in nmodes and k2sum and in no other sum.
   Collective over the ranks exactly as pf_fmax_pdf is: every rank sums the rows of its own ky-slab (with a replicated delta(k)
     too: its own n/P rows), the totals come through the installed pf_allreduce_fn (u64 and double) and every rank returns the
     box's numbers.  Every transform path (pf_transform_path 0, 1, 2) is served.
   The call reads the spectrum and changes nothing: products, flags, pf_device_bytes after the call and the arithmetic setting
     are as before; its scratch is allocated for the call and freed before it returns.
   No floating-point atomics: terms are added as fixed-point integers scaled to the largest term of their own shell (radius),
     so the result is bitwise the same from run to run and for any launch geometry; what is dropped lies below 2^-95 of that
     largest term.  The integer columns are identical for every rank count, the double ones differ between rank counts by rounding.
   Refused (1, pf_last_error, nothing launched): null ctx / nmodes / k2sum / power / info, which outside 0..3, ns outside
     [0, PF_MAX_SMOOTH], ns > 0 with a null radius_cells or variance, a radius that is negative or not finite, no density set
     (which = 0), no resident source spectrum (which >= 1).
   pf_debug_power_spectrum: test tap without a context, the production kernels on the rows y0 .. y0 + nyl - 1 of a caller's
     spectrum -- a ky-slab [nyl][n (kx)][n/2+1][2] in fp64 on the host, converted to field_bytes on the way in; it returns that
     slab's partial sums (the nmodes add up to info->modes = nyl n n).
   pf_debug_power_times: with PF_POWER_TIMES=1 in the environment, ms[0] = device ms of the last call between events; 0 otherwise. */
int pf_power_bins(int n);   /* number of shells for a grid of n points per side */
typedef struct {
  unsigned long long modes;      /* modes of this call's spectrum, full sphere: n^3 over all ranks */
  unsigned long long nonfinite;  /* modes with a NaN or infinite part: counted here, in no sum */
} pf_power_info;
int pf_power_spectrum(pf_ctx *ctx, int which, int ns, const double *radius_cells,
                      unsigned long long *nmodes, unsigned long long *k2sum, double *power,
                      double *variance, pf_power_info *info);
int pf_debug_power_spectrum(int field_bytes, int n, int y0, int nyl, const double *spec_host,
                            int ns, const double *radius_cells,
                            unsigned long long *nmodes, unsigned long long *k2sum, double *power,
                            double *variance, pf_power_info *info);
int pf_debug_power_times(double *ms);

/* --- matter density of the LPT-displaced particles and its spectra ---
   What the reference checks its mode 3 with (the auto and cross power of the particle density against the linear field, the plots
   under tests/ICs_piti_vs_pinocchio), from the twelve displacement columns in HBM: cloud-in-cell assignment of one particle per
   cell, the density contrast, the context's forward transform, and shell sums with the resident delta(k).  Mass assignment and
   spectra have no counterpart in the reference's code; the positions are its initialize_POS (src/write_snapshot.c:907-954).
   Position of the particle of global cell (q0, q1, q2), axis j, PRODFLOAT T, columns k = j, 3 + j, 6 + j, 9 + j of vel12 (those of
     LPT orders the context does not compute read zero):
       pos = (T)((double)q_j + 0.5 + (double)V1);  pos = pos + V2;  pos = pos + (V31 + V32);
       if (pos >= (T)n) pos -= (T)n;  if (pos < 0) pos += (T)n;                         (once, in T arithmetic)
     weight != NULL: each column value v of order k (0 Zel'dovich, 1 2LPT, 2 3LPT(a), 3 3LPT(b)) is first replaced by
     (T)(weight[k] (double)v) -- {1,0,0,0} gives the Zel'dovich positions, {1,1,0,0} 2LPT, from the same columns.
   A particle with a position that is not finite on any axis is counted in info->nonfinite, one outside [0, n] after the single wrap
     in info->outside; neither is deposited.  The others are counted in info->deposited.
   CIC in integers: u = pos - 0.5, i0 = floor(u), d = u - i0, t = (uint32)(d 65536) truncated; weight 65536 - t to cell i0 mod n and
     t to (i0 + 1) mod n; the eight contributions are the products of three such factors as 64-bit integers, so every deposited
     particle adds exactly 2^48 and the grid is the same bits for any order of the additions.  Headroom: fewer than 2^16 whole
     particles may meet in one cell (info->max_cell, in units of 2^-48 particle, says how close a call came).
     PF_MATTER_NGP: the whole 2^48 to the cell floor(pos) mod n.
   delta = cell / 2^48 - 1 in double, rounded once to the field type.  info->empty_cells, info->max_cell and
     info->sum_hi32 2^32 + info->sum_lo32 = deposited 2^48 (the sums of the high and low 32 bits of the cells) come from the same pass.
   density_host != NULL: delta of this rank's slab [nxl][n][n] as the transform reads it, widened to fp64.
   Shells, weights, nmodes and k2sum: exactly pf_power_spectrum's.  power[b] = sum of w |delta_m|^2 / N^6.  cross != NULL:
     cross[b] = (sum of the positive terms w Re(delta_m conj delta) - sum of the negated negative ones) / N^6 with the resident
     delta(k), each of the two a fixed-point sum of its own, the difference formed once in double.  Parts are widened to double
     first; |delta_m|^2 = re^2 + im^2 and Re(..) = re_m re + im_m im are two products and a sum, each rounded once.
     PF_MATTER_DECONVOLVE: every term carries (c[|kx|] c[|ky|]) c[kz], c[j] = sinc(pi j / n)^(-p), p = 1 for NGP and 2 for CIC,
     squared for power and once for cross.  info->nonfinite_modes: modes (counted with w) with a term that is not finite: in nmodes
     and k2sum and in no other sum.  info->modes = n^3.  No floating-point atomics: the bits are the same for any launch geometry.
   One rank only: particles leave their x-slab (pf_matter_power_slabs below is the collective call).  Every transform path, both field and both product types.
   The grid (8 bytes per cell) and the tables are allocated for the call and freed before it returns; delta and its spectrum live in
     the scratch field of the transform taps (pf_forward_transform).  pf_device_bytes, the products, the resident spectra, the
     arithmetic setting and every state flag are as before.
   Refused (1, pf_last_error, nothing launched): null ctx / nmodes / k2sum / power / info, unknown flag bits, a weight that is not
     finite, products not computed, cross != NULL without a density, more than one rank, a failed allocation (with the bytes).
   pf_debug_matter_deposit: test tap without a context, the production deposit on a caller's columns [12][n^3] of pb-byte
     PRODFLOATs (x0 = 0, nxl = n) -> the grid [n^3] and the counters of info (modes = 0).
   pf_debug_matter_shells: the production shell passes on the rows y0 .. y0 + nyl - 1 of two caller's spectra, ky-slabs
     [nyl][n (kx)][n/2+1][2] in fp64 converted to field_bytes on the way in; spec_lin (and cross) may be NULL.
   PF_MATTER_LDS (environment, read per call; default 1): the deposit stages bricks of 4 x 4 x 16 particles in an LDS tile where n is a
     multiple of 16 and nxl one of 4; 0, or any other grid: one particle per lane straight into the grid.  The grids are identical.
   pf_debug_matter_times: with PF_MATTER_TIMES=1 in the environment, ms[0..3] = device ms of the deposit (with the clearing of the
     grid), the contrast, the transform and the shell passes of the calling thread's last call; 0 otherwise.
   pf_debug_matter_form: what the calling thread's last call launched -- form[0] = the deposit (0 one particle per lane, 1 LDS-staged,
     -1 none yet), form[1] = the scans of its shell passes (1: one scan for the three sums, 3: a scan per sum -- grids above about
     1800, or PF_MATTER_SCAN_EACH=1, which the tests use to reach that way on a small grid; 0 none yet). */
#define PF_MATTER_NGP 1
#define PF_MATTER_DECONVOLVE 2
typedef struct {
  unsigned long long deposited, nonfinite, outside, empty_cells, max_cell, sum_hi32, sum_lo32, modes, nonfinite_modes;
} pf_matter_info;
int pf_matter_power(pf_ctx *ctx, int flags, const double *weight,
                    unsigned long long *nmodes, unsigned long long *k2sum, double *power, double *cross,
                    double *density_host, pf_matter_info *info);
int pf_debug_matter_deposit(int pb, int n, const void *vel12_host, int flags, const double *weight,
                            unsigned long long *grid_host, pf_matter_info *info);
int pf_debug_matter_shells(int field_bytes, int n, int y0, int nyl, const double *spec_m, const double *spec_lin,
                           int flags, unsigned long long *nmodes, unsigned long long *k2sum, double *power, double *cross,
                           pf_matter_info *info);
int pf_debug_matter_times(double *ms);
int pf_debug_matter_form(int *form);

/* --- the same on any number of ranks: pf_matter_power_slabs ---
   pf_matter_power for a context of P x-slabs, collective over its ranks like pf_power_spectrum: ON ANY NUMBER OF RANKS EVERY RANK
   RECEIVES EXACTLY THE BITS ONE RANK RETURNS FOR THE SAME BOX.  Arguments, flags, positions, integer CIC / NGP, contrast, shells,
   deconvolution and weight are pf_matter_power's, word for word; every rank passes the same flags and weight.  nmodes, k2sum, power
   and cross are the box's on every rank; density_host is this rank's slab [nxl][n][n]; info is the box's: deposited, nonfinite,
   outside, empty_cells, sum_hi32, sum_lo32 and nonfinite_modes summed over the ranks, max_cell the largest over the ranks,
   modes = n^3.
   The particles of a slab leave it, so:
     reach     one pass over the four x columns (k_matter_reach): of every particle whose x position is finite and inside [0, n] the
               x planes it adds to (CIC: i0 and, where its weight t is not zero, i0 + 1; NGP: floor(pos)) as signed minimal-image
               offsets s = ((plane - q0 + n/2) mod n) - n/2 from its own plane q0; Hlo = max(0, -min s), Hhi = max(0, max s).  A
               particle that only its y or z position keeps out of the grid still counts: a window can be a plane wider than
               needed, never narrower.  The ranks agree on the largest Hlo and Hhi (first all-reduce).
     window    every rank deposits its own particles into the planes [x0 - Hlo, x0 + nxl + Hhi) (mod n), or into the whole box once
               nxl + Hlo + Hhi >= n: nothing a particle adds falls outside.
     exchange  plane g belongs to rank g / nxl.  Rank r sends rank q != r a block of B planes, slot j the j-th (ascending local index)
               plane of q inside the window of r; B is the longest such list over all pairs, found by every rank from (n, P, Hlo, Hhi)
               alone.  ONE call of the context's all-to-all (pf_set_exchange / pf_init_rccl / the fabric), bytes_per_peer = 8 B n^2;
               the owner adds the filled slots to its planes (k_matter_fold: 64-bit integer adds, no atomics).  The uniform
               all-to-all carries P B planes per rank of which only those of the neighbours are filled.  Hlo = Hhi = 0, or one
               rank: no exchange.
     spectra   the contrast of the rank's own planes goes into the field the slab transform reads (receive field 0 with more than
               one rank, as in pf_forward_transform); the scans' maxima of every shell are taken over the ranks, then every rank
               adds its limbs under the box's exponent and the integer tables are summed over the ranks: the sums of the one-rank call.
   The installed all-reduce only sums: a maximum over the ranks is the sum of vectors in which every rank fills its own slot.
   Memory: (wn + 2 P B) n^2 8 bytes (wn = nxl + Hlo + Hhi, at most n: the window, the send and the receive blocks) and the tables,
     allocated for the call and freed before it returns.  pf_device_bytes, the products, the resident spectra, the arithmetic
     setting and every state flag are as before; a sweep after the call gives what it gave before.
   With one rank the call is pf_matter_power bit for bit, with the reach pass in front and no exchange.
   Refused (1, pf_last_error names pf_matter_power_slabs) as pf_matter_power refuses, except for the number of ranks, and: more
     than one rank without an installed all-to-all and all-reduce; an odd grid on more than one rank.  A rank that refuses on its
     own tells the others in the first all-reduce: every rank returns 1 and nothing but the reach pass of the other ranks was
     launched.  A failed allocation (message with the bytes) is agreed on in a second all-reduce, before any rank enters the all-to-all.
   pf_debug_matter_times: the reach pass, pack, exchange and fold count to ms[0] (deposit).
   pf_debug_matter_slabs: collective test tap on a live context of any rank count: the production reach pass, deposit, exchange and
     fold on the caller's columns [12][nxl*n*n] of this rank's slab (PRODFLOATs of the context's product type) -> this rank's planes
     of the grid [nxl][n][n] and the box's counters in info (modes = 0).  Needs no density, no products; leaves the context as it
     found it.
   pf_debug_matter_exchange: what the calling thread's last pf_matter_power_slabs / pf_debug_matter_slabs did: out[0] = form (0 no
     exchange: one rank or reach 0 both ways, 1 ghost planes, 2 every rank deposits the whole box), out[1] / out[2] = reach below /
     above in planes (common to all ranks), out[3] = planes of the deposit window, out[4] = planes per peer block, out[5] =
     bytes_per_peer handed to the all-to-all (0 without an exchange). */
int pf_matter_power_slabs(pf_ctx *ctx, int flags, const double *weight,
                          unsigned long long *nmodes, unsigned long long *k2sum, double *power, double *cross,
                          double *density_host, pf_matter_info *info);
int pf_debug_matter_slabs(pf_ctx *ctx, const void *vel12_slab_host, int flags, const double *weight,
                          unsigned long long *grid_slab_host, pf_matter_info *info);
int pf_debug_matter_exchange(unsigned long long out[6]);

/* --- halo power spectrum and bias: pf_halo_power ---
   The clustering of a halo catalogue, the second standard check of a run after the mass function: per mass bin the auto power of
   the haloes, their cross power with the resident delta(k) (the bias is b(k) = cross / P_dd of pf_power_spectrum, shell by shell)
   and the integers of the shot noise.  The reference has no code for it; the arithmetic is defined here.
   Inputs: pos[3 count] (doubles, x y z of halo i at 3 i) and mass[count] (ints) are host arrays, as in pf_map_update -- x and n of
     pf_catalog's records, or Pos (plus the start of the sub-box) and Mass of groups[].  Only they are uploaded, once per call: 28
     bytes per halo.
   Position on axis j: p = pos[3 i + j] * scale, one double product, in grid cells of the global box (scale = 1 / (InterPartDist
     hfactor) brings the Mpc/h of a catalogue to cells; 1 when the positions are in cells already).  One wrap: if (p >= n) p -= n;
     if (p < 0) p += n;  A halo with p
     not finite on any axis is `nonfinite`, one with p outside [0, n] on any axis after the single wrap is `outside`; neither is
     deposited nor enters a bin's sums.
   Bins: bin b, 0 <= b < nbins, 1 <= nbins <= PF_HALO_MAX_BINS, takes the haloes with mass_range[2 b] <= mass <= mass_range[2 b + 1],
     both ends inclusive.  Ranges may overlap (cumulative thresholds are the usual use).
   Weight: W = 1, or W = mass with PF_HALO_MASS_WEIGHT.
   Per bin: power[b nb + s] and cross[b nb + s], nb = pf_power_bins(n), and info[b].  nmodes[nb] and k2sum[nb] are returned once:
     they depend on the grid only.
   info[b], over the haloes whose mass lies in the range of bin b: nonfinite and outside as above; selected = the others, the
     haloes of the bin; weight_sum = sum of W over the selected; weight2_hi 2^64 + weight2_lo = sum of W^2, a 128-bit integer
     (formed from two 64-bit sums of the high and low 32 bits of W^2: no floating point).  The shot-noise level of power / nmodes
     is sum W^2 / (sum W)^2; the caller forms it.
   Assignment in integers, unit 2^30: CIC: u = p - 0.5, i0 = floor(u), d = u - i0, t = (uint32)(d 1024) truncated; factor 1024 - t
     to the cell i0 mod n and t to (i0 + 1) mod n; the eight contributions are W times the product of three factors, 64-bit
     integers.  PF_HALO_NGP: W << 30 into floor(p) mod n.  Every deposited halo adds exactly W 2^30: the grid is the same bits for
     any order of the additions (and of the list).
   Headroom is a condition: weight_sum >= 2^34 could overflow a cell, so the call returns 1 after the selection pass, the message
     naming the bin, and nothing is deposited.  (A real catalogue has sum M <= n^3 <= 2^33.)
   Contrast: mean = (double)(weight_sum << 30) / (double)n^3; delta = (double)cell / mean - 1.0, rounded once to the field type
     (the file is compiled without contraction).  info[b].empty_cells and max_cell (units of 2^-30) come from that pass.
   An empty bin (weight_sum == 0) launches no transform: zeros in power and cross, selected = 0 (modes = n^3 all the same).
   Shells, the weights w, the deconvolution (PF_HALO_DECONVOLVE: p = 1 for NGP, 2 for CIC), the two-sided cross sums,
     nonfinite_modes and modes: exactly pf_matter_power's -- the same passes (pf_power.hip) behind the context's own forward
     transform.  No floating-point atomics anywhere.
   cross == NULL needs no density; cross != NULL needs the resident delta(k).  Products are not needed.
   Any number of ranks, collective: every rank passes the WHOLE list, in any order, and deposits only what falls on the planes of
     its own x-slab [x0, x0 + nxl): no grid is exchanged.  The list-derived counters are equal on every rank by construction;
     empty_cells, max_cell, nonfinite_modes and the shell tables go through the installed all-reduce as in pf_matter_power_slabs:
     every rank returns the bits one rank returns for the same list.  Before any deposit the ranks agree in ONE all-reduce (every
     rank fills a slot of its own: count, nbins, flags and each bin's selected and weight_sum) that these are the same everywhere
     -- the summed value is then P times the rank's own -- ; otherwise every rank returns 1.  A rank that refuses on its own (a
     bad argument, a failed allocation, the headroom) raises its flag in the same all-reduce and every rank returns 1.
   The context is left as found: the grid (8 bytes per cell of the slab), the tables and the uploaded list are allocated for the
     call and freed before it returns; delta and its spectrum live in the scratch field of the transform taps; pf_device_bytes,
     products, resident spectra, arithmetic setting and flags are unchanged, and a sweep afterwards gives what it gave before.
   Refused (1, pf_last_error, nothing launched): a null ctx / pos / mass / mass_range / nmodes / k2sum / power / info, unknown
     flag bits, nbins out of range, a range with lo < 1 or hi < lo, scale not finite or <= 0, count > 2^31, cross without a
     density, more than one rank without an exchange and all-reduce installed, a failed allocation (with the bytes).
   pf_debug_halo_deposit: test tap without a context: the production selection and deposit for the one range [lo, hi] on the
     planes [x0, x0 + nxl) of a grid of n (x0 + nxl <= n) -> the grid [nxl][n][n] and the counters (empty_cells and max_cell of
     those planes; modes = nonfinite_modes = 0).
   pf_debug_halo_times: with PF_HALO_TIMES=1 in the environment, ms[0..4] = device ms of the selection, the deposits (with the
     clearing of the grid), the contrasts, the transforms and the shell passes of the calling thread's last pf_halo_power, summed
     over its bins; 0 otherwise.  The upload is in none of them. */
#define PF_HALO_NGP 1
#define PF_HALO_DECONVOLVE 2
#define PF_HALO_MASS_WEIGHT 4
#define PF_HALO_MAX_BINS 8
typedef struct {
  unsigned long long selected, weight_sum, weight2_hi, weight2_lo, nonfinite, outside,
                     empty_cells, max_cell, modes, nonfinite_modes;
} pf_halo_info;
int pf_halo_power(pf_ctx *ctx, int flags, size_t count, const double *pos, double scale, const int *mass,
                  int nbins, const int *mass_range,
                  unsigned long long *nmodes, unsigned long long *k2sum,
                  double *power, double *cross, pf_halo_info *info);
int pf_debug_halo_deposit(int n, int x0, int nxl, int flags, size_t count, const double *pos, double scale,
                          const int *mass, int lo, int hi, unsigned long long *grid_host, pf_halo_info *info);
int pf_debug_halo_times(double *ms);   /* PF_HALO_TIMES=1: select, deposit, contrast, transform, shells of the last call */

/* --- redshift-space multipoles of the halo power: pf_halo_multipoles ---
   pf_halo_power with the list moved along one axis of the box by its velocities (the plane-parallel line of sight `los`, 0, 1 or
   2) and every mode weighted by the Legendre polynomials L0, L2, L4 of mu = k_los / |k|: per mass bin the monopole, quadrupole and
   hexadecapole sums of the auto power and of the cross power with the resident delta(k).  Everything not said here is
   pf_halo_power's, word for word: flags, bins, weights, integer CIC / NGP, the headroom refusal, the contrast, empty bins, the
   collective protocol, "context left as found", the refusal conventions, and pf_debug_halo_times, which reports this call too.
   Position: vel is [3 count] like pos (the v of pf_catalog's records); only component los is read and uploaded (8 bytes per halo
     more).  On axis j != los, or with vel == NULL, s = pos[3 i + j]; on axis los s = pos[3 i + los] + vel[3 i + los] * vfac -- the
     product, then the sum, each rounded once.  Then p = s * scale and the single wrap of pf_halo_power.  vfac is position units per
     velocity unit: for km/s and Mpc/h it is (1 + z) / (100 E(z)); the caller forms it.  A velocity that is not finite makes the
     halo `nonfinite` even with vfac == 0 (NaN 0 is NaN); vel == NULL is real space.  A halo moved by more than a box is `outside`.
   Weights: with s_los the signed wavenumber of the mode on axis los, a = s_los^2 and k2 as in pf_power_spectrum, exact integers:
     L0 = 1; for k2 > 0  L2 = (double)(3 a - k2) / (double)(2 k2)  and  L4 = (double)(35 a^2 - 30 a k2 + 3 k2^2) / (double)(8 k2^2),
     the integers formed in 64 bits (below 2^50 for n <= 2048), one division each; for k2 = 0  L2 = L4 = 0 and the mode enters no
     sum of l > 0.  A mode and its Hermitian partner share mu^2, so the weights w of the half-spectrum stand.
   Terms: t L_l, one product, of the auto and the cross term of pf_matter_power (deconvolved or not).  PF_MULTIPOLE_SUMS = 11
     positive fixed-point sums per shell, each under the exponent of its own largest term:  0 auto l0;  1, 2 auto l2, the positive
     and the negated negative terms;  3, 4 auto l4;  5, 6 cross l0;  7, 8 cross l2;  9, 10 cross l4.  A mode with a term that is not
     finite is in nmodes and k2sum and in no other sum.
   Outputs: with nb = pf_power_bins(n), power[(b 3 + l/2) nb + s] = (positive - negative) / N^6, cross likewise or NULL (then no
     density is needed and the six cross sums are skipped).  No factor (2 l + 1): P_l = (2 l + 1) power / nmodes Box^3 is the
     caller's.  The l = 0 rows are pf_halo_power's bits on the same positions.  nmodes and k2sum are pf_power_spectrum's.
   The agreeing all-reduce of the ranks also covers los, the bits of vfac and whether vel is NULL.
   Refused in addition to pf_halo_power's list (pf_last_error names pf_halo_multipoles): los outside 0..2, vfac not finite,
     vfac != 0 with vel == NULL.
   A shell pass carries as many of the sums as fit its LDS tables, spread evenly over the passes; the sums are integers, so the
     grouping changes no bit.  PF_MULTIPOLE_SCAN_EACH=1 (environment, read per call, tests only): one sum per scan and per
     accumulation.  pf_debug_multipole_form: form[0] = scans, form[1] = accumulation passes launched by the calling thread's last
     shell pass (0: none yet).
   pf_debug_halo_deposit_rsd: pf_debug_halo_deposit with the velocities; vel == NULL gives its grids.
   pf_debug_multipole_shells: pf_debug_matter_shells with the weights: power and cross are [3][nb]; parts (may be NULL) is
     [PF_MULTIPOLE_SUMS][nb], each positive sum / N^6; of info only modes and nonfinite_modes are filled. */
#define PF_MULTIPOLE_ORDERS 3   /* l = 0, 2, 4 */
#define PF_MULTIPOLE_SUMS  11   /* positive sums per shell, see above */
int pf_halo_multipoles(pf_ctx *ctx, int flags, size_t count, const double *pos, const double *vel,
                       double scale, double vfac, int los, const int *mass, int nbins, const int *mass_range,
                       unsigned long long *nmodes, unsigned long long *k2sum,
                       double *power, double *cross, pf_halo_info *info);
int pf_debug_halo_deposit_rsd(int n, int x0, int nxl, int flags, size_t count, const double *pos, const double *vel,
                              double scale, double vfac, int los, const int *mass, int lo, int hi,
                              unsigned long long *grid_host, pf_halo_info *info);
int pf_debug_multipole_shells(int field_bytes, int n, int y0, int nyl, const double *spec_m, const double *spec_lin,
                              int flags, int los, unsigned long long *nmodes, unsigned long long *k2sum,
                              double *power, double *cross, double *parts, pf_matter_info *info);
int pf_debug_multipole_form(int *form);

/* --- two-point correlation function of the haloes: pf_halo_correlation ---
   The third standard check of a catalogue: per mass bin the circular correlation of the halo contrast with itself, xi_hh, and with
   the resident density, xi_hd, summed in shells of the separation |r| with the Legendre weights L0, L2, L4 of mu = r_los / |r| --
   where the BAO peak and the large-scale RSD are read off.  The list, the bins, the deposit, the contrast, the forward transform and
   the collective protocol are pf_halo_multipoles', word for word: flags, inclusive mass ranges, pos + vel * vfac on axis los (vel ==
   NULL: real space), the single wrap and the nonfinite / outside counters, integer CIC / NGP in units of 2^30, the headroom refusal,
   the contrast with the bin's own mean, an empty bin launching nothing and returning zeros, every rank passing the whole list, the
   agreeing all-reduce (with los, vfac and whether vel is NULL), "context left as found", the refusal conventions.  One body serves
   the three calls.
   Form pass: every stored mode of delta_h(k) (the ky-slab half-spectrum) becomes ((F)(t / (double)N3), 0), N3 = n^3 as a double:
     one division and one rounding to the field type F.  For xi: t = the auto term of pf_matter_power (with PF_HALO_DECONVOLVE the
     deconvolution factors squared); for xi_cross: t = the cross term with the resident delta(k), the factors once.  The k = 0 mode is
     written as zero.  A term that is not finite is written as zero and counted, with the mode's weight w, in
     info[b].halo.nonfinite_modes (both passes add to it).  With xi_cross the cross spectrum is formed first, into one field
     allocated for the call and freed before it returns; the auto spectrum is formed where the reverse transform works.
   Reverse transform: the context's, with its 1 / N^3: because of the division above the real field is the circular correlation
     sum_x delta(x) delta(x + r) / N^3 directly, and the zero-lag cell of the auto field is the variance of the contrast.
   Shell pass, on this rank's x-slab of that field: the cell (x, y, z) lies at the signed separations s = i > n/2 ? i - n : i (n/2
     stays positive); r2 = sx^2 + sy^2 + sz^2, its shell is that of pf_power_spectrum with r2 for k2, nb = pf_power_bins(n) shells,
     weight 1.  L2 and L4 are pf_halo_multipoles' from a = s_los^2 and r2 (at r2 = 0, L2 = L4 = 0).  The cell's value v gives the
     terms v, v L2, v L4, one product each; a term that is not zero enters, as its absolute value, the positive or the negative sum
     of its order -- l = 0 can be negative here, so there are six positive sums per field, PF_CORR_SUMS = 12 for both: auto l0 +, -;
     l2 +, -; l4 +, -; then the same six of the cross field.  A value that is not finite enters ncells and r2sum and no other sum,
     and is counted in nonfinite_cells.  The sums are pf_power_spectrum's fixed point (exponents from a scan pass, three limbs,
     integer adds: no floating-point atomics), as many sums per pass as the LDS tables hold; the grouping changes no bit.
     PF_CORR_SCAN_EACH=1 (environment, read per call, tests only): one sum per scan and per accumulation.  Over the ranks the
     per-shell maxima go through slots of the all-reduce and the integer tables are summed, as in pf_halo_multipoles: every rank
     returns the bits of one rank.
   Outputs: ncells[nb] and r2sum[nb], returned once (they are nmodes and k2sum of pf_power_spectrum: the whole lattice of
     separations has the counts of the Hermitian-weighted half-spectrum).  xi[(b 3 + l/2) nb + s] = (positive - negative), formed
     once in double; xi_cross likewise, or NULL: then no density is needed, no extra field is allocated and no second reverse
     transform runs.  No factor (2 l + 1) and no division by ncells: xi_l(r) = (2 l + 1) xi / ncells is the caller's to form.
     info[b].halo is what pf_halo_multipoles returns for the bin (modes = n^3); info[b].cells = n^3; info[b].nonfinite_cells is
     summed over both fields and over the ranks.
   Refused (1, pf_last_error names pf_halo_correlation, nothing launched): everything pf_halo_multipoles refuses; a null ncells,
     r2sum, xi or info; xi_cross without a density.  A failed allocation names its bytes and, on several ranks, is agreed on before
     any collective.
   pf_debug_corr_form: test tap without a context: the production form pass on the rows y0 .. y0 + nyl - 1 of the caller's fp64
     spectra (ky-slabs [nyl][n][n/2+1] complex, staged as pf_debug_multipole_shells stages them); which = 0 auto, 1 cross (needs
     spec_lin); flags: PF_HALO_NGP | PF_HALO_DECONVOLVE; spec_out: the formed spectrum widened to fp64 in the same layout; of info
     only nonfinite_modes and modes are filled.
   pf_debug_corr_shells: test tap without a context: the production shell passes on the planes x0 .. x0 + nxl - 1 of the caller's
     fp64 real field [nxl][n][n], converted to field_bytes on the way in -> ncells, r2sum, xi[3][nb], parts[6][nb] (the positive
     sums; may be NULL) and the cells that are not finite.
   pf_debug_corr_passes: passes[0] = scans, passes[1] = accumulation passes launched by the calling thread's last separation-space
     shell pass (0: none yet), as pf_debug_multipole_form tells them of the multipole passes.
   pf_debug_corr_times: with PF_CORR_TIMES=1 in the environment, ms[0..5] = device ms of the selection, the deposits, the contrasts,
     the transforms (forward and reverse), the form passes and the shell passes of the calling thread's last pf_halo_correlation,
     summed over its bins; 0 otherwise. */
#define PF_CORR_ORDERS 3    /* l = 0, 2, 4 */
#define PF_CORR_SUMS   12   /* positive sums per shell: auto l0 +,-; l2 +,-; l4 +,-; then the same six for cross */
typedef struct { pf_halo_info halo; unsigned long long cells, nonfinite_cells; } pf_corr_info;
int pf_halo_correlation(pf_ctx *ctx, int flags, size_t count, const double *pos, const double *vel,
                        double scale, double vfac, int los, const int *mass, int nbins, const int *mass_range,
                        unsigned long long *ncells, unsigned long long *r2sum,
                        double *xi, double *xi_cross, pf_corr_info *info);
int pf_debug_corr_form(int field_bytes, int n, int y0, int nyl, const double *spec_m, const double *spec_lin,
                       int flags, int which, double *spec_out, pf_matter_info *info);
int pf_debug_corr_shells(int field_bytes, int n, int x0, int nxl, const double *real_host, int los,
                         unsigned long long *ncells, unsigned long long *r2sum,
                         double *xi, double *parts, unsigned long long *nonfinite_cells);
int pf_debug_corr_passes(int *passes);
int pf_debug_corr_times(double *ms);   /* PF_CORR_TIMES=1: select, deposit, contrast, transforms (forward and reverse), form, shells */

/* --- bispectrum of the haloes: pf_halo_bispectrum ---
   The three-point check of a catalogue, by the FFT estimator of Scoccimarro (2000) / Sefusatti et al. (2016): per k-bin the halo
   contrast is band-filtered, and the sum over cells of the product of three filtered fields is the sum of delta delta delta over
   the closed triangles of the three bins.  The list, the mass bins, the deposit, the contrast, the forward transform and the
   collective protocol are pf_halo_correlation's, word for word: flags, inclusive mass ranges, pos + vel * vfac on axis los (vel ==
   NULL: real space), the single wrap, integer CIC / NGP, the headroom refusal, an empty mass bin launching nothing and returning
   zeros, every rank passing the whole list, the agreeing all-reduce (which also covers kmin, dk and nk), "context left as found".
   k-bins: nk linear bins in integer units of the fundamental, kmin >= 1, dk >= 1, 1 <= nk <= PF_BISPEC_MAX_KBINS.  Bin i takes the
     modes with (kmin + i dk)^2 <= k2 < (kmin + (i + 1) dk)^2, k2 the exact integer of pf_power_spectrum; kmax = kmin + nk dk.  A
     sum over cells closes triangles modulo n; with 3 kmax <= n every component sum is below n in magnitude and only true triangles
     close, so 3 kmax > n is refused: a condition, not a tolerance.
   Mask pass, on the ky-slab half-spectrum: the data field of bin i holds a stored mode inside the bin as it is -- with
     PF_HALO_DECONVOLVE each part times the window factor (c[|kx|] c[|ky|]) c[kz] of pf_halo_correlation's table, once -- rounded
     to the field type F, and zero outside (k = 0 is in no bin); the count field holds ((F)N3, 0) inside and zero outside.  A mode
     inside the bin that is not finite is written as zero and counted with its Hermitian weight in nonfinite_modes; the same pass
     counts the bin's modes with their Hermitian weights, kmodes[i].  The count fields are made once per call and read no spectrum.
   Reverse transform: the context's, with its 1 / N3: D_i(x), the band-filtered contrast, and I_i(x) with I_i(0) == kmodes[i].
   Keep pass: every reversed field is copied into a compact store [nxl][n][n] of F, nk stores allocated for the call; the pass
     finds the largest |value| M_i (over the ranks through per-rank slots of the all-reduce) and the cells that are not finite,
     which are stored as zero and counted in nonfinite_cells.
   Triangles: the ordered bin triples i <= j <= l with kmin + l dk < 2 kmin + (i + j + 2) dk; the others cannot close and are
     neither computed nor returned.  pf_bispectrum_triangles returns their number nt (-1: kmin, dk or nk out of range) and, with
     ijl != NULL, the list [nt][3] in lexicographic order; the outputs below are indexed by it.
   Triple pass: per closed triple and cell t = (a b) c in double of the three stores' values, each product rounded once; |t| enters
     the positive or the negative sum of the triple in pf_power_spectrum's fixed point under the exponent of M = (M_i M_j) M_l,
     formed the same way (rounding is monotone: |t| <= M; no scan pass).  Integer adds only, no floating-point atomics: the bits
     are the same for any launch geometry, any order of the list and any number of ranks.  psum[i] = sum_x D_i^2 likewise, one
     positive sum under M_i M_i.  The count fields go through the same pass.
   Outputs: bsum[b nt + t] = positive - negative of the data fields of mass bin b: the sum over the closed triangles of delta delta
     delta / N3^2.  ntri[t] = positive - negative of the count fields over N3: the number of (k1 in i, k2 in j, k3 in l) with k1 +
     k2 + k3 = 0, an integer up to the transforms' error, returned once.  psum[b nk + i]; kmodes[i].  B = Box^6 bsum / (N3 ntri) and
     P_i = Box^3 psum / (N3 kmodes) are the caller's to form, as is the shot noise (unit weights: from info[b].halo.selected).
     info[b].halo as pf_halo_correlation fills it (nonfinite_modes: summed over the k-bins), cells = N3, nonfinite_cells summed
     over the k-bins and the ranks.
   Refused (1, pf_last_error names pf_halo_bispectrum, nothing launched): everything pf_halo_correlation refuses of the list; a null
     kmodes, ntri, bsum, psum or info; kmin, dk or nk out of range; 3 kmax > n; n > 1024 (a limb counter takes N3 terms below 2^32
     and stays below 2^63 up to there); a failed allocation, naming its bytes (the nk stores, one copy of the spectrum, the tables)
     and, on several ranks, agreed on before any collective.
   pf_debug_bispec_mask: test tap without a context: the production mask pass of k-bin `bin` on the rows y0 .. y0 + nyl - 1 of the
     caller's fp64 ky-slab [nyl][n][n/2+1] complex; kind 0 the data field, 1 the count field (here the spectrum is read and a mode
     that is not finite is zeroed and counted in either kind); flags: PF_HALO_NGP | PF_HALO_DECONVOLVE -> the field widened to fp64,
     kmodes and nonfinite_modes of the rows.
   pf_debug_bispec_triples: test tap without a context: the production keep, triple and pair passes on the planes x0 .. x0 + nxl - 1
     of the caller's nk fp64 real fields [nk][nxl][n][n], converted to field_bytes on the way in -> sums[nt], parts[2][nt] (the
     positive sums: of the positive terms, of the negated negative ones), pair[nk], maxima[nk], nonfinite_cells.
   pf_debug_bispec_times: with PF_BISPEC_TIMES=1 in the environment, ms[0..6] = device ms of the selection, the deposits, the
     contrasts, the transforms (forward and reverse), the mask, keep and triple passes of the calling thread's last
     pf_halo_bispectrum, summed over its mass bins and the count fields; 0 otherwise. */
#define PF_BISPEC_MAX_KBINS 32
typedef struct { pf_halo_info halo; unsigned long long cells, nonfinite_cells; } pf_bispec_info;
int pf_bispectrum_triangles(int kmin, int dk, int nk, int *ijl);
int pf_halo_bispectrum(pf_ctx *ctx, int flags, size_t count, const double *pos, const double *vel,
                       double scale, double vfac, int los, const int *mass, int nbins, const int *mass_range,
                       int kmin, int dk, int nk,
                       unsigned long long *kmodes, double *ntri, double *bsum, double *psum, pf_bispec_info *info);
int pf_debug_bispec_mask(int field_bytes, int n, int y0, int nyl, const double *spec, int flags, int kind,
                         int kmin, int dk, int nk, int bin, double *spec_out,
                         unsigned long long *kmodes, unsigned long long *nonfinite_modes);
int pf_debug_bispec_triples(int field_bytes, int n, int x0, int nxl, const double *fields, int kmin, int dk, int nk,
                            double *sums, double *parts, double *pair, double *maxima, unsigned long long *nonfinite_cells);
int pf_debug_bispec_times(double *ms);   /* PF_BISPEC_TIMES=1: select, deposit, contrast, transforms, mask, keep, triples */

/* --- measurement --- */
int pf_get_cputime(pf_ctx *ctx, pf_cputime *t);
int pf_reset_cputime(pf_ctx *ctx);
/* per-kernel-class HIP-event statistics over the launches since the last reset
   (PF_FLAG_TIMING).  Fills up to `max` entries; returns the count in *n. */
typedef struct {
  char     name[48];
  uint64_t launches;
  double   total_ms;
  double   alg_bytes;   /* algorithmic HBM bytes summed over those launches */
} pf_kernel_stat;
int pf_kernel_stats(pf_ctx *ctx, pf_kernel_stat *out, int max, int *n);
int pf_reset_kernel_stats(pf_ctx *ctx);
int pf_synchronize(pf_ctx *ctx);
/* bytes of device memory held by the context */
size_t pf_device_bytes(pf_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* PINFMAX_H */
