/*
 * peaks_validation.c -- the reference's committed validation run (HMF_Validation/: 128^3, seed 486604, Eisenstein & Hu
 * spectrum, sigma8 = 0.8, nine smoothing radii) up to the first step of fragmentation, from a plain C host through the
 * C ABI of libpinfmax_hip.so: initial conditions and the collapse-time sweep on the device as in hmf_validation.c, then
 * count_peaks (src/fragment.c:605-706) where the Fmax column lives -- pf_count_peaks -- and the seeds of the first halos in
 * the order in which fragmentation opens them -- pf_select_peaks.  Prints the reference's own log line.
 *
 *     make -C examples && ./examples/peaks_validation
 *
 * Expected (HMF_Validation/log_RUN.txt): "Task 0 found 114993 peaks, 114993 in the well resolved region. Total number of
 * peaks: 114993" (this build: within one peak: it collapses one cell more than the reference).  The second part counts the
 * well resolved peaks of the four sub-boxes a run on four tasks would cut (2 x 2 x 1, a boundary layer of three cells): they add
 * up to the same total, which is how the reference's example log on four tasks comes by its number.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "../include/pinfmax.h"

#define NKNOTS 210 /* NBINS, src/pinocchio.h:65 */

/* growing mode of flat LCDM without radiation, D(a) = 2.5 Om H(a) int_0^a da' / (a' H(a'))^3, normalised to D(1) = 1
   (the reference integrates the equivalent ODE, src/cosmo.c:229-401); Gauss-Legendre in t with a' = a t^2 */
static double growth(double a, double om) {
  static const double xg[8] = {0.0950125098376374, 0.2816035507792589, 0.4580167776572274, 0.6178762444026438,
                               0.7554044083550030, 0.8656312023878318, 0.9445750230732326, 0.9894009349916499};
  static const double wg[8] = {0.1894506104550685, 0.1826034150449236, 0.1691565193950025, 0.1495959888165767,
                               0.1246289712555339, 0.0951585116824928, 0.0622535239386479, 0.0271524594117541};
  const double ol = 1.0 - om;
  double s = 0.0;
  const int panels = 64;
  for (int p = 0; p < panels; p++) {
    const double t0 = (double)p / panels, t1 = (double)(p + 1) / panels, c = 0.5 * (t0 + t1), h = 0.5 * (t1 - t0);
    for (int i = 0; i < 16; i++) {
      const double t = c + (i < 8 ? -xg[i] : xg[i - 8]) * h, w = wg[i & 7] * h;
      const double ap = a * t * t, H = sqrt(om / (ap * ap * ap) + ol);
      s += w * 2.0 * a * t / pow(ap * H, 3.0);
    }
  }
  return 2.5 * om * sqrt(om / (a * a * a) + ol) * s;
}

int main(void) {
  const int n = 128, ns = 9;
  const double h100 = 0.7, box = 128.0 / h100, cell = box / n; /* BoxSize 128 Mpc/h in true Mpc */
  const double radius[9] = {20.635922, 13.996056, 9.026099, 5.465945, 3.058354, 1.548258, 0.689079, 0.258729, 0.0};
  const double flast = 1.0; /* outputs.Flast = 1 + z of the last output, z = 0 */
  pf_config cfg = {n, 0, 1, 0, 8, 0};
  pf_ctx *ctx = NULL;
  pf_genic_params ic = {0.25, 0.044, h100, 0.96, box, 2.03146e7 /* PkNorm as logged */, 486604u, 0, 0, 0, NULL, NULL /* Eisenstein & Hu, no table */,
                        0 /* spectrum: by pk_n */, 0.0 /* no warm-dark-matter cut-off */, 0.0 /* UnitLength_in_cm: the default */};
  double x[NKNOTS], y[NKNOTS], rs[9], tv[9], d1;
  unsigned long long peaks[2], sum_good = 0;
  unsigned int seed_cell[3];
  float seed_f[3];
  size_t nseeds = 0;

  if (pf_create(&ctx, &cfg)) return 1; /* prints "ERROR on task 0: ..." itself */
  if (pf_genic_density(ctx, &ic)) return 1;
  d1 = growth(1.0, ic.Omega0);
  for (int i = 0; i < NKNOTS; i++) { /* SPLINE[SP_INVGROW]: x = log10 D(a), y = log10 a on log10 a = -4 + 0.02 i */
    y[i] = -4.0 + 0.02 * i;
    x[i] = log10(growth(pow(10.0, y[i]), ic.Omega0) / d1);
  }
  if (pf_set_invgrow(ctx, -1, x, y, NKNOTS)) return 1;
  for (int i = 0; i < ns; i++) rs[i] = radius[i] / cell; /* Rsmooth = R / CellSize, src/fmax.c:233 */
  if (pf_sweep(ctx, ns, rs, tv)) return 1;

  /* one task: the sub-box is the whole periodic box */
  if (pf_count_peaks(ctx, flast, NULL, peaks)) return 1;
  printf("Task 0 found %llu peaks, %llu in the well resolved region. Total number of peaks: %llu\n", peaks[0], peaks[1], peaks[1]);

  /* the seeds of the first three groups: descending Fmax (index_compare_F, src/fragment.c:118-126) */
  if (pf_select_peaks(ctx, flast, 3, seed_cell, seed_f, &nseeds)) return 1;
  for (size_t i = 0; i < 3 && i < nseeds; i++)
    printf("seed %zu: cell (%u, %u, %u), Fmax = %.6f\n", i, seed_cell[i] / (n * n), seed_cell[i] / n % n, seed_cell[i] % n, seed_f[i]);

  /* four tasks: 2 x 2 x 1 sub-boxes with a boundary layer of three cells, periodic along z */
  for (int t = 0; t < 4; t++) {
    const int b = 3, core = n / 2;
    pf_peak_region rg = {{(t / 2) * core - b, (t % 2) * core - b, 0}, {core + 2 * b, core + 2 * b, n}, {b, b, 0}};
    if (pf_count_peaks(ctx, flast, &rg, peaks)) return 1;
    printf("sub-box %d found %llu peaks, %llu in the well resolved region\n", t, peaks[0], peaks[1]);
    sum_good += peaks[1];
  }
  printf("Sum of the well resolved peaks of the four sub-boxes: %llu\n", sum_good);
  pf_destroy(ctx);
  return 0;
}
