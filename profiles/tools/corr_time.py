"""Times pf_halo_correlation beside pf_halo_multipoles on the same list and box: the box of bench.py's flagship workload (the
synthetic density, sigma0 = 2.5, slope -2), one rank, the synthetic catalogue of profiles/tools/halo_time.py with Gaussian velocities
of 1.5 cells along the line of sight, three cumulative bins, cloud-in-cell, deconvolved, with the cross field --
profiles/corr_notes.md.

After a warm-up call of each: `reps` calls of each, the device ms of the phases between events (PF_CORR_TIMES=1 and
pf_debug_corr_times: select, deposit, contrast, transforms forward and reverse, form, shells; PF_HALO_TIMES=1 and
pf_debug_halo_times for the multipole call; each summed over the three bins) and the wall ms.  Then the correlation call with one
sum per shell pass (PF_CORR_SCAN_EACH=1, read per call) and without the cross field.

    python profiles/tools/corr_time.py [--n 1024] [--haloes 1000000] [--reps 3] [--field-bytes 8] [--los 2] [--out FILE]
one JSON line on stdout.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from halo_time import RANGES, catalogue  # noqa: E402
from multipole_time import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--haloes", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--field-bytes", type=int, default=8, choices=(4, 8))
    ap.add_argument("--los", type=int, default=2, choices=(0, 1, 2))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ["PF_HALO_TIMES"] = "1"
    os.environ["PF_CORR_TIMES"] = "1"
    os.environ.pop("PF_CORR_SCAN_EACH", None)
    from pinocchio_amd import api, synth
    n = args.n
    pos, mass = catalogue(args.haloes, n)
    vel = np.zeros_like(pos)
    vel[:, args.los] = np.random.default_rng(2).normal(0.0, 1.5, size=len(mass))
    with api.Fmax(n, field_bytes=args.field_bytes) as f:
        f.synth_density(synth.SEED, 2.5, -2.0)
        kw = dict(vfac=1.0, los=args.los, deconvolve=True)
        multi, multi_dev, multi_wall = timed(lambda: f.halo_multipoles(pos, vel, mass, RANGES, **kw), api.halo_times, args.reps)
        got, dev, wall = timed(lambda: f.halo_correlation(pos, vel, mass, RANGES, **kw), api.debug_corr_times, args.reps)
        os.environ["PF_CORR_SCAN_EACH"] = "1"
        each, each_dev, each_wall = timed(lambda: f.halo_correlation(pos, vel, mass, RANGES, **kw), api.debug_corr_times, args.reps)
        os.environ.pop("PF_CORR_SCAN_EACH")
        assert all(np.array_equal(got[k], each[k]) for k in ("ncells", "r2sum", "xi", "xi_cross", "max_cell", "empty_cells"))
        _, auto_dev, auto_wall = timed(lambda: f.halo_correlation(pos, vel, mass, RANGES, cross=False, **kw), api.debug_corr_times, args.reps)
        # Parseval beside the times: the zero-lag cell against the sum over the shells of the multipole call's l = 0 row
        parseval = [float(got["xi"][b, 0, 0] / multi["power"][b, 0, 1:].sum() - 1.0) for b in range(len(RANGES))]
        best = lambda rows: [min(r[i] for r in rows) for i in range(len(rows[0]))]
        row = {"n": n, "field_bytes": args.field_bytes, "haloes": args.haloes, "bins": len(RANGES), "los": args.los,
               "corr_phases": list(api.CORR_TIME_KEYS), "corr_device_ms": dev, "corr_wall_ms": wall, "corr_best_ms": best(dev),
               "corr_each_device_ms": each_dev, "corr_each_wall_ms": each_wall,
               "corr_without_cross_device_ms": auto_dev, "corr_without_cross_wall_ms": auto_wall,
               "multipoles_phases": list(api.HALO_TIME_KEYS), "multipoles_device_ms": multi_dev, "multipoles_wall_ms": multi_wall, "multipoles_best_ms": best(multi_dev),
               "selected": got["selected"].tolist(), "nonfinite_cells": got["nonfinite_cells"].tolist(), "variance": got["variance"].tolist(),
               "zero_lag_over_power_sum_minus_one": parseval}
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(row, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
