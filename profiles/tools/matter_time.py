"""Times pf_matter_power on the boxes of bench.py -- the synthetic density of its flagship workload (sigma0 = 2.5, slope -2, the
twelve radii, all LPT orders), one rank, fp64 fields, float products -- at 256^3, 512^3 and 1024^3 (profiles/matter_notes.md).

Per size, after a warm-up call: `reps` calls, the device ms of the four phases between events of each (PF_MATTER_TIMES=1,
pf_debug_matter_times: deposit with the clearing of the grid, contrast, forward transform, shell passes) and the wall ms of the
call, which adds the allocation of the grid and the download of the columns.  `added_GBps` is what the deposit adds to HBM per
second if every particle issues eight 8-byte adds (64 bytes per particle; an add of zero is left out, so this overstates the
traffic of a lattice at rest), to set beside the rate of float atomics of the device; `max_cell` is the largest cell in particles.

    python profiles/tools/matter_time.py [--n 256 512 1024] [--reps 3] [--field-bytes 8] [--ngp] [--sigma0 2.5] [--out profiles/matter_times.json]
one JSON line per size on stdout.  The A/B of the two deposit forms: the same command under PF_MATTER_LDS=0 and =1.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--field-bytes", type=int, default=8, choices=(4, 8))
    ap.add_argument("--ngp", action="store_true")
    ap.add_argument("--sigma0", type=float, default=2.5, help="amplitude of the synthetic density (2.5: the bench workload; 0.05: an early initial condition)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ["PF_MATTER_TIMES"] = "1"
    from pinocchio_amd import api, synth
    rows = []
    for n in args.n:
        with api.Fmax(n, field_bytes=args.field_bytes) as f:
            f.synth_density(synth.SEED, args.sigma0, -2.0)
            f.set_invgrow(*synth.invgrow_table("lcdm"))
            f.set_growth(synth.growth_multipliers())
            f.compute_fmax(synth.radii_ladder(12), do_lpt=True)
            first = f.matter_power(ngp=args.ngp, deconvolve=True)
            dev, wall = [], []
            for _ in range(args.reps):
                t = time.perf_counter()
                got = f.matter_power(ngp=args.ngp, deconvolve=True)
                wall.append((time.perf_counter() - t) * 1e3)
                dev.append(api.matter_times())
            assert all(np.array_equal(got[k], first[k]) for k in ("nmodes", "k2sum", "power", "cross")) and got["max_cell"] == first["max_cell"]
            best = [min(d[i] for d in dev) for i in range(4)]
            pl = f.power_spectrum("density")["power"]
            with np.errstate(invalid="ignore", divide="ignore"):
                r = got["cross"][1:5] / np.sqrt(got["power"][1:5] * pl[1:5])
            vel = f.products()["Vel"] if n <= 256 else None
            row = {"n": n, "field_bytes": args.field_bytes, "ngp": bool(args.ngp), "sigma0": args.sigma0,
                   "zeldovich_rms_cells": float(np.sqrt(np.mean(vel.astype(np.float64) ** 2))) if vel is not None else None, "phases": ["deposit", "contrast", "transform", "shells"],
                   "device_ms": [[round(x, 3) for x in d] for d in dev], "wall_ms": [round(x, 3) for x in wall],
                   "added_GBps": round(64.0 * got["deposited"] / (best[0] * 1e-3) / 1e9, 1) if best[0] > 0 else None,
                   "max_cell": got["max_cell"] / float(1 << 48), "empty_cells": got["empty_cells"], "deposited": got["deposited"], "outside": got["outside"],
                   "nonfinite": got["nonfinite"], "r_shells_1_4": [float(x) for x in r]}
            print(json.dumps(row), flush=True)
            rows.append(row)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
