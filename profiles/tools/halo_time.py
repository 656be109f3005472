"""Times pf_halo_power on the box of bench.py's flagship workload (the synthetic density, sigma0 = 2.5, slope -2), one rank, with a
synthetic catalogue: `--haloes` points uniform in the box, masses from 10 particles up on a power law dn/dM ~ M^-2, three cumulative
bins (all, M >= 100, M >= 1000) -- profiles/halo_notes.md.

After a warm-up call: `reps` calls, the device ms of the five phases between events of each (PF_HALO_TIMES=1, pf_debug_halo_times:
select, deposit with the clearing of the grid, contrast, forward transform, shell passes, each summed over the three bins) and the
wall ms of the call, which adds the allocations, the upload of the list and the fetch.  With --matter the same context then computes
its products (the twelve radii, all LPT orders) and pf_matter_power is timed the same way (PF_MATTER_TIMES=1): its transform and
shell passes are what one bin of the halo call is held against.

    python profiles/tools/halo_time.py [--n 1024] [--haloes 10000000] [--reps 3] [--field-bytes 8] [--mass-weight] [--ngp] [--matter] [--out FILE]
one JSON line on stdout.
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

RANGES = [(10, 2 ** 31 - 1), (100, 2 ** 31 - 1), (1000, 2 ** 31 - 1)]


def catalogue(count, n, seed=1):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, float(n), size=(count, 3))
    mass = np.minimum(10.0 / (1.0 - rng.uniform(0.0, 1.0, size=count)), 1.0e6).astype(np.int32)     # P(M > m) = 10 / m
    return pos, mass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--haloes", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--field-bytes", type=int, default=8, choices=(4, 8))
    ap.add_argument("--mass-weight", action="store_true")
    ap.add_argument("--ngp", action="store_true")
    ap.add_argument("--matter", action="store_true", help="then time pf_matter_power on the same context")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ["PF_HALO_TIMES"] = "1"
    os.environ["PF_MATTER_TIMES"] = "1"
    from pinocchio_amd import api, synth
    n = args.n
    pos, mass = catalogue(args.haloes, n)
    with api.Fmax(n, field_bytes=args.field_bytes) as f:
        f.synth_density(synth.SEED, 2.5, -2.0)
        kw = dict(mass_weight=args.mass_weight, ngp=args.ngp, deconvolve=True)
        first = f.halo_power(pos, mass, RANGES, **kw)
        dev, wall = [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            got = f.halo_power(pos, mass, RANGES, **kw)
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(api.halo_times())
        assert all(np.array_equal(got[k], first[k]) for k in ("nmodes", "k2sum", "power", "cross", "max_cell", "empty_cells"))
        t = time.perf_counter()
        f.halo_power(pos, mass, RANGES, cross=False, **kw)
        nocross_wall, nocross = (time.perf_counter() - t) * 1e3, api.halo_times()
        hi = slice(n // 4, n // 2)
        row = {"n": n, "field_bytes": args.field_bytes, "haloes": args.haloes, "bins": len(RANGES), "mass_weight": bool(args.mass_weight), "ngp": bool(args.ngp),
               "phases": list(api.HALO_TIME_KEYS), "device_ms": [[round(x, 3) for x in d] for d in dev], "wall_ms": [round(x, 3) for x in wall],
               "device_ms_without_cross": [round(x, 3) for x in nocross], "wall_ms_without_cross": round(nocross_wall, 3),
               "selected": got["selected"].tolist(), "max_cell": (got["max_cell"] / float(1 << 30)).tolist(), "empty_cells": got["empty_cells"].tolist(),
               "power_per_mode_over_shot_quarter_to_half_nyquist": [float((got["power"][b][hi] / got["nmodes"][hi]).mean() / got["shot"][b]) for b in range(len(RANGES))]}
        if args.matter:
            f.set_invgrow(*synth.invgrow_table("lcdm"))
            f.set_growth(synth.growth_multipliers())
            f.compute_fmax(synth.radii_ladder(12), do_lpt=True)
            f.matter_power(deconvolve=True)
            mdev = []
            for _ in range(args.reps):
                f.matter_power(deconvolve=True)
                mdev.append(api.matter_times())
            row["matter_phases"] = ["deposit", "contrast", "transform", "shells"]
            row["matter_device_ms"] = [[round(x, 3) for x in d] for d in mdev]
            again = f.halo_power(pos, mass, RANGES, **kw)              # ... and the halo call once more, behind the products
            row["device_ms_after_products"] = [round(x, 3) for x in api.halo_times()]
            assert all(np.array_equal(again[k], first[k]) for k in ("nmodes", "k2sum", "power", "cross"))
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(row, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
