"""Times pf_halo_multipoles beside pf_halo_power on the same list and box: the box of bench.py's flagship workload (the synthetic
density, sigma0 = 2.5, slope -2), one rank, the synthetic catalogue of profiles/tools/halo_time.py with Gaussian velocities of 1.5
cells along the line of sight, three cumulative bins, cloud-in-cell, deconvolved, with cross power -- profiles/multipole_notes.md.

After a warm-up call of each: `reps` calls of each, the device ms of the five phases between events (PF_HALO_TIMES=1,
pf_debug_halo_times, each summed over the three bins) and the wall ms.  Then the multipole call with one sum per shell pass
(PF_MULTIPOLE_SCAN_EACH=1, read per call) and without cross, to price the grouping of the sums.

    python profiles/tools/multipole_time.py [--n 1024] [--haloes 10000000] [--reps 3] [--field-bytes 8] [--los 2] [--out FILE]
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
sys.path.insert(0, HERE)

from halo_time import RANGES, catalogue  # noqa: E402


def timed(call, times, reps):
    call()
    dev, wall = [], []
    for _ in range(reps):
        t = time.perf_counter()
        got = call()
        wall.append(round((time.perf_counter() - t) * 1e3, 3))
        dev.append([round(x, 3) for x in times()])
    return got, dev, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--haloes", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--field-bytes", type=int, default=8, choices=(4, 8))
    ap.add_argument("--los", type=int, default=2, choices=(0, 1, 2))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ["PF_HALO_TIMES"] = "1"
    os.environ.pop("PF_MULTIPOLE_SCAN_EACH", None)
    from pinocchio_amd import api, synth
    n = args.n
    pos, mass = catalogue(args.haloes, n)
    vel = np.zeros_like(pos)
    vel[:, args.los] = np.random.default_rng(2).normal(0.0, 1.5, size=len(mass))
    with api.Fmax(n, field_bytes=args.field_bytes) as f:
        f.synth_density(synth.SEED, 2.5, -2.0)
        kw = dict(deconvolve=True)
        real, real_dev, real_wall = timed(lambda: f.halo_power(pos, mass, RANGES, **kw), api.halo_times, args.reps)
        got, dev, wall = timed(lambda: f.halo_multipoles(pos, vel, mass, RANGES, vfac=1.0, los=args.los, **kw), api.halo_times, args.reps)
        form = api.multipole_form()
        os.environ["PF_MULTIPOLE_SCAN_EACH"] = "1"
        each, each_dev, each_wall = timed(lambda: f.halo_multipoles(pos, vel, mass, RANGES, vfac=1.0, los=args.los, **kw), api.halo_times, args.reps)
        each_form = api.multipole_form()
        os.environ.pop("PF_MULTIPOLE_SCAN_EACH")
        assert all(np.array_equal(got[k], each[k]) for k in ("nmodes", "k2sum", "power", "cross", "max_cell", "empty_cells"))
        _, auto_dev, auto_wall = timed(lambda: f.halo_multipoles(pos, vel, mass, RANGES, vfac=1.0, los=args.los, cross=False, **kw), api.halo_times, args.reps)
        auto_form = api.multipole_form()
        same = f.halo_multipoles(pos, None, mass, RANGES, los=args.los, **kw)
        assert np.array_equal(same["power"][:, 0], real["power"]) and np.array_equal(same["cross"][:, 0], real["cross"])
        shells = lambda rows: min(r[4] for r in rows)
        hi = slice(n // 4, n // 2)
        row = {"n": n, "field_bytes": args.field_bytes, "haloes": args.haloes, "bins": len(RANGES), "los": args.los, "phases": list(api.HALO_TIME_KEYS),
               "halo_power_device_ms": real_dev, "halo_power_wall_ms": real_wall,
               "multipoles_device_ms": dev, "multipoles_wall_ms": wall, "multipoles_form": form,
               "multipoles_each_device_ms": each_dev, "multipoles_each_wall_ms": each_wall, "multipoles_each_form": each_form,
               "multipoles_without_cross_device_ms": auto_dev, "multipoles_without_cross_wall_ms": auto_wall, "multipoles_without_cross_form": auto_form,
               "shells_ratio_to_halo_power": round(shells(dev) / shells(real_dev), 3), "shells_ratio_each_to_grouped": round(shells(each_dev) / shells(dev), 3),
               "selected": got["selected"].tolist(),
               "quadrupole_over_monopole_quarter_to_half_nyquist": [float((got["power"][b, 1][hi] / got["power"][b, 0][hi]).mean()) for b in range(len(RANGES))]}
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(row, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
