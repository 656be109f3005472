"""Times pf_power_spectrum on the boxes of bench.py -- the synthetic density of its flagship workload, one rank, fp64 and fp32
fields -- with ns = 0 and ns = 12 radii (the ladder bench.py sweeps), beside the time the library's read-only streaming kernel
(pf_debug_stream_rate kind 0) needs for the same bytes on the same box (profiles/power_notes.md).

Per (field_bytes, ns), after a warm-up call: `reps` calls, the device ms between events of each (PF_POWER_TIMES=1,
pf_debug_power_times: both passes over the spectrum and the finishing kernel) and the wall ms of the call, which adds the scratch
allocation and the download of the columns.  The call reads the spectrum twice, the streaming kernel once: `ratio` is device ms over
the time of ONE read, `ratio_per_read` half of that.

    python profiles/tools/power_time.py [--n 1024] [--reps 3] [--out profiles/power_times.json]
one JSON line per (field_bytes, ns) on stdout.
"""
import argparse
import ctypes as C
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
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ["PF_POWER_TIMES"] = "1"
    from pinocchio_amd import api, synth
    rows = []
    for fb in (8, 4):
        with api.Fmax(args.n, field_bytes=fb) as f:
            f.synth_density(synth.SEED, 2.5, -2.0)
            v = C.c_double()
            if f.L.pf_debug_stream_rate(f.h, 0, 5, C.byref(v)) != 0:
                raise SystemExit("pf_debug_stream_rate failed")
            nzp = args.n // 2 + 64 // fb
            field = args.n * args.n * nzp * 2 * fb                   # the bytes of one spectrum-sized field, row padding included
            read_ms = field / (v.value * 1e9) * 1e3
            for ns in (0, 12):
                radii = synth.radii_ladder(ns) if ns else ()
                first = f.power_spectrum("density", radii)
                dev, wall = [], []
                for _ in range(args.reps):
                    t = time.perf_counter()
                    got = f.power_spectrum("density", radii)
                    wall.append((time.perf_counter() - t) * 1e3)
                    dev.append(api.power_times())
                assert all(np.array_equal(got[k], first[k]) for k in ("nmodes", "k2sum", "power", "variance"))
                row = {"n": args.n, "field_bytes": fb, "ns": ns, "device_ms": [round(x, 3) for x in dev], "wall_ms": [round(x, 3) for x in wall],
                       "read_GBps": round(v.value, 1), "read_ms": round(read_ms, 3), "ratio": round(min(dev) / read_ms, 2), "ratio_per_read": round(min(dev) / read_ms / 2, 2),
                       "sigma_R0": float(np.sqrt(got["power"].sum())), "nonfinite": got["nonfinite"]}
                if ns:
                    row["variance"] = [float(x) for x in got["variance"]]
                print(json.dumps(row), flush=True)
                rows.append(row)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
