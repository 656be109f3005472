"""The flavour census of one box and what it costs (profiles/census_notes.md).

Workload: the benchmark's -- synthetic density (seed synth.SEED, sigma0 2.5, slope -2), the lcdm inverse-growth table, the ladder
of `ns` radii -- on one rank with float products.  One JSON line on stdout:
  census        every field of pf_census (the histogram as its non-empty bins); of the first `--records` outlier records the first
                sixteen, the one of max_abs_cell and those whose Rmax differ
  ms            wall ms, each after a warm-up sweep and behind a synchronise (pf_sweep ends with one): a plain sweep in the fast
                flavour (mean of `--reps`), one in the exact flavour, and the whole pf_flavour_census call
  stream_GBps   pf_debug_stream_rate(kind 0) of this context: a kernel that only reads one spectrum-sized field
  column_bytes  what the census kernel reads: (2 product bytes + 8) per cell
The census kernels' own time comes from a run of this tool under a kernel trace (--census-only leaves the timing sweeps out).

    python profiles/tools/census_time.py [--n 1024] [--ns 12] [--field-bytes 8] [--reps 2] [--records 16] [--census-only]
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
    ap.add_argument("--ns", type=int, default=12)
    ap.add_argument("--field-bytes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--records", type=int, default=16)
    ap.add_argument("--census-only", action="store_true")
    a = ap.parse_args()
    from pinocchio_amd import api, synth
    radii = synth.radii_ladder(a.ns) * (a.n / 1024.0)
    radii[-1] = 0.0
    out = {"n": a.n, "ns": a.ns, "field_bytes": a.field_bytes, "radii_cells": [float(r) for r in radii]}
    with api.Fmax(a.n, field_bytes=a.field_bytes) as f:
        f.synth_density(synth.SEED, 2.5, -2.0)
        f.set_invgrow(*synth.invgrow_table("lcdm"))
        f.set_growth(synth.growth_multipliers())
        ms = {}

        def timed(call):
            f.synchronize()
            t0 = time.perf_counter()
            r = call()
            f.synchronize()
            return 1e3 * (time.perf_counter() - t0), r

        if not a.census_only:
            f.sweep(radii)    # warm-up: first-use allocations, code objects
            ms["sweep_fast"] = float(np.mean([timed(lambda: f.sweep(radii))[0] for _ in range(a.reps)]))
            f.set_arithmetic("exact")
            ms["sweep_exact"] = timed(lambda: f.sweep(radii))[0]
            f.set_arithmetic("fast")
        before = f.device_bytes
        ms["census_call"], (tv, cen, rec) = timed(lambda: f.flavour_census(radii, capacity=a.records))
        assert f.device_bytes == before and f.arithmetic == "fast"
        if not a.census_only:
            g = C.c_double()
            if f.L.pf_debug_stream_rate(f.h, 0, 5, C.byref(g)) == 0:
                out["stream_GBps"] = g.value
        out["device_GB"] = 1e-9 * before
    hist = cen.pop("hist")
    cen["hist"] = {int(k): int(hist[k]) for k in np.flatnonzero(hist)}
    out["census"] = cen
    out["beyond_2ulp_fraction"] = cen["beyond_2ulp"] / cen["cells"]
    plain = lambda r: {k: (float(r[k]) if k in ("fast", "exact") else int(r[k])) for k in rec.dtype.names}
    out["records"] = [plain(r) for r in rec[:16]]
    out["records_returned"] = len(rec)
    hit = rec[rec["cell"] == cen["max_abs_cell"]]    # the record of the largest difference, when the capacity reached it
    out["max_abs_record"] = plain(hit[0]) if len(hit) else None
    out["rmax_differing_records"] = [plain(r) for r in rec[rec["rmax_fast"] != rec["rmax_exact"]][:16]]
    out["ms"] = ms
    out["column_bytes"] = cen["cells"] * 16
    out["true_variance_last"] = float(tv[-1])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
