"""Times count_peaks on the device beside the passes it is to be compared with (profiles/r07_peaks.md).

A 1024^3 context with fp64 fields and a synthetic density, one sweep, then -- in one process, warmed, `--reps` repetitions each,
alternating -- pf_fmax_pdf (reads the Fmax column once: the yardstick), pf_count_peaks(1.0), pf_select_sorted(1.0) and
pf_select_peaks(1.0), device events on the library's stream around each call (the calls synchronise before they return: the span
is the device part, allocations and the small copies of the call included).  Before it times anything it checks
pf_count_peaks against the numpy restatement (tests/np_peaks.py) on three full planes of block("FMAX") with their neighbours,
so that the timed kernel is shown to do the work at that size.

    python profiles/tools/peaks_time.py [--n 1024] [--reps 20] [--only count]      one JSON line on stdout

--only count: the count pass alone, for a counter run of its own (one counter per run: the two together are more than the
hardware collects in one pass)
    rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d DIR -- python profiles/tools/peaks_time.py --only count --reps 3 --no-check
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()
    import torch
    import np_peaks
    from pinocchio_amd import api
    n = a.n
    f = api.Fmax(n, field_bytes=8)
    f.synth_density(1234)
    from pinocchio_amd import synth
    f.set_invgrow(*synth.invgrow_table("lcdm"))
    f.sweep(np.array([4.0, 2.0, 1.0, 0.0]))
    out = {"n": n, "reps": a.reps}
    if not a.no_check:
        fmax = f.block("FMAX").reshape(n, n, n)
        for x in (0, n // 2 + 1, n - 1):     # three planes with their neighbours, periodic in y and z: a region one plane thick is
            # never examined (its borders are skipped), so the slab x-1 .. x+1 with the well resolved part = the middle plane
            rg = ((x - 1, 0, 0), (3, n, n), (1, 0, 0))
            got = f.count_peaks(1.0, rg)
            want = np_peaks.count_peaks(fmax, 1.0, rg)
            assert got == want, (x, got, want)
            out["plane_%d" % x] = got[0]
        del fmax
    st = torch.cuda.ExternalStream(f.L.pf_get_stream(f.h))
    calls = {"fmax_pdf": f.Fmax_PDF, "count_peaks": lambda: f.count_peaks(1.0), "select_sorted": lambda: f.select_sorted(1.0),
             "select_peaks": lambda: f.select_peaks(1.0)}
    if a.only:
        calls = {k: v for k, v in calls.items() if k.startswith(a.only)}
    ms = {k: [] for k in calls}
    res = {}
    for rep in range(a.reps + 2):                # two warm-up rounds
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            r = fn()
            e1.record(st)
            e1.synchronize()
            if rep >= 2:
                ms[k].append(e0.elapsed_time(e1))
            res[k] = r
    for k in calls:
        v = np.array(ms[k])
        out[k + "_ms"] = {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}
    if "count_peaks" in res:
        out["peaks"] = res["count_peaks"][0]
        out["count_gbps_algorithmic"] = 4.0 * n ** 3 / (out["count_peaks_ms"]["median"] * 1e-3) / 1e9
    if "fmax_pdf" in res:
        out["stored"] = int(res["fmax_pdf"][10:].sum())
        out["pdf_gbps_algorithmic"] = 4.0 * n ** 3 / (out["fmax_pdf_ms"]["median"] * 1e-3) / 1e9
    if "count_peaks" in res and "fmax_pdf" in res:
        out["count_over_pdf"] = out["count_peaks_ms"]["median"] / out["fmax_pdf_ms"]["median"]
    if "select_peaks" in res and "select_sorted" in res:
        out["keys_peaks_over_sorted"] = len(res["select_peaks"][0]) / max(1, len(res["select_sorted"][0]))
        out["select_peaks_over_sorted"] = out["select_peaks_ms"]["median"] / out["select_sorted_ms"]["median"]
    print(json.dumps(out))
    f.close()


if __name__ == "__main__":
    main()
