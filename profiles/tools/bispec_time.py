"""Times pf_halo_bispectrum: one rank, the synthetic catalogue of profiles/tools/halo_time.py, one mass bin, cloud-in-cell,
deconvolved, real space -- profiles/bispec_notes.md.

After a warm-up call: `reps` calls, the device ms of the phases between events (PF_BISPEC_TIMES=1 and pf_debug_bispec_times:
select, deposit, contrast, transforms forward and reverse, mask, keep, triples; the count fields of the call included) and the wall
ms, beside the read rate of a streaming kernel on the same context (pf_debug_stream_rate, kind 0) and what the triple pass would
take at that rate for the fields it reads.

    python profiles/tools/bispec_time.py [--n 128] [--kmin 2] [--dk 5] [--nk 8] [--haloes 200000] [--reps 3] [--field-bytes 8] [--lc 4] [--out FILE]
one JSON line on stdout.  --lc: the l per group the library was built with (PF_BISPEC_LC; for the streamed bytes alone).
"""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from halo_time import catalogue  # noqa: E402
from multipole_time import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--kmin", type=int, default=2)
    ap.add_argument("--dk", type=int, default=5)
    ap.add_argument("--nk", type=int, default=8)
    ap.add_argument("--haloes", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--field-bytes", type=int, default=8, choices=(4, 8))
    ap.add_argument("--lc", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ["PF_BISPEC_TIMES"] = "1"
    from pinocchio_amd import api
    n = args.n
    pos, mass = catalogue(args.haloes, n)
    tri = api.bispectrum_triangles(args.kmin, args.dk, args.nk)
    # the fields a launch of the triple pass streams: per pair (i, j) and per run of up to lc consecutive l, 2 + the run
    runs = {}
    for i, j, l in tri:
        runs[(i, j)] = runs.get((i, j), 0) + 1
    streamed = sum(2 * ((c + args.lc - 1) // args.lc) + c for c in runs.values()) + args.nk
    with api.Fmax(n, field_bytes=args.field_bytes) as f:
        got, dev, wall = timed(lambda: f.halo_bispectrum(pos, None, mass, [(10, 2 ** 31 - 1)], args.kmin, args.dk, args.nk, deconvolve=True, box=1000.0), api.debug_bispec_times,
                               args.reps)
        rate = C.c_double(0.0)
        f._chk(f.L.pf_debug_stream_rate(f.h, 0, 5, C.byref(rate)))
    best = [min(r[i] for r in dev) for i in range(len(dev[0]))]
    gbytes = 2 * streamed * float(n) ** 3 * args.field_bytes / 1e9          # the count fields and one mass bin
    row = {"n": n, "field_bytes": args.field_bytes, "kmin": args.kmin, "dk": args.dk, "nk": args.nk, "triangles": len(tri), "haloes": args.haloes, "lc": args.lc,
           "phases": list(api.BISPEC_TIME_KEYS), "device_ms": dev, "wall_ms": wall, "best_ms": best, "stream_read_GBps": round(rate.value, 1),
           "triples_streamed_GB": round(gbytes, 3), "triples_ms_at_stream_rate": round(gbytes / rate.value * 1e3, 3) if rate.value else None,
           "terms": 2 * (len(tri) + args.nk) * n ** 3, "ntri_first": got["ntri"][:3].tolist(), "Q_first": got["Q"][0, :3].tolist()}
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(row, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
