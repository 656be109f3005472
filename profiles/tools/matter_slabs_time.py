"""Times pf_matter_power_slabs (profiles/matter_slabs_notes.md) on the synthetic density of bench.py's workload (slope -2, all LPT
orders, fp64 fields, float products).

  --one N ...        one rank: after a warm-up call, `reps` calls each of matter_power and matter_power_slabs
                     on the same context and products, the device ms of the four phases of each (PF_MATTER_TIMES=1: deposit --
                     with the reach pass, pack, exchange and fold of the slab call --, contrast, transform, shells) and the wall ms.
                     (pf_matter_power before the slab call existed: profiles/tools/matter_time.py on that commit.)
  --ranks N:P ...    P contexts on ONE GPU through the in-process fabric, a host thread each: the same per rank, with the measured
                     reach, bytes_per_peer and the wire planes P B.  The ranks share the device, so a rank's device ms hold the
                     kernels of the others that ran in between: they say what the call costs the box on one GPU, not what a rank
                     of an eight-GPU run waits.

    python profiles/tools/matter_slabs_time.py --one 1024 --ranks 256:2 256:4 256:8 512:2 512:4 512:8 [--reps 3] [--sigma0 2.5] [--out FILE]
one JSON line per configuration on stdout."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
RADII = np.array([1.0, 0.0])      # (the displacements do not depend on the radii of the sweep)


def prepare(f, synth, sigma0):
    f.synth_density(synth.SEED, sigma0, -2.0)
    f.set_invgrow(*synth.invgrow_table("lcdm"))
    f.set_growth(synth.growth_multipliers())
    f.compute_fmax(RADII, do_lpt=True)


def timed(api, call, reps):
    first = call()
    dev, wall = [], []
    for _ in range(reps):
        t = time.perf_counter()
        got = call()
        wall.append(round((time.perf_counter() - t) * 1e3, 3))
        dev.append([round(x, 3) for x in api.matter_times()])
    assert all(np.array_equal(got[k], first[k]) for k in ("nmodes", "k2sum", "power", "cross")) and got["max_cell"] == first["max_cell"]
    return got, dev, wall


def one_rank(api, synth, n, args):
    with api.Fmax(n, field_bytes=8) as f:
        prepare(f, synth, args.sigma0)
        row = {"n": n, "ranks": 1, "sigma0": args.sigma0, "phases": ["deposit", "contrast", "transform", "shells"]}
        got, row["matter_power_device_ms"], row["matter_power_wall_ms"] = timed(api, lambda: f.matter_power(deconvolve=True), args.reps)
        slab, row["slabs_device_ms"], row["slabs_wall_ms"] = timed(api, lambda: f.matter_power_slabs(deconvolve=True), args.reps)
        assert all(np.array_equal(got[k].view(np.uint64), slab[k].view(np.uint64)) for k in ("nmodes", "k2sum", "power", "cross"))
        row["exchange"] = slab["exchange"]
        row["max_cell"] = got["max_cell"] / float(1 << 48)
    return row


def many_ranks(api, synth, n, P, args):
    from pinocchio_amd import _lib
    L = _lib.load()
    fab = L.pf_fabric_create(P)
    ctxs = [api.Fmax(n, rank=r, nranks=P, field_bytes=8) for r in range(P)]
    for c in ctxs:
        assert L.pf_fabric_attach(fab, c.h) == 0
    out, err = [None] * P, [None] * P

    def work(r):
        try:
            prepare(ctxs[r], synth, args.sigma0)
            out[r] = timed(api, lambda: ctxs[r].matter_power_slabs(deconvolve=True), args.reps)
        except BaseException as e:  # noqa: BLE001
            err[r] = e

    th = [threading.Thread(target=work, args=(r,)) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for c in ctxs:
        c.close()
    L.pf_fabric_destroy(fab)
    for e in err:
        if e is not None:
            raise e
    ex = out[0][0]["exchange"]
    return {"n": n, "ranks": P, "sigma0": args.sigma0, "phases": ["deposit", "contrast", "transform", "shells"], "exchange": ex,
            "wire_planes_per_rank": P * ex["block_planes"], "filled_planes_per_rank": ex["reach_below"] + ex["reach_above"],
            "scratch_bytes_per_rank": (ex["window_planes"] + 2 * P * ex["block_planes"]) * n * n * 8,
            "device_ms_by_rank": [o[1] for o in out], "wall_ms_by_rank": [o[2] for o in out], "max_cell": out[0][0]["max_cell"] / float(1 << 48)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", type=int, nargs="*", default=[])
    ap.add_argument("--ranks", nargs="*", default=[])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sigma0", type=float, default=2.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ["PF_MATTER_TIMES"] = "1"
    from pinocchio_amd import api, synth
    rows = []
    for n in args.one:
        rows.append(one_rank(api, synth, n, args))
        print(json.dumps(rows[-1]), flush=True)
    for item in args.ranks:
        n, P = (int(x) for x in item.split(":"))
        rows.append(many_ranks(api, synth, n, P, args))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
