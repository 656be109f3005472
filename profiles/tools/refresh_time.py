"""Times the velocity refresh of a redshift segment -- pf_gather_velocities and pf_refresh_velocities, with and without `order` --
beside pf_distribute_sorted_map on the same sub-box, the route the same step took before them (profiles/refresh_notes.md).

Workload: the whole periodic n^3 box as one sub-box on one rank, fp32 fields and products, a synthetic density, four radii, 3LPT, two
segments (one pf_shift_displacements).  The stored set is the cells with Fmax >= flast, flast the quantile of Fmax that stores the
wanted fraction of the box (1.0: every cell); frag[] is what pf_distribute_sorted_map returns -- 104-byte records in descending Fmax,
frag_pos[] random in space -- and `order` is its indices[].

Per stored fraction, in a process of its own that the parent ends at a time limit (a step that fails or runs out of time ends the run),
`reps` times each:
 (a) pf_distribute_sorted_map into the 104-byte records: wall time, and the device time of its kernels of the "distribute" class;
 (b) pf_gather_velocities (index + vel24) with order = NULL and with order = indices[]: wall time and the device time of its three
     kernels (the "distribute" class of pf_kernel_stats, which holds nothing else in these calls);
 (c) pf_refresh_velocities into the records, all eight fields, likewise.
The results of (b) and (c) are checked: both orders give the same bytes, the Vel* fields (c) writes are those (a) delivered, and the
first 2^20 records hold the 24 values of (b).  The device times cover all three kernels of a call (flag, scan, gather).

    python profiles/tools/refresh_time.py [--n 512] [--fractions 0.02,0.2,1.0] [--reps 3] [--limit 600] [--out FILE.json]
one JSON line per fraction on stdout.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def _span(v):
    return {"min": float(min(v)), "max": float(max(v)), "all": [float(x) for x in v]}


def one(n, fraction, reps):
    from pinocchio_amd import _lib, api, synth
    box = ((0, 0, 0), (n, n, n), (0, 0, 0))
    lay = _lib.ProductLayout(104, 0, 4, 8, 20, 32, 44)      # product_data of -DRECOMPUTE_DISPLACEMENTS
    prev = api.prev_layout(56, 68, 80, 92)
    g = synth.growth_multipliers()
    out = {"n": n, "fraction": fraction}
    with api.Fmax(n, field_bytes=4, timing=True) as f:
        f.synth_density(synth.SEED, 2.5, -2.0)
        f.set_invgrow(*synth.invgrow_table("lcdm"))
        f.sweep(np.array([2.0, 1.0, 0.5, 0.0]))
        f.set_growth(g)
        f.compute_displacements(1, 0)
        f.shift_displacements()
        f.set_growth(g * np.array([0.75, 0.5, 0.625, 0.875]))
        f.compute_displacements(0, 0)
        fmax = f.block("FMAX")
        flast = -1e30 if fraction >= 1.0 else float(np.quantile(fmax, 1.0 - fraction))
        del fmax
        m = f.frag_map(*box)
        m.fill_box()
        m.commit(False)

        def timed(call):
            f.synchronize()
            f.reset_kernel_stats()
            t0 = time.perf_counter()
            r = call()
            wall = 1e3 * (time.perf_counter() - t0)
            ks = [k for k in f.kernel_stats() if k["name"] == "distribute"]
            return r, wall, (ks[0]["total_ms"] if ks else float("nan"))

        count = f.distribute_sorted(flast, box[0], box[1], map=m, layout=lay, capacity=0)[4]
        out.update(particles=count, stored_fraction=count / float(n ** 3), record_bytes=104 * count, vel24_bytes=96 * count)
        walls, kernels = [], []
        for rep in range(reps + 1):                           # the first pass is the warm-up: first touch, code objects, the pinned pieces
            (rec, pos, spos, ind, _), w, k = timed(lambda: f.distribute_sorted(flast, box[0], box[1], map=m, layout=lay, capacity=count))
            if rep:
                walls.append(w)
                kernels.append(k)
        out["distribute_sorted_map"] = {"wall_ms": _span(walls), "kernel_ms": _span(kernels)}
        kept = {}
        for name, order in (("natural", None), ("ordered", ind)):
            walls, kernels = [], []
            for rep in range(reps + 1):
                (index, vel), w, k = timed(lambda: f.gather_velocities(box, pos, order=order))
                if rep:
                    walls.append(w)
                    kernels.append(k)
            out["gather_" + name] = {"wall_ms": _span(walls), "kernel_ms": _span(kernels)}
            ok = len(index) == count and np.array_equal(index, np.arange(count, dtype=np.uint32))
            if name == "natural":
                kept["vel"] = vel
            else:
                ok = ok and vel.tobytes() == kept["vel"].tobytes()
            out["gather_" + name]["ok"] = bool(ok)
            del index, vel
        sample = min(count, 1 << 20)                          # every particle is found and index[j] = j: record j gets vel24[j]
        want = np.ascontiguousarray(kept["vel"][:sample]).view(np.uint8).reshape(sample, 96)
        del kept
        for name, order in (("natural", None), ("ordered", ind)):
            work = rec.copy()
            work[:, 8:] = 0xA5
            walls, kernels = [], []
            for rep in range(reps + 1):
                found, w, k = timed(lambda: f.refresh_velocities(box, pos, work, lay, prev, order=order))
                if rep:
                    walls.append(w)
                    kernels.append(k)
            out["refresh_" + name] = {"wall_ms": _span(walls), "kernel_ms": _span(kernels),
                                      "ok": bool(found == count and work[:, :56].tobytes() == rec[:, :56].tobytes() and work[:sample, 8:].tobytes() == want.tobytes())}
            del work
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--fractions", default="0.02,0.2,1.0")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=600, help="seconds a fraction may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", type=float, default=0.0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        one(a.n, a.one, a.reps)
        return 0
    results = []
    for fr in (float(v) for v in a.fractions.split(",")):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--n", str(a.n), "--reps", str(a.reps), "--one", repr(fr)], capture_output=True, text=True,
                               timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"fraction {fr}: no answer within {a.limit} s; nothing more is started", file=sys.stderr)
            return 1
        sys.stderr.write(r.stderr)
        if r.returncode:
            print(f"fraction {fr}: exit status {r.returncode}; nothing more is started", file=sys.stderr)
            return 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        results.append(json.loads(line))
        if a.out:
            with open(a.out, "w") as fh:
                json.dump(results, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
