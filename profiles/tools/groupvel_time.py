"""Times pf_refresh_segment -- the loose particles' records and the group means of a redshift segment in one call -- beside
pf_refresh_velocities with order = indices[] on the same set, the route the same step took before it (profiles/groupvel_notes.md).

Workload: the whole periodic n^3 box as one sub-box on one rank, fp32 fields and products, a synthetic density, four radii, 3LPT, two
segments (one pf_shift_displacements), the stored set of profiles/tools/refresh_time.py: the cells with Fmax >= flast, flast the
quantile that stores the wanted fraction of the box.  The grouping is synthetic: the box is cut into cubes of `cube`^3 Lagrangian
cells, a chosen share of the cubes are groups (ID 2 + cube number; the stored particles of the cube are its members), the particles
of the other cubes are loose (group_ID 0).  What share of the stored set is grouped in a real run at each segment has not been
measured by anyone: the shares here are a scan, not a claim.

Per (stored fraction, grouped share), in a process of its own that the parent ends at a time limit (a step that fails or runs out of
time ends the run), `reps` times each after a warm-up:
 (a) pf_refresh_velocities, order = indices[], all eight fields: wall time and the device time of its kernels (the "distribute" class
     of pf_kernel_stats, which holds nothing else in these calls);
 (b) pf_refresh_segment, order = indices[], all eight fields of either record: wall time, the device time of all its kernels, and --
     PF_GROUPVEL_TIMES=1 -- the device time of keys + sort, head flags + scan and reduce + fold on their own (with these the call
     synchronises three times more: its wall time is measured in a second series without them);
 (c) pf_group_velocity_sums alone: wall time and device time.
Checked: the records (b) writes for the loose particles are those of (a), the grouped ones keep their fill; the means of 2000 groups
are those of numpy's float64 mean over (a)'s records within 1e-6 of the largest value; no Mass mismatch.

    python profiles/tools/groupvel_time.py [--n 512] [--fractions 0.2,1.0] [--shares 0,0.5,0.9] [--cube 4] [--reps 3] [--limit 600] [--out FILE.json]
one JSON line per configuration on stdout.
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

GOFF = (16, 28, 40, 52, 64, 76, 88, 100)     # group_data: Mass, Pos[3], then Vel, Vel_2LPT, Vel_3LPT_1, Vel_3LPT_2 and their *_prev
GSTRIDE = 160


def _span(v):
    return {"min": float(min(v)), "max": float(max(v)), "all": [float(x) for x in v]}


def one(n, fraction, share, cube, reps):
    from pinocchio_amd import _lib, api, synth
    box = ((0, 0, 0), (n, n, n), (0, 0, 0))
    lay = _lib.ProductLayout(104, 0, 4, 8, 20, 32, 44)      # product_data of -DRECOMPUTE_DISPLACEMENTS
    prev = api.prev_layout(56, 68, 80, 92)
    gl = api.group_layout(GSTRIDE, 0, *GOFF)
    g = synth.growth_multipliers()
    out = {"n": n, "fraction": fraction, "share": share, "cube": cube}
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
        count = f.distribute_sorted(flast, box[0], box[1], map=m, layout=lay, capacity=0)[4]
        rec, pos, spos, ind, _ = f.distribute_sorted(flast, box[0], box[1], map=m, layout=lay, capacity=count)
        del rec, spos
        # the grouping: cube number of every particle, a share of the cubes are groups
        nc = n // cube
        p = pos.astype(np.int64)
        cnum = (p % n) // cube + nc * (((p // n) % n) // cube + nc * ((p // (n * n)) // cube))
        del p
        ngroups = nc ** 3 + 1
        is_group = np.random.default_rng(7).random(nc ** 3) < share
        gid = np.where(is_group[cnum], cnum + 2, 0).astype(np.int32)
        del cnum
        mass = np.bincount(gid, minlength=ngroups + 1).astype(np.int32)
        mass[:2] = 0
        grouped_want = int(mass.sum())
        out.update(particles=count, stored_fraction=count / float(n ** 3), grouped=grouped_want, grouped_share=grouped_want / float(max(count, 1)),
                   groups=int((mass > 0).sum()))

        def timed(call):
            f.synchronize()
            f.reset_kernel_stats()
            t0 = time.perf_counter()
            r = call()
            wall = 1e3 * (time.perf_counter() - t0)
            ks = [k for k in f.kernel_stats() if k["name"] == "distribute"]
            return r, wall, (ks[0]["total_ms"] if ks else float("nan"))

        def series(call):
            walls, kernels, r = [], [], None
            for rep in range(reps + 1):                       # the first pass is the warm-up
                r, w, k = timed(call)
                if rep:
                    walls.append(w)
                    kernels.append(k)
            return r, {"wall_ms": _span(walls), "kernel_ms": _span(kernels)}

        full = np.full((count, 104), 0xA5, dtype=np.uint8)
        found, out["refresh_velocities_ordered"] = series(lambda: f.refresh_velocities(box, pos, full, lay, prev, order=ind))
        work = np.full((count, 104), 0xA5, dtype=np.uint8)
        groups = np.zeros((ngroups + 1, GSTRIDE), dtype=np.uint8)
        groups[:, :4] = mass.view(np.uint8).reshape(-1, 4)
        os.environ.pop("PF_GROUPVEL_TIMES", None)
        res, out["refresh_segment"] = series(lambda: f.refresh_segment(box, pos, gid, work, lay, prev, groups, ngroups, gl, order=ind))
        _, out["group_velocity_sums"] = series(lambda: f.group_velocity_sums(box, pos, gid, capacity=0))
        os.environ["PF_GROUPVEL_TIMES"] = "1"
        stages = {"sort_ms": [], "heads_ms": [], "reduce_ms": []}
        for rep in range(reps + 1):
            f.refresh_segment(box, pos, gid, work, lay, prev, groups, ngroups, gl, order=ind)
            if rep:
                for k, v in api.debug_groupvel_times().items():
                    stages[k].append(v)
        os.environ.pop("PF_GROUPVEL_TIMES", None)
        out["refresh_segment"]["stages"] = {k: _span(v) for k, v in stages.items()} if grouped_want else {}
        # checks
        loose = gid < 2
        ok = found == count and res == (int(loose.sum()), grouped_want, 0)
        sample = slice(0, min(count, 1 << 21))
        ok = ok and work[sample][loose[sample]].tobytes() == full[sample][loose[sample]].tobytes() and bool(np.all(work[sample][~loose[sample]] == 0xA5))
        worst = 0.0
        if grouped_want:
            ids = np.flatnonzero(mass > 0)[:: max(1, int((mass > 0).sum()) // 2000)][:2000]
            order = np.argsort(gid, kind="stable")
            first = np.searchsorted(gid[order], ids)
            scale = float(np.abs(full[: 1 << 20, 8:].copy().view(np.float32)).max())
            for gnum, a in zip(ids.tolist(), first.tolist()):
                mem = order[a:a + int(mass[gnum])]
                want = full[mem, 8:].copy().view(np.float32).reshape(len(mem), 24).astype(np.float64).mean(axis=0)
                got = np.concatenate([groups[gnum, o:o + 12].copy().view(np.float32) for o in GOFF]).astype(np.float64)
                worst = max(worst, float(np.abs(got - want).max()) / scale)
            ok = ok and worst <= 1e-6
        out["ok"] = bool(ok)
        out["worst_mean_difference"] = worst
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--fractions", default="0.2,1.0")
    ap.add_argument("--shares", default="0,0.5,0.9")
    ap.add_argument("--cube", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=600, help="seconds a configuration may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        fr, sh = (float(v) for v in a.one.split(","))
        one(a.n, fr, sh, a.cube, a.reps)
        return 0
    results = []
    for fr in (float(v) for v in a.fractions.split(",")):
        for sh in (float(v) for v in a.shares.split(",")):
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--n", str(a.n), "--reps", str(a.reps), "--cube", str(a.cube), "--one", f"{fr!r},{sh!r}"],
                                   capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                print(f"fraction {fr} share {sh}: no answer within {a.limit} s; nothing more is started", file=sys.stderr)
                return 1
            sys.stderr.write(r.stderr)
            if r.returncode:
                print(f"fraction {fr} share {sh}: exit status {r.returncode}; nothing more is started", file=sys.stderr)
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
