"""Times pf_catalog -- write_catalog() and compute_mf() of one output on the device -- beside pf_catalog_core.h compiled for the host
and run group by group on one thread, the loop the reference runs (tests/cpu_emul/catalog_emul.cpp; profiles/catalog_notes.md).

Workload: the generator of tests/catalog_cases.py (the fixture's cosmology tables, a sub-box of 64 cells in a box of 128, float
products, segment 0, order 3, the mass function of 100 bins); masses 10 ... 499 with nk = 1 and the list of plc_cases with nk = 10.

Per batch, in a process of its own that the parent ends at a time limit (a batch that fails or runs out of time ends the run):
`reps` calls after a warm-up -- wall ms of the call, the host's wall ms of its pack / upload / device / download parts
(pf_debug_catalog_parts) and, with PF_CATALOG_TIMES=1, the device ms of the flag + scan passes and of the record + histogram passes
(pf_debug_catalog_times); then the host form on the first `host_groups` groups on one core, its time scaled to all of them.
Checked: the host form's records for those groups are the device's bit for bit.

    python profiles/tools/catalog_time.py [--batches 100000,1000000,10000000] [--nk 1,10] [--reps 3] [--host-groups 1000000] [--limit 300] [--out profiles/catalog_times.json]
one JSON line per (batch, nk) on stdout.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_form(c, n):
    src, so = os.path.join(ROOT, "tests", "cpu_emul", "catalog_emul.cpp"), os.path.join(ROOT, "tests", "cpu_emul", "libcatalog_emul.so")
    hdrs = [os.path.join(ROOT, "pinocchio_amd", "csrc", h) for h in ("pf_catalog_core.h", "pf_plc_core.h", "pf_collapse_core.h")]
    if not os.path.exists(so) or any(os.path.getmtime(so) < os.path.getmtime(p) for p in [src] + hdrs):   # as tests/test_catalog_cpu.py
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DCATALOG_EMUL_LIB", "-o", so, src])
    L = C.CDLL(so)
    L.catalog_emul_run.restype = C.c_longlong
    L.catalog_emul_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    full = c.groups
    c.groups, c.n = full[:n], n
    hdr, data = c.flat()
    c.groups, c.n = full, len(full)
    rec, idx, nin, mas = np.zeros((n + 1, 10)), np.zeros(n + 1, np.int32), np.zeros(c.nbin + 1, np.int32), np.zeros(c.nbin + 1)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    t = time.perf_counter()
    count = L.catalog_emul_run(vp(hdr), vp(data), n, vp(rec), vp(idx), vp(nin), vp(mas))
    return (time.perf_counter() - t) * 1e3, int(count), rec[:count], idx[:count]


def child(n, nk, reps, host_groups):
    os.environ["PF_CATALOG_TIMES"] = "1"
    import catalog_cases as cc
    from pinocchio_amd import api
    c = cc.Case("time", n=n, nk=nk, min_mass=cc.MIN_MASS if nk == 1 else 0, seed=1)
    o = None
    with api.Fmax(16) as f:
        f.plc_set_cosmology(**cc.pc.cosmology_tables(nk))
        call = lambda: f.catalog(groups=c.groups, out_dtype=cc.catalog_dtype(c.T), **c.call_kwargs())
        call()
        wall, dev, parts = [], [], []
        for _ in range(reps):
            t = time.perf_counter()
            o = call()
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(api.catalog_times())
            parts.append(api.catalog_parts())
    hn = min(host_groups, n)
    host_ms, hcount, hrec, hidx = host_form(c, hn)
    first = o[1] < hn
    r = o[0][first]
    same = int(first.sum()) == hcount and np.array_equal(o[1][first], hidx) and np.array_equal(r["M"].astype(np.float64), hrec[:, 0])
    same = bool(same and all(np.array_equal(r[k].astype(np.float64), hrec[:, a:a + 3]) for k, a in (("x", 1), ("v", 4), ("q", 7))))
    rnd = lambda a: [round(x, 3) for x in a]
    print(json.dumps({"groups": n, "nk": nk, "records": o[2], "binned": int(o[3].sum()), "wall_ms": rnd(wall), "pack_ms": rnd(p[0] for p in parts),
                      "upload_ms": rnd(p[1] for p in parts), "device_part_ms": rnd(p[2] for p in parts), "download_records_ms": rnd(p[3] for p in parts),
                      "device_ms_flag_scan": rnd(d[0] for d in dev), "device_ms_records_hist": rnd(d[1] for d in dev), "host_groups": hn,
                      "host_one_core_ms_measured": round(host_ms, 1), "host_one_core_ms_scaled_to_all": round(host_ms * n / hn, 1), "host_matches_device": same}))
    return 0 if same else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="100000,1000000,10000000")
    ap.add_argument("--nk", default="1,10")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-groups", type=int, default=1000000)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        n, nk = (int(t) for t in a.child.split("x"))
        sys.exit(child(n, nk, a.reps, a.host_groups))
    lines = []
    for cfg in [f"{n}x{k}" for k in a.nk.split(",") for n in a.batches.split(",")]:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", cfg, "--reps", str(a.reps), "--host-groups", str(a.host_groups)],
                               capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"{cfg}: ran out of its {a.limit} s; stopping", file=sys.stderr)
            sys.exit(2)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        lines += [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode:
            sys.stderr.write(r.stderr[-2000:])
            print(f"{cfg}: exit status {r.returncode}; stopping", file=sys.stderr)
            sys.exit(r.returncode if r.returncode > 0 else 1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
