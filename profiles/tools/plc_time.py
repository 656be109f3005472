"""Times pf_plc_cross -- the light-cone test of build_groups() on the device -- beside pf_plc_core.h compiled for the host and run per
(group, replication) pair on one thread, the reference's form (tests/cpu_emul/plc_emul.cpp; profiles/plc_notes.md).

Workload: the generator of tests/plc_cases.py (the fixture's cosmology tables and cone, a sub-box of 64 cells, displacements of order
one cell), PF_PLC_EVENTS with intervals of 0.003 in F so that a small share of the tried pairs cross, as in a run; the replications
are whole-box shifts of 8 cells taken from a cube around the observer -- `nrep` of them, up to 343 (a deep cone).  What share of the
pairs is tried and crosses in a real cone has been measured by nobody but for the example's last check (119 of about 89 000 x 13);
the share here is printed with the times.

Per configuration (candidates x replications), in a process of its own that the parent ends at a time limit (a configuration that
fails or runs out of time ends the run): `reps` calls after a warm-up -- wall ms of the call, and with PF_PLC_TIMES=1 the device ms
of the candidate passes and of the root + store passes (pf_debug_plc_times); then the host form on the first `host_cand` candidates,
its time scaled to all of them.  Checked: the host form's records for those candidates are the device's (pairs, z bit for bit).

    python profiles/tools/plc_time.py [--configs 4096x13,65536x13,65536x343] [--reps 3] [--host-cand 4096] [--nk 1] [--limit 300] [--out FILE.json]
one JSON line per configuration on stdout.
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


def make_case(ncand, nrep, nk):
    import plc_cases as pc
    c = pc.Case("time", ncand=ncand, nrep=65, events=True, nk=nk, seed=1)
    shifts = sorted(((i, j, k) for i in range(-3, 4) for j in range(-3, 4) for k in range(-3, 4)), key=lambda s: (s[0] ** 2 + s[1] ** 2 + s[2] ** 2, s))[:nrep]
    c.reps = [(i, j, k, 1.5, 1.0) for (i, j, k) in shifts]
    c.f_lo = np.maximum(c.groups["Flast"] - 0.003, 1.0).astype(c.T)
    return c, pc


def host_form(c, pc, ncand):
    src, so = os.path.join(ROOT, "tests", "cpu_emul", "plc_emul.cpp"), os.path.join(ROOT, "tests", "cpu_emul", "libplc_emul.so")
    hdrs = [os.path.join(ROOT, "pinocchio_amd", "csrc", h) for h in ("pf_plc_core.h", "pf_collapse_core.h")]
    if not os.path.exists(so) or any(os.path.getmtime(so) < os.path.getmtime(p) for p in [src] + hdrs):   # as tests/test_plc_cpu.py
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DPLC_EMUL_LIB", "-o", so, src])
    L = C.CDLL(so)
    L.plc_emul_run.restype = C.c_longlong
    L.plc_emul_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong)]
    full_g, full_f = c.groups, c.f_lo
    c.groups, c.f_lo, c.ncand = full_g[:ncand], full_f[:ncand], ncand
    hdr, data = c.flat()
    c.groups, c.f_lo, c.ncand = full_g, full_f, len(full_g)
    cap = ncand * len(c.reps)
    rec, oc, orr, nz, unc = np.zeros((cap + 1, 7)), np.zeros(cap + 1, np.int32), np.zeros(cap + 1, np.int32), np.zeros(c.nzbins + 1), C.c_longlong()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    t = time.perf_counter()
    n = L.plc_emul_run(vp(hdr), vp(data), cap, vp(rec), vp(oc), vp(orr), vp(nz), C.byref(unc))
    return (time.perf_counter() - t) * 1e3, int(n), rec[:n, 0], oc[:n], orr[:n]


def child(ncand, nrep, nk, reps, host_cand):
    os.environ["PF_PLC_TIMES"] = "1"
    from pinocchio_amd import api
    c, pc = make_case(ncand, nrep, nk)
    o = None
    with api.Fmax(16) as f:
        f.plc_set_cosmology(**pc.cosmology_tables(nk))
        f.plc_set_geometry(**c.geometry_kwargs())
        call = lambda: f.plc_cross(api.PLC_EVENTS, c.myseg, c.z_seg, c.stabl, c.groups, f_lo=c.f_lo, min_mass=c.min_mass, capacity=ncand * 4, out_dtype=pc.out_dtype(c.T))
        call()
        wall, dev = [], []
        for _ in range(reps):
            t = time.perf_counter()
            o = call()
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(api.plc_times())
    hc = min(host_cand, ncand)
    host_ms, hn, hz, hcand, hrep = host_form(c, pc, hc)
    first = o[1] < hc
    same = int(first.sum()) == hn and np.array_equal(o[1][first], hcand) and np.array_equal(o[2][first], hrep) and np.array_equal(o[0]["z"][first].astype(np.float64), hz)
    geo = c.np_objects()[1]
    import np_plc as npp
    tried = int(npp.tried(True, c.f_lo, c.groups["Flast"], geo, c.T).sum())
    print(json.dumps({"ncand": ncand, "nrep": nrep, "nk": nk, "pairs": ncand * nrep, "tried": tried, "stored": o[3], "unconverged": o[4],
                      "wall_ms": [round(w, 3) for w in wall], "device_ms_candidates": [round(d[0], 3) for d in dev], "device_ms_root_store": [round(d[1], 3) for d in dev],
                      "host_cand": hc, "host_ms_measured": round(host_ms, 1), "host_ms_scaled_to_all": round(host_ms * ncand / hc, 1), "host_matches_device": bool(same)}))
    return 0 if same and o[4] == 0 else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="4096x13,65536x13,65536x343")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-cand", type=int, default=4096)
    ap.add_argument("--nk", type=int, default=1)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        nc, nr = (int(t) for t in a.child.split("x"))
        sys.exit(child(nc, nr, a.nk, a.reps, a.host_cand))
    lines = []
    for cfg in a.configs.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", cfg, "--reps", str(a.reps), "--host-cand", str(a.host_cand), "--nk", str(a.nk)],
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
