"""Times pf_point_states -- the states of the stored particles of a sub-box at their own collapse times -- beside pf_points_core.h
compiled for the host and run particle by particle on one thread (tests/cpu_emul/points_emul.cpp; profiles/points_notes.md).

Device workload: a box of n^3 cells on one rank after a sweep of four radii and the displacements (synthetic density, float
products, LPT order 3), the fixture's cosmology tables (tests/plc_cases.py); the sub-box is the whole box, the particles are the
cells with Fmax >= 1 in descending Fmax -- the order the group loop walks them in --, segment 0, order 2 (ORDER_FOR_GROUPS).  Per
(n, nk), in a process of its own that the parent ends at a time limit (one that fails or runs out of time ends the run): `reps`
calls after a warm-up without and with the `order` hint -- wall ms of the call and, with PF_POINT_TIMES=1, the device ms of the
select + scan passes and of the state pass (pf_debug_point_times); what is left of the wall time is allocation, the upload of 4 (8)
bytes per particle and the download of 36.
Host form: the case generator of tests/points_cases.py on a box of 64^3 with `host_particles` particles on one core; its time per
particle is scaled to the device workload's count.  Checked and reported: whether the device tap on that same case gives the host
form's states bit for bit.

    python profiles/tools/points_time.py [--sizes 128,256] [--nk 1,10] [--reps 3] [--host-particles 1000000] [--limit 300] [--out profiles/points_times.json]
one JSON line per (n, nk) on stdout.
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


def host_form(c):
    src, so = os.path.join(ROOT, "tests", "cpu_emul", "points_emul.cpp"), os.path.join(ROOT, "tests", "cpu_emul", "libpoints_emul.so")
    hdrs = [os.path.join(ROOT, "pinocchio_amd", "csrc", h) for h in ("pf_points_core.h", "pf_plc_core.h", "pf_refresh_core.h", "pf_back_core.h", "pf_neigh_core.h",
                                                                      "pf_collapse_core.h")]
    if not os.path.exists(so) or any(os.path.getmtime(so) < os.path.getmtime(p) for p in [src] + hdrs):   # as tests/test_points_cpu.py
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DPOINTS_EMUL_LIB", "-o", so, src])
    L = C.CDLL(so)
    L.points_emul_run.restype = C.c_longlong
    L.points_emul_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    hdr, data = c.flat()
    rec, idx = np.zeros((c.count + 1, 8)), np.zeros(c.count + 1, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    t = time.perf_counter()
    found = L.points_emul_run(vp(hdr), vp(data), c.count, vp(rec), vp(idx))
    return (time.perf_counter() - t) * 1e3, int(found), rec[:found].astype(c.T), idx[:found]


def child(n, nk, reps, host_particles):
    os.environ["PF_POINT_TIMES"] = "1"
    import plc_cases as pc
    import points_cases as qc
    from pinocchio_amd import api, synth
    box = ((0, 0, 0), (n, n, n), (0, 0, 0))
    out = {"n": n, "nk": nk}
    with api.Fmax(n) as f:
        f.set_density(synth.make_density(n, seed=synth.SEED))
        f.set_invgrow(*synth.invgrow_table("lcdm"))
        f.sweep(np.array([2.0, 1.0, 0.5, 0.0]))
        f.set_growth(synth.growth_multipliers())
        f.compute_displacements(1, 0)
        f.plc_set_cosmology(**pc.cosmology_tables(nk))
        F = f.products()["Fmax"].reshape(-1)
        cells = np.flatnonzero(F >= 1.0)
        pos = cells[np.argsort(-F[cells], kind="stable")].astype(np.uint32)      # x-slab cell index = sub-box position: the sub-box is the box
        hint = np.argsort(pos, kind="stable").astype(np.int32)
        out["particles"] = int(pos.size)
        for label, h in (("natural", None), ("hinted", hint)):
            call = lambda: f.point_states(0, 0.0, box, pos, qc.SIGMA0, 0.1 if nk == 1 else 1.2, 0.1 if nk == 1 else 0.02, order=h)
            first = call()
            wall, dev = [], []
            for _ in range(reps):
                t = time.perf_counter()
                got = call()
                wall.append((time.perf_counter() - t) * 1e3)
                dev.append(api.point_times())
            assert got[2] == pos.size and got[1].tobytes() == first[1].tobytes()
            rnd = lambda a: [round(x, 3) for x in a]
            out[label] = {"wall_ms": rnd(wall), "device_ms_select_scan": rnd(d[0] for d in dev), "device_ms_states": rnd(d[1] for d in dev),
                          "rest_ms": rnd(w - d[0] - d[1] for w, d in zip(wall, dev))}
    hbox = dict(n=64, x0=0, nxl=64, start=(0, 0, 0), length=(64, 64, 64), safe=(0, 0, 0))
    c = qc.Case("time", box=hbox, count=host_particles, nk=nk, k_point=0.1 if nk == 1 else 0.02, k_sigma=0.1 if nk == 1 else 1.2, seed=1)
    host_ms, found, hrec, hidx = host_form(c)
    with api.Fmax(16) as tab:
        tab.plc_set_cosmology(**pc.cosmology_tables(nk))
        index, st = api.debug_point_states(c.n, c.x0, c.fmax, c.cols, tab, c.myseg, qc.Z_SEG, (c.start, c.length, c.safe), c.pos, qc.SIGMA0, c.k_sigma, c.k_point,
                                           groups_order=c.order, z_prev=qc.Z_PREV)
    out.update({"host_particles": found, "host_one_core_ms_measured": round(host_ms, 1), "host_one_core_ms_scaled_to_all": round(host_ms * out["particles"] / max(found, 1), 1),
                "host_matches_device_bit_for_bit": bool(np.array_equal(index, hidx) and st.tobytes() == hrec.tobytes()),
                "host_device_values_that_differ": int((st != hrec).sum()) if st.shape == hrec.shape else -1})
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--nk", default="1,10")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-particles", type=int, default=1000000)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        n, nk = (int(t) for t in a.child.split("x"))
        sys.exit(child(n, nk, a.reps, a.host_particles))
    lines = []
    for cfg in [f"{n}x{k}" for k in a.nk.split(",") for n in a.sizes.split(",")]:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", cfg, "--reps", str(a.reps), "--host-particles", str(a.host_particles)],
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
