"""Times pf_distribute_back and the ZACC block beside the reference's loop on the host (profiles/back_notes.md).

Workload: the whole periodic n^3 box as one sub-box on one rank, a random 60 % of its cells stored, in random order (the order after
sort_and_organize is by Fmax, which says nothing about the position), fp32 zacc and group_ID in packed arrays.

Per n, in a process of its own that the parent ends at a time limit (a step that fails or runs out of time ends the run):
 (a) the device time of the scatter kernel (HIP events of a PF_FLAG_TIMING context: the "distribute" class of pf_kernel_stats, which
     holds nothing else in these calls);
 (b) the wall time of pf_distribute_back: staging, the upload of 12 bytes per particle through the hand-off pieces, the kernel, the
     count;
 (c) the wall time of pf_get_block("ZACC"): 4 bytes per cell through the hand-off pieces;
 (d) the loop of keep_data_back (src/distribute.c:806-834) on the host for the same arrays: port_back of
     tests/cpu_emul/back_emul.cpp, -O2, one thread.  Its columns are also the check of the device's.

    python profiles/tools/back_time.py [--n 128,256,512] [--limit 300] [--out FILE.json]
one JSON line per n on stdout.
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
BIN = os.path.join(HERE, "bin")
EMUL = os.path.join(ROOT, "tests", "cpu_emul", "back_emul.cpp")


def host_lib():
    os.makedirs(BIN, exist_ok=True)
    so = os.path.join(BIN, "libback_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(EMUL):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, EMUL])
    L = C.CDLL(so)
    ip, up, fp = C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(C.c_float)
    L.port_back.restype = C.c_ulonglong
    L.port_back.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip, ip, C.c_size_t, up, fp, ip, fp, ip]
    return L


def one(n):
    from pinocchio_amd import api
    H = host_lib()
    rng = np.random.default_rng(n)
    cells = n ** 3
    m = int(round(0.6 * cells))
    pos = rng.permutation(cells)[:m].astype(np.uint32)
    zacc = rng.random(m, dtype=np.float32) * np.float32(10.0)
    gid = rng.integers(1, 2 ** 31, m, dtype=np.int64).astype(np.int32)
    box = ((0, 0, 0), (n, n, n), (0, 0, 0))
    out = {"n": n, "particles": m, "upload_bytes": 12 * m}
    with api.Fmax(n, field_bytes=4, timing=True) as f:
        f.distribute_back(*box, pos, zacc, gid)                             # warm-up: first touch, code objects, the columns, the pinned pieces
        f.block("ZACC")
        walls, kernels, blocks = [], [], []
        for rep in range(3):
            f.back_reset()
            f.synchronize()
            f.reset_kernel_stats()
            t0 = time.perf_counter()
            stored = f.distribute_back(*box, pos, zacc, gid)
            walls.append(1e3 * (time.perf_counter() - t0))
            ks = [k for k in f.kernel_stats() if k["name"] == "distribute"]
            kernels.append(ks[0]["total_ms"] if ks else float("nan"))
            t0 = time.perf_counter()
            z = f.block("ZACC")
            blocks.append(1e3 * (time.perf_counter() - t0))
        g = f.block("GRUP")
    out.update(stored=stored, scatter_kernel_ms=float(np.median(kernels)), scatter_kernel_ms_all=kernels, call_wall_ms=float(np.median(walls)),
               call_wall_ms_all=walls, block_zacc_wall_ms=float(np.median(blocks)), block_zacc_wall_ms_all=blocks)
    out["upload_GBps_of_the_call"] = 12e-9 * m / (1e-3 * out["call_wall_ms"])
    hz = np.full(cells, -1.0, dtype=np.float32)
    hg = np.zeros(cells, dtype=np.int32)
    i3 = (C.c_int * 3)
    t0 = time.perf_counter()
    hs = H.port_back(n, 0, n, i3(0, 0, 0), i3(n, n, n), i3(0, 0, 0), m, pos.ctypes.data_as(C.POINTER(C.c_uint)), zacc.ctypes.data_as(C.POINTER(C.c_float)),
                     gid.ctypes.data_as(C.POINTER(C.c_int)), hz.ctypes.data_as(C.POINTER(C.c_float)), hg.ctypes.data_as(C.POINTER(C.c_int)))
    out["host_loop_ms"] = 1e3 * (time.perf_counter() - t0)
    out["host_agrees"] = bool(int(hs) == stored and np.array_equal(hz, z) and np.array_equal(hg, g))
    out["kernel_share_of_call"] = out["scatter_kernel_ms"] / out["call_wall_ms"]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="128,256,512")
    ap.add_argument("--limit", type=int, default=300, help="seconds a size may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        one(a.one)
        return 0
    host_lib()
    results = []
    for n in (int(v) for v in a.n.split(",")):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n)], capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"n = {n}: no answer within {a.limit} s; nothing more is started", file=sys.stderr)
            return 1
        sys.stderr.write(r.stderr)
        if r.returncode:
            print(f"n = {n}: exit status {r.returncode}; nothing more is started", file=sys.stderr)
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
