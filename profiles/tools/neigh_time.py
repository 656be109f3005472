"""Times the context-free pf_neighbours beside the reference's way of finding neighbours (profiles/neigh_notes.md).

Synthetic stored sets: a box of Lx = Ly and the given Lz with about twice as many cells as records, every direction periodic, every
cell stored with probability 0.5 (so that half of the lookups find a particle), continuous fp32 Fmax drawn independently of the
position, the records in the order after sort_and_organize (descending Fmax).

Per set, after one warm-up call:
 (a) the device time of the position sort and of the table kernels (HIP events: PF_NEIGH_STATS=1, pf_debug_neigh_ms) in the row
     form (the default) and with PF_NEIGH_ROWS=0 (one search of the whole of sorted_pos per neighbour);
 (b) the wall time of the whole call of either form: staging, uploads (8 bytes per record), sort, kernels and the 25 bytes per record
     that come back;
 (c) the reference's way on the host: per particle in Fmax order INDEX_TO_COORD, the six wrapped neighbours, one bsearch over
     sorted_pos each, indices[], the Fmax comparison (src/fragment.c:592-603, src/build_groups.c:274-323) -- written here from that
     description, compiled with cc -O2, one thread.  It is given sorted_pos / indices ready made; building them is not in its time.
     Its table and count are also the check of the device's.

    python profiles/tools/neigh_time.py [--counts 1000000,10000000,100000000] [--lz 256,1024] [--no-host-above N] [--out FILE.json]
one JSON line per set on stdout.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
BIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bin")

HOST_C = r"""
#include <stdlib.h>
static int cmp_u32(const void *a, const void *b) {
  const unsigned int x = *(const unsigned int *)a, y = *(const unsigned int *)b;
  return x < y ? -1 : (x > y ? 1 : 0);
}
/* every direction periodic; returns Npeaks */
long long host_neighbours(int lx, int ly, int lz, long long count, const unsigned int *frag_pos, const float *fmax, const unsigned int *sorted_pos,
                          const int *indices, int *neigh) {
  long long npeaks = 0;
  for (long long iz = 0; iz < count; iz++) {
    const unsigned int pos = frag_pos[iz];
    const int k = (int)(pos % (unsigned int)lz), j = (int)((pos / (unsigned int)lz) % (unsigned int)ly), i = (int)(pos / ((unsigned int)lz * (unsigned int)ly));
    int peak = 1;
    for (int nn = 0; nn < 6; nn++) {
      int i1 = i, j1 = j, k1 = k;
      switch (nn) {
        case 0: i1 = i == 0 ? lx - 1 : i - 1; break;
        case 1: i1 = i == lx - 1 ? 0 : i + 1; break;
        case 2: j1 = j == 0 ? ly - 1 : j - 1; break;
        case 3: j1 = j == ly - 1 ? 0 : j + 1; break;
        case 4: k1 = k == 0 ? lz - 1 : k - 1; break;
        default: k1 = k == lz - 1 ? 0 : k + 1; break;
      }
      const unsigned int key = (unsigned int)k1 + (unsigned int)lz * ((unsigned int)j1 + (unsigned int)ly * (unsigned int)i1);
      const unsigned int *hit = (const unsigned int *)bsearch(&key, sorted_pos, (size_t)count, sizeof(unsigned int), cmp_u32);
      int q = -1;
      if (hit) { q = indices[hit - sorted_pos]; peak &= (fmax[iz] > fmax[q]); }
      neigh[6 * iz + nn] = q;
    }
    npeaks += peak;
  }
  return npeaks;
}
"""


def host_lib():
    os.makedirs(BIN, exist_ok=True)
    src, so = os.path.join(BIN, "neigh_host.c"), os.path.join(BIN, "libneigh_host.so")
    if not os.path.exists(so) or not os.path.exists(src) or open(src).read() != HOST_C:
        with open(src, "w") as fh:
            fh.write(HOST_C)
        subprocess.check_call(["cc", "-O2", "-shared", "-fPIC", "-o", so, src])
    L = C.CDLL(so)
    L.host_neighbours.restype = C.c_longlong
    L.host_neighbours.argtypes = [C.c_int, C.c_int, C.c_int, C.c_longlong, C.POINTER(C.c_uint), C.POINTER(C.c_float), C.POINTER(C.c_uint),
                                  C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return L


def stored_set(count, lz, seed):
    side = int(np.ceil(np.sqrt(2.0 * count / lz)))
    length = (side, side, lz)
    cells = side * side * lz
    assert cells < 1 << 32
    rng = np.random.default_rng(seed)
    spos = np.flatnonzero(rng.random(cells, dtype=np.float32) < np.float32(0.5)).astype(np.uint32)      # ascending
    m = len(spos)
    f = np.sort(rng.random(m, dtype=np.float32) * np.float32(4.0))[::-1].copy()                          # the sorted order's Fmax
    indices = rng.permutation(m).astype(np.int32)                                                        # rank -> particle
    pos = np.empty(m, dtype=np.uint32)
    pos[indices] = spos
    return length, pos, f, spos, indices


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="1000000,10000000,100000000")
    ap.add_argument("--lz", default="256,1024")
    ap.add_argument("--no-host-above", type=int, default=0, help="skip the host's way for sets larger than this (0: never skip)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from pinocchio_amd import _lib, api
    L = _lib.load()
    H = host_lib()
    up, ip = C.POINTER(C.c_uint), C.POINTER(C.c_int)
    results = []
    for count in (int(v) for v in a.counts.split(",")):
        for lz in (int(v) for v in a.lz.split(",")):
            length, pos, f, spos, indices = stored_set(count, lz, seed=count % 1000 + lz)
            m = len(pos)
            out = {"records": m, "box": list(length), "fill": m / (length[0] * length[1] * length[2])}
            rg = api._region(((0, 0, 0), length, (0, 0, 0)))
            neigh = {k: np.empty((m, 6), dtype=np.int32) for k in ("rows", "plain")}
            flags = np.empty(m, dtype=np.uint8)
            peaks = (C.c_ulonglong * 2)()

            def call(form):
                os.environ["PF_NEIGH_ROWS"] = "1" if form == "rows" else "0"
                t0 = time.perf_counter()
                rc = L.pf_neighbours(None, C.byref(rg), m, pos.ctypes.data_as(up), C.c_void_p(f.ctypes.data), 4, neigh[form].ctypes.data_as(ip),
                                     flags.ctypes.data_as(C.POINTER(C.c_ubyte)), peaks)
                wall = time.perf_counter() - t0
                if rc:
                    raise RuntimeError(L.pf_last_error().decode())
                return 1e3 * wall

            os.environ["PF_NEIGH_STATS"] = "1"
            call("rows")                                                     # warm-up: first touch of the host arrays, code objects
            for form in ("rows", "plain"):
                walls, sorts, tables = [], [], []
                for rep in range(3):
                    walls.append(call(form))
                    s, t = C.c_double(), C.c_double()
                    if L.pf_debug_neigh_ms(C.byref(s), C.byref(t)):
                        raise RuntimeError(L.pf_last_error().decode())
                    sorts.append(s.value); tables.append(t.value)
                out[form] = {"table_kernels_ms": float(np.median(tables)), "table_kernels_ms_all": tables, "sort_ms": float(np.median(sorts)),
                             "call_wall_ms": float(np.median(walls)), "call_wall_ms_all": walls, "peaks": [int(peaks[0]), int(peaks[1])]}
            out["same_arrays"] = bool(np.array_equal(neigh["rows"], neigh["plain"]) and out["rows"]["peaks"] == out["plain"]["peaks"])
            out["plain_over_rows_table_kernels"] = out["plain"]["table_kernels_ms"] / out["rows"]["table_kernels_ms"]
            if not a.no_host_above or m <= a.no_host_above:
                hneigh = neigh["plain"]                                      # reuse the memory: "plain" has been compared already
                keep = out["same_arrays"]
                hneigh[:] = -2
                t0 = time.perf_counter()
                hp = H.host_neighbours(length[0], length[1], length[2], m, pos.ctypes.data_as(up), f.ctypes.data_as(C.POINTER(C.c_float)),
                                       spos.ctypes.data_as(up), indices.ctypes.data_as(ip), hneigh.ctypes.data_as(ip))
                out["host_reference_way_ms"] = 1e3 * (time.perf_counter() - t0)
                out["host_agrees"] = bool(keep and np.array_equal(hneigh, neigh["rows"]) and int(hp) == out["rows"]["peaks"][0])
                out["host_over_rows_call"] = out["host_reference_way_ms"] / out["rows"]["call_wall_ms"]
            print(json.dumps(out), flush=True)
            results.append(out)
            del neigh, flags, pos, f, spos, indices
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
