"""Times pf_distribute_sorted beside pf_distribute and beside the host work it replaces (profiles/organize_notes.md).

One rank, an n^3 context with fp64 fields, fp32 products and the bench's synthetic density, one sweep with the bench radii
(synth.radii_ladder(12)) and the displacements; then flast = 1, map = NULL, the whole periodic box as the sub-box and the 104-byte
record of a RECOMPUTE_DISPLACEMENTS build (src/pinocchio.h:233-259):

 (a) wall time of pf_distribute (records + frag_pos) and of pf_distribute_sorted (records, frag_pos, sorted_pos, indices);
 (b) device time of pf_distribute_sorted by part, from HIP events of the "distribute" kernel class (pf_kernel_stats) of four calls
     that differ in the outputs they ask for: S = flag + scan (a count-only call), O = pack of cell_index / frag_pos + keys + pair
     sort, I = position gather + pair sort by position, G = the gather of the records:
         count-only = S, indices only = S + O + I, records only = S + O + G, everything = S + O + I + G;
 (c) the gather's bytes per second -- per record the record's words read and written, perm, cell_index, frag_pos read and frag_pos
     written -- against the context's read stream rate (pf_debug_stream_rate, kind 0);
 (d) the same gather with PF_DISTRIBUTE_LDS=0, one lane per record, in a second context;
 (e) a stand-in for the host work the call replaces: numpy's stable argsort by -Fmax, the permutation of the 104-byte records and of
     frag_pos, and the stable argsort by position (tests/np_organize.py), single-threaded as numpy's sorts are.  A stand-in for the
     reference's qsort + reorder + qsort, not a measurement of them.
 A per-kernel trace is a run of its own:
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/tools/organize_time.py --only-kernels --reps 1

Warm-up: two calls of each kind before anything is timed; `--reps` timed repetitions, alternating; median, min and max reported.

    python profiles/tools/organize_time.py [--n 256] [--reps 5] [--out FILE.json]     one JSON line on stdout
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STRIDE = 104


def spread(v):
    v = np.array(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(len(v))}


def context(n, lds):
    from pinocchio_amd import api, synth
    os.environ["PF_DISTRIBUTE_LDS"] = "1" if lds else "0"
    f = api.Fmax(n, field_bytes=8, timing=True)
    f.synth_density(synth.SEED, 2.5, -2.0)
    f.set_invgrow(*synth.invgrow_table("lcdm"))
    f.set_growth(synth.growth_multipliers())
    f.compute_fmax(synth.radii_ladder(12), do_lpt=True)
    return f


def kernel_ms(f):
    return sum(k["total_ms"] for k in f.kernel_stats() if k["name"] == "distribute")


class Caller:
    def __init__(self, f, n, cnt):
        from pinocchio_amd import _lib, api
        self.f, self.n = f, n
        self.lay = _lib.ProductLayout(STRIDE, 0, 4, 8, 20, 32, 44)
        self.sub = api._subbox((0, 0, 0), (n, n, n))
        self.rec = np.zeros((cnt, STRIDE), dtype=np.uint8)
        self.pos = np.zeros(cnt, dtype=np.uint32)
        self.spos = np.zeros(cnt, dtype=np.uint32)
        self.ind = np.zeros(cnt, dtype=np.int32)
        self.cnt = C.c_size_t()

    def sorted(self, rec=True, pos=True, index=True, count_only=False):
        f, up = self.f, C.POINTER(C.c_uint)
        f._chk(f.L.pf_distribute_sorted(f.h, 1.0, C.byref(self.sub), None, C.byref(self.lay), 0 if count_only else len(self.pos),
                                        self.rec.ctypes.data_as(C.c_void_p) if rec else None, self.pos.ctypes.data_as(up) if pos else None,
                                        self.spos.ctypes.data_as(up) if index else None,
                                        self.ind.ctypes.data_as(C.POINTER(C.c_int)) if index else None, C.byref(self.cnt)))

    def plain(self):
        f = self.f
        f._chk(f.L.pf_distribute(f.h, 1.0, C.byref(self.sub), None, C.byref(self.lay), len(self.pos), self.rec.ctypes.data_as(C.c_void_p),
                                 self.pos.ctypes.data_as(C.POINTER(C.c_uint)), C.byref(self.cnt)))


def parts(c, reps):
    """-> S, O, I, G in ms per repetition"""
    out = {k: [] for k in "SOIG"}
    for rep in range(reps + 2):
        ms = []
        for kw in (dict(count_only=True), dict(rec=False, pos=False), dict(index=False, pos=False), dict()):
            c.f.reset_kernel_stats()
            c.sorted(**kw)
            ms.append(kernel_ms(c.f))
        s, soi, sog, all_ = ms
        if rep >= 2:
            out["S"].append(s); out["G"].append(all_ - soi); out["I"].append(all_ - sog); out["O"].append(soi + sog - all_ - s)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-kernels", action="store_true", help="the sorted call alone, for a kernel trace")
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import np_organize as npo
    n, nc = a.n, a.n ** 3
    out = {"n": n, "reps": a.reps, "flast": 1.0, "map": None, "subbox": "whole box", "stride": STRIDE}
    f = context(n, lds=True)
    cnt = f.distribute(1.0, (0, 0, 0), (n, n, n), capacity=0)[2]
    out["selected"], out["selected_fraction"] = cnt, cnt / nc
    c = Caller(f, n, cnt)
    if a.only_kernels:
        for _ in range(a.reps + 1):
            c.sorted()
        f.close()
        print(json.dumps(out))
        return
    g = C.c_double()
    f._chk(f.L.pf_debug_stream_rate(f.h, 0, 10, C.byref(g)))
    out["read_stream_gbps"] = g.value
    f._chk(f.L.pf_debug_stream_rate(f.h, 2, 10, C.byref(g)))
    out["copy_stream_gbps"] = g.value
    p = parts(c, a.reps)
    for k, name in (("S", "flag_scan_ms"), ("O", "pack_keys_sort_ms"), ("I", "position_index_ms"), ("G", "gather_ms")):
        out[name] = spread(p[k])
    per_record = 2.0 * STRIDE + 4 + 4 + 4 + 4
    out["gather_bytes"] = per_record * cnt
    out["gather_gbps"] = per_record * cnt / (out["gather_ms"]["median"] * 1e-3) / 1e9
    out["gather_fraction_of_read_stream"] = out["gather_gbps"] / out["read_stream_gbps"]
    wall_plain, wall_sorted = [], []
    for rep in range(a.reps + 2):
        t0 = time.perf_counter()
        c.plain()
        t1 = time.perf_counter()
        if rep == 0:
            rec0, pos0 = c.rec.copy(), c.pos.copy()
        c.sorted()
        t2 = time.perf_counter()
        if rep >= 2:
            wall_plain.append(1e3 * (t1 - t0)); wall_sorted.append(1e3 * (t2 - t1))
    out["distribute_wall_ms"], out["distribute_sorted_wall_ms"] = spread(wall_plain), spread(wall_sorted)
    f.close()
    # (e) the host stand-in, which is also the check that the timed call did the work
    host = []
    for rep in range(a.host_reps):
        t0 = time.perf_counter()
        fm = np.ascontiguousarray(rec0[:, 4:8]).view(np.float32).ravel()
        o = npo.order(fm)
        hrec, hpos = rec0[o], pos0[o]
        hspos, hind = npo.index(hpos)
        host.append(1e3 * (time.perf_counter() - t0))
    assert np.array_equal(hpos, c.pos) and np.array_equal(hspos, c.spos) and np.array_equal(hind, c.ind) and np.array_equal(hrec, c.rec)
    out["numpy_stand_in_ms"] = spread(host)
    del hrec, rec0
    f = context(n, lds=False)
    c2 = Caller(f, n, cnt)
    p = parts(c2, a.reps)
    out["gather_plain_ms"] = spread(p["G"])
    out["ratio_plain_over_staged"] = out["gather_plain_ms"]["median"] / out["gather_ms"]["median"]
    assert np.array_equal(c2.rec, c.rec)
    f.close()
    out["scratch_bytes_per_record"] = 28
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
