"""Times pf_distribute beside the calls it is to be compared with (profiles/r08_distribute.md and .json).

One rank, an n^3 context (1024 by default) with fp64 fields and the bench's synthetic density, one sweep with the bench radii
(synth.radii_ladder(12)), then flast = 1, map = NULL and the whole box as the sub-box:

 (a) wall time of pf_distribute (records + frag_pos into host arrays) against pf_get_products of the same context, with the
     selected fraction beside it -- both are bound by the same host link;
 (b) device time of the flag + scan + pack kernels alone (HIP events of the "distribute" kernel class: a count-only call gives flag +
     scan, the difference to a full call the packs) against the time the context's read stream rate (pf_debug_stream_rate, kind 0)
     needs for the bytes they must touch: the Fmax column once, plus the record's words per selected cell read and written;
 (c) the same packs with PF_DISTRIBUTE_LDS=0, the plain one-lane-per-record form, in a second context;
 (d) is a counter run of its own, kernels only:
       rocprofv3 --pmc FETCH_SIZE WRITE_SIZE --kernel-trace --output-format csv -d DIR -- python profiles/tools/distribute_time.py --only-kernels --reps 1

Warm-up: two calls of each kind before anything is timed; `--reps` timed repetitions, alternating; median, min and max reported.

    python profiles/tools/distribute_time.py [--n 1024] [--reps 5] [--out DIR]     one JSON line on stdout; DIR: also the .md and .json
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


def spread(v):
    v = np.array(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(len(v))}


def _api():
    from pinocchio_amd import api
    return api


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


def time_kernels(f, n, reps, rec, pos):
    """-> (flag + scan ms, pack ms, count) per repetition: device events of the kernel class"""
    lay, _ = f.product_layout()
    sub = _api()._subbox((0, 0, 0), (n, n, n))
    cnt = C.c_size_t()
    fs, pk = [], []
    for rep in range(reps + 2):
        f.reset_kernel_stats()
        f._chk(f.L.pf_distribute(f.h, 1.0, C.byref(sub), None, C.byref(lay), 0, None, None, C.byref(cnt)))
        a = kernel_ms(f)
        f.reset_kernel_stats()
        f._chk(f.L.pf_distribute(f.h, 1.0, C.byref(sub), None, C.byref(lay), len(pos), rec.ctypes.data_as(C.c_void_p),
                                 pos.ctypes.data_as(C.POINTER(C.c_uint)), C.byref(cnt)))
        b = kernel_ms(f)
        if rep >= 2:
            fs.append(a)
            pk.append(b - a)
    return fs, pk, cnt.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-kernels", action="store_true", help="no pf_get_products, no second context: for a counter run")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, nc = a.n, a.n ** 3
    out = {"n": n, "reps": a.reps, "flast": 1.0, "map": None, "subbox": "whole box"}
    f = context(n, lds=True)
    lay, dtype = f.product_layout()
    cnt = f.distribute(1.0, (0, 0, 0), (n, n, n), capacity=0)[2]
    out["selected"], out["selected_fraction"] = cnt, cnt / nc
    rec = np.zeros((cnt, lay.stride), dtype=np.uint8)
    pos = np.zeros(cnt, dtype=np.uint32)
    g = C.c_double()
    f._chk(f.L.pf_debug_stream_rate(f.h, 0, 10, C.byref(g)))
    out["read_stream_gbps"] = g.value
    fs, pk, got = time_kernels(f, n, a.reps, rec, pos)
    assert got == cnt
    out["flag_scan_ms"], out["pack_lds_ms"] = spread(fs), spread(pk)
    must = 4.0 * nc + 2.0 * lay.stride * cnt                  # the Fmax column once + the record's words read and written
    out["bytes_must_touch"] = must
    out["stream_ms_for_those_bytes"] = must / (g.value * 1e9) * 1e3
    out["ratio_b_kernels_over_stream"] = (out["flag_scan_ms"]["median"] + out["pack_lds_ms"]["median"]) / out["stream_ms_for_those_bytes"]
    if not a.only_kernels:
        sub_wall, get_wall = [], []
        products = np.zeros(nc, dtype=dtype)
        lay_p = C.byref(lay)
        sub = _api()._subbox((0, 0, 0), (n, n, n))
        c2 = C.c_size_t()
        for rep in range(a.reps + 2):
            t0 = time.perf_counter()
            f._chk(f.L.pf_distribute(f.h, 1.0, C.byref(sub), None, lay_p, cnt, rec.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.POINTER(C.c_uint)), C.byref(c2)))
            t1 = time.perf_counter()
            f._chk(f.L.pf_get_products(f.h, products.ctypes.data_as(C.c_void_p), lay_p))
            t2 = time.perf_counter()
            if rep >= 2:
                sub_wall.append(1e3 * (t1 - t0))
                get_wall.append(1e3 * (t2 - t1))
        # the timed call did the work: its records are the selected rows of the products, in order
        keep = np.flatnonzero(products["Fmax"] >= 1.0)
        assert len(keep) == cnt and np.array_equal(pos, keep) and rec.view(dtype).reshape(cnt)[::997].tobytes() == products[keep[::997]].tobytes()
        out["distribute_wall_ms"], out["get_products_wall_ms"] = spread(sub_wall), spread(get_wall)
        out["ratio_a_distribute_over_get_products"] = out["distribute_wall_ms"]["median"] / out["get_products_wall_ms"]["median"]
        out["get_products_gbps"] = nc * lay.stride / (out["get_products_wall_ms"]["median"] * 1e-3) / 1e9
        out["distribute_gbps"] = cnt * (lay.stride + 4) / (out["distribute_wall_ms"]["median"] * 1e-3) / 1e9
        del products
    f.close()
    if not a.only_kernels:
        f = context(n, lds=False)
        fs, pk, got = time_kernels(f, n, a.reps, rec, pos)
        assert got == cnt
        out["pack_plain_ms"] = spread(pk)
        out["ratio_c_plain_over_lds"] = out["pack_plain_ms"]["median"] / out["pack_lds_ms"]["median"]
        f.close()
    print(json.dumps(out))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "r08_distribute.json"), "w") as fh:
            json.dump(out, fh, indent=1)
        with open(os.path.join(a.out, "r08_distribute.md"), "w") as fh:
            fh.write(report(out))


def report(o):
    def ms(k):
        s = o[k]
        return "%.2f ms (min %.2f, max %.2f, %d repetitions)" % (s["median"], s["min"], s["max"], s["n"])
    lines = ["# pf_distribute at %d^3, one rank, flast = 1, map = NULL, the whole box as the sub-box" % o["n"], "",
             "Written by profiles/tools/distribute_time.py (one process, two warm-up calls of each kind, alternating repetitions).", "",
             "- selected: %d of %d cells, fraction %.4f" % (o["selected"], o["n"] ** 3, o["selected_fraction"]),
             "- read stream rate of the context (pf_debug_stream_rate, kind 0): %.0f GB/s" % o["read_stream_gbps"], ""]
    if "distribute_wall_ms" in o:
        lines += ["## (a) wall time against pf_get_products", "",
                  "- pf_distribute: " + ms("distribute_wall_ms") + ", %.1f GB/s of records and frag_pos" % o["distribute_gbps"],
                  "- pf_get_products: " + ms("get_products_wall_ms") + ", %.1f GB/s" % o["get_products_gbps"],
                  "- ratio %.3f beside a selected fraction of %.3f" % (o["ratio_a_distribute_over_get_products"], o["selected_fraction"]), ""]
    lines += ["## (b) the kernels alone against the stream rate", "",
              "- flag + scan: " + ms("flag_scan_ms"), "- pack (LDS-staged): " + ms("pack_lds_ms"),
              "- bytes they must touch (Fmax once + the record read and written per selected cell): %.2f GB = %.2f ms at the stream rate"
              % (o["bytes_must_touch"] / 1e9, o["stream_ms_for_those_bytes"]),
              "- ratio (b): %.2f" % o["ratio_b_kernels_over_stream"], ""]
    if "pack_plain_ms" in o:
        lines += ["## (c) the LDS-staged pack against the plain one", "", "- plain (PF_DISTRIBUTE_LDS=0): " + ms("pack_plain_ms"),
                  "- plain / staged: %.2f" % o["ratio_c_plain_over_lds"], ""]
    return "\n".join(lines)


if __name__ == "__main__":
    main()
