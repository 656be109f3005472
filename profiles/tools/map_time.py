"""Times the resident fragmentation maps (profiles/map_notes.md): pf_map_update, pf_distribute_sorted_map against
pf_distribute_sorted with the same words from the host, and k_peaks with a map against without.

One rank, an n^3 context with fp64 fields, fp32 products and the bench's synthetic density, one sweep with the bench radii
(synth.radii_ladder(12)) and the displacements; the sub-box is the whole periodic box (subbox.Lgwbl = n in every direction).

 (a) k_map_spheres.  A halo population with masses 10 .. 10^6 from dn/dM ~ M^-2 (uniform in 1/M), `--groups` of them (2 10^5) at
     uniform positions, BoundaryLayerFactor 3, on an EMPTY current map -- every cell of every sphere is requested, the most atomics
     a population can give.  Device time of the kernel from HIP events (the "distribute" kernel class of pf_kernel_stats around
     pf_map_update, which holds that one kernel), cube cells visited per second, atomics issued (pf_debug_map_atomics of a map
     created under PF_MAP_STATS=1, a run of its own: the timed kernels carry no counter), and the same
     with PF_MAP_WORDS=0 in a second map; both maps must hold the same words and counts.
 (b) pf_distribute_sorted_map against pf_distribute_sorted given the same words (every bit set: create_map on a periodic box),
     flast = 1, the 104-byte record: wall time of the full call and of a count-only call (capacity 0: selection alone, where the
     upload of maplength words is the larger share).
 (c) k_peaks with the map (every bit set: the same counts) against the region form: device time of the "peaks" kernel class.

Warm-up: two calls of each kind before anything is timed; `--reps` timed repetitions (five at least), alternating between the two
sides of a comparison; min, median and max reported -- max - min of a side is the run-to-run spread a difference is read against.

    python profiles/tools/map_time.py [--n 512] [--groups 200000] [--reps 5] [--out FILE.json]     one JSON line on stdout
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


def kernel_ms(f, name):
    return sum(k["total_ms"] for k in f.kernel_stats() if k["name"] == name)


def population(n, count, seed=1):
    rng = np.random.default_rng(seed)
    mass = (1.0 / rng.uniform(1e-6, 1e-1, count)).astype(np.int32)          # dn/dM ~ M^-2 on [10, 10^6]
    pos = rng.uniform(0.0, n - 0.6, (count, 3))
    return pos, mass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--groups", type=int, default=200000)
    ap.add_argument("--blf", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-distribute", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from pinocchio_amd import _lib, api, synth
    n = a.n
    out = {"n": n, "groups": a.groups, "blf": a.blf, "reps": a.reps}
    f = api.Fmax(n, field_bytes=8, timing=True)
    f.synth_density(synth.SEED, 2.5, -2.0)
    f.set_invgrow(*synth.invgrow_table("lcdm"))
    f.set_growth(synth.growth_multipliers())
    f.compute_fmax(synth.radii_ladder(12), do_lpt=True)
    box = ((0, 0, 0), (n, n, n), (0, 0, 0))

    # (a) the spheres
    pos, mass = population(n, a.groups)
    size = (a.blf * np.power(mass / 4.188790205, 0.333333333333333) + 0.5).astype(np.int64)
    out["size_min"], out["size_max"], out["size_median"] = int(size.min()), int(size.max()), float(np.median(size))
    out["cube_cells"] = int((8 * size ** 3).sum())
    out["rows"] = int((4 * size ** 2).sum())
    res = {}
    for form in ("1", "0"):
        os.environ["PF_MAP_WORDS"] = form
        with f.frag_map(*box) as m:
            ms = []
            for rep in range(a.reps + 2):
                f.reset_kernel_stats()
                nadd = m.update(pos, mass, a.blf)
                if rep >= 2:
                    ms.append(kernel_ms(f, "distribute"))
            res[form] = dict(ms=spread(ms), nadd=list(nadd), bits=m.count("update"), words=m.words("update"))
        os.environ["PF_MAP_STATS"] = "1"          # the counting instantiation, in a run of its own that is not timed
        with f.frag_map(*box) as m:
            assert list(m.update(pos, mass, a.blf)) == res[form]["nadd"]
            res[form]["atomics"] = m.atomics()
        os.environ.pop("PF_MAP_STATS")
    os.environ.pop("PF_MAP_WORDS")
    assert res["1"]["nadd"] == res["0"]["nadd"] and np.array_equal(res["1"]["words"], res["0"]["words"])
    assert res["0"]["atomics"] == res["0"]["nadd"][0]
    for form, key in (("1", "words_form"), ("0", "bit_form")):
        r = res[form]
        out[key] = {"kernel_ms": r["ms"], "atomics": r["atomics"], "cube_cells_per_s": out["cube_cells"] / (r["ms"]["median"] * 1e-3)}
    out["nadd"], out["update_bits"] = res["1"]["nadd"], res["1"]["bits"]
    out["ratio_bit_over_words"] = res["0"]["ms"]["median"] / res["1"]["ms"]["median"]
    del res

    # (c) k_peaks with a map against the region form
    with f.frag_map(*box) as m:
        m.fill_box()
        m.commit(False)
        assert m.count("current") == n ** 3
        plain, mapped = [], []
        for rep in range(a.reps + 2):
            f.reset_kernel_stats()
            p0 = f.count_peaks(1.0, box)
            t0 = kernel_ms(f, "peaks")
            f.reset_kernel_stats()
            p1 = f.count_peaks(1.0, map=m)
            t1 = kernel_ms(f, "peaks")
            assert p0 == p1
            if rep >= 2:
                plain.append(t0); mapped.append(t1)
        out["peaks"] = list(p0)
        out["peaks_region_ms"], out["peaks_map_ms"] = spread(plain), spread(mapped)
        out["peaks_ratio_map_over_region"] = out["peaks_map_ms"]["median"] / out["peaks_region_ms"]["median"]

        # (b) resident against uploaded words
        if not a.skip_distribute:
            words = m.words("current")
            out["map_bytes"] = int(words.nbytes)
            lay = _lib.ProductLayout(STRIDE, 0, 4, 8, 20, 32, 44)
            sub = api._subbox(box[0], box[1])
            cnt = C.c_size_t()
            up, ip = C.POINTER(C.c_uint), C.POINTER(C.c_int)
            wp = words.ctypes.data_as(up)
            f._chk(f.L.pf_distribute_sorted_map(f.h, 1.0, m.h, 0, C.byref(lay), 0, None, None, None, None, C.byref(cnt)))
            total = cnt.value
            out["selected"] = total
            rec = np.zeros((total, STRIDE), dtype=np.uint8)
            fpos, spos, ind = np.zeros(total, dtype=np.uint32), np.zeros(total, dtype=np.uint32), np.zeros(total, dtype=np.int32)
            args = (rec.ctypes.data_as(C.c_void_p), fpos.ctypes.data_as(up), spos.ctypes.data_as(up), ind.ctypes.data_as(ip))
            none = (None, None, None, None)

            def host(cap, o):
                f._chk(f.L.pf_distribute_sorted(f.h, 1.0, C.byref(sub), wp, C.byref(lay), cap, *o, C.byref(cnt)))

            def resident(cap, o):
                f._chk(f.L.pf_distribute_sorted_map(f.h, 1.0, m.h, 0, C.byref(lay), cap, *o, C.byref(cnt)))

            t = {"host_full": [], "resident_full": [], "host_count": [], "resident_count": []}
            for rep in range(a.reps + 2):
                calls = [("host_full", host, total, args), ("resident_full", resident, total, args),
                         ("host_count", host, 0, none), ("resident_count", resident, 0, none)]
                if rep % 2:                      # neither side of a comparison always runs second
                    calls = [calls[1], calls[0], calls[3], calls[2]]
                for name, fn, cap, o in calls:
                    t0 = time.perf_counter()
                    fn(cap, o)
                    dt = 1e3 * (time.perf_counter() - t0)
                    assert cnt.value == total
                    if rep >= 2:
                        t[name].append(dt)
                    if name == "host_full" and rep == 0:
                        keep = (rec.copy(), fpos.copy(), spos.copy(), ind.copy())
                    if name == "resident_full" and rep == 0:
                        assert all(np.array_equal(x, y) for x, y in zip(keep, (rec, fpos, spos, ind)))
                        del keep
            for k, v in t.items():
                out[k + "_wall_ms"] = spread(v)
            out["gain_full_ms"] = out["host_full_wall_ms"]["median"] - out["resident_full_wall_ms"]["median"]
            out["gain_count_ms"] = out["host_count_wall_ms"]["median"] - out["resident_count_wall_ms"]["median"]
    f.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
