"""The flavour census (include/pinfmax.h: pf_flavour_census) restated in numpy from its definitions, on whole columns and without
any of the device code's bit handling: the ulp is numpy's spacing of max(|exact|, 1) in the product precision, u is a division and
the bins are found by comparing u with powers of two."""
import numpy as np

BINS = 64
NOCELL = 2 ** 64 - 1
CELL_DTYPE = np.dtype([("cell", "<u8"), ("fast", "<f8"), ("exact", "<f8"), ("rmax_fast", "<i4"), ("rmax_exact", "<i4")])
COUNTS = ("cells", "differing_bits", "beyond_2ulp", "rmax_differing", "nonfinite", "outliers")


def census(fast, exact, rmax_fast, rmax_exact, first_cell=0, capacity=None):
    """-> (census dict, records of the first min(outliers, capacity) outliers; capacity None: all of them)"""
    fast, exact = np.ascontiguousarray(fast), np.ascontiguousarray(exact)
    T = fast.dtype
    assert T == exact.dtype and T in (np.float32, np.float64) and fast.ndim == 1 and fast.shape == exact.shape
    U = np.uint32 if T == np.float32 else np.uint64
    rmax_fast, rmax_exact = np.asarray(rmax_fast, dtype=np.int32), np.asarray(rmax_exact, dtype=np.int32)
    differ = fast.view(U) != exact.view(U)
    nonfinite = differ & ~(np.isfinite(fast) & np.isfinite(exact))
    live = ~nonfinite
    with np.errstate(all="ignore"):
        d = np.abs(fast.astype(np.float64) - exact.astype(np.float64))
        a = np.maximum(np.abs(exact), T.type(1))
        # (numpy's spacing is the step up, which at the largest finite value leads to infinity: there the step down is the binade's)
        ulp = np.where(a == np.finfo(T).max, a - np.nextafter(a, T.type(0)), np.spacing(a)).astype(np.float64)
        u = d / ulp
    d[~differ] = 0.0    # identical bits: bin 0 whatever the value
    u[~differ] = 0.0
    b = np.zeros(len(fast), dtype=np.int64)
    b[u > 0] = 1
    for k in range(2, BINS):    # bin k: 2^(k-2) < u; the last one that holds wins, and the last bin is open at the top
        b[u > 2.0 ** (k - 2)] = k
    out = {"cells": len(fast), "differing_bits": int(differ.sum()), "rmax_differing": int((rmax_fast != rmax_exact).sum()), "nonfinite": int(nonfinite.sum())}
    out["hist"] = np.bincount(b[live], minlength=BINS).astype(np.uint64)
    out["beyond_2ulp"] = int((live & (u > 2.0)).sum())
    is_out = nonfinite | (live & (u > 2.0))
    out["outliers"] = int(is_out.sum())
    if live.any():
        dl = np.where(live, d, -1.0)
        out["max_abs"], out["max_ulps"] = float(dl.max()), float(np.where(live, u, -1.0).max())
        out["max_abs_cell"] = int(first_cell) + int(np.argmax(dl))    # argmax: the first, so the lowest cell
    else:
        out["max_abs"], out["max_ulps"], out["max_abs_cell"] = 0.0, 0.0, NOCELL
    idx = np.flatnonzero(is_out)
    if capacity is not None:
        idx = idx[:capacity]
    rec = np.zeros(len(idx), dtype=CELL_DTYPE)
    rec["cell"] = idx.astype(np.uint64) + np.uint64(first_cell)
    rec["fast"], rec["exact"] = fast[idx].astype(np.float64), exact[idx].astype(np.float64)
    rec["rmax_fast"], rec["rmax_exact"] = rmax_fast[idx], rmax_exact[idx]
    return out, rec


def invariants(c):
    """what holds for every census"""
    assert int(c["hist"].sum()) + c["nonfinite"] == c["cells"]
    assert c["beyond_2ulp"] == int(c["hist"][3:].sum())
    assert c["outliers"] == c["beyond_2ulp"] + c["nonfinite"]


def same(a, b):
    """two censuses agree in every field, the maxima bit for bit (-> None, or what differs)"""
    for k in COUNTS + ("max_abs_cell",):
        if int(a[k]) != int(b[k]):
            return "%s: %d against %d" % (k, a[k], b[k])
    if not np.array_equal(np.asarray(a["hist"], dtype=np.uint64), np.asarray(b["hist"], dtype=np.uint64)):
        return "hist: %s against %s" % (a["hist"], b["hist"])
    for k in ("max_abs", "max_ulps"):
        if np.float64(a[k]).tobytes() != np.float64(b[k]).tobytes():
            return "%s: %r against %r" % (k, a[k], b[k])
    return None


def same_records(a, b):
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()
