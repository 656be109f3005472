"""Planted columns for the flavour census, shared by the CPU and the GPU tests.  A case is (name, fast, exact, rmax_fast, rmax_exact,
first_cell); the Fmax columns are float32 or float64 and every planted distance is built with the product type's own spacing, so
that "exactly k ulp" is exact."""
import numpy as np

DTYPES = (np.float32, np.float64)


def _ulp1(T):
    return np.spacing(T(1))


def planted(T):
    """one column holding every special cell the census defines -> fast, exact, rmax_fast, rmax_exact"""
    T = np.dtype(T).type
    one = _ulp1(T)
    nan, inf = T(np.nan), T(np.inf)
    nan2 = np.array([0x7FC00001 if T is np.float32 else 0x7FF8000000000001], dtype=np.uint32 if T is np.float32 else np.uint64).view(T)[0]
    big = T(2.0) ** (50 if T is np.float64 else 20)    # 2^50 ulp(1) above 1 is 1.25 in double; float keeps 24 bits
    cells = [   # (fast, exact, rmax_fast, rmax_exact)
        (T(1.5), T(1.5), 3, 3),                                         # equal
        (T(0.0), -T(0.0), 0, 0),                                        # +0 against -0: different bits, bin 0
        (-T(0.0), T(0.0), 0, 0),
        (T(1.5) + np.spacing(T(1.5)), T(1.5), 1, 1),                    # exactly 1 ulp
        (T(1.5) + 2 * np.spacing(T(1.5)), T(1.5), 1, 1),                # exactly 2 ulp: not beyond
        (T(1.5) + 3 * np.spacing(T(1.5)), T(1.5), 1, 1),                # 3 ulp
        (T(1.5) - 4 * np.spacing(T(1.5)), T(1.5), 1, 1),                # exactly 4 ulp: still bin 3
        (T(1.5) + 5 * np.spacing(T(1.5)), T(1.5), 1, 1),                # 5 ulp: bin 4
        (T(0.25) + 2 * one, T(0.25), 2, 2),                             # |exact| < 1: the ulp of 1.0 applies, 2 ulp
        (T(0.25) + 3 * one, T(0.25), 2, 2),                             # ... 3 ulp
        (T(0.25) + np.spacing(T(0.25)), T(0.25), 2, 2),                 # ... a quarter of an ulp: bin 1
        (T(1e-30), T(0.0), 2, 2),                                       # ... far below one
        (T(2.0), T(2.0) - np.spacing(T(1.0)), 2, 2),                    # fast one binade above exact: one ulp of exact
        (T(-3.0) - 5 * np.spacing(T(3.0)), T(-3.0), 4, 4),              # negative values
        (T(-3.0), T(-3.0) - 2 * np.spacing(T(3.0)), 4, 4),
        (T(-1.0), T(1.0), 4, 4),                                        # opposite signs
        (T(1.0) + big * one, T(1.0), 5, 5),                             # a power of two of ulps
        (T(1.0) + (big * one) * T(1.5), T(1.0), 5, 5),                  # ... and between two
        (T(1.0), T(1.0) + T(2.0) ** 12, 5, 5),
        (np.finfo(T).max, T(1.0), 5, 5),                                # the open last bin (with double products: 2^1076 ulp)
        (np.finfo(T).max, -np.finfo(T).max, 5, 5),                      # d overflows a double with double products
        (nan, T(1.0), 6, 6), (T(1.0), nan, 6, 6), (nan, nan, 6, 6), (nan, nan2, 6, 6),    # NaN on either side, the same NaN, two NaNs
        (inf, T(1.0), 6, 6), (T(1.0), -inf, 6, 6), (inf, inf, 6, 6), (inf, -inf, 6, 6), (nan, inf, 6, 7),
        (T(7.0), T(7.0), 8, 9),                                         # equal Fmax, different Rmax
        (T(7.0) + 3 * np.spacing(T(7.0)), T(7.0), 8, 9),
    ]
    with np.errstate(all="ignore"):
        a = [np.array([c[k] for c in cells], dtype=T if k < 2 else np.int32) for k in range(4)]
    return a


def embedded(T, count, where, seed=5):
    """`count` equal cells with the planted column's cells at the positions `where` (one planted cell each, cyclically)"""
    pf, pe, prf, pre = planted(T)
    rng = np.random.default_rng(seed)
    exact = (rng.random(count) * 8.0 - 1.0).astype(T)
    fast = exact.copy()
    rf = rng.integers(-1, 12, count).astype(np.int32)
    re = rf.copy()
    for k, i in enumerate(where):
        j = k % len(pf)
        fast[i], exact[i], rf[i], re[i] = pf[j], pe[j], prf[j], pre[j]
    return fast, exact, rf, re


def random_columns(T, count=100000, frac=0.01, seed=11):
    """random columns, `frac` of the cells planted: small distances of 0 .. 9 ulp, large ones over many binades, Rmax changes and a
    few NaNs and infinities"""
    T = np.dtype(T).type
    rng = np.random.default_rng(seed)
    exact = (rng.standard_normal(count) * 3.0).astype(T)
    fast = exact.copy()
    rf = rng.integers(-1, 12, count).astype(np.int32)
    re = rf.copy()
    # the background: most cells equal, some one ulp apart
    near = rng.random(count) < 0.05
    fast[near] = np.nextafter(exact[near], T(np.inf))
    pick = rng.choice(count, int(count * frac), replace=False)
    kind = rng.integers(0, 5, len(pick))
    for i, k in zip(pick, kind):
        sp = np.spacing(max(abs(exact[i]), T(1)))
        if k == 0:
            fast[i] = exact[i] + T(rng.integers(-9, 10)) * sp
        elif k == 1:
            fast[i] = exact[i] + T(2.0) ** int(rng.integers(0, 60 if T is np.float64 else 40)) * sp * T(rng.choice([1.0, 1.25, -1.0]))
        elif k == 2:
            re[i] = rf[i] + 1
            fast[i] = exact[i] + T(3) * sp
        elif k == 3:
            fast[i] = T(rng.choice([np.nan, np.inf, -np.inf]))
        else:
            exact[i] = T(rng.choice([np.nan, np.inf]))
    return fast, exact, rf, re


def cases(T):
    """every planted case of one precision"""
    T = np.dtype(T).type
    out = [("planted",) + tuple(planted(T)) + (0,)]
    n = 300
    f, e, rf, re = embedded(T, n, [])
    f[0], f[n - 1] = e[0] + 3 * np.spacing(max(abs(e[0]), T(1))), T(np.nan)
    out.append(("outliers_first_and_last", f, e, rf, re, 0))
    f, e, rf, re = embedded(T, 11, [])
    f[2], f[4], f[5], f[10] = e[2] + 7 * np.spacing(max(abs(e[2]), T(1))), T(np.inf), e[5] - 3 * np.spacing(max(abs(e[5]), T(1))), e[10] + T(1)
    out.append(("across_2_32", f, e, rf, re, 2 ** 32 - 5))
    out.append(("all_equal",) + embedded(T, 77, []) + (9,))
    f, e, rf, re = embedded(T, 5, [])
    f[:] = T(np.nan)
    e[:] = T(np.inf)
    out.append(("all_nonfinite", f, e, rf, re, 3))
    out.append(("every_planted_cell_spread",) + embedded(T, 5000, range(7, 5000, 13)) + (0,))
    out.append(("random",) + random_columns(T) + (0,))
    return out


def for_count(T, count):
    """a column of `count` cells with planted cells every 5th position, beginning at the first and including the last"""
    where = sorted(set(range(0, count, 5)) | {count - 1})
    return embedded(T, count, where, seed=count % 1000)
