"""The bands at which the band-limited (pruned) 1-D passes are held against pocketfft (tests/test_gpu_lines.py), and the
library's rules that decide a band and the row pitch that goes with it, restated in plain Python.

A band b keeps the signed wavenumbers |s| <= b of the transformed axis (x and y) and the columns kz <= b (z); b >= n / 2
switches pruning off.  Every kernel family cuts the band in its own unit -- its granule g -- and a comparison that is off by
one element or by one block shows at b = k g - 2 .. k g + 1 and nowhere else:

  granule                                     kernel                                       where
  8 (fp64) / 16 (fp32): complex numbers per   band_zpitch rounds band + 1 up to it: the    csrc/pf_api.hip:653-658
    128-byte line                             compact row pitch of a pruned x-pass
  NT = n / 16, the threads of a z-pass line:  k_c2r (one-shot)                             csrc/pf_fft_kernels.hip:259, :276
    register m of a thread holds kz =         k_c2r_persistent                             csrc/pf_fft_kernels.hip:323, :346
    tl + m NT, so a band that ends on a       k_c2r_invariants / _spec                     csrc/pf_fft_kernels.hip:485, :524-526
    multiple of NT empties whole registers    k_c2r_invariants_pk2 (fp32, two rows)        csrc/pf_fft_kernels.hip:755, :838-842
  NT = (n / 2) / R0 (R0 = 8, or 4 where n / 2 k_mixed_c2r                                  csrc/pf_mixed_kernels.hip:372-374
    is no multiple of 8), the same for the    k_mixed_c2r_invariants                       csrc/pf_mixed_kernels.hip:497-499
    mixed-radix z-passes                      k_mixed_c2r_invariants_spec                  csrc/pf_mixed_kernels.hip:642-644
  64: a wavefront -- the unit in which the    every kernel above, and the 64-lane pieces   csrc/pf_fft_kernels.hip:604-618
    per-element comparisons above turn into   of the rows that go straight into LDS
    whole waves that load nothing
  128: the row blocks of the packed fp32      k_strided16 (2048 points)                    csrc/pf_fft16_kernels.hip:118, :124-127
    strided passes -- a block is read when    k_strided_pk8 (1024 points)                  csrc/pf_fft16_kernels.hip:299, :305-308
    one of its rows is in band (a uniform
    test), its other rows are then cleared
  (k_strided and k_mixed_strided mask per register and element: csrc/pf_fft_kernels.hip:133-137, csrc/pf_mixed_kernels.hip:254-257)
"""
import math

PRUNE_EPS = 2.0 ** -60         # PfTuning::prune_eps, csrc/pf_api.hip:366
PRODUCTION_1024 = (93, 132, 186, 261, 372)   # hess_band of synth.radii_ladder(12) at n = 1024 (the benchmark step)
PRODUCTION_2048 = (496,)                     # ... of R = 6 cells at n = 2048 (BASELINE config 5)
CAP = 40
OVER_CAP = {(768, 8): 42, (768, 4): 42, (1000, 8): 41, (1000, 4): 41, (1024, 4): 43}   # (see band_ladder)
# the line lengths of the ladder tests: between them every kernel family of the three launchers (tests/test_gpu_lines.py)
LADDER_SIZES = [16, 64, 256, 128, 1024, 2048, 512, 24, 40, 96, 200, 768, 1000]


def hess_band(n, rs, eps=PRUNE_EPS):
    """csrc/pf_api.hip:1060-1068: the Gaussian window exp(-k^2 rs^2 / 2) falls below eps beyond |k| = sqrt(-2 ln eps) / rs"""
    band = 1 << 30
    if rs > 0.0 and eps > 0.0:
        kc = math.sqrt(-2.0 * math.log(eps)) / rs
        kb = kc * n / (2.0 * 3.14159265358979323846)
        if kb < n // 2 - 1:
            band = int(kb) + 1
    return band


def line_granule(fb):
    """complex numbers per 128-byte line"""
    return 64 // fb


def band_zpitch(n, fb, band, nzp):
    """csrc/pf_api.hip:653-658: the row pitch (complex columns) of the fields a pruned x-pass writes and its y-pass reads"""
    if band >= n // 2:
        return nzp
    m = line_granule(fb)
    zp = (band + 1 + m - 1) & ~(m - 1)
    return min(zp, nzp)


def radius_of_band(n, band):
    """a smoothing radius (cells) whose hess_band is `band`: the middle of the interval of radii that give it"""
    assert 1 <= band < n // 2
    c = math.sqrt(-2.0 * math.log(PRUNE_EPS)) * n / (2.0 * 3.14159265358979323846)   # kb = c / rs
    rs = c / (band - 0.5)                                                            # int(kb) = band - 1
    assert hess_band(n, rs) == band, (n, band, rs)
    return rs


def zpass_threads(n):
    """threads of one z-pass line = the stride between the kz columns that one thread's registers hold"""
    m = n // 2
    if n & (n - 1) == 0:
        return max(m // 8, 1)               # k_c2r: NT = M / 8
    return m // (8 if m % 8 == 0 else 4)    # pf_radices(n / 2, allow4 = true): R0, csrc/pf_mixed_kernels.hip:704


def granules(n, fb):
    g = {line_granule(fb), zpass_threads(n), 64}
    if fb == 4 and n in (1024, 2048):
        g.add(128)                          # pf_launch_strided16, csrc/pf_fft16_kernels.hip:415-416
    return sorted(g)


def edge_multiples(n, g):
    """the first two multiples of g and the last one below n / 2"""
    below = [k * g for k in range(1, n) if k * g < n // 2]
    return sorted(set(below[:2] + below[-1:]))


def required(n, fb):
    """name of the class -> the bands it asks for (inside 1 .. n / 2)"""
    half = n // 2
    cls = {"low": [1, 2, 3], "top": [half - 2, half - 1], "off": [half]}
    for g in granules(n, fb):
        for kg in edge_multiples(n, g):
            cls["g%d@%d" % (g, kg)] = [kg - 2, kg - 1, kg, kg + 1]
    if n == 1024:
        cls["production"] = list(PRODUCTION_1024)
    if n == 2048:
        cls["production"] = list(PRODUCTION_2048)
    return {k: [b for b in v if 1 <= b <= half] for k, v in cls.items()}


def band_ladder(n, fb):
    """sorted bands for lines of n points in fields of fb bytes per scalar: exactly the required classes and nothing else.
    That is at most CAP values for every size of the line tests but three, whose granules share no edge multiple -- 768
    (42 values), 1000 (41) and 1024 with fp32 fields (43: three granules and the five production bands): OVER_CAP names
    them, and none of their required values is dropped to make the number"""
    return sorted({b for v in required(n, fb).values() for b in v})
