"""Which sums every launch of a shell pass carries -- TEST INFRASTRUCTURE: a Python restatement of the grouping rules in the comments of
pinocchio_amd/csrc/pf_power.hip, from the shell count nb, the 64 KB of LDS a workgroup may ask for, and the bytes per shell and sum
(a scan: one table of 8 bytes, and two tables more for the counts; an accumulation: three 64-bit limb counters and one exponent, 28).

  correlation  six sums, 2k and 2k + 1 the two signs of order k.  As many per launch as there is room for, an even number where
               there is room for two, spread evenly over the launches and made even again: no launch splits a pair
  multipoles   eleven sums (five without a second spectrum); sum 0 stands alone and 2k - 1, 2k are the two signs of term k, so the
               launches cut the indices -1 .. total - 1 into runs of one length: an even length splits no pair, and the run [-1, 0)
               of length one is empty and is not launched
  matter       three sums; one fused scan where five tables of 8 nb bytes fit, else a scan per sum; an accumulation per sum
  power        CG column groups of 256 threads cover the n/2 columns of a row: 1, 2 or 4
  rows         a tap's rows go to at most `maxwg` workgroups of equally many rows; the last one is ragged where they do not divide
A launch is the list of the sums it carries; `lds` is what it asks for, sized by the longest launch of its pass."""
LDS = 65536
TABLE, ACC = 8, 28
CORR_SUMS, MULTIPOLE_SUMS, MULTIPOLE_SUMS_AUTO = 6, 11, 5
BLOCK, MAXWG_SHELLS, MAXWG_RADII, POWER_NR = 256, 8192, 2048, 12


def scan_room(nb, each=False, lds=LDS):
    return 1 if each or lds // (TABLE * nb) < 3 else lds // (TABLE * nb) - 2


def acc_room(nb, each=False, lds=LDS):
    return 1 if each else lds // (ACC * nb)


def corr_per(room):
    g = max(1, min(room, CORR_SUMS))
    if g > 1:
        g -= g % 2
    launches = -(-CORR_SUMS // g)
    per = -(-CORR_SUMS // launches)
    if per > 1 and per % 2:
        per += 1
    return per


def multipole_per(total, room):
    slots = total + 1
    g = max(1, min(room, slots))
    launches = -(-slots // g)
    return -(-slots // launches)


def runs(start, total, per):
    """the indices start .. total - 1 in runs of per; what lies below 0 is nobody's, and a run without a sum is not launched"""
    out = []
    for v0 in range(start, total, per):
        sums = [s for s in range(v0, min(v0 + per, total)) if s >= 0]
        if sums:
            out.append(sums)
    return out


def corr(nb, each=False, lds=LDS):
    ps, pa = corr_per(scan_room(nb, each, lds)), corr_per(acc_room(nb, each, lds))
    return {"scans": runs(0, CORR_SUMS, ps), "accs": runs(0, CORR_SUMS, pa), "lds_scan": (ps + 2) * TABLE * nb, "lds_acc": pa * ACC * nb}


def multipoles(nb, total=MULTIPOLE_SUMS, each=False, lds=LDS):
    ps, pa = multipole_per(total, scan_room(nb, each, lds)), multipole_per(total, acc_room(nb, each, lds))
    return {"scans": runs(-1, total, ps), "accs": runs(-1, total, pa), "lds_scan": (min(ps, total) + 2) * TABLE * nb, "lds_acc": min(pa, total) * ACC * nb}


def matter(nb, two=True, each=False, lds=LDS):
    fused = two and 5 * TABLE * nb <= lds and not each
    sums = [0, 1, 2] if two else [0]
    return {"fused": fused, "scans": [sums] if fused else [[s] for s in sums], "accs": [[s] for s in sums], "lds_scan": 5 * TABLE * nb if fused else ACC * nb,
            "lds_acc": ACC * nb}                    # (a scan of one sum is launched with the accumulation's size)


def power(n, nb, radii=0):
    half = n // 2
    cg = 1 if half <= BLOCK else 2 if half <= 2 * BLOCK else 4
    assert cg * BLOCK >= half
    return {"cg": cg, "batches": max(1, -(-radii // POWER_NR)), "lds_scan": (3 * nb + POWER_NR + 1) * 8, "lds_acc": (3 * nb + 3 * POWER_NR) * 8 + 4 * nb}


def rows(rows_, maxwg=MAXWG_SHELLS):
    """(rows per workgroup, workgroups, rows of the last workgroup)"""
    rpw = -(-rows_ // maxwg)
    nwg = -(-rows_ // rpw)
    return rpw, nwg, rows_ - (nwg - 1) * rpw


def form(p):
    """(scans, accumulations) as pf_debug_multipole_form and pf_debug_corr_passes report them"""
    return len(p["scans"]), len(p["accs"])


def lengths(launches):
    return tuple(len(x) for x in launches)
