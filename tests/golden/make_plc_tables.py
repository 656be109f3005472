"""Makes tests/golden/plc_tables.json from what the reference's example run wrote (run by hand, never by a test):

    python tests/golden/make_plc_tables.py <reference>/example

From pinocchio.example.cosmology.out the rows with scale factor a >= 0.2: columns 1 (a), 3 (comoving distance, Mpc), 7-10 (the
growth rates of orders 1, 2, 31, 32) and 11-14 (their d ln D / d ln a).  From the log the cosmological parameters the Hubble table
of the tests is made of (lines 13-17), grid and inter-particle distance (26-31), and the cone with its 13 replications (70-92)."""
import json
import os
import re
import sys


def main(example):
    rows = []
    for line in open(os.path.join(example, "pinocchio.example.cosmology.out")):
        if line.startswith("#") or not line.strip():
            continue
        f = line.split()
        if float(f[0]) >= 0.2:
            rows.append([float(f[k - 1]) for k in (1, 3, 7, 8, 9, 10, 11, 12, 13, 14)])
    log = open(os.path.join(example, "log")).read().splitlines()

    def value(key):
        for line in log:
            if line.startswith(key):
                return [float(t) for t in line[len(key):].split()]
        raise KeyError(key)
    reps = []
    for line in log[69:92]:
        m = re.match(r"\s*Replication\s+\d+: shift \(\s*(-?\d+),\s*(-?\d+),\s*(-?\d+)\), from F=([\d.]+) to F=([\d.]+)", line)
        if m:
            reps.append([int(m.group(1)), int(m.group(2)), int(m.group(3)), float(m.group(4)), float(m.group(5))])
    centre = [float(t) for t in re.search(r"centred on point \[([^\]]*)\]", "\n".join(log)).group(1).split(",")]
    axis = [float(t) for t in re.search(r"pointed toward \[([^\]]*)\]", "\n".join(log)).group(1).split(",")]
    out = {
        "source": "example/pinocchio.example.cosmology.out (a >= 0.2, columns 1, 3, 7-14) and example/log:13-31, 70-92",
        "columns": ["a", "comvdist", "grow1", "grow2", "grow31", "grow32", "fomega1", "fomega2", "fomega31", "fomega32"],
        "rows": rows,
        "Omega0": value("Omega0")[0], "OmegaLambda": value("OmegaLambda")[0], "Hubble100": value("Hubble100")[0],
        "GridSize": [int(t) for t in value("GridSize")], "InterPartDist": value("Inter-part dist (true Mpc)")[0],
        "center": centre, "axis": axis, "PLCAperture": float(re.search(r"aperture of ([\d.]+) degrees", "\n".join(log)).group(1)),
        "Fstart": 1.3, "Fstop": 1.0, "nzbins": 6,
        "replications": reps,
    }
    assert len(reps) == 13 and len(rows) > 8
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plc_tables.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=0)
        fh.write("\n")
    print(path, len(rows), "rows", len(reps), "replications")


if __name__ == "__main__":
    main(sys.argv[1])
