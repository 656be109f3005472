"""Writes tests/golden/distribute_kat.json: what the reference logged about distribute() (src/distribute.c:58-175, reported by
src/fragment.c:285-301) in the committed runs the project reproduces end to end -- the FIRST "... re-distribution of Fmax done,
N particles stored by all tasks" line of each run (an all-periodic single-task run skips the first turn, src/fragment.c:207-209, so
its first line says "Second"), the "Smallest and largest overhead" line that follows it, and the sub-box geometry lines of the
run's header.  Data only.  Needs a checkout of the reference.

    python tests/golden/make_distribute_kat.py <reference tree>
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
RUNS = [  # name, log, fixture with the set-up of the run
    ("HMF_Validation", "HMF_Validation/log_RUN.txt", "hmf_validation_kat.json"),
    ("example", "example/log", "example_kat.json"),
    ("RECOMPUTE_DISPLACEMENTS_LCDM", "tests/only_HMF_tests/RECOMPUTE_DISPLACEMENTS_LCDM/log_RECOMPUTE", "hmf256_kat.json"),
    ("SCALE_DEP_LCDM", "tests/only_HMF_tests/SCALE_DEP_LCDM/log_SCALE_DEP", "hmf256_kat.json"),
    ("READ_PK_TABLE_and_SCALE_DEP", "tests/only_HMF_tests/READ_PK_TABLE_and_SCALE_DEP/log_READ_PK_and_SCALE_DEP", "readpk256_kat.json"),
    ("MOD_GRAV_and_SCALE_DEP", "tests/only_HMF_tests/MOD_GRAV_and_SCALE_DEP/log_MOD_GRAV_and_SCALE_DEP", "mg256_kat.json"),
]
STORED = re.compile(r"(First|Second) re-distribution of Fmax done, (\d+) particles stored by all tasks, average overhead: ([0-9.]+)")
OVER = re.compile(r"Smallest and largest overhead: ([0-9.]+), ([0-9.]+)")
GEOMETRY = [("particles_per_task", r"Reference number of particles:\s+(\d+)"),
            ("nbox", r"Number of sub-boxes per dimension:\s+(\d+) (\d+) (\d+)"),
            ("pbc", r"Periodic boundary conditions:\s+(\d+) (\d+) (\d+)"),
            ("Lgwbl", r"Core 0 will work on a grid:\s+(\d+) (\d+) (\d+)"),
            ("Lgrid", r"The resolved box will be:\s+(\d+) (\d+) (\d+)"),
            ("safe", r"Boundary layer:\s+(\d+) (\d+) (\d+)")]


def main():
    REF = sys.argv[1]
    runs = []
    for name, log, fixture in RUNS:
        run = {"run": name, "log": log, "setup": fixture, "tasks": 1, "log_lines": []}
        lines = open(os.path.join(REF, log), errors="replace").read().splitlines()
        for i, l in enumerate(lines):
            m = re.search(r"running on (\d+) MPI tasks", l)
            if m:
                run["tasks"] = int(m.group(1))
            for key, pat in GEOMETRY:
                m = re.match(pat, l)
                if m and key not in run:
                    v = [int(g) for g in m.groups()]
                    run[key] = v[0] if len(v) == 1 else v
                    run["log_lines"].append(l.strip())
            m = STORED.search(l)
            if m and "stored" not in run:
                o = OVER.search(lines[i + 1])
                assert o, (log, lines[i + 1])
                run["turn"] = m.group(1)
                run["stored"] = int(m.group(2))
                run["average_overhead"] = float(m.group(3))
                run["smallest_overhead"], run["largest_overhead"] = float(o.group(1)), float(o.group(2))
                run["log_lines"] += [l[l.index(m.group(1)):].strip(), lines[i + 1][lines[i + 1].index("Smallest"):].strip()]
        assert "stored" in run and all(k in run for k, _ in GEOMETRY), log
        runs.append(run)
        print(name, run["turn"], run["stored"], run["smallest_overhead"], run["largest_overhead"], run["nbox"], run["safe"])
    kat = {"_provenance": "Totals logged by the reference's committed runs after distribute() (src/fragment.c:285-301) and the sub-box "
                          "geometry of their headers.  Data only.", "Flast": 1.0, "runs": runs}
    json.dump(kat, open(os.path.join(HERE, "distribute_kat.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
