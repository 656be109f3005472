"""Writes tests/golden/peaks_kat.json: the peak totals the reference logged in count_peaks (src/fragment.c:605-706) in the five
committed runs the project reproduces end to end -- run name, the KAT fixture that holds the run's set-up, the log line
"Task 0 found N peaks, G in the well resolved region. Total number of peaks: T" (the first one of a run with more
than one fragmentation pass) and its three numbers.  Data only.  Needs /root/reference.

    python tests/golden/make_peaks_kat.py
"""
import json
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
RUNS = [  # name, log, fixture with the set-up of the run
    ("HMF_Validation", "HMF_Validation/log_RUN.txt", "hmf_validation_kat.json"),
    ("example", "example/log", "example_kat.json"),
    ("RECOMPUTE_DISPLACEMENTS_LCDM", "tests/only_HMF_tests/RECOMPUTE_DISPLACEMENTS_LCDM/log_RECOMPUTE", "hmf256_kat.json"),
    ("SCALE_DEP_LCDM", "tests/only_HMF_tests/SCALE_DEP_LCDM/log_SCALE_DEP", "hmf256_kat.json"),
    ("READ_PK_TABLE_and_SCALE_DEP", "tests/only_HMF_tests/READ_PK_TABLE_and_SCALE_DEP/log_READ_PK_and_SCALE_DEP", "readpk256_kat.json"),
    ("MOD_GRAV_and_SCALE_DEP", "tests/only_HMF_tests/MOD_GRAV_and_SCALE_DEP/log_MOD_GRAV_and_SCALE_DEP", "mg256_kat.json"),
]
LINE = re.compile(r"Task 0 found (\d+) peaks, (\d+) in the well resolved region\. Total number of peaks: (\d+)")


def main():
    runs = []
    for name, log, fixture in RUNS:
        hit, tasks = None, 1    # ("running on 4 MPI tasks"; the serial runs print nothing of the kind)
        for l in open(os.path.join(REF, log), errors="replace"):
            m = re.search(r"running on (\d+) MPI tasks", l)
            if m:
                tasks = int(m.group(1))
            m = LINE.search(l)
            if m:
                hit = (l[l.index("Task 0"):].strip(), m)
                break
        assert hit, log
        line, m = hit
        runs.append({"run": name, "log": log, "setup": fixture, "tasks": tasks, "log_line": line, "task0_peaks": int(m.group(1)),
                     "task0_well_resolved": int(m.group(2)), "total_peaks": int(m.group(3))})
        print(name, line)
    kat = {"_provenance": "Peak totals logged by the reference's committed runs (count_peaks).  Data only.", "Flast": 1.0, "runs": runs}
    json.dump(kat, open(os.path.join(HERE, "peaks_kat.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
