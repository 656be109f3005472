"""The C example examples/peaks_validation.c: a plain C host over the C ABI prints the reference's peak log line."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_peaks_example_compiles_against_the_header():
    """gcc only needs include/pinfmax.h and the shared object"""
    if not os.path.exists(os.path.join(ROOT, "pinocchio_amd", "libpinfmax_hip.so")):
        import __graft_entry__ as g
        g.build()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s", "peaks_validation"])
    assert os.path.exists(os.path.join(ROOT, "examples", "peaks_validation"))


@pytest.mark.gpu
def test_c_host_prints_the_logged_peak_line():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s", "peaks_validation"])
    out = subprocess.run([os.path.join(ROOT, "examples", "peaks_validation")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    with open(os.path.join(ROOT, "tests", "golden", "peaks_kat.json")) as fh:
        run = [r for r in json.load(fh)["runs"] if r["run"] == "HMF_Validation"][0]
    m = re.search(r"Task 0 found (\d+) peaks, (\d+) in the well resolved region\. Total number of peaks: (\d+)", out.stdout)
    assert m, out.stdout
    found, good, total = (int(g) for g in m.groups())
    print(m.group(0), "| logged:", run["log_line"])
    assert found == good == total
    assert abs(total - run["total_peaks"]) <= 5      # the bound of the collapsed-cell check of this run (tests/test_peaks_kat.py)
    # the well resolved peaks of the four sub-boxes add up to the total (what the reference's log on four tasks shows)
    assert int(re.search(r"Sum of the well resolved peaks of the four sub-boxes: (\d+)", out.stdout).group(1)) == total
    seeds = [float(v) for v in re.findall(r"seed \d: cell \(\d+, \d+, \d+\), Fmax = ([0-9.]+)", out.stdout)]
    assert len(seeds) == 3 and seeds == sorted(seeds, reverse=True) and seeds[-1] >= 1.0
