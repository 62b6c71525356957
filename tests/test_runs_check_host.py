"""The run bit sets of the scan's mask path on the CPU (device/mg_runs.hpp, the
header k_scan shares): the stand-alone ASan + UBSan check program
(tools/mg_runs_check_main.cpp, make runs_check_asan) records the runs of random
and adversarial key sequences as the kernel does, decodes them with the shared
helpers and compares every (p, jlo, jhi) with a brute-force per-window minimum.
Its cases: n - m and J on every chunk edge up to the width's maximum, w = 1,
19, 31, 32, 33 and w > 64, all keys equal (J runs), strictly increasing and
decreasing keys, many ties, and lanes held past their read."""
import os
import subprocess

from conftest import ROOT


def test_runs_check_asan():
    csrc = os.path.join(ROOT, "metagenomics_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "runs_check_asan"], check=True)
    exe = os.path.join(ROOT, "metagenomics_amd", "lib", "asan", "mg_runs_check")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "mg_runs_check: ok" in r.stdout and "runtime error" not in r.stderr
