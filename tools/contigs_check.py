#!/usr/bin/env python3
"""Run the stand-alone sanitizer check of the contig host code on every fixture.

  make -C metagenomics_amd/csrc contigs_check_asan
  python tools/contigs_check.py

For each fixture of tests/conftest.py and each hand case of
tests/golden/contig_cases.json: unpack the reads (ID order), the .unitig golden
and the reference's two printGraph files, and run
metagenomics_amd/lib/asan/mg_contigs_check on them (ASan + UBSan, host code
only, its own main; see metagenomics_amd/csrc/tools/mg_contigs_check_main.cpp).
Exit status 0 = every run passed.
"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

from conftest import FIXTURES, GOLDEN, fixture_input, load_meta  # noqa: E402
from metagenomics_amd.overlap import Dataset  # noqa: E402

EXE = os.path.join(ROOT, "metagenomics_amd", "lib", "asan", "mg_contigs_check")


def gz(name):
    with gzip.open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def run(tag, ds, unitig, gdl, fasta):
    with tempfile.TemporaryDirectory() as d:
        paths = {k: os.path.join(d, k) for k in ("reads.txt", "g.unitig", "want.gdl", "want.fa")}
        with open(paths["reads.txt"], "w") as f:
            f.write("".join(ds.read(i) + "\n" for i in range(1, ds.num_unique + 1)))
        for k, data in (("g.unitig", unitig), ("want.gdl", gdl), ("want.fa", fasta)):
            with open(paths[k], "wb") as f:
                f.write(data)
        r = subprocess.run([EXE] + list(paths.values()), capture_output=True, text=True)
    print(tag, (r.stdout + r.stderr).strip())
    return r.returncode


def main():
    if not os.path.exists(EXE):
        raise SystemExit(f"{EXE} missing: make -C metagenomics_amd/csrc contigs_check_asan")
    with open(os.path.join(GOLDEN, "contigs.json")) as f:
        index = json.load(f)
    bad = 0
    for name in FIXTURES:
        meta = load_meta(name)
        ds = Dataset.from_files([fixture_input(name)], meta["l"])
        bad += run(name, ds, gz(meta["unitig"]["file"]), gz(index[name]["gdl"]), gz(index[name]["fasta"])) != 0
    with open(os.path.join(GOLDEN, "contig_cases.json")) as f:
        cases = json.load(f)
    for c in cases:
        with tempfile.NamedTemporaryFile("w", suffix=".fa", delete=False) as t:
            t.write(c["fasta"])
        ds = Dataset.from_files([t.name], c["l"])
        os.unlink(t.name)
        bad += run(c["name"], ds, c["unitig"].encode(), c["gdl"].encode(), c["contigs_fa"].encode()) != 0
    print("failed runs:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
