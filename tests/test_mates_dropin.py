"""The drop-in's mate lists (include/mg_api.hpp): Read::getMatePairList() after
new OverlapGraph(ht) equals the reference's lists after its
buildOverlapGraphFromHashTable (golden block 1), built on the device and, with
MG_DEVICE_MATES=0, by the host mirror; after the resume path's setDataset it
equals the lists of a Dataset whose superReadIDs are all zero (block 0).
Driven through the CLI (mg_overlap -mates), a C++ caller of mg_api.hpp."""
import os
import subprocess

import pytest

import mates_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "metagenomics_amd", "lib", "mg_overlap")


def dump_lines(g, block):
    start, recs = g.blocks[block]
    return ["#M %d %d %d %d" % (a, r["id"], r["orient"], r["dataset"])
            for a in range(1, len(g.reads) + 1) for r in recs[int(start[a]):int(start[a + 1])]]


def run_cli(g, tmp_path, extra, env=None):
    pe, se = g.write_files(tmp_path)
    prefix = str(tmp_path / "out")
    cmd = [EXE, "-pe", str(len(pe))] + pe
    if se:
        cmd += ["-se", str(len(se))] + se
    cmd += ["-f", prefix, "-l", str(g.l), "-mates"] + extra
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=120, env={**os.environ, **(env or {})})
    return prefix


@pytest.mark.parametrize("name", R.FIXTURES + ("odd_fasta", "crlf_fastq"))
def test_get_mate_pair_list_after_the_build(name, tmp_path):
    g = R.golden(name) if name in R.FIXTURES else R.hand_cases()[name]
    prefix = run_cli(g, tmp_path, [])
    assert open(prefix + ".mates").read().split("\n")[:-1] == dump_lines(g, 1)
    # the resume path (OverlapGraph() -> setDataset -> readGraphFromFile): superReadIDs all zero
    run_cli(g, tmp_path, ["-s"])
    assert open(prefix + ".resumed.mates").read().split("\n")[:-1] == dump_lines(g, 0)


def test_host_mirror_inside_the_drop_in(tmp_path):
    g = R.golden("pairs_mixed")
    prefix = run_cli(g, tmp_path, [], env={"MG_DEVICE_MATES": "0"})
    assert open(prefix + ".mates").read().split("\n")[:-1] == dump_lines(g, 1)
