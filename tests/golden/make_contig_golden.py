#!/usr/bin/env python3
"""Generate the contig fixtures in tests/golden/ from the REFERENCE itself.

Compiles tests/golden/ref_contigs_main.cpp against the reference's own sources
(in place, as oracle/Makefile does for ref_harness) into the ignored
oracle/_ref/ref_contigs and stores what the reference's printGraph and
getStringInEdge give:

  <name>.contigs.fa.gz   printGraph's FASTA file, verbatim     (build mode: Dataset ->
  <name>.gdl.gz          printGraph's .gdl file, verbatim       HashTable -> OverlapGraph(ht)
  <name>.estrings.gz     "src dst orient offset nreads string"  -> sortEdges -> printGraph,
                         of every edge of every list in list    for every fixture of
                         order, both directions                 tests/conftest.py)
  contigs.json           per fixture: the three file names and "other_twin", the
                         self-loop contigs [src, list position] where the reference
                         listed the other twin than the library's rule (lower
                         creation index); the library must be built for that
  contig_cases.json      hand-made reads + .unitig files the build never yields
                         (resume mode: setDataset -> readGraphFromFile -> sortEdges
                         -> printGraph) with the same three dumps inline

calculateFlow is skipped (its CS2 run fails on its own input), so Flow and
Coverage are 0 in every header.  Only runs where the reference tree is present.
No test runs this.
Usage: python tests/golden/make_contig_golden.py [reference dir]
"""
from __future__ import annotations

import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

from conftest import FIXTURES, fixture_input, golden_rows, load_meta  # noqa: E402


def default_ref() -> str:
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        for line in f:
            if line.startswith("REF ?="):
                return line.split("=", 1)[1].strip()
    raise SystemExit("oracle/Makefile has no REF ?= line: pass the reference directory")


REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REF") or default_ref()
DRIVER = os.path.join(ROOT, "oracle", "_ref", "ref_contigs")
REF_SRCS = ["Dataset.cpp", "Edge.cpp", "HashTable.cpp", "OverlapGraph.cpp", "Read.cpp"]
COMP = str.maketrans("ACGT", "TGCA")


def rc(s: str) -> str:
    return s.translate(COMP)[::-1]


def compile_driver():
    os.makedirs(os.path.dirname(DRIVER), exist_ok=True)
    subprocess.run(["g++", "-std=gnu++98", "-O2", "-w", f"-I{REF}", "-o", DRIVER,
                    os.path.join(HERE, "ref_contigs_main.cpp")] + [os.path.join(REF, s) for s in REF_SRCS], check=True)


def run_driver(args, prefix):
    subprocess.run([DRIVER] + args, check=True, stdout=subprocess.DEVNULL)
    out = {}
    for ext in ("fa", "gdl", "estrings", "loops"):
        with open(f"{prefix}.{ext}", "rb") as f:
            out[ext] = f.read()
    return out


def library_loops(name):
    """[src, list position] of the self-loop contigs the library's rule lists."""
    from metagenomics_amd.overlap import EDGE_DTYPE, Dataset, UnitigGraph

    meta = load_meta(name)
    t = golden_rows(name)
    rows = np.zeros(t.shape[0], dtype=EDGE_DTYPE)
    rows["src"], rows["dst"], rows["orient"], rows["offset"] = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
    ds = Dataset.from_files([fixture_input(name)], meta["l"])
    g = UnitigGraph(rows, ds.packed()[1], meta["l"])
    g.sort_edges()
    return loops_of(g)


def loops_of(g):
    every = g.contig_edges(all_edges=True)[0]
    chosen = g.contig_edges()[0]
    key = lambda e: (int(e["src"]), int(e["dst"]), int(e["orient"]), int(e["offset"]), int(e["n"]), int(e["tail"]))
    pos, at, out, k = {}, 0, [], 0
    for e in every:  # list positions restart at every source read
        p = pos.get(int(e["src"]), 0)
        pos[int(e["src"])] = p + 1
        if k < chosen.shape[0] and key(chosen[k]) == key(e):
            if e["src"] == e["dst"]:
                out.append([int(e["src"]), p])
            k += 1
    assert k == chosen.shape[0]
    return out


def hand_cases(rng):
    lens = [30, 33, 35, 40, 41, 45, 50, 52, 55, 60, 64, 70]
    raw = ["".join("ACGT"[i] for i in rng.integers(0, 4, n)) for n in lens]
    canon = sorted({min(s, rc(s)) for s in raw})
    assert len(canon) == len(lens)
    id_of = {len(s): i + 1 for i, s in enumerate(canon)}  # every length occurs once

    def rec(src, dst, orient, offset, lst=()):
        v = [id_of[src], id_of[dst], orient, offset, len(lst)]
        for r, off, o in lst:
            v += [id_of[r], off, o]
        return "".join(f"{x}\n" for x in v)

    cases = [
        {"name": "orient4", "unitig": rec(30, 40, 0, 5) + rec(33, 45, 1, 10) + rec(35, 50, 2, 20) + rec(41, 52, 3, 41)},
        {"name": "n_join", "unitig": rec(40, 60, 3, 70, [(50, 40, 1)])},
        {"name": "empty_piece", "unitig": rec(50, 45, 2, 30, [(30, 20, 0)])},
        {"name": "composite_mixed",
         "unitig": rec(64, 52, 1, 135, [(35, 40, 1), (70, 10, 0), (33, 50, 0), (55, 5, 1)])},
        {"name": "self_loops", "unitig": rec(60, 60, 3, 25) + rec(41, 41, 0, 15) + rec(45, 45, 3, 33, [(33, 20, 1)])},
        {"name": "lines_100_101", "unitig": rec(45, 60, 3, 40) + rec(50, 64, 3, 37)},
    ]
    # (no case without edges: printGraph's closing statistics then read an uninitialised node number)
    fasta = "".join(f">r{k}\n{s}\n" for k, s in enumerate(raw))
    for c in cases:
        c["l"] = 10
        c["fasta"] = fasta
        with tempfile.TemporaryDirectory() as d:
            fa, un = os.path.join(d, "reads.fa"), os.path.join(d, "g.unitig")
            with open(fa, "w") as f:
                f.write(fasta)
            with open(un, "w") as f:
                f.write(c["unitig"])
            out = run_driver(["resume", "10", os.path.join(d, "out"), un, fa], os.path.join(d, "out"))
        c["contigs_fa"] = out["fa"].decode()
        c["gdl"] = out["gdl"].decode()
        c["estrings"] = out["estrings"].decode()
        c["ref_loops"] = [list(map(int, ln.split())) for ln in out["loops"].decode().splitlines()]
    return cases


def main():
    compile_driver()
    index = {}
    for name in FIXTURES:
        meta = load_meta(name)
        with tempfile.TemporaryDirectory() as d:
            out = run_driver(["build", str(meta["l"]), os.path.join(d, "out"), fixture_input(name)],
                             os.path.join(d, "out"))
        files = {"fasta": f"{name}.contigs.fa.gz", "gdl": f"{name}.gdl.gz", "estrings": f"{name}.estrings.gz"}
        for key, ext in (("fasta", "fa"), ("gdl", "gdl"), ("estrings", "estrings")):
            with gzip.GzipFile(os.path.join(HERE, files[key]), "wb", mtime=0) as f:
                f.write(out[ext])
        ref = [list(map(int, ln.split())) for ln in out["loops"].decode().splitlines()]
        ours = library_loops(name)
        files["other_twin"] = [x for x in ref if x not in ours]
        index[name] = files
        print(name, out["fa"].count(b">"), "contigs,", out["estrings"].count(b"\n"), "edge strings, other twin:",
              files["other_twin"])
    with open(os.path.join(HERE, "contigs.json"), "w") as f:
        json.dump(index, f, indent=1, sort_keys=True)
    cases = hand_cases(np.random.default_rng(20240917))
    with open(os.path.join(HERE, "contig_cases.json"), "w") as f:
        json.dump(cases, f, indent=1)
    print("hand cases:", [(c["name"], c["contigs_fa"].count(">")) for c in cases])


if __name__ == "__main__":
    main()
