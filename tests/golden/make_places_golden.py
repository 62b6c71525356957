#!/usr/bin/env python3
"""Generate the placement fixtures in tests/golden/ from the REFERENCE itself.

Compiles tests/golden/ref_places_main.cpp against the reference's own sources
(in place, as oracle/Makefile does for ref_harness) into the ignored
oracle/_ref/ref_places and stores what the reference's updateReadLocations,
calculateMeanAndSdOfInsertSize and getBaseByBaseCoverage leave (the driver's
dump: reads, mate lists, every edge with its lists, every read's four location
lists, the statistic's stdout lines, mean / SD / count per dataset,
coverageDepth / SD per edge):

  pairs_<name>.places.gz    the build path (Dataset -> HashTable -> OverlapGraph(ht)
                            -> sortEdges) on the three mate-pair fixtures and on
  pairs_branchy.<k>.fa.gz   one new paired-end set of two files on a branching
  pairs_branchy.json        graph: a genome with a 300-bp repeat at three places
                            (one reverse-complemented) and 1-substitution reads,
                            the recipe of the `branchy` fixture; asserted: at
                            least 6 composite edges, at least 20 insert sizes in
                            every dataset, an edge with a non-zero coverage SD
  places.json               the four names
  places_cases.json         hand cases on the resume path (OverlapGraph() ->
                            setDataset -> readGraphFromFile -> sortEdges): the
                            reads, the pair files, the .unitig text and the dump
                            inline.  Only this path places a read on several
                            edges.  Covered: a read with two forward placements
                            (its intervals are zeroed) beside reads with one; the
                            same pair on two edges; insert sizes 999, 1000 and
                            1001; equal locations; a read paired with itself; a
                            pair in two datasets; a dataset without values; an
                            edge with one list read; a simple edge; list reads
                            inside the zeroed spans (count = 0); interval ends
                            that are not monotone; frequencies above 1.
Left out, because the reference cannot produce them: a read with one forward
and two reverse placements (readGraphFromFile gives every record a twin with
the strands flipped, so a read has as many forward as reverse placements; the
synthetic tests cover it), and datasetNumber 255 (needs 256 files).  A hand
case on which the reference throws would be dropped with a message; none does.

Only runs where the reference tree is present.  No test runs this.
Usage: python tests/golden/make_places_golden.py [reference dir]
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


def default_ref() -> str:
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        for line in f:
            if line.startswith("REF ?="):
                return line.split("=", 1)[1].strip()
    raise SystemExit("oracle/Makefile has no REF ?= line: pass the reference directory")


REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REF") or default_ref()
DRIVER = os.path.join(ROOT, "oracle", "_ref", "ref_places")
REF_SRCS = ["Dataset.cpp", "Edge.cpp", "HashTable.cpp", "OverlapGraph.cpp", "Read.cpp"]
COMP = str.maketrans("ACGT", "TGCA")


def rc(s: str) -> str:
    return s.translate(COMP)[::-1]


def rand_dna(rng, n: int) -> str:
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def compile_driver():
    os.makedirs(os.path.dirname(DRIVER), exist_ok=True)
    subprocess.run(["g++", "-std=gnu++98", "-O2", "-w", f"-I{REF}", "-o", DRIVER,
                    os.path.join(HERE, "ref_places_main.cpp")] + [os.path.join(REF, s) for s in REF_SRCS], check=True)


def run_driver(mode, l, pe, se, unitig=None) -> str:
    with tempfile.NamedTemporaryFile("r", suffix=".txt", delete=False) as t:
        out = t.name
    subprocess.run([DRIVER, mode, str(l), out] + ([unitig] if unitig else []) + [str(len(pe))] + pe + se, check=True)
    with open(out) as f:
        text = f.read()
    os.unlink(out)
    return text


def fasta(seqs) -> str:
    return "".join(f">s{k}\n{s}\n" for k, s in enumerate(seqs))


def stats(dump):
    d = [ln.split() for ln in dump.splitlines()]
    return {"composite": sum(1 for t in d if t[0] == "#E" and int(t[6]) > 0),
            "counts": [int(t[4]) for t in d if t[0] == "#D"],
            "cov_sd": [int(t[3]) for t in d if t[0] == "#C" and t[2] != "!"],
            "threw": sum(1 for t in d if t[0] == "#C" and t[2] == "!")}


def unpack(d, fn):
    with gzip.open(os.path.join(HERE, fn), "rb") as f, open(os.path.join(d, fn[:-3]), "wb") as g:
        g.write(f.read())
    return os.path.join(d, fn[:-3])


def build_fixture(name):
    with open(os.path.join(HERE, name + ".json")) as f:
        meta = json.load(f)
    with tempfile.TemporaryDirectory() as d:
        dump = run_driver("build", meta["l"], [unpack(d, x) for x in meta["pe"]], [unpack(d, x) for x in meta["se"]])
    with gzip.GzipFile(os.path.join(HERE, f"{name}.places.gz"), "wb", mtime=0) as f:
        f.write(dump.encode())
    print(name, stats(dump))
    return dump


def make_branchy(rng):
    """Two paired-end FASTA files of 100-bp mates from a genome with a 300-bp repeat at three places, l = 40."""
    G, R = rand_dna(rng, 6000), rand_dna(rng, 300)
    g = G[:1500] + R + G[1500:3200] + rc(R) + G[3200:4800] + R + G[4800:]
    files = []
    for n_pairs in (900, 700):
        seqs = []
        for _ in range(n_pairs):
            frag = int(rng.integers(220, 420))
            p = int(rng.integers(0, len(g) - frag))
            fr = g[p:p + frag]
            if rng.integers(0, 2):
                fr = rc(fr)
            a, b = fr[:100], rc(fr[-100:])
            if rng.random() < 0.04:  # a substitution: tips and bubbles
                q = int(rng.integers(5, 95))
                a = a[:q] + "ACGT"[("ACGT".index(a[q]) + int(rng.integers(1, 4))) % 4] + a[q + 1:]
            seqs += [a, b]
        files.append(fasta(seqs))
    listed = []
    for k, text in enumerate(files):
        fn = f"pairs_branchy.{k}.fa.gz"
        with gzip.GzipFile(os.path.join(HERE, fn), "wb", mtime=0) as f:
            f.write(text.encode())
        listed.append(fn)
    with open(os.path.join(HERE, "pairs_branchy.json"), "w") as f:
        json.dump({"l": 40, "pe": listed, "se": [], "places": "pairs_branchy.places.gz"}, f, indent=1)
    dump = build_fixture("pairs_branchy")
    s = stats(dump)
    assert s["composite"] >= 6 and min(s["counts"]) >= 20 and max(s["cov_sd"]) > 0 and len(s["counts"]) == 2, s


def hand_cases(rng):
    lens = [30, 33, 35, 38, 40, 41, 45, 47, 50, 52, 55, 60, 64, 70]
    raw = {n: rand_dna(rng, n) for n in lens}
    canon = sorted({min(s, rc(s)) for s in raw.values()})
    assert len(canon) == len(lens)
    id_of = {len(s): i + 1 for i, s in enumerate(canon)}  # every length occurs once
    fwd = {len(s): s for s in canon}
    # frequencies above 1: reads 35, 40 and 45 occur several times in the single-end file
    se = fasta([raw[n] for n in lens] + [raw[35], rc(raw[35]), raw[40], raw[45], raw[45], raw[45]])

    def rec(src, dst, orient, offset, lst=()):
        v = [id_of[src], id_of[dst], orient, offset, len(lst)]
        for r, off, o in lst:
            v += [id_of[r], off, o]
        return "".join(f"{x}\n" for x in v)

    def pairs(*p):
        return fasta([fwd[x] for ab in p for x in ab])

    two_edges = (rec(60, 70, 3, 120, [(35, 50, 1), (40, 30, 1)]) +
                 rec(52, 45, 3, 150, [(35, 55, 1), (40, 45, 1)]))
    cases = [
        # 35 and 40 lie forward on two edges each (zeroed everywhere); the pair matches on both edges and both twins
        {"name": "pair_on_two_edges", "unitig": two_edges + rec(64, 55, 3, 100, [(33, 60, 1)]),
         "pe": [pairs((35, 40), (33, 35))]},
        # distances 100, 1099, 1100, 1101, 1101, 2101: insert sizes 999, 1000, 1001, equal locations, a self pair
        {"name": "boundaries", "unitig": rec(60, 70, 3, 2200, [(30, 100, 1), (33, 999, 1), (35, 1, 1), (40, 1, 1),
                                                                (41, 0, 0), (45, 1000, 1)]),
         "pe": [pairs((33, 30), (35, 30), (40, 30), (41, 40), (45, 41), (30, 30))]},
        # the same pair in datasets 0 and 1; dataset 2 holds only pairs that share no edge
        {"name": "datasets", "unitig": two_edges + rec(64, 55, 3, 100, [(33, 60, 1)]),
         "pe": [pairs((35, 40), (40, 40)), pairs((35, 40)), pairs((33, 35), (47, 50))]},
        # one list read; a simple edge
        {"name": "single_and_simple", "unitig": rec(50, 52, 3, 80, [(38, 45, 1)]) + rec(47, 55, 3, 20),
         "pe": [pairs((38, 50))]},
        # both list reads lie inside the zeroed source / destination spans: no counter is left
        {"name": "all_inside_spans", "unitig": rec(70, 64, 3, 30, [(30, 10, 1), (33, 45, 1)]),
         "pe": [pairs((33, 30))]},
        # interval ends 120, 85, 129; the twin's UINT16 offsets wrap, so the offset is large enough to hold them
        {"name": "non_monotone", "unitig": rec(41, 47, 3, 140000, [(70, 50, 1), (30, 5, 1), (64, 10, 0)]),
         "pe": [pairs((30, 70), (64, 30))]},
        # reverse-strand entries on an orientation-0 edge
        {"name": "reverse_entries", "unitig": rec(55, 60, 0, 90, [(45, 30, 0), (50, 20, 0), (52, 15, 1)]),
         "pe": [pairs((50, 45), (52, 50), (45, 52))]},
        # a self-loop: the record and its twin join the same two nodes
        {"name": "self_loop", "unitig": rec(64, 64, 3, 100, [(38, 70, 1), (40, 20, 1)]),
         "pe": [pairs((40, 38), (38, 38))]},
    ]
    kept = []
    for c in cases:
        c["l"], c["se"] = 10, se
        with tempfile.TemporaryDirectory() as d:
            paths = []
            for k, text in enumerate(c["pe"]):
                paths.append(os.path.join(d, f"pe{k}.fa"))
                with open(paths[-1], "w") as f:
                    f.write(text)
            sp, up = os.path.join(d, "se.fa"), os.path.join(d, "g.unitig")
            with open(sp, "w") as f:
                f.write(se)
            with open(up, "w") as f:
                f.write(c["unitig"])
            c["dump"] = run_driver("resume", 10, paths, [sp], up)
        s = stats(c["dump"])
        print(c["name"], s)
        if s["threw"]:
            print("  dropped: the reference's at() throws on", s["threw"], "edge(s)")
            continue
        kept.append(c)
    assert len(kept) >= 8
    return kept


def main():
    compile_driver()
    for name in ("pairs_small", "pairs_mixed", "pairs_long"):
        build_fixture(name)
    make_branchy(np.random.default_rng(20241020))
    with open(os.path.join(HERE, "places.json"), "w") as f:
        json.dump({n: f"{n}.places.gz" for n in ("pairs_small", "pairs_mixed", "pairs_long", "pairs_branchy")}, f,
                  indent=1)
    cases = hand_cases(np.random.default_rng(20241021))
    with open(os.path.join(HERE, "places_cases.json"), "w") as f:
        json.dump(cases, f, indent=1)


if __name__ == "__main__":
    main()
