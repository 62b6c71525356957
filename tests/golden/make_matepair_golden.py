#!/usr/bin/env python3
"""Generate the mate-pair fixtures in tests/golden/ from the REFERENCE itself.

Compiles tests/golden/ref_matepairs_main.cpp against the reference's own
sources (in place, as oracle/Makefile does for ref_harness) into the ignored
oracle/_ref/ref_matepairs, writes small deterministic paired-end inputs and
stores what the reference's readMatePairsFromFile() leaves in every
Read::getMatePairList():

  pairs_<name>.<k>.{fq,fa}.gz  the input files (data); pairs_<name>.json lists
                               them (paired-end first), with l
  pairs_<name>.mates.gz        the driver's dump: "#N", "#R id string", "#S id
                               super", then "#B 1" + "#M id mate orient dataset"
                               (after markContainedReads) and "#B 0" + "#M ..."
                               (all superReadIDs zero: the setDataset case)
  matepair_cases.json          hand-made files for the pair reader's quirks with
                               the same dump

Only runs where the reference tree is present.  No test runs this.
Usage: python tests/golden/make_matepair_golden.py [reference dir]
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
    """The reference tree oracle/Makefile compiles ref_harness from (its REF ?= line)."""
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        for line in f:
            if line.startswith("REF ?="):
                return line.split("=", 1)[1].strip()
    raise SystemExit("oracle/Makefile has no REF ?= line: pass the reference directory")


REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REF") or default_ref()
DRIVER = os.path.join(ROOT, "oracle", "_ref", "ref_matepairs")
REF_SRCS = ["Dataset.cpp", "Edge.cpp", "HashTable.cpp", "OverlapGraph.cpp", "Read.cpp"]

COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def rc(s: str) -> str:
    return s.translate(COMP)[::-1]


def rand_dna(rng, n: int) -> str:
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def compile_driver():
    os.makedirs(os.path.dirname(DRIVER), exist_ok=True)
    subprocess.run(["g++", "-std=gnu++98", "-O2", "-w", f"-I{REF}", "-o", DRIVER,
                    os.path.join(HERE, "ref_matepairs_main.cpp")] + [os.path.join(REF, s) for s in REF_SRCS],
                   check=True)


def run_driver(l: int, pe: list[str], se: list[str]) -> str:
    with tempfile.NamedTemporaryFile("r", suffix=".txt", delete=False) as t:
        out = t.name
    subprocess.run([DRIVER, str(l), out, str(len(pe))] + pe + se, check=True)
    with open(out) as f:
        text = f.read()
    os.unlink(out)
    return text


def fastq(pairs, newline_at_end=True) -> str:
    lines = []
    for k, (a, b) in enumerate(pairs):
        for tag, s in (("1", a), ("2", b)):
            lines += [f"@p{k}/{tag}", s, "+", "I" * len(s)]
    return "\n".join(lines) + ("\n" if newline_at_end else "")


def fasta(seqs, wrap=60, newline_at_end=True) -> str:
    out = []
    for k, s in enumerate(seqs):
        out.append(f">s{k}")
        out += [s[i:i + wrap] for i in range(0, len(s), wrap)] or [""]
    return "\n".join(out) + ("\n" if newline_at_end else "")


def fragment_pair(rng, genome: str, rl1: int, rl2: int, frag: int):
    p = int(rng.integers(0, len(genome) - frag))
    f = genome[p:p + frag]
    if rng.integers(0, 2):
        f = rc(f)
    return f[:rl1], rc(f[-rl2:])


def make_small(rng):
    """FASTQ, 150 bp, l = 50."""
    g = rand_dna(rng, 3000)
    pairs = [fragment_pair(rng, g, 150, 150, int(rng.integers(300, 500))) for _ in range(260)]
    a, b = pairs[3]
    pairs.append(pairs[0])                       # an exact duplicate pair
    x = pairs[5][0]
    pairs += [(x, pairs[6][1]), (x, pairs[7][1]), (x, pairs[8][0])]  # one read with three more mates
    pairs += [(b, a)]                            # the same two reads in the other file order
    pairs += [(a, a), (a, rc(a))]                # a read paired with itself, equal and opposite strands
    h = rand_dna(rng, 75)
    pal = h + rc(h)                              # its own reverse complement
    pairs += [(pal, b), (pal, pal), (a, pal)]
    pairs += [(pairs[10][0].lower(), pairs[10][1]), (pairs[11][0], pairs[11][1].swapcase()),
              (pairs[12][0][:70] + pairs[12][0][70:].lower(), pairs[12][1].lower())]
    n1 = pairs[13][0][:40] + "N" + pairs[13][0][41:]
    pairs += [(n1, pairs[13][1]), (pairs[14][0], pairs[14][1][:149] + "N")]   # one mate holds N
    pairs += [("A" * 125 + rand_dna(rng, 25), pairs[15][1])]                   # >= 80 % A
    pairs += [(pairs[16][0][:50], pairs[16][1])]                                # a mate of length l
    pairs += [fragment_pair(rng, g, 150, 150, 350) for _ in range(20)]
    return {"l": 50, "pe": [("fq", fastq(pairs, newline_at_end=True))], "se": []}


def make_mixed(rng):
    """Two paired-end FASTA files + one single-end file, lengths 60-250, wrapped lines, l = 40."""
    g = rand_dna(rng, 4000)

    def read_at(p, n, flip):
        s = g[p:p + n]
        return rc(s) if flip else s

    def rand_read():
        n = int(rng.integers(60, 251))
        return read_at(int(rng.integers(0, len(g) - n)), n, bool(rng.integers(0, 2)))

    f0 = []
    for _ in range(70):
        f0 += [rand_read(), rand_read()]
    # reads contained in longer ones, on either strand, as mates
    for k in range(24):
        p = int(rng.integers(0, len(g) - 260))
        big = read_at(p, 250, bool(rng.integers(0, 2)))
        q = p + int(rng.integers(0, 150))
        small = read_at(q, int(rng.integers(60, 100)), bool(rng.integers(0, 2)))
        if k % 3 == 0:
            f0 += [small, big]          # a contained read and its container as one pair
        elif k % 3 == 1:
            f0 += [small, rand_read()]
            f0 += [rand_read(), big]
        else:
            f0 += [big, rc(small)]
    # a chain A in B in C
    A, B, C = read_at(1000, 70, False), read_at(990, 120, True), read_at(960, 250, False)
    f0 += [A, rand_read(), B, A, rand_read(), C]
    same = (rand_read(), rand_read())
    f0 += list(same)
    f1 = list(same)                      # the same pair in dataset 0 and dataset 1
    for _ in range(40):
        f1 += [rand_read(), rand_read()]
    f1 += [f0[0], f0[1], f0[1], f0[0], rc(A), C]
    f1 += [rand_read()]                  # an odd record count: the last one pairs with itself
    se = [read_at(int(rng.integers(0, len(g) - 250)), 250, bool(rng.integers(0, 2))) for _ in range(30)]
    se += [read_at(900, 250, True)]      # a container that only the single-end file holds
    return {"l": 40,
            "pe": [("fa", fasta(f0, newline_at_end=False)), ("fa", fasta(f1, wrap=70))],
            "se": [("fa", fasta(se, wrap=80))]}


def make_long(rng):
    """40 pairs of 1.1-3 kb with a few 150-bp mates, FASTQ, l = 50."""
    g = rand_dna(rng, 12000)
    pairs = []
    for k in range(40):
        n1, n2 = int(rng.integers(1100, 3001)), int(rng.integers(1100, 3001))
        if k % 8 == 3:
            n2 = 150
        if k % 8 == 6:
            n1 = 150
        frag = max(n1, n2) + int(rng.integers(0, 1500))
        pairs.append(fragment_pair(rng, g, n1, n2, min(frag, len(g) - 1)))
    pairs.append((pairs[0][1], pairs[0][0]))
    pairs.append(pairs[1])
    return {"l": 50, "pe": [("fq", fastq(pairs, newline_at_end=False))], "se": []}


def hand_cases(rng):
    r = [rand_dna(rng, 36) for _ in range(8)]
    cases = []
    # CRLF on the second pair only: '\r' stays in those mates, which then fail testRead
    fq = f"@a/1\n{r[0]}\n+\n{'I' * 36}\n@a/2\n{r[1]}\n+\n{'I' * 36}\n"
    fq += f"@b/1\r\n{r[2]}\r\n+\r\n{'I' * 36}\r\n@b/2\r\n{r[3]}\r\n+\r\n{'I' * 36}\r\n"
    fq += f"@c/1\n{r[1]}\n+\n{'I' * 36}\n@c/2\n{r[0]}\n+\n{'I' * 36}"
    cases.append({"name": "crlf_fastq", "l": 10, "pe": [fq], "se": []})
    fa = f">a first>mate x\n{r[0][:20]}\n{r[0][20:]}\n>a second > mate\n{r[1]}\n>b>1\n{r[2]}\n>b>2\n{rc(r[0])}\n"
    cases.append({"name": "gt_in_fasta_header", "l": 10, "pe": [fa], "se": []})
    # the last record stops after its first mate's sequence: the remaining getlines keep that text
    fq = f"@a/1\n{r[4]}\n+\n{'I' * 36}\n@a/2\n{r[5]}\n+\n{'I' * 36}\n@b/1\n{r[6]}"
    cases.append({"name": "truncated_fastq", "l": 10, "pe": [fq], "se": []})
    fq = f"@a/1\n{r[4]}\n+\n{'I' * 36}\n@a/2\n{r[5]}\n+\n{'I' * 36}\n@b/1\n{r[6]}\n+\n{'I' * 36}\n@b/2\n"
    cases.append({"name": "truncated_fastq_header_only", "l": 10, "pe": [fq], "se": []})
    fa = f">a\n{r[0]}\n>b\n{r[1]}\n>c\n{r[2]}\n"
    cases.append({"name": "odd_fasta", "l": 10, "pe": [fa], "se": []})
    fq = f"@a/1\n{r[0].lower()}\n+\n{'I' * 36}\n@a/2\n{r[7]}\n+\n{'I' * 36}\n\n"
    cases.append({"name": "two_trailing_newlines", "l": 10, "pe": [fq], "se": [f">s\n{r[3]}\n"]})
    return cases


def main():
    compile_driver()
    rng = np.random.default_rng(20240611)
    for name, make in (("small", make_small), ("mixed", make_mixed), ("long", make_long)):
        fx = make(rng)
        with tempfile.TemporaryDirectory() as d:
            paths = {"pe": [], "se": []}
            listed = {"pe": [], "se": []}
            k = 0
            for kind in ("pe", "se"):
                for ext, text in fx[kind]:
                    fn = f"pairs_{name}.{k}.{ext}"
                    k += 1
                    with open(os.path.join(d, fn), "w", newline="") as f:
                        f.write(text)
                    with gzip.GzipFile(os.path.join(HERE, fn + ".gz"), "wb", mtime=0) as f:
                        f.write(text.encode())
                    paths[kind].append(os.path.join(d, fn))
                    listed[kind].append(fn + ".gz")
            dump = run_driver(fx["l"], paths["pe"], paths["se"])
        with gzip.GzipFile(os.path.join(HERE, f"pairs_{name}.mates.gz"), "wb", mtime=0) as f:
            f.write(dump.encode())
        with open(os.path.join(HERE, f"pairs_{name}.json"), "w") as f:
            json.dump({"l": fx["l"], "pe": listed["pe"], "se": listed["se"], "mates": f"pairs_{name}.mates.gz"}, f,
                      indent=1)
        print(name, dump.count("#M"), "list entries in both blocks")
    cases = hand_cases(rng)
    for c in cases:
        with tempfile.TemporaryDirectory() as d:
            pe, se = [], []
            for kind, lst in (("pe", pe), ("se", se)):
                for k, text in enumerate(c[kind]):
                    p = os.path.join(d, f"{kind}{k}")
                    with open(p, "w", newline="") as f:
                        f.write(text)
                    lst.append(p)
            c["dump"] = run_driver(c["l"], pe, se)
    with open(os.path.join(HERE, "matepair_cases.json"), "w") as f:
        json.dump(cases, f, indent=1)
    print("hand cases:", [c["name"] for c in cases])


if __name__ == "__main__":
    main()
