#!/usr/bin/env python3
"""Generate the mate-pair path fixtures in tests/golden/ from the REFERENCE itself.

Compiles tests/golden/ref_paths_main.cpp against the reference's own sources
(in place, as oracle/Makefile does for ref_harness) into the ignored
oracle/_ref/ref_paths and stores what the reference's
calculateMeanAndSdOfInsertSize, findPathBetweenMatepairs (per mate entry, in the
loop order of OverlapGraph.cpp:1904-1916) and findSupportByMatepairsAndMerge
leave (the driver's dump: reads, mate lists, every edge with its twin, every
read's location lists in list order, mean / SD per dataset, return value, path
and flags per mate entry, the "Merging" lines and the six summary counts, the
lists after the merge) and the .unitig file saved after the merge:

  pairs_<name>.paths.gz       the build path (Dataset -> HashTable ->
  pairs_<name>.support.unitig.gz   OverlapGraph(ht) -> sortEdges) on the four
  paths.json                  mate-pair fixtures
  paths_cases.json.gz         hand cases on the resume path (OverlapGraph() ->
                              setDataset -> readGraphFromFile -> sortEdges):
                              300 reads of 30 bp, the pair files, the .unitig
                              text, the dump and the .unitig after the merge,
                              inline.

Every hand case carries one calibration edge whose pairs fix mean and SD (two
distances m - s and m + s, seen on the edge and on its twin: mean m, SD s).
With m = 210, s = 10 the window is [180, 240].  Cases:
  bound        d1 + d2 at the bound - 1 (explored, a path) and at the bound
  totals       totals 179, 180, 240, 241: none, path, path, none
  wrap         3 sd > mean (mean 500, sd 490): explored, never in range
  empty_lists  a read on no edge, on either side: counted as on the same edge
  twin_edges   the two reads on an edge and on its twin
  self_pair    a read paired with itself (A = B is processed)
  mean0        a second dataset without insert sizes: its entries are skipped
  cycle        `last` reached out of range, then in range round a cycle
  cycle_twice  round twice: the pair (e23, e32) twice in one path
  bubble       two paths in one combo: the pairs inside the bubble are cleared
  two_combos   a read on two edges: the first combo finds no path
  across       two combos with paths: a flag cleared across combos
  self_loop    a self-loop walked twice and three times; (loop, loop) never listed
  chain101     a path of exactly 101 edges, and none of 102
  orient16     all 16 orientation pairs of matchEdgeType round one node
  merge3       three mate pairs over one chain: pairs with support 3 merged,
               one freed by an earlier merge; a pair seen in both orientations
Asserted over the committed fixtures together (which fixture meets which is
printed): pathsFound > 0, noPathsFound > 0, mpOnSameEdge > 0; a flag cleared
inside a combo (bubble) and across combos (across); a pair reached in both
orientations (merge3); a pair with support >= 3 merged and a supported pair
freed by an earlier merge (merge3, pairs_branchy).
Not producible by the reference, covered against the plain-Python restatement
only: orientations above 3, reads whose forward and reverse lists differ in
length, datasetNumber 255, offsets near 2^64.

Only runs where the reference tree is present.  No test runs this.
Usage: python tests/golden/make_paths_golden.py [reference dir]
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
DRIVER = os.path.join(ROOT, "oracle", "_ref", "ref_paths")
REF_SRCS = ["Dataset.cpp", "Edge.cpp", "HashTable.cpp", "OverlapGraph.cpp", "Read.cpp"]
COMP = str.maketrans("ACGT", "TGCA")
FIXTURES = ("pairs_small", "pairs_mixed", "pairs_long", "pairs_branchy")


def rc(s: str) -> str:
    return s.translate(COMP)[::-1]


def compile_driver():
    os.makedirs(os.path.dirname(DRIVER), exist_ok=True)
    subprocess.run(["g++", "-std=gnu++98", "-O2", "-w", f"-I{REF}", "-o", DRIVER,
                    os.path.join(HERE, "ref_paths_main.cpp")] + [os.path.join(REF, s) for s in REF_SRCS], check=True)


def run_driver(mode, l, pe, se, unitig=None):
    """(dump, .unitig after the merge)"""
    with tempfile.NamedTemporaryFile("r", suffix=".txt", delete=False) as t:
        out = t.name
    subprocess.run([DRIVER, mode, str(l), out] + ([unitig] if unitig else []) + [str(len(pe))] + pe + se, check=True)
    with open(out) as f:
        text = f.read()
    with open(out + ".unitig") as f:
        after = f.read()
    os.unlink(out)
    os.unlink(out + ".unitig")
    return text, after


def fasta(seqs) -> str:
    return "".join(f">s{k}\n{s}\n" for k, s in enumerate(seqs))


class Dump:
    def __init__(self, text):
        rows = [ln.split() for ln in text.splitlines()]
        self.edges = [(int(t[2]), int(t[3])) for t in rows if t[0] == "#E"]
        self.mates = [(int(t[1]), int(t[2])) for t in rows if t[0] == "#M"]
        self.datasets = [(int(t[2]), int(t[3])) for t in rows if t[0] == "#D"]
        self.entries = []
        for t in rows:
            if t[0] != "#P":
                continue
            if t[2] in "S0":
                self.entries.append((t[2], [], []))
            else:
                n = int(t[3])
                self.entries.append(("1", [int(x) for x in t[4:4 + n]], [int(x) for x in t[5 + n:]]))
        self.out = [" ".join(t[1:]) for t in rows if t[0] == "#O"]
        self.merged = int(next(t[1] for t in rows if t[0] == "#X"))

    def entry(self, a, b):
        """the processed entry of the pair (a, b), a < b: (kind, path as (src, dst) pairs, flags)"""
        k, path, flags = self.entries[self.mates.index((a, b))]
        return k, [self.edges[e] for e in path], flags

    def counts(self):
        if not self.out:
            return (0, 0, 0)
        g = lambda head, i: int(next(x for x in self.out if x.startswith(head)).split()[i])
        return g("No paths found", 4), g("Paths found", 3), g("Total matepairs on same edge", 5)

    def pairs(self):
        """(supported pairs, cleared flags, pairs seen in both orientations: from the paths themselves)"""
        seen = set()
        for k, path, flags in self.entries:
            for i, f in enumerate(flags):
                if f == 1:
                    seen.add((path[i], path[i + 1]))
        return seen


def unpack(d, fn):
    with gzip.open(os.path.join(HERE, fn), "rb") as f, open(os.path.join(d, fn[:-3]), "wb") as g:
        g.write(f.read())
    return os.path.join(d, fn[:-3])


def gz_write(fn, text):
    with gzip.GzipFile(os.path.join(HERE, fn), "wb", mtime=0) as f:
        f.write(text.encode())
    assert os.path.getsize(os.path.join(HERE, fn)) < (1 << 20), fn


def build_fixture(name):
    with open(os.path.join(HERE, name + ".json")) as f:
        meta = json.load(f)
    with tempfile.TemporaryDirectory() as d:
        dump, after = run_driver("build", meta["l"], [unpack(d, x) for x in meta["pe"]],
                                 [unpack(d, x) for x in meta["se"]])
    gz_write(f"{name}.paths.gz", dump)
    gz_write(f"{name}.support.unitig.gz", after)
    return Dump(dump)


# ---- hand cases: 300 reads of 30 bp; IDs 1..230 are nodes, 234..265 first reads (A), 266..300 second reads (B)
N_READS, LEN = 300, 30
K1, K2, K3, CAL_U, CAL_V = 231, 232, 233, 229, 230  # the calibration edge and its reads


def hand_cases(rng):
    canon = set()
    while len(canon) < N_READS:
        s = "".join("ACGT"[i] for i in rng.integers(0, 4, LEN))
        canon.add(min(s, rc(s)))
    read = [None] + sorted(canon)  # read[id] = the canonical string
    se = fasta(read[1:])

    def rec(src, dst, orient, offset, lst=()):
        v = [src, dst, orient, offset, len(lst)]
        for r, off, o in lst:
            v += [r, off, o]
        return "".join(f"{x}\n" for x in v)

    def pairs(*p):
        """(a, b): a as it is, b reverse-complemented (forward-reverse mates); (a, b, oa, ob) sets the strands"""
        out = []
        for t in p:
            a, b, oa, ob = t if len(t) == 4 else (t[0], t[1], 1, 0)
            out += [read[a] if oa else rc(read[a]), read[b] if ob else rc(read[b])]
        return fasta(out)

    def calib(small, big):
        return (rec(CAL_U, CAL_V, 3, 2000, [(K1, 100, 1), (K2, small, 1), (K3, big - small, 1)]), [(K2, K1), (K3, K1)])

    def chain(nodes, offsets, a=None, b=None, a_loc=40, b_loc=50, first_off=100, last_off=100):
        """nodes[0] -> nodes[1] -> ...: the first edge holds a at a_loc, the last b at b_loc, the others `offsets`"""
        out = ""
        for i in range(len(nodes) - 1):
            lst, off = (), offsets[i - 1] if 0 < i < len(nodes) - 2 else None
            if i == 0:
                off, lst = first_off, ([(a, a_loc, 1)] if a else ())
            if i == len(nodes) - 2:
                off, lst = last_off, ([(b, b_loc, 1)] if b else ())
            out += rec(nodes[i], nodes[i + 1], 3, off, lst)
        return out

    A, B = list(range(234, 266)), list(range(266, 301))
    cal, cal_pairs = calib(200, 220)  # mean 210, sd 10: the window is [180, 240]
    cases = []

    def case(name, unitig, pe, datasets=((210, 10),), cal_text=cal):
        cases.append({"name": name, "unitig": cal_text + unitig, "pe": pe, "expect_datasets": list(datasets)})

    # d1 = first_off - a_loc, d2 = b_loc, total = d2 + d1 + the offsets between
    case("bound", chain([1, 2, 3, 4], [1], A[0], B[0], a_loc=111, first_off=300) +      # d1 + d2 = 239: explored, total 240
         chain([5, 6, 7, 8], [1], A[1], B[1], a_loc=110, first_off=300),                 # d1 + d2 = 240: not explored
         [pairs(*cal_pairs, (A[0], B[0]), (A[1], B[1]))])
    case("totals", "".join(chain([4 * i + 1, 4 * i + 2, 4 * i + 3, 4 * i + 4], [x], A[i], B[i])
                           for i, x in enumerate((69, 70, 130, 131))),
         [pairs(*cal_pairs, *[(A[i], B[i]) for i in range(4)])])
    wcal, wpairs = calib(10, 990)
    case("wrap", chain([1, 2, 3, 4], [70], A[0], B[0]), [pairs(*wpairs, (A[0], B[0]))], ((500, 490),), wcal)
    case("empty_lists", chain([1, 2, 3, 4], [70], A[0], B[0]),
         [pairs(*cal_pairs, (A[0], B[1]), (A[1], B[0]), (A[0], B[0]))])  # B[1] and A[1] lie on no edge
    # A's forward list: the edge; B's reverse list: its twin (a second dataset: the pair is an insert size of 20)
    case("twin_edges", rec(1, 2, 3, 100, [(A[0], 40, 1), (B[0], 20, 1)]),
         [pairs(*cal_pairs), pairs((A[0], B[0], 1, 1))], ((210, 10), (20, 0)))
    case("self_pair", chain([1, 2, 3, 4], [70], A[0], B[0]), [pairs(*cal_pairs, (A[0], A[0]), (A[0], B[0]))])
    case("mean0", chain([1, 2, 3, 4], [70], A[0], B[0]), [pairs(*cal_pairs, (A[0], B[0])), pairs((A[0], B[0]))],
         ((210, 10), (0, 0)))
    cyc = lambda x: rec(1, 2, 3, 100, [(A[0], 40, 1)]) + rec(2, 3, 3, x, [(B[0], 50, 1)]) + rec(3, 2, 3, x)
    case("cycle", cyc(40), [pairs(*cal_pairs, (A[0], B[0]))])        # totals 110, then 190
    case("cycle_twice", cyc(20), [pairs(*cal_pairs, (A[0], B[0]))])  # totals 110, 150, then 190
    bubble = (rec(1, 2, 3, 100, [(A[0], 40, 1)]) + rec(2, 3, 3, 20) + rec(3, 4, 3, 20) + rec(4, 6, 3, 20) +
              rec(3, 5, 3, 25) + rec(5, 6, 3, 20) + rec(6, 7, 3, 20) + rec(7, 8, 3, 100, [(B[0], 50, 1)]))
    case("bubble", bubble, [pairs(*cal_pairs, (A[0], B[0]))])
    case("two_combos", rec(9, 10, 3, 100, [(A[0], 40, 1)]) + chain([1, 2, 3, 4], [70], A[0], B[0]),
         [pairs(*cal_pairs, (A[0], B[0]))])  # A's first placement is a dead end
    case("across", rec(1, 2, 3, 100, [(A[0], 40, 1)]) + rec(9, 2, 3, 100, [(A[0], 40, 1)]) + rec(2, 3, 3, 70) +
         rec(3, 4, 3, 100, [(B[0], 50, 1)]), [pairs(*cal_pairs, (A[0], B[0]))])
    case("self_loop", rec(1, 2, 3, 100, [(A[0], 40, 1)]) + rec(2, 2, 3, 40) + rec(2, 3, 3, 100, [(B[0], 50, 1)]),
         [pairs(*cal_pairs, (A[0], B[0]))])  # totals 110, 150, 190 (twice round), 230 (three times), 270
    # 101 edges: the last at level 100, total = 50 + 31 + 99 = 180; 102 edges: level 101 returns at once
    case("chain101", chain(list(range(1, 103)), [1] * 99, A[0], B[0], a_loc=9, first_off=40) +
         chain(list(range(103, 206)), [1] * 100, A[1], B[1], a_loc=9, first_off=40),
         [pairs(*cal_pairs, (A[0], B[0]), (A[1], B[1]))])
    star, sp = "", []
    for a in range(4):  # in-edges 10 + a -> 1 of orientation a, out-edges 1 -> 20 + b of orientation b
        star += rec(10 + a, 1, a, 200, [(A[a], 60, 1)]) + rec(1, 20 + a, a, 100, [(B[a], 50, 1)])
        sp += [(A[a], B[b]) for b in range(4)]
    case("orient16", star, [pairs(*cal_pairs, *sp)])
    m3 = (rec(1, 2, 3, 100, [(A[0], 40, 1), (A[1], 5, 1), (A[2], 5, 1), (B[3], 5, 1)]) + rec(2, 3, 3, 45) +
          rec(3, 4, 3, 45) + rec(4, 5, 3, 100, [(B[0], 40, 1), (B[1], 5, 1), (B[2], 5, 1), (A[3], 5, 1)]))
    # the fourth pair has its higher ID on the first edge: its entry walks the twins from 5 -> 4 to 2 -> 1, so each
    # pair of the chain is also seen as (twin[b], twin[a]).  Every total is 190.
    case("merge3", m3, [pairs(*cal_pairs, (A[0], B[0]), (A[1], B[1]), (A[2], B[2]), (B[3], A[3]))])
    kept = []
    for c in cases:
        c["l"], c["se"] = 10, se
        with tempfile.TemporaryDirectory() as d:
            paths = []
            for k, text in enumerate(c["pe"]):
                paths.append(os.path.join(d, f"pe{k}.fa"))
                with open(paths[-1], "w") as f:
                    f.write(text)
            sp_, up = os.path.join(d, "se.fa"), os.path.join(d, "g.unitig")
            with open(sp_, "w") as f:
                f.write(se)
            with open(up, "w") as f:
                f.write(c["unitig"])
            c["dump"], c["unitig_after"] = run_driver("resume", 10, paths, [sp_], up)
        d = Dump(c["dump"])
        assert d.datasets == [tuple(x) for x in c.pop("expect_datasets")], (c["name"], d.datasets)
        print(c["name"], d.counts(), "merged", d.merged, [e for e in d.entries if e[0] == "1"][:2])
        kept.append((c, d))
    return kept, A, B


def check_cases(kept, A, B):
    by = {c["name"]: d for c, d in kept}
    found = lambda d, a, b: d.entry(a, b)[0] == "1" and bool(d.entry(a, b)[1])
    none = lambda d, a, b: d.entry(a, b)[0] == "1" and not d.entry(a, b)[1]
    same = lambda d, a, b: d.entry(a, b)[0] == "0"
    d = by["bound"]
    assert found(d, A[0], B[0]) and none(d, A[1], B[1])
    d = by["totals"]
    assert [found(d, A[i], B[i]) for i in range(4)] == [False, True, True, False]
    assert none(by["wrap"], A[0], B[0])
    d = by["empty_lists"]
    assert same(d, A[0], B[1]) and same(d, A[1], B[0]) and found(d, A[0], B[0])
    assert same(by["twin_edges"], A[0], B[0])
    assert same(by["self_pair"], A[0], A[0]) and found(by["self_pair"], A[0], B[0])
    d = by["mean0"]
    assert [k for k, _, _ in d.entries].count("S") > len(d.entries) // 2 and d.counts()[1] == 1
    assert by["cycle"].entry(A[0], B[0])[1] == [(1, 2), (2, 3), (3, 2), (2, 3)]
    assert by["cycle_twice"].entry(A[0], B[0])[1] == [(1, 2), (2, 3), (3, 2), (2, 3), (3, 2), (2, 3)]
    k, path, flags = by["bubble"].entry(A[0], B[0])
    assert len(path) == 6 and flags == [1, 0, 0, 0, 1], (path, flags)
    k, path, flags = by["two_combos"].entry(A[0], B[0])
    assert path[0] == (1, 2) and flags == [1, 1]
    k, path, flags = by["across"].entry(A[0], B[0])
    assert flags == [0, 1] and len(path) == 3, (path, flags)
    k, path, flags = by["self_loop"].entry(A[0], B[0])
    assert path == [(1, 2), (2, 2), (2, 2), (2, 2), (2, 3)] and flags == [1, 1, 1, 1], (path, flags)  # found deepest first
    d = by["chain101"]
    assert len(d.entry(A[0], B[0])[1]) == 101 and none(d, A[1], B[1])
    d = by["orient16"]
    match = lambda a, b: (a in (1, 3) and b in (2, 3)) or (a in (0, 2) and b in (0, 1))
    assert [[found(d, A[a], B[b]) for b in range(4)] for a in range(4)] == [[match(a, b) for b in range(4)] for a in range(4)]
    d = by["merge3"]
    assert d.merged == 2 and "out of 3 supported" in " ".join(d.out) and " 4 times" in " ".join(d.out), d.out
    assert d.entry(A[3], B[3])[1] == [(5, 4), (4, 3), (3, 2), (2, 1)]


def main():
    compile_driver()
    names = {}
    totals = np.zeros(3, dtype=np.int64)
    for name in FIXTURES:
        d = build_fixture(name)
        names[name] = {"dump": f"{name}.paths.gz", "unitig_after": f"{name}.support.unitig.gz"}
        print(name, d.counts(), "merged", d.merged, "cleared flags", sum(f.count(0) for _, _, f in d.entries))
        totals += d.counts()
    with open(os.path.join(HERE, "paths.json"), "w") as f:
        json.dump(names, f, indent=1)
    kept, A, B = hand_cases(np.random.default_rng(20241101))
    check_cases(kept, A, B)
    for _, d in kept:
        totals += d.counts()
    assert (totals > 0).all(), totals
    with gzip.GzipFile(os.path.join(HERE, "paths_cases.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps([c for c, _ in kept], indent=0).encode())
    assert os.path.getsize(os.path.join(HERE, "paths_cases.json.gz")) < (1 << 20)


if __name__ == "__main__":
    main()
