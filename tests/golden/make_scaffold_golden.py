#!/usr/bin/env python3
"""Generate the scaffolder fixtures in tests/golden/ from the REFERENCE itself.

Compiles tests/golden/ref_scaffold_main.cpp against the reference's own sources
(in place, as make_paths_golden.py does) into the ignored oracle/_ref/ref_scaffold
and stores what the reference's calculateMeanAndSdOfInsertSize and scaffolder()
leave (the driver's dump: reads, mate lists, every edge with its twin, every
read's location lists in list order, mean / SD per dataset, every "are
supported" line, the return value, the lists after the merge) and the .unitig
file saved after it:

  pairs_<name>.scaffold.gz            the build path on the four mate-pair
  pairs_branchy.scaffold.unitig.gz    fixtures (the other three hold one edge
  scaffold.json                       and its twin: nothing is counted)
  scaffold_cases.json.gz              hand cases on the resume path: 300 reads
                                      of 30 bp, l = 10, inline

listOfPairedEdges is a local of the reference, so only records of support >=
minimumSupport (3) that no earlier merge freed are observable, as a line.  Each
hand case therefore decides between support 3 (a line) and support 2 (none),
on edge pairs that share no edge, so nothing is freed.  Every case carries the
calibration edge of make_paths_golden.py (mean 210, sd 10: the bound is 240).

All reads are 30 bp, so a read at location p on an edge of offset O lies at
O - p on the twin (readGraphFromFile :1330-1349).  A pair (a, b) written "a as
it is, b reverse-complemented" gives a's entry orient 2: a's list is its
reverse list (the twin, O - p), b's its forward list.

  bound         the third pair at dist 239 (a line) and at 240 (none)
  not_unique    the third pair's second read also lies on another edge (none)
  strand        all four orients on four edge pairs with unequal locations: the
                printed edges and average distances pin the list choice
  same_edge     both reads on one edge, same strand (L1 == L2)
  twin_edge     both reads on one edge, opposite strands (L1 == twin[L2])
  self_pair     a read paired with itself
  mean0         a second dataset without insert sizes counts nothing
  both_orients  support 3 only because (twin[L2], L1) joins (twin[L1], L2); the
                flipped pair is seen first, so the line shows the twins
  average       distances 110, 111, 113: the average 111 is 334 / 3 truncated
  connected           dst(edge1) == src(edge2) and matchEdgeType: mergeEdges
  connected_mismatch  the same node shared, orientations 3 and 0: the
                      disconnected merge
  overlap10 / overlap9 / no_overlap / overlap29
                      crafted node reads round findOverlap's limits (10 is
                      found, 9 is not, 29 = length - 1), once on the forward
                      strands (orientations 3, 3) and once on the reverse strands
                      (orientations 2, 1)
  offset16      an edge of offset 70,000: the UINT16 truncations of its twin's
                list and of offset - sum in the merged list
  freed         a supported pair freed through an edge, and one through a twin
  ties20        20 disjoint pairs of support 3 and three of 4: the ranks pin
                std::sort's permutation of equal supports
Asserted over all fixtures together: a disconnected and a connected merge, a
freed pair, an entry of each status (the statuses by the restatement of
tests/scaffold_ref.py over the dumps, in tests/test_scaffold_host.py: the
reference does not print them).
Not producible by the reference, covered against the plain-Python restatement
only: a read whose forward and reverse lists differ in length (so "unique on
one strand only": every placement of a read on an edge is one on its twin on
the other strand, so the second half of not_unique, a second placement on the
other strand only, cannot be built), orient > 3, dataset 255, sums near 2^64.

Only runs where the reference tree is present.  No test runs this.
Usage: python tests/golden/make_scaffold_golden.py [reference dir]
"""
from __future__ import annotations

import gzip
import json
import os
import re
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
DRIVER = os.path.join(ROOT, "oracle", "_ref", "ref_scaffold")
REF_SRCS = ["Dataset.cpp", "Edge.cpp", "HashTable.cpp", "OverlapGraph.cpp", "Read.cpp"]
COMP = str.maketrans("ACGT", "TGCA")
FIXTURES = ("pairs_small", "pairs_mixed", "pairs_long", "pairs_branchy")
LINE = re.compile(r"\s*(\d+) \(\s*(\d+),\s*(\d+)\) Length:\s*(\d+) Flow:\s*(\d+) and \(\s*(\d+),\s*(\d+)\) Length:\s*(\d+) "
                  r"Flow:\s*(\d+) are supported\s*(\d+) times. Average distance:\s*(\d+)")


def rc(s: str) -> str:
    return s.translate(COMP)[::-1]


def compile_driver():
    os.makedirs(os.path.dirname(DRIVER), exist_ok=True)
    subprocess.run(["g++", "-std=gnu++98", "-O2", "-w", f"-I{REF}", "-o", DRIVER,
                    os.path.join(HERE, "ref_scaffold_main.cpp")] + [os.path.join(REF, s) for s in REF_SRCS], check=True)


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
        self.n_edges = sum(t[0] == "#E" for t in rows)
        self.n_after = sum(t[0] == "#G" for t in rows)
        self.datasets = [(int(t[2]), int(t[3])) for t in rows if t[0] == "#D"]
        self.merged = int(next(t[1] for t in rows if t[0] == "#X"))
        self.after = [(int(t[1]), int(t[2]), int(t[3]), int(t[4])) for t in rows if t[0] == "#G"]
        self.lines = []  # (rank, (src1, dst1), (src2, dst2), support, average distance)
        for ln in text.splitlines():
            if ln.startswith("#O "):
                v = [int(x) for x in LINE.match(ln[3:]).groups()]
                assert v[4] == 0 and v[8] == 0, ln  # Flow 0
                self.lines.append((v[0], (v[1], v[2]), (v[5], v[6]), v[9], v[10]))

    def supported(self):
        return sorted((e1, e2, s, d) for _, e1, e2, s, d in self.lines)


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
    gz_write(f"{name}.scaffold.gz", dump)
    files = {"dump": f"{name}.scaffold.gz"}
    if name == "pairs_branchy":
        gz_write(f"{name}.scaffold.unitig.gz", after)
        files["unitig_after"] = f"{name}.scaffold.unitig.gz"
    return files, Dump(dump)


# ---- hand cases: 300 reads of 30 bp; IDs 1..228 are nodes, 234..265 first reads (A), 266..300 second reads (B)
N_READS, LEN = 300, 30
K1, K2, K3, CAL_U, CAL_V = 231, 232, 233, 229, 230  # the calibration edge and its reads
O = 300  # the offset of every case edge


def find_overlap(s1, s2):
    """findOverlap (OverlapGraph.cpp:2368-2379)"""
    for i in range(min(len(s1), len(s2)) - 1, 9, -1):
        if s1[-i:] == s2[:i]:
            return i
    return 0


OVERLAPS = (("overlap10", 10, 10), ("overlap9", 9, 0), ("no_overlap", 0, 0), ("overlap29", 29, 29))


def hand_cases(rng):
    rand = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, n))
    while True:  # the crafted node reads of the findOverlap cases must get IDs no other role uses
        crafted = {}
        for name, k, want in OVERLAPS:  # P's last k bases are Q's first k; findOverlap(P, Q) = want
            while True:
                P = rand(LEN)
                Q = (P[-k:] if k else "") + rand(LEN - k)
                if P == min(P, rc(P)) and Q == min(Q, rc(Q)) and P != Q and find_overlap(P, Q) == want and \
                        find_overlap(rc(Q), rc(P)) == want and (k == 0 or P[-k:] == Q[:k]):
                    break
            crafted[name] = (P, Q)
        canon = {x for pq in crafted.values() for x in pq}
        while len(canon) < N_READS:
            s = rand(LEN)
            canon.add(min(s, rc(s)))
        read = [None] + sorted(canon)  # read[id] = the canonical string
        ids = {name: (read.index(P), read.index(Q)) for name, (P, Q) in crafted.items()}
        if all(17 <= i <= 228 for pq in ids.values() for i in pq):
            break
    se = fasta(read[1:])

    def rec(src, dst, orient, offset, lst=()):
        v = [src, dst, orient, offset, len(lst)]
        for r, off, o in lst:
            v += [r, off, o]
        return "".join(f"{x}\n" for x in v)

    def edge(src, dst, placed, off=O, orient=3):
        """src -> dst (offset off) holding reads forward at the given locations: [(read, location)]"""
        lst, at = [], 0
        for r, p in sorted(placed, key=lambda x: x[1]):
            lst.append((r, p - at, 1))
            at = p
        return rec(src, dst, orient, off, lst)

    def pairs(*p):
        """(a, b): a as it is, b reverse-complemented (forward-reverse mates); (a, b, oa, ob) sets the strands"""
        out = []
        for t in p:
            a, b, oa, ob = t if len(t) == 4 else (t[0], t[1], 1, 0)
            out += [read[a] if oa else rc(read[a]), read[b] if ob else rc(read[b])]
        return fasta(out)

    cal = rec(CAL_U, CAL_V, 3, 2000, [(K1, 100, 1), (K2, 200, 1), (K3, 20, 1)])  # insert sizes 200 and 220
    cal_pairs = [(K2, K1), (K3, K1)]
    A, B = list(range(234, 266)), list(range(266, 301))
    cases = []

    def case(name, unitig, pe, expect, merged=None, datasets=((210, 10),), after=()):
        """after: (src, dst, orient, offset) of edges the graph must hold after the merge"""
        cases.append({"name": name, "unitig": cal + unitig, "pe": pe, "expect": sorted(expect),
                      "expect_merged": len(expect) if merged is None else merged, "expect_datasets": list(datasets),
                      "expect_after": list(after)})

    def group(k, locs_a, locs_b, a0=0, off=O):
        """edges (4k+1 -> 4k+2) holding A[a0 ..] at locs_a and (4k+3 -> 4k+4) holding B[a0 ..] at locs_b"""
        n = 4 * k
        return (edge(n + 1, n + 2, [(A[a0 + i], p) for i, p in enumerate(locs_a)], off) +
                edge(n + 3, n + 4, [(B[a0 + i], p) for i, p in enumerate(locs_b)], off))

    # a's entry (orient 2): dist = (O - location of a) + location of b
    case("bound", group(0, [240, 230, 100], [50, 40, 39]) + group(1, [240, 230, 100], [50, 40, 40], 3),
         [pairs(*cal_pairs, *[(A[i], B[i]) for i in range(6)])],
         [((1, 2), (3, 4), 3, (110 + 110 + 239) // 3)])  # 5 -> 6 and 7 -> 8: the third pair is at 240
    case("not_unique", group(0, [240, 230, 220], [50, 40, 30]) + group(1, [240, 230, 220], [50, 40, 30], 3) +
         edge(9, 10, [(B[5], 20)]),
         [pairs(*cal_pairs, *[(A[i], B[i]) for i in range(6)])],
         [((1, 2), (3, 4), 3, (110 + 110 + 110) // 3)])
    # edges of offset 200, so all four list choices stay under the bound: A at 90, 80, 70 (110, 120, 130 on the
    # twin), B at 99, 98, 97 (101, 102, 103 on the twin); every choice gives other edges and another average
    st, sp, se_ = "", [], []
    for k, (oa, ob) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        st += group(k, [90, 80, 70], [99, 98, 97], 3 * k, off=200)
        sp += [(A[3 * k + i], B[3 * k + i], oa, ob) for i in range(3)]
        n = 4 * k
        e1, d1 = ((n + 2, n + 1), 90 + 80 + 70) if oa == 0 else ((n + 1, n + 2), 110 + 120 + 130)
        e2, d2 = ((n + 3, n + 4), 99 + 98 + 97) if ob == 0 else ((n + 4, n + 3), 101 + 102 + 103)
        se_.append((e1, e2, 3, (d1 + d2) // 3))
    case("strand", st, [pairs(*cal_pairs, *sp)], se_)
    # one edge of offset 100: dist 50, 70, 90 (same strand) and 130 (opposite strands), all under the bound
    one = edge(1, 2, [(A[0], 10), (A[1], 20), (A[2], 30), (B[0], 40), (B[1], 50), (B[2], 60)], off=100)
    # (the three pairs are insert sizes of 30 themselves: 200, 220, 30, 30, 30 give mean 102, sd 88, the bound 366)
    case("same_edge", one, [pairs(*cal_pairs, *[(A[i], B[i], 0, 0) for i in range(3)])], [], datasets=((102, 88),))
    case("twin_edge", one, [pairs(*cal_pairs, *[(A[i], B[i]) for i in range(3)])], [], datasets=((102, 88),))
    # a read and itself: location p and 200 - p on the twin, dist 200
    case("self_pair", group(0, [90, 80, 70], [99, 98, 97], off=200),
         [pairs(*cal_pairs, *[(A[i], A[i]) for i in range(3)])], [])
    case("mean0", group(0, [240, 230, 220], [50, 40, 30]) + group(1, [240, 230, 220], [50, 40, 30], 3),
         [pairs(*cal_pairs, *[(A[i], B[i]) for i in range(3)]), pairs(*[(A[i], B[i]) for i in range(3, 6)])],
         [((1, 2), (3, 4), 3, 110)], datasets=((210, 10), (0, 0)))
    # A[0] lies on 3 -> 4 and B[0] on 1 -> 2: its entry (owner A[0], the lowest ID) is seen first and names the twins
    case("both_orients", edge(1, 2, [(B[0], 240), (A[1], 230), (A[2], 220)]) + edge(3, 4, [(A[0], 50), (B[1], 40), (B[2], 30)]),
         [pairs(*cal_pairs, (B[0], A[0]), (A[1], B[1]), (A[2], B[2]))],
         [((4, 3), (2, 1), 3, 110)])
    case("average", group(0, [240, 230, 220], [50, 41, 33]), [pairs(*cal_pairs, *[(A[i], B[i]) for i in range(3)])],
         [((1, 2), (3, 4), 3, 111)])
    three = lambda a0=0: pairs(*cal_pairs, *[(A[a0 + i], B[a0 + i]) for i in range(3)])
    std_a, std_b = [240, 230, 220], [50, 40, 30]  # dist 110 each
    # dst(edge1) == src(edge2): mergeEdges when matchEdgeType (3, 3), mergeEdgesDisconnected when not (3, 0)
    case("connected", edge(1, 2, [(A[i], std_a[i]) for i in range(3)]) + edge(2, 3, [(B[i], std_b[i]) for i in range(3)]),
         [three()], [((1, 2), (2, 3), 3, 110)], after=[(1, 3, 3, 600)])
    case("connected_mismatch",
         edge(1, 2, [(A[i], std_a[i]) for i in range(3)]) + edge(2, 3, [(B[i], std_b[i]) for i in range(3)], orient=0),
         [three()], [((1, 2), (2, 3), 3, 110)], after=[(1, 3, 2, 630)])
    # findOverlap between dst(edge1) and src(edge2): forward strands (orientations 3, 3), and the reverse strands
    # (orientations 2 and 1, the crafted reads in the other roles)
    for name, k, want in OVERLAPS:
        ip, iq = ids[name]
        case(name, edge(1, ip, [(A[i], std_a[i]) for i in range(3)]) + edge(iq, 4, [(B[i], std_b[i]) for i in range(3)]) +
             edge(5, iq, [(A[3 + i], std_a[i]) for i in range(3)], orient=2) +
             edge(ip, 8, [(B[3 + i], std_b[i]) for i in range(3)], orient=1),
             [pairs(*cal_pairs, *[(A[i], B[i]) for i in range(6)])],
             [((1, ip), (iq, 4), 3, 110), ((5, iq), (ip, 8), 3, 110)],
             after=[(1, 4, 3, 600 + LEN - want), (5, 8, 3, 600 + LEN - want)])
    # an edge of offset 70,000 whose twin's first list offset (69,920) and offset - sum pass 65,535; the pairs'
    # first reads are taken on their forward strand, so the record's edge1 is that twin
    case("offset16", edge(1, 2, [(A[0], 60), (A[1], 70), (A[2], 80)], off=70000) + edge(3, 4, [(B[i], std_b[i]) for i in range(3)]),
         [pairs(*cal_pairs, *[(A[i], B[i], 0, 0) for i in range(3)])], [((2, 1), (3, 4), 3, 110)])
    # support 4 on (1 -> 2, 3 -> 4) frees (1 -> 2, 5 -> 6) through an edge; support 4 on (9 -> 10, 11 -> 12) frees
    # (10 -> 9, 13 -> 14) through a twin: four records of support >= 3, two lines
    four_a, four_b = [240, 230, 220, 210], [50, 40, 30, 20]
    case("freed",
         edge(1, 2, [(A[i], four_a[i]) for i in range(4)] + [(A[4 + i], 239 - 10 * i) for i in range(3)]) +
         edge(3, 4, [(B[i], four_b[i]) for i in range(4)]) + edge(5, 6, [(B[4 + i], std_b[i]) for i in range(3)]) +
         edge(9, 10, [(A[7 + i], four_a[i]) for i in range(4)] + [(A[11 + i], std_b[i]) for i in range(3)]) +
         edge(11, 12, [(B[7 + i], four_b[i]) for i in range(4)]) + edge(13, 14, [(B[11 + i], std_b[i]) for i in range(3)]),
         [pairs(*cal_pairs, *[(A[i], B[i]) for i in range(11)], *[(A[11 + i], B[11 + i], 0, 0) for i in range(3)])],
         [((1, 2), (3, 4), 4, 110), ((9, 10), (11, 12), 4, 110)])
    # 20 disjoint pairs of support 3 and 3 of support 4 (the 5th, 12th and 19th group): std::sort leaves its
    # insertion sort above 16 elements, so the printed ranks pin its permutation of equal supports
    TA, TB = list(range(93, 165)), list(range(165, 229)) + list(range(266, 274))
    tu, tp, te, at = "", [], [], 0
    for k in range(23):
        m = 4 if k in (4, 11, 18) else 3
        n = 4 * k
        tu += edge(n + 1, n + 2, [(TA[at + i], four_a[i]) for i in range(m)]) + \
            edge(n + 3, n + 4, [(TB[at + i], four_b[i]) for i in range(m)])
        tp += [(TA[at + i], TB[at + i]) for i in range(m)]
        te.append(((n + 1, n + 2), (n + 3, n + 4), m, 110))
        at += m
    case("ties20", tu, [pairs(*cal_pairs, *tp)], te)
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
        print(c["name"], d.datasets, "merged", d.merged, d.supported())
        assert d.datasets == [tuple(x) for x in c.pop("expect_datasets")], (c["name"], d.datasets)
        want = [(tuple(e1), tuple(e2), s, a) for e1, e2, s, a in c.pop("expect")]
        assert d.supported() == want, (c["name"], d.supported(), want)
        assert d.merged == c.pop("expect_merged"), (c["name"], d.merged)
        for e in c.pop("expect_after"):
            assert tuple(e) in d.after, (c["name"], e, d.after)
        kept.append(c)
    ranks = [x[0] for x in Dump(kept[-1]["dump"]).lines]
    assert kept[-1]["name"] == "ties20" and sorted(ranks) == list(range(1, 24)), ranks
    return kept


def main():
    compile_driver()
    names = {}
    for name in FIXTURES:
        names[name], d = build_fixture(name)
        print(name, "edges", d.n_edges, "->", d.n_after, "merged", d.merged, "ranks", [x[0] for x in d.lines],
              "supports", [x[3] for x in d.lines])
        if name == "pairs_branchy":
            assert (d.n_edges, d.n_after, d.merged) == (142, 122, 10) and d.lines[0][3] == 37
            assert [x[0] for x in d.lines] != list(range(1, d.merged + 1))  # a supported pair was freed
        else:
            assert d.merged == 0 and not d.lines
    with open(os.path.join(HERE, "scaffold.json"), "w") as f:
        json.dump(names, f, indent=1)
    kept = hand_cases(np.random.default_rng(20241101))
    with gzip.GzipFile(os.path.join(HERE, "scaffold_cases.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(kept, indent=0).encode())
    assert os.path.getsize(os.path.join(HERE, "scaffold_cases.json.gz")) < (1 << 20)


if __name__ == "__main__":
    main()
