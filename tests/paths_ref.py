"""Plain-Python restatement of the mate-pair path definitions
(include/mg_overlap.h, "mate-pair path support") and the inputs the path tests
share.

  explore      exploreGraph (OverlapGraph.cpp:1781-1870), recursive as the
               reference is, its statics as attributes;
  entry        findPathBetweenMatepairs (:1645-1730) for one mate entry;
  restate      the loop of :1904-1916: per mate entry (status, work units, path,
               flags);
  pair_list    listOfPairedEdges before the sort (:1929-1964) and the three
               counters, by the reference's linear search;
  merge_order  std::sort's permutation is taken from the library (the same
               libstdc++ algorithm); the loop of :1972-1992 is restated over it.
All arithmetic is masked to 64 bits where the reference's wraps."""
import functools
import gzip
import json
import os
import sys

import numpy as np

from conftest import GOLDEN
from metagenomics_amd.overlap import (CONTIG_EDGE_DTYPE, MATE_DTYPE, PAIR_DTYPE, PATH_FOUND, PATH_NONE, PATH_SAME_EDGE,
                                      PATH_SKIPPED, PLACE_DTYPE)

M64 = (1 << 64) - 1
sys.setrecursionlimit(10000)


def match_edge_type(a, b):
    return (a in (1, 3) and b in (2, 3)) or (a in (0, 2) and b in (0, 1))


class Search:
    """One graph: edges[k] = (src, dst, offset, orient) in u order, twin[k]."""

    def __init__(self, edges, twin):
        self.src = [int(x) for x in edges["src"]]
        self.dst = [int(x) for x in edges["dst"]]
        self.off = [int(x) for x in edges["offset"]]
        self.ori = [int(x) for x in edges["orient"]]
        self.twin = [int(x) for x in twin]
        assert all(a <= b for a, b in zip(self.src, self.src[1:]))
        self.adj = {}
        for k, s in enumerate(self.src):
            self.adj.setdefault(s, []).append(k)
        self.units = 0

    def explore(self, first, last, d1, d2, bhi, blo, level, fp, flags):
        if level == 0:
            self.found = 0
            del fp[:], flags[:]
            self.loe, self.pl = [], []
        else:
            del self.loe[level:], self.pl[level:]
        if level > 100:
            return 0
        if level == 0:
            self.loe.append(first)
            self.pl.append(d1)
        else:
            total = (d2 + self.pl[level - 1]) & M64
            if first == last and blo <= total <= bhi:
                self.loe.append(first)
                self.pl.append(total)
                self.found += 1
                if self.found == 1:
                    fp[:] = self.loe
                    flags[:] = [1] * (len(self.loe) - 1)
                else:
                    for i in range(len(fp) - 1):
                        self.units += 1
                        if not any(fp[i] == self.loe[j] and fp[i + 1] == self.loe[j + 1] for j in range(len(self.loe) - 1)):
                            flags[i] = 0
                return 1
            self.loe.append(first)
            self.pl.append((d1 + self.pl[level - 1]) & M64)
        for nxt in self.adj.get(self.dst[first], []):
            self.units += 1
            if match_edge_type(self.ori[first], self.ori[nxt]) and self.pl[level] < bhi:
                self.explore(nxt, last, self.off[nxt], d2, bhi, blo, level + 1, fp, flags)
        return self.found

    def entry(self, list1, list2, mean, sd):
        """list1 / list2 = [(edge, location)] of read1 / read2; (found, path, flags); found = False: same edge"""
        self.units = 0
        if not list1 or not list2:
            return False, [], []
        for e1, _ in list1:
            for e2, _ in list2:
                self.units += 1
                if e1 == e2 or e1 == self.twin[e2]:
                    return False, [], []
        bhi, blo = (mean + 3 * sd) & M64, (mean - 3 * sd) & M64
        cp, cf, fp, ff = [], [], [], []
        for e1, loc1 in list1:
            for e2, loc2 in list2:
                d1, d2 = (self.off[e1] - loc1) & M64, loc2
                if (d1 + d2) & M64 < bhi:
                    if self.explore(e1, e2, d1, d2, bhi, blo, 0, fp, ff) > 0:
                        if not cp:
                            cp, cf = list(fp), list(ff)
                        else:
                            for k in range(len(cp) - 1):
                                self.units += 1
                                if not any(cp[k] == fp[l] and cp[k + 1] == fp[l + 1] and ff[l] == 1
                                           for l in range(len(fp) - 1)):
                                    cf[k] = 0
        return True, cp, cf


def split_lists(pstart, precs):
    """per read ID: (forward list, reverse list) of (edge, location) in CSR order"""
    out = []
    for a in range(len(pstart) - 1):
        r = precs[int(pstart[a]):int(pstart[a + 1])]
        out.append(([(int(p["edge"]), int(p["distance"])) for p in r if int(p["flags"]) & 1],
                    [(int(p["edge"]), int(p["distance"])) for p in r if not int(p["flags"]) & 1]))
    return out


def restate(edges, twin, places, mates, mean, sd):
    """[(status, units, path, flags)] per mate entry in (A, j) order"""
    s = Search(edges, twin)
    lists = split_lists(*places)
    mstart, mrecs = mates
    out = []
    for a in range(1, len(mstart) - 1):
        for m in range(int(mstart[a]), int(mstart[a + 1])):
            b, o, d = int(mrecs["id"][m]), int(mrecs["orient"][m]), int(mrecs["dataset"][m])
            if a > b or int(mean[d]) == 0:
                out.append((PATH_SKIPPED, 0, [], []))
                continue
            l1 = lists[a][0] if o in (2, 3) else lists[a][1]
            l2 = lists[b][0] if o in (0, 2) else lists[b][1]
            ok, path, flags = s.entry(l1, l2, int(mean[d]), int(sd[d]))
            out.append((PATH_SAME_EDGE if not ok else PATH_FOUND if path else PATH_NONE, s.units, path, flags))
    return out


def pair_list(edges, twin, entries):
    """([(edge1, edge2, support)] in first-seen order, (noPathsFound, pathsFound, mpOnSameEdge))"""
    src, dst = edges["src"], edges["dst"]
    pairs, counters = [], [0, 0, 0]
    for status, _, path, flags in entries:
        if status == PATH_NONE:
            counters[0] += 1
        elif status == PATH_FOUND:
            counters[1] += 1
        elif status == PATH_SAME_EDGE:
            counters[2] += 1
        for k, f in enumerate(flags):
            if f != 1:
                continue
            a, b = path[k], path[k + 1]
            for p in pairs:
                if (p[0] == a and p[1] == b) or (int(twin[p[1]]) == a and int(twin[p[0]]) == b):
                    p[2] += 1
                    break
            else:
                if src[a] != dst[a] or src[b] != dst[b]:
                    pairs.append([a, b, 1])
    return [tuple(p) for p in pairs], tuple(counters)


def entries_of(ps):
    """a PathSupport as restate's rows"""
    return [(int(st), int(v), p, f) for st, v, (p, f) in zip(ps.status, ps.visits, ps.paths())]


def pairs_of(ps):
    return [(int(p["edge1"]), int(p["edge2"]), int(p["support"])) for p in ps.pairs]


# ---- synthetic inputs

def random_case(rng, n_nodes, n_records, n_list_reads, mates_per_read, n_datasets=2, min_off=25, max_off=60,
                max_mean=160, max_sd=30, self_loops=1):
    """A random graph with twins in u order, reads placed on its edges in both
    list kinds, and a mate CSR.  Returns a dict of mate_paths' arguments.  The
    search is exponential in (mean + 3 sd) / offset: the defaults keep a path
    below some 10 edges, so an entry costs at most some 10^5 work units."""
    recs = []  # (src, dst, orient, offset, creation index); the twin of record 2i is 2i + 1
    for i in range(n_records):
        u, v = int(rng.integers(1, n_nodes + 1)), int(rng.integers(1, n_nodes + 1))
        if i < self_loops:
            v = u
        o, off = int(rng.integers(0, 4)), int(rng.integers(min_off, max_off + 1))
        recs.append((u, v, o, off))
        recs.append((v, u, {0: 3, 3: 0}.get(o, o), int(rng.integers(min_off, max_off + 1))))
    order = sorted(range(len(recs)), key=lambda k: recs[k][0])  # stable: list order = creation order
    where = {k: i for i, k in enumerate(order)}
    edges = np.zeros(len(recs), dtype=CONTIG_EDGE_DTYPE)
    twin = np.zeros(len(recs), dtype=np.uint32)
    for i, k in enumerate(order):
        s, d, o, off = recs[k]
        edges[i] = (s, d, off, 0, 0, 0, o)
        twin[i] = where[k ^ 1]
    n = n_nodes + n_list_reads
    lists = [[] for _ in range(n + 2)]
    for r in range(1, n + 1):
        for _ in range(int(rng.integers(0, 4))):
            k = int(rng.integers(0, len(recs)))
            lists[r].append((k, int(rng.integers(0, 2)), int(rng.integers(0, int(edges["offset"][k]) + 5))))
    pstart = np.zeros(n + 2, dtype=np.uint64)
    pstart[1:] = np.cumsum([len(x) for x in lists[:-1]])
    flat = [p for x in lists for p in x]
    precs = np.zeros(len(flat), dtype=PLACE_DTYPE)
    if flat:
        precs["edge"], precs["flags"], precs["distance"] = (np.array(c, dtype=np.uint64) for c in zip(*flat))
    mstart = np.zeros(n + 2, dtype=np.uint64)
    ms = []
    for a in range(1, n + 1):
        mstart[a] = len(ms)
        for _ in range(mates_per_read(a) if callable(mates_per_read) else mates_per_read):
            ms.append((int(rng.integers(1, n + 1)), int(rng.integers(0, 4)), int(rng.integers(0, n_datasets)), 0))
    mstart[n + 1] = len(ms)
    mrecs = np.array(ms, dtype=MATE_DTYPE) if ms else np.zeros(0, dtype=MATE_DTYPE)
    mean = rng.integers(0, max_mean + 1, n_datasets).astype(np.uint64)
    sd = rng.integers(0, max_sd + 1, n_datasets).astype(np.uint64)
    return {"n_reads": n, "edges": edges, "twin": twin, "places": (pstart, precs), "mates": (mstart, mrecs),
            "mean": mean, "sd": sd}


def host_args(c):
    return (c["n_reads"], c["edges"], c["twin"], c["places"], c["mates"], c["mean"], c["sd"])


# ---- goldens (tests/golden/make_paths_golden.py)

class Golden:
    """One dump of the reference driver (tests/golden/ref_paths_main.cpp)."""

    def __init__(self, name, l, pe, se, dump, unitig=None, unitig_after=None):
        self.name, self.l, self.pe, self.se, self.unitig, self.unitig_after = name, l, pe, se, unitig, unitig_after
        rows = [ln.split(" ") for ln in dump.splitlines()]
        self.n = int(next(t[1] for t in rows if t[0] == "#N"))
        self.lens = np.zeros(self.n, dtype=np.uint16)
        mates = [[] for _ in range(self.n + 2)]
        fwd = [[] for _ in range(self.n + 2)]
        rev = [[] for _ in range(self.n + 2)]
        edges, twin, mean, sd = [], [], [], []
        lreads, loffs, lors = [], [], []
        self.entries, self.stdout, self.graph_after, self.merged = [], [], [], None
        for t in rows:
            if t[0] == "#R":
                self.lens[int(t[1]) - 1] = int(t[3])
            elif t[0] == "#M":
                mates[int(t[1])].append((int(t[2]), int(t[3]), int(t[4]), 0))
            elif t[0] == "#E":
                assert int(t[1]) == len(edges)
                lst = [tuple(map(int, x.split(":"))) for x in t[7:] if x]
                assert len(lst) == int(t[6])
                edges.append((int(t[2]), int(t[3]), int(t[5]), len(lreads), len(lst), 0, int(t[4])))
                lreads += [x[0] for x in lst]
                loffs += [x[1] for x in lst]
                lors += [x[2] for x in lst]
            elif t[0] == "#T":
                assert int(t[1]) == len(twin)
                twin.append(int(t[2]))
            elif t[0] == "#L":
                (fwd if t[1] == "F" else rev)[int(t[2])].append((int(t[3]), 1 if t[1] == "F" else 0, int(t[4])))
            elif t[0] == "#D":
                mean.append(int(t[2])), sd.append(int(t[3]))
            elif t[0] == "#P":
                assert int(t[1]) == len(self.entries)
                if t[2] == "S":
                    self.entries.append((PATH_SKIPPED, [], []))
                elif t[2] == "0":
                    self.entries.append((PATH_SAME_EDGE, [], []))
                else:
                    n = int(t[3])
                    path, bar = [int(x) for x in t[4:4 + n]], 4 + n
                    assert t[bar] == "|"
                    flags = [int(x) for x in t[bar + 1:]]
                    assert len(flags) == max(n - 1, 0)
                    self.entries.append((PATH_FOUND if n else PATH_NONE, path, flags))
            elif t[0] == "#O":
                self.stdout.append(" ".join(x for x in t[1:] if x))
            elif t[0] == "#X":
                self.merged = int(t[1])
            elif t[0] == "#G":
                self.graph_after.append(" ".join(t[1:]))
        self.edges = np.array(edges, dtype=CONTIG_EDGE_DTYPE) if edges else np.zeros(0, dtype=CONTIG_EDGE_DTYPE)
        self.twin = np.array(twin, dtype=np.uint32)
        # the edges with their read lists, as build_placements takes them
        self.graph = (self.edges, np.array(lreads, np.uint32), np.array(loffs, np.uint16), np.array(lors, np.uint8))
        self.mean, self.sd = np.array(mean, dtype=np.uint64), np.array(sd, dtype=np.uint64)
        lists = [f + r for f, r in zip(fwd, rev)]  # the forward list in list order, then the reverse list
        start = np.zeros(self.n + 2, dtype=np.uint64)
        start[1:] = np.cumsum([len(x) for x in lists[:-1]])
        flat = [p for x in lists for p in x]
        recs = np.zeros(len(flat), dtype=PLACE_DTYPE)
        if flat:
            recs["edge"], recs["flags"], recs["distance"] = (np.array(c, dtype=np.uint64) for c in zip(*flat))
        self.places = (start, recs)
        start = np.zeros(self.n + 2, dtype=np.uint64)
        start[1:] = np.cumsum([len(x) for x in mates[:-1]])
        flat = [m for x in mates for m in x]
        self.mates = (start, np.array(flat, dtype=MATE_DTYPE) if flat else np.zeros(0, dtype=MATE_DTYPE))

    def args(self):
        return (self.n, self.edges, self.twin, self.places, self.mates, self.mean, self.sd)

    def summary(self):
        """(pairs merged, supported pairs, noPathsFound, pathsFound, mpOnSameEdge) from the reference's stdout"""
        if not self.stdout:  # no mate dataset: the reference returns before any line
            return None
        first = lambda head: next(x for x in self.stdout if x.startswith(head)).split()
        line = next(x for x in self.stdout if "Pairs of Edges merged out of" in x).split()
        return (int(line[0]), int(line[7]), int(first("No paths found")[4]), int(first("Paths found")[3]),
                int(first("Total matepairs on same edge")[5]))

    def merging(self):
        """[(position, (src1, dst1, len1), (src2, dst2, len2), support)] from the reference's "Merging" lines"""
        out = []
        for x in self.stdout:
            if " Merging (" not in x and not x.startswith("Merging ("):
                continue
            v = [int(w) for w in x.replace("(", " ").replace(")", " ").replace(",", " ").split() if w.isdigit()]
            # position, src1, dst1, len1, flow1, src2, dst2, len2, flow2, support
            out.append((v[0], (v[1], v[2], v[3]), (v[5], v[6], v[7]), v[9]))
        return out

    def write_files(self, d):
        out = ([], [])
        for lst, datas, tag in ((out[0], self.pe, "p"), (out[1], self.se, "s")):
            for i, data in enumerate(datas):
                lst.append(os.path.join(str(d), f"{self.name}.{tag}{i}"))
                with open(lst[-1], "wb") as f:
                    f.write(data)
        return out


GOLDEN_FIXTURES = ("pairs_small", "pairs_mixed", "pairs_long", "pairs_branchy")


def _gz(fn):
    with gzip.open(os.path.join(GOLDEN, fn), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def golden(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        meta = json.load(f)
    with open(os.path.join(GOLDEN, "paths.json")) as f:
        files = json.load(f)[name]
    return Golden(name, meta["l"], [_gz(x) for x in meta["pe"]], [_gz(x) for x in meta["se"]],
                  _gz(files["dump"]).decode(), None, _gz(files["unitig_after"]).decode())


@functools.lru_cache(maxsize=None)
def hand_cases():
    with gzip.open(os.path.join(GOLDEN, "paths_cases.json.gz"), "rt") as f:
        cases = json.load(f)
    return {c["name"]: Golden(c["name"], c["l"], [x.encode() for x in c["pe"]], [c["se"].encode()], c["dump"],
                              c["unitig"], c["unitig_after"]) for c in cases}


def hand_case_names():
    return tuple(hand_cases())


def any_golden(name):
    return golden(name) if name in GOLDEN_FIXTURES else hand_cases()[name]


def unitig_text(g):
    """the .unitig text of the graph a dump's #E rows describe (saveGraphToFile's
    layout and choice of one edge per twin pair), for a fixture whose dump was
    taken on the build path and so has no .unitig file of its own"""
    e, (_, reads, offs, ors) = g.edges, g.graph
    out = []
    for k in range(len(e)):
        s, d = int(e["src"][k]), int(e["dst"][k])
        if not (s < d or (s == d and k < int(g.twin[k]))):
            continue
        a, n = int(e["first"][k]), int(e["n"][k])
        out += [s, d, int(e["orient"][k]), int(e["offset"][k]), n]
        for i in range(a, a + n):
            out += [int(reads[i]), int(offs[i]), int(ors[i])]
    return "".join(f"{v}\n" for v in out)


def unitig_graph(g, tmp_path):
    """the UnitigGraph a dump was taken from: its .unitig text re-read, after sortEdges"""
    from metagenomics_amd.overlap import UnitigGraph

    path = tmp_path / "case.unitig"
    path.write_text(g.unitig if g.unitig is not None else unitig_text(g))
    u = UnitigGraph.from_unitig_file(str(path), g.lens)
    u.sort_edges()
    return u


def summary_lines(g):
    """the reference's stdout after its "Merging" lines: the merged count and the five matepair counts"""
    return [x for x in g.stdout if " Merging (" not in x and not x.startswith("Merging (")]


def run_cli_support(g, tmp_path, resume, env=None):
    """mg_overlap ... -support on a golden's files (resume: its .unitig
    re-read with -s).  Returns (the summary lines, the text of <prefix>.support.unitig)."""
    import subprocess

    from conftest import ROOT

    exe = os.path.join(ROOT, "metagenomics_amd", "lib", "mg_overlap")
    pe, se = g.write_files(tmp_path)
    prefix = str(tmp_path / "out")
    cmd = [exe, "-pe", str(len(pe))] + pe + (["-se", str(len(se))] + se if se else [])
    cmd += ["-f", prefix, "-l", str(g.l), "-support"] + (["-s"] if resume else [])
    if resume:
        with open(prefix + ".unitig", "w") as f:
            f.write(g.unitig)
    p = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=120, env={**os.environ, **(env or {})})
    lines = [ln for ln in p.stdout.splitlines() if not ln.startswith("{")]
    keep = ("Pairs of Edges merged", "No paths found", "Paths found", "Total matepairs")
    with open(prefix + ".support.unitig") as f:
        return [ln for ln in lines if any(k in ln for k in keep)], f.read()
