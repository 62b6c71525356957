"""Plain-Python restatement of the three placement definitions
(include/mg_overlap.h) and the inputs the placement tests share.

  placements   updateReadLocations (OverlapGraph.cpp:1048-1071) of every edge:
               entry i of edge k places reads[first + i] at D = the sum of
               offs[first .. first + i], forward iff ors[first + i] == 1;
  insert sizes the quadruple loop of :1140-1179: read A, each mate entry (B, d),
               each placement p of A and q of B on one edge with 0 < p.D - q.D <
               1000; count, sum and sum of squares per dataset, mod 2^64;
  coverage     getBaseByBaseCoverage (:2722-2792): counters c[0 .. L], L = offset
               + len(dst); += frequency over [D, D + len); intervals of reads
               with more than one forward placement zeroed; source and
               destination spans zeroed; count / sum / sum of squares over the
               non-zero counters.
mean_sd finishes either as the reference does."""
import functools
import gzip
import json
import math
import os
import subprocess

import numpy as np

from conftest import GOLDEN
from metagenomics_amd.overlap import CONTIG_EDGE_DTYPE, MATE_DTYPE, PLACE_DTYPE

M64 = (1 << 64) - 1


class Invalid(Exception):
    """where the reference's at() would throw, or a read ID out of range"""

    def __init__(self, edge, entry=None):
        super().__init__(f"edge {edge}" + ("" if entry is None else f", list entry {entry}"))
        self.edge, self.entry = edge, entry


def placements(n_reads, edges, reads, offs, ors):
    """per read ID (0 .. n_reads + 1): [(edge, forward, distance)] in ascending (edge, position)"""
    out = [[] for _ in range(n_reads + 2)]
    for k, e in enumerate(edges):
        d, a = 0, int(e["first"])
        for i in range(int(e["n"])):
            d += int(offs[a + i])
            r = int(reads[a + i])
            if r < 1 or r > n_reads:
                raise Invalid(k, i)
            out[r].append((k, 1 if int(ors[a + i]) == 1 else 0, d))
    return out


def csr_of(lists):
    """(start uint64[n + 2], records): the layout mg_copy_placements gives
    (lists = the n + 2 per-ID lists; the last is empty, so start[n + 1] = total)"""
    assert not lists[0] and not lists[-1]
    start = np.zeros(len(lists), dtype=np.uint64)
    start[1:] = np.cumsum([len(x) for x in lists[:-1]])
    flat = [p for x in lists for p in x]
    recs = np.zeros(len(flat), dtype=PLACE_DTYPE)
    if flat:
        recs["edge"], recs["flags"], recs["distance"] = (np.array(c, dtype=np.uint64) for c in zip(*flat))
    return start, recs


def lists_of(start, recs):
    """the inverse of csr_of"""
    return [[(int(p["edge"]), int(p["flags"]), int(p["distance"])) for p in recs[int(start[a]):int(start[a + 1])]]
            for a in range(len(start) - 1)] + [[]]


def insert_size_sums(place_lists, mate_start, mates, n_datasets, max_distance=1000):
    sums = [[0, 0, 0] for _ in range(n_datasets)]
    n = len(place_lists) - 2
    for a in range(1, n + 1):
        for m in range(int(mate_start[a]), int(mate_start[a + 1])):
            b, d = int(mates["id"][m]), int(mates["dataset"][m])
            for (ke, _, pd) in place_lists[a]:
                for (le, _, qd) in place_lists[b]:
                    if ke == le and pd > qd and pd - qd < max_distance:
                        x = pd - qd
                        sums[d][0] += 1
                        sums[d][1] = (sums[d][1] + x) & M64
                        sums[d][2] = (sums[d][2] + x * x) & M64
    return np.array(sums, dtype=np.uint64).reshape(n_datasets, 3)


def edge_coverage(lens, freq, edges, reads, offs, ors):
    n = len(lens)
    fwd = [sum(1 for p in x if p[1]) for x in placements(n, edges, reads, offs, ors)]
    out = np.zeros((len(edges), 3), dtype=np.uint64)
    for k, e in enumerate(edges):
        src, dst = int(e["src"]), int(e["dst"])
        if src < 1 or src > n or dst < 1 or dst > n:
            raise Invalid(k)
        L = int(e["offset"]) + int(lens[dst - 1])
        c = [0] * (L + 1)
        a, d, spans = int(e["first"]), 0, []
        for i in range(int(e["n"])):
            d += int(offs[a + i])
            r = int(reads[a + i])
            if d + int(lens[r - 1]) > L + 1:
                raise Invalid(k, i)
            spans.append((d, d + int(lens[r - 1]), r))
        if int(lens[src - 1]) > L + 1:
            raise Invalid(k)
        if not spans:
            continue
        for lo, hi, r in spans:
            for j in range(lo, hi):
                c[j] += int(freq[r - 1])
        for lo, hi, r in spans:
            if fwd[r] > 1:
                for j in range(lo, hi):
                    c[j] = 0
        for j in range(int(lens[src - 1])):
            c[j] = 0
        for j in range(int(lens[dst - 1])):
            c[len(c) - 1 - j] = 0
        nz = [x for x in c if x]
        out[k] = (len(nz), sum(nz) & M64, sum(x * x for x in nz) & M64)
    return out


def mean_sd(count, total, sumsq):
    if not count:
        return 0, 0, 0
    mean = total // count
    var = (sumsq - 2 * mean * total + count * mean * mean) & M64
    return mean, int(math.sqrt(float(var // count))), count


# ---- synthetic inputs

def make_edges(lists, src_dst_offset):
    """lists: per edge [(read, off, orient)]; src_dst_offset: per edge (src, dst, offset)"""
    edges = np.zeros(len(lists), dtype=CONTIG_EDGE_DTYPE)
    reads, offs, ors = [], [], []
    for k, (lst, (s, d, o)) in enumerate(zip(lists, src_dst_offset)):
        edges[k] = (s, d, o, len(reads), len(lst), 0, 3)
        for r, f, q in lst:
            reads.append(r), offs.append(f), ors.append(q)
    return edges, np.array(reads, np.uint32), np.array(offs, np.uint16), np.array(ors, np.uint8)


def random_graph(rng, lens, list_sizes, max_off=40):
    """Edges with the given list sizes over reads of `lens`: random reads,
    offsets and strands; offset (so L) is chosen so that every interval fits,
    with non-monotone interval ends whenever read lengths differ."""
    n = len(lens)
    lists, sdo = [], []
    for m in list_sizes:
        src, dst = int(rng.integers(1, n + 1)), int(rng.integers(1, n + 1))
        rs = rng.integers(1, n + 1, m)
        fs = rng.integers(0, max_off + 1, m)
        qs = rng.integers(0, 2, m)
        lst = list(zip(rs.tolist(), fs.tolist(), qs.tolist()))
        ends = np.cumsum(fs) + lens[rs - 1].astype(np.int64) if m else np.zeros(0, np.int64)
        need = max(int(ends.max()) - 1 if m else 0, int(lens[src - 1]) - 1, 0)  # L >= need
        L = need + int(rng.integers(0, 30))
        off = max(0, L - int(lens[dst - 1]))
        lists.append(lst)
        sdo.append((src, dst, off))
    return make_edges(lists, sdo)


def random_mates(rng, n_reads, sizes, n_datasets, near=None):
    """A mate CSR: sizes[A] entries for read A (others 0); near = (place lists):
    half of the mates are drawn from reads on one of A's edges."""
    start = np.zeros(n_reads + 2, dtype=np.uint64)
    recs = []
    by_edge = {}
    if near is not None:
        for r, lst in enumerate(near):
            for (k, _, _) in lst:
                by_edge.setdefault(k, []).append(r)
    for a in range(1, n_reads + 1):
        start[a] = len(recs)
        for _ in range(sizes.get(a, 0)):
            b = int(rng.integers(1, n_reads + 1))
            if near is not None and near[a] and rng.random() < 0.5:
                cand = by_edge[near[a][int(rng.integers(0, len(near[a])))][0]]
                b = cand[int(rng.integers(0, len(cand)))]
            recs.append((b, int(rng.integers(0, 4)), int(rng.integers(0, n_datasets)), 0))
    start[n_reads + 1] = len(recs)
    return start, np.array(recs, dtype=MATE_DTYPE) if recs else np.zeros(0, dtype=MATE_DTYPE)


# ---- goldens (tests/golden/make_places_golden.py)

class Golden:
    """One dump of the reference driver (tests/golden/ref_places_main.cpp)."""

    def __init__(self, name, l, pe, se, dump):
        self.name, self.l, self.pe, self.se = name, l, pe, se
        rows = [ln.split(" ") for ln in dump.splitlines()]
        self.n = int(next(t[1] for t in rows if t[0] == "#N"))
        self.freq = np.zeros(self.n, dtype=np.uint32)
        self.lens = np.zeros(self.n, dtype=np.uint16)
        mates = [[] for _ in range(self.n + 2)]
        lists, sdo = [], []
        self.locations = [[] for _ in range(self.n + 2)]  # (edge, forward, location), sorted
        self.stdout, self.datasets, self.coverage = [], [], []
        for t in rows:
            if t[0] == "#R":
                self.freq[int(t[1]) - 1], self.lens[int(t[1]) - 1] = int(t[2]), int(t[3])
            elif t[0] == "#M":
                mates[int(t[1])].append((int(t[2]), int(t[3]), int(t[4]), 0))
            elif t[0] == "#E":
                assert int(t[1]) == len(lists)
                sdo.append((int(t[2]), int(t[3]), int(t[5]), int(t[4])))
                lists.append([tuple(map(int, x.split(":"))) for x in t[7:]])
                assert len(lists[-1]) == int(t[6])
            elif t[0] == "#L":
                self.locations[int(t[2])].append((int(t[3]), 1 if t[1] == "F" else 0, int(t[4])))
            elif t[0] == "#O":
                self.stdout.append(" ".join(t[1:]))
            elif t[0] == "#D":
                self.datasets.append((int(t[2]), int(t[3]), int(t[4])))
            elif t[0] == "#C":
                assert t[2] != "!"
                self.coverage.append((int(t[2]), int(t[3])))
        self.locations = [sorted(x) for x in self.locations]
        self.graph = make_edges(lists, [(s, d, off) for s, d, off, _ in sdo])
        self.graph[0]["orient"] = [o for _, _, _, o in sdo]
        start = np.zeros(self.n + 2, dtype=np.uint64)
        start[1:] = np.cumsum([len(x) for x in mates[:-1]])
        flat = [m for x in mates for m in x]
        self.mates = (start, np.array(flat, dtype=MATE_DTYPE) if flat else np.zeros(0, dtype=MATE_DTYPE))

    def write_files(self, d):
        """the input files under directory d: (pe paths, se paths)"""
        out = ([], [])
        for lst, datas, tag in ((out[0], self.pe, "p"), (out[1], self.se, "s")):
            for i, data in enumerate(datas):
                lst.append(os.path.join(str(d), f"{self.name}.{tag}{i}"))
                with open(lst[-1], "wb") as f:
                    f.write(data)
        return out


GOLDEN_FIXTURES = ("pairs_small", "pairs_mixed", "pairs_long", "pairs_branchy")


@functools.lru_cache(maxsize=None)
def golden(name):
    def gz(fn):
        with gzip.open(os.path.join(GOLDEN, fn), "rb") as f:
            return f.read()

    with open(os.path.join(GOLDEN, name + ".json")) as f:
        meta = json.load(f)
    with open(os.path.join(GOLDEN, "places.json")) as f:
        dump = gz(json.load(f)[name]).decode()
    return Golden(name, meta["l"], [gz(x) for x in meta["pe"]], [gz(x) for x in meta["se"]], dump)


@functools.lru_cache(maxsize=None)
def hand_cases():
    with open(os.path.join(GOLDEN, "places_cases.json")) as f:
        cases = json.load(f)
    out = {}
    for c in cases:
        out[c["name"]] = Golden(c["name"], c["l"], [x.encode() for x in c["pe"]], [c["se"].encode()], c["dump"])
        out[c["name"]].unitig = c["unitig"]
    return out


HAND_CASES = ("pair_on_two_edges", "boundaries", "datasets", "single_and_simple", "all_inside_spans", "non_monotone",
              "reverse_entries", "self_loop")
ALL_GOLDENS = GOLDEN_FIXTURES + HAND_CASES


def any_golden(name):
    return golden(name) if name in GOLDEN_FIXTURES else hand_cases()[name]


def sorted_lists(start, recs):
    """a placement CSR as per-read sorted lists, comparable with Golden.locations"""
    return [sorted(x) for x in lists_of(start, recs)]


# ---- the CLI (mg_overlap -insert), a C++ caller of the drop-in (include/mg_api.hpp)

def run_cli_insert(g, tmp_path, resume, env=None):
    """mg_overlap ... -insert on a golden's files (resume: its .unitig re-read
    with -s).  Returns (stdout lines before the JSON line, sorted coverage rows)."""
    from conftest import ROOT

    exe = os.path.join(ROOT, "metagenomics_amd", "lib", "mg_overlap")
    pe, se = g.write_files(tmp_path)
    prefix = str(tmp_path / "out")
    cmd = [exe, "-pe", str(len(pe))] + pe + (["-se", str(len(se))] + se if se else [])
    cmd += ["-f", prefix, "-l", str(g.l), "-insert"] + (["-s"] if resume else [])
    if resume:
        with open(prefix + ".unitig", "w") as f:
            f.write(g.unitig)
    p = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=120, env={**os.environ, **(env or {})})
    lines = [ln for ln in p.stdout.splitlines() if not ln.startswith("{")]
    with open(prefix + ".coverage") as f:
        rows = sorted(tuple(map(int, ln.split())) for ln in f)
    return lines, rows


def golden_coverage_rows(g):
    """what <prefix>.coverage must hold: per edge its key and the reference's (coverageDepth, SD), twice"""
    e = g.graph[0]
    return sorted((int(x["src"]), int(x["dst"]), int(x["orient"]), int(x["offset"]), int(x["n"])) + c + c
                  for x, c in zip(e, g.coverage))


def case_unitig_graph(g, tmp_path):
    """the UnitigGraph of a hand case: its .unitig text re-read over the golden's read lengths, after sortEdges"""
    from metagenomics_amd.overlap import UnitigGraph

    path = tmp_path / "case.unitig"
    path.write_text(g.unitig)
    u = UnitigGraph.from_unitig_file(str(path), g.lens)
    u.sort_edges()
    return u


def coverage_rows_of(u, cov):
    """UnitigGraph.edge_coverage's result keyed as golden_coverage_rows keys it (one (depth, SD) pair)"""
    e = u.contig_edges(all_edges=True)[0]
    return sorted((int(x["src"]), int(x["dst"]), int(x["orient"]), int(x["offset"]), int(x["n"])) + c[:2] + c[:2]
                  for x, c in zip(e, cov))
