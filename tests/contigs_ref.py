"""Plain-Python restatement of OverlapGraph::getStringInEdge (OverlapGraph.cpp:
2009-2041) as pieces, on strings, plus the loaders the contig tests share.

An edge's string is the whole source read, one suffix per list read and a
suffix of the destination read:
  piece 0      the source read, forward strand iff orient in {2, 3};
  piece i + 1  reads[i], forward iff ors[i] == 1; prev = length of the previous
               piece's read; the strand from position prev - offs[i] on, after
               an 'N' iff offs[i] == prev;
  tail         the destination read, forward iff orient in {1, 3}, from position
               len(src) - offset (simple edge) or len(dst) - rev.offs[0].
A position outside [0, len] is what std::string::substr throws on: InvalidPiece.
"""
import gzip
import json
import os

import numpy as np

from conftest import GOLDEN, fixture_input, golden_rows, load_meta
from metagenomics_amd.overlap import CONTIG_EDGE_DTYPE, EDGE_DTYPE, Dataset, UnitigGraph

COMP = str.maketrans("ACGT", "TGCA")


def rc(s: str) -> str:
    return s.translate(COMP)[::-1]


class InvalidPiece(Exception):
    pass


def edge_string(read, src, dst, orient, offset, reads, offs, ors, tail) -> str:
    """read(id) -> forward string.  reads / offs / ors: the edge's lists; tail = rev.offs[0]."""
    r1 = read(src) if orient in (2, 3) else rc(read(src))
    out = [r1]
    prev = len(r1)
    for k, (r, off, o) in enumerate(zip(reads, offs, ors)):
        s = read(r) if o == 1 else rc(read(r))
        pos = prev - off
        if pos < 0 or pos > len(s):
            raise InvalidPiece(f"list entry {k}")
        out.append(("N" if off == prev else "") + s[pos:])
        prev = len(s)
    r2 = read(dst) if orient in (1, 3) else rc(read(dst))
    pos = len(r1) - offset if not len(reads) else len(r2) - tail
    if pos < 0 or pos > len(r2):
        raise InvalidPiece("the destination read")
    out.append(r2[pos:])
    return "".join(out)


def strings_of(read, edges, reads, offs, ors):
    """edge_string of every CONTIG_EDGE_DTYPE record."""
    out = []
    for e in edges:
        a, n = int(e["first"]), int(e["n"])
        out.append(edge_string(read, int(e["src"]), int(e["dst"]), int(e["orient"]), int(e["offset"]),
                               reads[a:a + n].tolist(), offs[a:a + n].tolist(), ors[a:a + n].tolist(), int(e["tail"])))
    return out


def split(start, data):
    return [data[int(start[k]):int(start[k + 1])].decode() for k in range(len(start) - 1)]


def contig_index():
    with open(os.path.join(GOLDEN, "contigs.json")) as f:
        return json.load(f)


def golden_file(name, key) -> bytes:
    with gzip.open(os.path.join(GOLDEN, contig_index()[name][key]), "rb") as f:
        return f.read()


def parse_estrings(text: str):
    """[(src, dst, orient, offset, nreads, string)]; string "!" = the reference threw."""
    out = []
    for ln in text.splitlines():
        f = ln.split(" ")
        out.append((int(f[0]), int(f[1]), int(f[2]), int(f[3]), int(f[4]), f[5] if len(f) > 5 else ""))
    return out


def to_edges(t: np.ndarray) -> np.ndarray:
    r = np.zeros(t.shape[0], dtype=EDGE_DTYPE)
    r["src"], r["dst"], r["orient"], r["offset"] = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
    return r


_graphs = {}


def fixture_graph(name):
    """(Dataset, UnitigGraph after sortEdges) of a fixture, built once from its golden rows."""
    if name not in _graphs:
        meta = load_meta(name)
        ds = Dataset.from_files([fixture_input(name)], meta["l"])
        g = UnitigGraph(to_edges(golden_rows(name)), ds.packed()[1], meta["l"])
        g.sort_edges()
        _graphs[name] = (ds, g)
    return _graphs[name]


def hand_cases():
    with open(os.path.join(GOLDEN, "contig_cases.json")) as f:
        return json.load(f)


def case_graph(case, tmp_path):
    """(Dataset, UnitigGraph after sortEdges) of a hand case: its reads and its .unitig file re-read."""
    fa, un = tmp_path / "reads.fa", tmp_path / "g.unitig"
    fa.write_text(case["fasta"])
    un.write_text(case["unitig"])
    ds = Dataset.from_files([str(fa)], case["l"])
    g = UnitigGraph.from_unitig_file(str(un), ds.packed()[1])
    g.sort_edges()
    return ds, g


def ulists_edges(name, lens):
    """Every edge of the golden .ulists dump (the reference's own lists before
    sortEdges) as CONTIG_EDGE_DTYPE records with `tail` taken from the twin:
    the edge dst -> src with the twin orientation, the reverse offset and the
    reversed read list."""
    meta = load_meta(name)
    with gzip.open(os.path.join(GOLDEN, meta["unitig"]["lists_file"]), "rt") as f:
        rows = [ln.split() for ln in f if ln[0].isdigit()]
    parsed = []
    for r in rows:
        lst = [tuple(map(int, x.split(":"))) for x in r[5:]]
        parsed.append((int(r[0]), int(r[1]), int(r[2]), int(r[3]), lst))
    twin_orient = {0: 3, 1: 1, 2: 2, 3: 0}
    by_key = {}
    for u, v, o, off, lst in parsed:
        by_key.setdefault((u, v, o, off, tuple(x[0] for x in lst)), []).append(lst)
    edges = np.zeros(len(parsed), dtype=CONTIG_EDGE_DTYPE)
    reads, offs, ors = [], [], []
    for k, (u, v, o, off, lst) in enumerate(parsed):
        tail = 0
        if lst:
            roff = off + int(lens[v - 1]) - int(lens[u - 1])
            twins = by_key[(v, u, twin_orient[o], roff, tuple(x[0] for x in reversed(lst)))]
            assert len({t[0][1] for t in twins}) == 1
            tail = twins[0][0][1]
        edges[k] = (u, v, off, len(reads), len(lst), tail, o)
        for r, d, q in lst:
            reads.append(r), offs.append(d), ors.append(q)
    return edges, np.array(reads, np.uint32), np.array(offs, np.uint16), np.array(ors, np.uint8)


# ---- a three-read set and every form of an invalid piece (host and device tests)

LENS = np.array([40, 50, 30], dtype=np.uint16)
WORDS = np.arange(1, 7, dtype=np.uint64).reshape(3, 2) << np.uint64(40)


def one_edge(src, dst, orient, offset, lst=(), tail=0):
    e = np.zeros(1, dtype=CONTIG_EDGE_DTYPE)
    e[0] = (src, dst, offset, 0, len(lst), tail, orient)
    return (e, np.array([x[0] for x in lst], np.uint32), np.array([x[1] for x in lst], np.uint16),
            np.array([x[2] for x in lst], np.uint8))


INVALID = {
    "simple_offset_past_source": one_edge(1, 2, 3, 41),              # len1 - offset < 0
    "simple_tail_longer_than_dst": one_edge(2, 3, 3, 10),            # len1 - offset = 40 > len2 = 30
    "list_offset_past_prev": one_edge(1, 2, 3, 60, [(3, 41, 1)], 5),  # prev - off < 0
    "list_read_shorter_than_gap": one_edge(2, 1, 3, 60, [(3, 10, 1)], 5),  # prev - off = 40 > 30
    "second_list_entry": one_edge(1, 2, 3, 60, [(2, 10, 1), (3, 51, 0)], 5),
    "composite_tail_past_dst": one_edge(1, 3, 3, 60, [(2, 10, 1)], 31),  # rev.offs[0] > len2
    "src_zero": one_edge(0, 2, 3, 10),
    "dst_past_n": one_edge(1, 4, 3, 10),
    "list_read_zero": one_edge(1, 2, 3, 60, [(0, 10, 1)], 5),
    "list_read_past_n": one_edge(1, 2, 3, 60, [(4, 10, 1)], 5),
}
