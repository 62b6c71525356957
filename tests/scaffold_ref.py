"""Plain-Python restatement of the scaffolder's scoring half
(include/mg_overlap.h, "scaffolder"; OverlapGraph.cpp:2120-2195) and the inputs
the scaffold tests share.

  restate      the loop of :2130-2195: per mate entry its status, and
               listOfPairedEdges before the sort, by the reference's linear
               search (:2166-2191) -- not by a key, so it also checks the
               canonical key the library uses;
  random_case  a random twin table, placement CSR and mate CSR;
  golden / hand_cases / run_cli_scaffold / assert_graph_after
               the reference's own scaffolder() runs (tests/golden/
               make_scaffold_golden.py): inputs, lines character for character,
               return value, lists and .unitig after the merge.  The merge has
               no restatement here: the library's is compared with the
               reference directly.
All arithmetic is masked to 64 bits where the reference's wraps."""
import functools
import gzip
import json
import os
import re

import numpy as np

from conftest import GOLDEN
from paths_ref import Golden
from metagenomics_amd.overlap import (MATE_DTYPE, PLACE_DTYPE, SCAF_COUNTED, SCAF_FAR, SCAF_NOT_UNIQUE, SCAF_SAME_EDGE,
                                      SCAF_SKIPPED, SCAFFOLD_PAIR_DTYPE)

M64 = (1 << 64) - 1


def restate(n_reads, twin, places, mates, mean, sd):
    """(status list, [(edge1, edge2, support, distance)], counters tuple)"""
    pstart, precs = places
    mstart, mrecs = mates
    twin = [int(x) for x in twin]
    status, pairs = [], []
    for a in range(1, n_reads + 1):
        for m in range(int(mstart[a]), int(mstart[a + 1])):
            b, orient, d = int(mrecs["id"][m]), int(mrecs["orient"][m]), int(mrecs["dataset"][m])
            if a > b:  # :2137
                status.append(SCAF_SKIPPED)
                continue
            fwd1, fwd2 = orient in (0, 1), orient in (0, 2)  # :2149, :2153
            l1 = [(int(r["edge"]), int(r["distance"])) for r in precs[int(pstart[a]):int(pstart[a + 1])]
                  if bool(int(r["flags"]) & 1) == fwd1]
            l2 = [(int(r["edge"]), int(r["distance"])) for r in precs[int(pstart[b]):int(pstart[b + 1])]
                  if bool(int(r["flags"]) & 1) == fwd2]
            if len(l1) != 1 or len(l2) != 1:  # :2157
                status.append(SCAF_NOT_UNIQUE)
                continue
            dist = (l1[0][1] + l2[0][1]) & M64
            if not dist < ((int(mean[d]) + 3 * int(sd[d])) & M64):
                status.append(SCAF_FAR)
                continue
            e1, e2 = l1[0][0], l2[0][0]
            if e1 == e2 or e1 == twin[e2]:  # :2161
                status.append(SCAF_SAME_EDGE)
                continue
            status.append(SCAF_COUNTED)
            for rec in pairs:  # :2166-2180
                if (rec[0] == twin[e1] and rec[1] == e2) or (rec[0] == twin[e2] and rec[1] == e1):
                    rec[2] += 1
                    rec[3] = (rec[3] + dist) & M64
                    break
            else:
                pairs.append([twin[e1], e2, 1, dist])  # :2184-2190
    counters = tuple(status.count(s) for s in range(5))
    return status, [tuple(p) for p in pairs], counters


def pairs_of(s):
    return [(int(p["edge1"]), int(p["edge2"]), int(p["support"]), int(p["distance"])) for p in s.pairs]


def assert_equals_restatement(s, c):
    """a ScaffoldSupport against the restatement over the case dict c"""
    status, pairs, counters = restate(c["n_reads"], c["twin"], c["places"], c["mates"], c["mean"], c["sd"])
    assert s.status.tolist() == status
    assert pairs_of(s) == pairs
    assert s.counters == counters


def assert_same(a, b):
    """two ScaffoldSupports array for array"""
    assert np.array_equal(a.status, b.status), "status differs"
    assert a.pairs.dtype == b.pairs.dtype == SCAFFOLD_PAIR_DTYPE
    assert np.array_equal(a.pairs, b.pairs), "pairs differ"
    assert a.counters == b.counters


def csr(lists, dtype):
    """lists[A] for A in 0..n_reads + 1 -> (start uint64[n_reads + 2], records)"""
    start = np.zeros(len(lists), dtype=np.uint64)
    start[1:] = np.cumsum([len(x) for x in lists[:-1]])
    flat = [tuple(r) for x in lists for r in x]
    return start, (np.array(flat, dtype=dtype) if flat else np.zeros(0, dtype=dtype))


def make_case(n_reads, twin, place_lists, mate_lists, mean, sd):
    """place_lists[A] = [(edge, flags, distance)], mate_lists[A] = [(id, orient, dataset)] for A in 1..n_reads"""
    places = csr([[]] + [place_lists.get(a, []) for a in range(1, n_reads + 1)] + [[]], PLACE_DTYPE)
    mates = csr([[]] + [[(i, o, d, 0) for i, o, d in mate_lists.get(a, [])] for a in range(1, n_reads + 1)] + [[]],
                MATE_DTYPE)
    return {"n_reads": n_reads, "twin": np.asarray(twin, dtype=np.uint32), "places": places, "mates": mates,
            "mean": np.asarray(mean, dtype=np.uint64), "sd": np.asarray(sd, dtype=np.uint64)}


def random_case(rng, n_reads, n_half_edges, n_entries, max_loc=160, mean=(200, 0), sd=(10, 0), p_multi=0.15):
    """Edges 2k and 2k + 1 are twins.  Most reads have one or two placements
    (one per strand is common, so all four orients find unique lists), some
    none or several; exactly n_entries mate entries over the reads, three a
    read from read 1 on, one in 16 in the dataset without insert sizes."""
    E = 2 * n_half_edges
    twin = np.arange(E, dtype=np.uint32) ^ 1
    place_lists, mate_lists = {}, {}
    for a in range(1, n_reads + 1):
        k = int(rng.integers(0, 5)) if rng.random() < p_multi else int(rng.integers(1, 3))
        place_lists[a] = [(int(rng.integers(0, E)), (i + int(rng.integers(0, 2))) & 1 if k > 2 else i & 1,
                           int(rng.integers(0, max_loc))) for i in range(k)]
    left, a = n_entries, 1
    while left:
        assert a <= n_reads, "n_entries needs more reads"
        k = min(3, left)
        mate_lists[a] = [(int(rng.integers(1, n_reads + 1)), int(rng.integers(0, 4)), int(rng.integers(0, 16) == 0))
                         for _ in range(k)]
        left -= k
        a += 1
    return make_case(n_reads, twin, place_lists, mate_lists, mean, sd)


def host_args(c):
    return (c["n_reads"], c["twin"], c["places"], c["mates"], c["mean"], c["sd"])


def from_golden(g):
    """the case dict of a dump of one of the reference drivers (paths_ref.Golden):
    its reads, twins, location lists in list order, mate lists and mean / SD"""
    return {"n_reads": g.n, "twin": g.twin, "places": g.places, "mates": g.mates, "mean": g.mean, "sd": g.sd}


# ---- the reference's own scaffolder() runs (tests/golden/ref_scaffold_main.cpp, make_scaffold_golden.py)
GOLDEN_FIXTURES = ("pairs_small", "pairs_mixed", "pairs_long", "pairs_branchy")
LINE = re.compile(r"\s*(\d+) \(\s*(\d+),\s*(\d+)\) Length:\s*(\d+) Flow:\s*(\d+) and \(\s*(\d+),\s*(\d+)\) Length:\s*(\d+) "
                  r"Flow:\s*(\d+) are supported\s*(\d+) times. Average distance:\s*(\d+)")


def _gz(fn):
    with gzip.open(os.path.join(GOLDEN, fn), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def golden(name):
    """the build path on a paired fixture: the dump in the layout paths_ref.Golden reads"""
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        meta = json.load(f)
    with open(os.path.join(GOLDEN, "scaffold.json")) as f:
        files = json.load(f)[name]
    after = _gz(files["unitig_after"]).decode() if "unitig_after" in files else None
    g = Golden(name, meta["l"], [_gz(x) for x in meta["pe"]], [_gz(x) for x in meta["se"]], _gz(files["dump"]).decode(),
               None, after)
    g.raw_lines = raw_lines(_gz(files["dump"]).decode())
    return g


@functools.lru_cache(maxsize=None)
def hand_cases():
    with gzip.open(os.path.join(GOLDEN, "scaffold_cases.json.gz"), "rt") as f:
        cases = json.load(f)
    out = {}
    for c in cases:
        g = Golden(c["name"], c["l"], [x.encode() for x in c["pe"]], [c["se"].encode()], c["dump"], c["unitig"],
                   c["unitig_after"])
        g.raw_lines = raw_lines(c["dump"])
        out[c["name"]] = g
    return out


def raw_lines(dump):
    """the reference's "are supported" lines, character for character, as one string"""
    return "".join(ln[3:] + "\n" for ln in dump.splitlines() if ln.startswith("#O "))


def packed_reads(g, tmp_path):
    """(words, lens) of the case's reads in ID order, as Dataset packs them"""
    from metagenomics_amd.overlap import Dataset

    pe, se = g.write_files(tmp_path)
    ds = Dataset.from_files(pe + se, g.l)
    assert ds.num_unique == g.n
    words, lens = ds.packed()
    return np.array(words), np.array(lens)


def hand_case_names():
    return tuple(hand_cases())


def any_golden(name):
    return golden(name) if name in GOLDEN_FIXTURES else hand_cases()[name]


def reference_lines(g):
    """the "are supported" lines of the reference's scaffolder(): [(rank, (src1,
    dst1, offset1), (src2, dst2, offset2), support, average distance)]; Flow is 0"""
    out = []
    for ln in g.stdout:
        v = [int(x) for x in LINE.match(ln).groups()]
        assert v[4] == 0 and v[8] == 0
        out.append((v[0], (v[1], v[2], v[3]), (v[5], v[6], v[7]), v[9], v[10]))
    return out


def assert_explains_reference(s, g, nothing_freed):
    """The records of the ScaffoldSupport s against what the reference's run g
    shows of its listOfPairedEdges (a local): one line per record of support >=
    3 that no earlier merge freed, with its edges in the first-seen orientation,
    its support, distance / support, and its 1-based position after the sort by
    descending support.  nothing_freed: the case's pairs share no edge, so every
    record of support >= 3 has its line."""
    name = lambda k: (int(g.edges["src"][k]), int(g.edges["dst"][k]), int(g.edges["offset"][k]))
    recs = [(name(e1), name(e2), sup, dist // sup) for e1, e2, sup, dist in pairs_of(s)]
    lines = reference_lines(g)
    assert len(lines) == g.merged
    sups = sorted((r[2] for r in recs), reverse=True)
    for rank, e1, e2, sup, avg in lines:
        assert recs.count((e1, e2, sup, avg)) == 1, (rank, e1, e2, sup, avg)
        above, not_below = sum(x > sup for x in sups), sum(x >= sup for x in sups)
        assert above < rank <= not_below
    if nothing_freed:
        assert sorted(r for r in recs if r[2] >= 3) == sorted(ln[1:] for ln in lines)
    elif lines:  # the first record of the sorted list is never freed
        assert lines[0][0] == 1 and lines[0][3] == sups[0]


def run_cli_scaffold(g, tmp_path, resume, env=None):
    """mg_overlap ... -scaffold on a golden's files (resume: its .unitig re-read
    with -s).  Returns (the "are supported" lines as printed, the text of
    <prefix>.scaffold.unitig)."""
    import subprocess

    from conftest import ROOT

    exe = os.path.join(ROOT, "metagenomics_amd", "lib", "mg_overlap")
    pe, se = g.write_files(tmp_path)
    prefix = str(tmp_path / "out")
    cmd = [exe, "-pe", str(len(pe))] + pe + (["-se", str(len(se))] + se if se else [])
    cmd += ["-f", prefix, "-l", str(g.l), "-scaffold"] + (["-s"] if resume else [])
    if resume:
        with open(prefix + ".unitig", "w") as f:
            f.write(g.unitig)
    p = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=120, env={**os.environ, **(env or {})})
    with open(prefix + ".scaffold.unitig") as f:
        return "".join(ln + "\n" for ln in p.stdout.splitlines() if " are supported " in ln), f.read()


def assert_graph_after(u, g, tmp_path):
    """the graph's lists and its .unitig bytes equal the reference's after its scaffolder()"""
    e, st, reads, offs, ors = u.unitig_edges()
    rows = []
    for k, x in enumerate(e):
        a, n = int(st[k]), int(x["n_reads"])
        rows.append(" ".join([str(int(x[f])) for f in ("src", "dst", "orient", "offset", "n_reads")] +
                             [f"{reads[a + i]}:{offs[a + i]}:{ors[a + i]}" for i in range(n)]))
    assert rows == g.graph_after
    if g.unitig_after is not None:
        out = tmp_path / "after.unitig"
        u.save_unitig(str(out))
        assert out.read_text() == g.unitig_after
