"""Contig sequences on the host: the mirror of getStringInEdge and printGraph
(OverlapGraph.cpp:2009-2041, 428-520; metagenomics_amd/csrc/host/mg_contigs.cpp,
C-ABI mgh_graph_contig_edges / mgh_contigs_build / mgh_graph_print).

Golden: tests/golden/make_contig_golden.py, i.e. the reference's own
getStringInEdge of every edge of every list (<name>.estrings.gz) and its own
printGraph files (<name>.contigs.fa.gz, <name>.gdl.gz) on every fixture, and the
same dumps of hand-made .unitig files (contig_cases.json).  Runs on the CPU."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import contigs_ref as R
from conftest import FIXTURES, GOLDEN, ROOT, fixture_input, load_meta
from metagenomics_amd.overlap import CONTIG_EDGE_DTYPE, Dataset, MgError, UnitigGraph, host_contigs

CASES = R.hand_cases()
CASE_NAMES = [c["name"] for c in CASES]


def check_estrings(ds, g, golden_text):
    """mirror and Python restatement == the reference's strings, edge for edge in list order"""
    want = R.parse_estrings(golden_text)
    e, reads, offs, ors = g.contig_edges(all_edges=True)
    assert [(int(x["src"]), int(x["dst"]), int(x["orient"]), int(x["offset"]), int(x["n"])) for x in e] == \
        [w[:5] for w in want]
    words, lens = ds.packed()
    good = np.array([w[5] != "!" for w in want], dtype=bool)
    start, data = host_contigs(words, lens, e[good], reads, offs, ors)
    assert R.split(start, data) == [w[5] for w in want if w[5] != "!"]
    assert R.strings_of(ds.read, e[good], reads, offs, ors) == [w[5] for w in want if w[5] != "!"]
    for k in np.flatnonzero(~good):  # where the reference's substr throws, the mirror reports the edge
        with pytest.raises(MgError, match=r"edge 0 \(%d, %d\)" % (e["src"][k], e["dst"][k])):
            host_contigs(words, lens, e[k:k + 1], reads, offs, ors)
        with pytest.raises(R.InvalidPiece):
            R.strings_of(ds.read, e[k:k + 1], reads, offs, ors)


@pytest.mark.parametrize("name", FIXTURES)
def test_mirror_matches_reference_strings(name):
    ds, g = R.fixture_graph(name)
    check_estrings(ds, g, R.golden_file(name, "estrings").decode())


@pytest.mark.parametrize("name", FIXTURES)
def test_mirror_from_golden_ulists(name):
    """The same strings from the reference's own list dump (no graph code of ours
    in between): compared as a multiset, since the dump precedes sortEdges."""
    ds, _ = R.fixture_graph(name)
    words, lens = ds.packed()
    e, reads, offs, ors = R.ulists_edges(name, lens)
    start, data = host_contigs(words, lens, e, reads, offs, ors)
    got = sorted((int(x["src"]), int(x["dst"]), int(x["orient"]), int(x["offset"]), int(x["n"]), s)
                 for x, s in zip(e, R.split(start, data)))
    assert got == sorted(R.parse_estrings(R.golden_file(name, "estrings").decode()))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_hand_case_strings(name, tmp_path):
    case = CASES[CASE_NAMES.index(name)]
    ds, g = R.case_graph(case, tmp_path)
    check_estrings(ds, g, case["estrings"])


def test_hand_cases_cover_what_they_claim():
    by = {c["name"]: R.parse_estrings(c["estrings"]) for c in CASES}
    assert any("N" in w[5] for w in by["n_join"])
    assert sorted(w[2] for w in by["orient4"]) == [0, 0, 1, 1, 2, 2, 3, 3]
    assert {len(w[5]) for w in by["lines_100_101"]} == {100, 101}
    assert all(w[0] == w[1] for w in by["self_loops"]) and any(w[4] for w in by["self_loops"])
    assert any(w[4] == 4 for w in by["composite_mixed"])
    # the empty piece: the composite string is no longer than its source read plus its tail
    # (50-bp source + nothing of the 30-bp list read + 25 of the destination; its twin: 45 + 10 + 20)
    assert [len(w[5]) for w in by["empty_piece"]] == [75, 75] and all(w[4] == 1 for w in by["empty_piece"])


def print_and_read(g, ds, tmp_path, engine=None, tag="x"):
    gdl, fa = tmp_path / f"{tag}.gdl", tmp_path / f"{tag}.fa"
    g.print_graph(ds, str(gdl), str(fa), engine=engine)
    return gdl.read_bytes(), fa.read_bytes()


def self_loop_choice(g):
    """[src, list position] of the self-loop edges listed as contigs"""
    every, chosen = g.contig_edges(all_edges=True)[0], g.contig_edges()[0]
    key = lambda x: tuple(int(x[f]) for f in ("src", "dst", "orient", "offset", "n", "tail"))
    pos, out, k = {}, [], 0
    for x in every:
        p = pos.get(int(x["src"]), 0)
        pos[int(x["src"])] = p + 1
        if k < chosen.shape[0] and key(chosen[k]) == key(x):
            if x["src"] == x["dst"]:
                out.append([int(x["src"]), p])
            k += 1
    assert k == chosen.shape[0]
    return out


@pytest.mark.parametrize("name", FIXTURES)
def test_print_graph_matches_reference(name, tmp_path):
    # the reference lists the self-loop twin with the lower address (:460); the
    # generator found no fixture where that is not the twin created first
    assert R.contig_index()[name]["other_twin"] == []
    ds, g = R.fixture_graph(name)
    gdl, fa = print_and_read(g, ds, tmp_path)
    assert gdl == R.golden_file(name, "gdl")
    assert fa == R.golden_file(name, "fasta")


@pytest.mark.parametrize("name", CASE_NAMES)
def test_print_graph_hand_cases(name, tmp_path):
    case = CASES[CASE_NAMES.index(name)]
    ds, g = R.case_graph(case, tmp_path)
    assert self_loop_choice(g) == case["ref_loops"]  # only self-loops could differ, and none does
    gdl, fa = print_and_read(g, ds, tmp_path)
    assert gdl.decode() == case["gdl"]
    assert fa.decode() == case["contigs_fa"]


@pytest.mark.parametrize("name", FIXTURES)
def test_resume_from_unitig_gives_the_same_files(name, tmp_path):
    meta = load_meta(name)
    ds = Dataset.from_files([fixture_input(name)], meta["l"])
    with gzip.open(os.path.join(GOLDEN, meta["unitig"]["file"]), "rb") as f:
        (tmp_path / "in.unitig").write_bytes(f.read())
    g = UnitigGraph.from_unitig_file(str(tmp_path / "in.unitig"), ds.packed()[1])
    g.sort_edges()
    gdl, fa = print_and_read(g, ds, tmp_path)
    assert gdl == R.golden_file(name, "gdl")
    assert fa == R.golden_file(name, "fasta")


@pytest.mark.parametrize("name", ["small", "branchy", "longreads"])
def test_cli_resume_contigs(name, tmp_path):
    """mg_overlap -s -contigs: main.cpp:36-42 and :55 without a device (the host mirror spells the strings)."""
    meta = load_meta(name)
    prefix = tmp_path / name
    with gzip.open(os.path.join(GOLDEN, meta["unitig"]["file"]), "rb") as f:
        (tmp_path / f"{name}.unitig").write_bytes(f.read())
    exe = os.path.join(ROOT, "metagenomics_amd", "lib", "mg_overlap")
    env = dict(os.environ, MG_DEVICE_CONTIGS="0")
    subprocess.run([exe, "-se", "1", fixture_input(name), "-f", str(prefix), "-l", str(meta["l"]), "-s", "-contigs"],
                   check=True, stdout=subprocess.DEVNULL, timeout=120, env=env)
    assert (tmp_path / f"{name}graph1.gdl").read_bytes() == R.golden_file(name, "gdl")
    assert (tmp_path / f"{name}contigs1.fasta").read_bytes() == R.golden_file(name, "fasta")
    # the drop-in's getStringInEdge(Edge*) on every Edge object of every list
    assert (tmp_path / f"{name}.estrings").read_bytes() == R.golden_file(name, "estrings")


# ---- invalid pieces: -2, the edge named, nothing read out of range

LENS, WORDS, one_edge, INVALID = R.LENS, R.WORDS, R.one_edge, R.INVALID


@pytest.mark.parametrize("what", sorted(INVALID))
def test_invalid_piece_is_reported(what):
    e, reads, offs, ors = INVALID[what]
    good = one_edge(1, 2, 3, 10)[0]
    edges = np.concatenate([good, e])  # the bad edge is edge 1
    with pytest.raises(MgError, match=r"edge 1 \(%d, %d\).*\(-2\)" % (e["src"][0], e["dst"][0])):
        host_contigs(WORDS, LENS, edges, reads, offs, ors)


def test_valid_edge_cases():
    # offset == len1: nothing of the source is shared, the whole destination follows (no 'N' for the tail)
    start, data = host_contigs(WORDS, LENS, *one_edge(1, 2, 3, 40))
    assert start.tolist() == [0, 90]
    # an empty tail and an empty list piece are valid
    start, data = host_contigs(WORDS, LENS, *one_edge(2, 3, 3, 20))  # pos = 30 = len2
    assert start.tolist() == [0, 50]
    start, data = host_contigs(WORDS, LENS, *one_edge(2, 1, 3, 60, [(3, 20, 1)], 0))
    assert start.tolist() == [0, 50] and b"N" not in data
    # a list range outside the lists is a bad argument, not a crash
    e = one_edge(1, 2, 3, 60, [(3, 20, 1)], 0)
    e[0]["first"] = 1
    with pytest.raises(MgError, match="list range"):
        host_contigs(WORDS, LENS, *e)


def test_zero_edges_and_no_contigs(tmp_path):
    start, data = host_contigs(WORDS, LENS, np.zeros(0, CONTIG_EDGE_DTYPE), [], [], [])
    assert start.tolist() == [0] and data == b""
    # a graph without edges: header block, no node lines, the closing brace; an empty FASTA
    (tmp_path / "e.unitig").write_text("")
    g = UnitigGraph.from_unitig_file(str(tmp_path / "e.unitig"), LENS)
    assert g.contig_edges()[0].shape[0] == 0
    gdl, fa = print_and_read(g, (WORDS, LENS), tmp_path)
    assert fa == b"" and gdl == R.golden_file("tworead", "gdl")
    # device-built strings handed to the writer must be consistent
    ds, g2 = R.fixture_graph("small")
    e, reads, offs, ors = g2.contig_edges()
    words, lens = ds.packed()
    start, data = host_contigs(words, lens, e, reads, offs, ors)
    buf = np.frombuffer(data, dtype=np.uint8)
    err = None
    rc = g2._L.mgh_graph_print(g2._g, None, None, 0, 0, start.ctypes.data, buf.ctypes.data,
                               os.fsencode(str(tmp_path / "s.gdl")), os.fsencode(str(tmp_path / "s.fa")), err, 0)
    assert rc == 0 and (tmp_path / "s.fa").read_bytes() == R.golden_file("small", "fasta")
    bad = start.copy()
    bad[1], bad[2] = bad[2], bad[1]
    rc = g2._L.mgh_graph_print(g2._g, None, None, 0, 0, bad.ctypes.data, buf.ctypes.data,
                               os.fsencode(str(tmp_path / "t.gdl")), os.fsencode(str(tmp_path / "t.fa")), err, 0)
    assert rc == -1
