"""Contig sequences on the device: mg_build_contigs / mg_copy_contigs
(metagenomics_amd/csrc/device/mg_contigs.hip) against the reference's own
getStringInEdge / printGraph output (tests/golden/make_contig_golden.py) and,
on synthetic chains, against the host mirror, which the goldens pin
(tests/test_contigs_host.py) -- so random lists are fair inputs.

Shapes: the copy kernel takes 64 consecutive pieces per wavefront and stages
sub-runs of up to 4,096 output bytes in LDS; a longer piece is written by the
whole wavefront.  The synthetic sets are the smallest that reach every path:
one edge of 5,000 pieces (79 wavefronts), 2,000 simple edges (three pieces
each, so wavefronts straddle edge boundaries 2,000 times), read lengths that
give one word, a full last word, 5, 8 and 32 words and the long layout, both
slot layouts, and pieces exactly at, one over and across the 4,096-byte span.
The edge of three 60,000-bp reads has a context of its own: in the same context
it would force the long layout on every other length.  Positions are 64-bit in
the ABI; no test can reach 4 GiB of output."""
import os
import subprocess

import numpy as np
import pytest

import contigs_ref as R
from conftest import FIXTURES, ROOT, fixture_input, load_meta
from metagenomics_amd.overlap import CONTIG_EDGE_DTYPE, MgError, OverlapEngine, host_contigs

pytestmark = pytest.mark.gpu

CASES = R.hand_cases()
CASE_NAMES = [c["name"] for c in CASES]
SPAN = 4096  # kSpan of mg_contigs.hip


def engine_for(words, lens, layout=1):
    eng = OverlapEngine(0)
    eng.set_option("layout", layout)
    eng.upload_packed(words, lens)
    return eng


def check_all_edges(ds, g, golden_text):
    want = R.parse_estrings(golden_text)
    e, reads, offs, ors = g.contig_edges(all_edges=True)
    good = np.array([w[5] != "!" for w in want], dtype=bool)
    eng = OverlapEngine(0)
    eng.upload(ds)
    try:
        start, data = eng.build_contigs(e[good], reads, offs, ors)
        assert R.split(start, data) == [w[5] for w in want if w[5] != "!"]
        for k in np.flatnonzero(~good):
            with pytest.raises(MgError, match=r"edge 0 \(%d, %d\)" % (e["src"][k], e["dst"][k])):
                eng.build_contigs(e[k:k + 1], reads, offs, ors)
    finally:
        eng.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_device_strings_match_reference(name):
    ds, g = R.fixture_graph(name)
    if name == "longreads":
        assert int(ds.packed()[1].max()) > 1024  # the long slot layout
    check_all_edges(ds, g, R.golden_file(name, "estrings").decode())


@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_hand_cases(name, tmp_path):
    case = CASES[CASE_NAMES.index(name)]
    ds, g = R.case_graph(case, tmp_path)
    check_all_edges(ds, g, case["estrings"])
    eng = OverlapEngine(0)
    eng.upload(ds)
    g.print_graph(ds, str(tmp_path / "x.gdl"), str(tmp_path / "x.fa"), engine=eng)
    eng.close()
    assert (tmp_path / "x.gdl").read_text() == case["gdl"]
    assert (tmp_path / "x.fa").read_text() == case["contigs_fa"]


@pytest.mark.parametrize("name", FIXTURES)
def test_print_graph_through_engine(name, tmp_path):
    ds, g = R.fixture_graph(name)
    eng = OverlapEngine(0)
    eng.upload(ds)
    g.print_graph(ds, str(tmp_path / "x.gdl"), str(tmp_path / "x.fa"), engine=eng)
    eng.close()
    assert (tmp_path / "x.gdl").read_bytes() == R.golden_file(name, "gdl")
    assert (tmp_path / "x.fa").read_bytes() == R.golden_file(name, "fasta")


@pytest.mark.parametrize("name", ["small", "branchy", "longreads"])
def test_cli_contigs(name, tmp_path):
    """mg_overlap -contigs: the build path of main.cpp:45-55, strings built on the device."""
    meta = load_meta(name)
    prefix = tmp_path / name
    exe = os.path.join(ROOT, "metagenomics_amd", "lib", "mg_overlap")
    subprocess.run([exe, "-se", "1", fixture_input(name), "-f", str(prefix), "-l", str(meta["l"]), "-contigs"],
                   check=True, stdout=subprocess.DEVNULL, timeout=120)
    assert (tmp_path / f"{name}graph1.gdl").read_bytes() == R.golden_file(name, "gdl")
    assert (tmp_path / f"{name}contigs1.fasta").read_bytes() == R.golden_file(name, "fasta")
    assert (tmp_path / f"{name}.estrings").read_bytes() == R.golden_file(name, "estrings")


# ---- synthetic chains: device == mirror, array for array

def random_reads(rng, n, lo, hi):
    """n packed reads of lengths in [lo, hi] (at least one of each bound): words [n, W] zero past the length"""
    lens = rng.integers(lo, hi + 1, n).astype(np.uint16)
    lens[0], lens[-1] = hi, lo
    wpr = (hi + 31) // 32
    words = rng.integers(0, np.iinfo(np.uint64).max, (n, wpr), dtype=np.uint64, endpoint=True)
    cnt = np.clip(lens[:, None].astype(np.int64) - 32 * np.arange(wpr)[None, :], 0, 32)  # bases of each word
    keep = ~np.uint64(0) << np.where(cnt == 0, 0, 64 - 2 * cnt).astype(np.uint64)
    words &= np.where(cnt == 0, np.uint64(0), keep)  # zero past the read
    return words, lens


def draw(rng, lo, hi):
    """an offset in [lo, hi], the two ends (empty piece / 'N') one time in five each"""
    u = rng.random()
    return lo if u < 0.2 else hi if u < 0.4 else int(rng.integers(lo, hi + 1))


def random_edges(rng, lens, list_sizes):
    n = lens.shape[0]
    edges = np.zeros(len(list_sizes), dtype=CONTIG_EDGE_DTYPE)
    reads, offs, ors = [], [], []
    for k, m in enumerate(list_sizes):
        src, dst = int(rng.integers(1, n + 1)), int(rng.integers(1, n + 1))
        first, prev, total = len(reads), int(lens[src - 1]), 0
        for _ in range(m):
            r = int(rng.integers(1, n + 1))
            ln = int(lens[r - 1])
            off = draw(rng, max(0, prev - ln), prev)  # keeps prev - off <= len
            reads.append(r), offs.append(off), ors.append(int(rng.integers(0, 2)))
            prev, total = ln, total + off
        len1, len2 = int(lens[src - 1]), int(lens[dst - 1])
        if m:
            tail, offset = draw(rng, 0, len2), total + int(rng.integers(0, 50))
        else:
            tail, offset = 0, draw(rng, max(0, len1 - len2), len1)
        edges[k] = (src, dst, offset, first, m, tail, int(rng.integers(0, 4)))
    return edges, np.array(reads, np.uint32), np.array(offs, np.uint16), np.array(ors, np.uint8)


def assert_same(eng, words, lens, e, reads, offs, ors):
    hs, hd = host_contigs(words, lens, e, reads, offs, ors)
    ds_, dd = eng.build_contigs(e, reads, offs, ors)
    assert np.array_equal(ds_, hs)
    assert dd == hd
    return ds_, dd


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("length", [20, 64, 150, 250, 1024, 1500])
def test_synthetic_chains(length, layout):
    rng = np.random.default_rng(1000 * length + layout)
    words, lens = random_reads(rng, 600, max(12, length // 2), length)
    e, reads, offs, ors = random_edges(rng, lens, [0] * 700 + [5000] + [0] * 1300 + [3, 1, 64, 62, 63])
    eng = engine_for(words, lens, layout)
    try:
        start, data = assert_same(eng, words, lens, e, reads, offs, ors)
        assert b"N" in data and (np.diff(start.astype(np.int64)) > 0).all()
        assert eng.build_contigs(e, reads, offs, ors)[1] == data  # two calls, identical bytes
    finally:
        eng.close()


def test_equal_length_chains():
    """one read length: offset 0 is the empty piece, offset = length the 'N' join"""
    rng = np.random.default_rng(5)
    words, lens = random_reads(rng, 300, 150, 150)
    e, reads, offs, ors = random_edges(rng, lens, [5000] + [0] * 2000)
    assert (offs == 0).any() and (offs == 150).any()
    eng = engine_for(words, lens)
    try:
        assert_same(eng, words, lens, e, reads, offs, ors)
    finally:
        eng.close()


def test_three_60000_bp_reads():
    rng = np.random.default_rng(6)
    words, lens = random_reads(rng, 5, 60000, 60000)
    lst = [(2, 31000, 0), (3, 60000, 1), (4, 1, 1)]
    e = np.zeros(2, dtype=CONTIG_EDGE_DTYPE)
    e[0] = (1, 5, 100000, 0, 3, 59999, 1)
    e[1] = (5, 1, 1234, 0, 0, 0, 2)
    args = (e, np.array([x[0] for x in lst], np.uint32), np.array([x[1] for x in lst], np.uint16),
            np.array([x[2] for x in lst], np.uint8))
    eng = engine_for(words, lens)
    try:
        start, _ = assert_same(eng, words, lens, *args)
        assert int(start[1]) == 60000 + 31000 + 60001 + 1 + 59999
    finally:
        eng.close()


def test_forward_chains_spell_the_genome():
    """forward-strand chains cut from a random genome: the contig is the genome substring itself"""
    rng = np.random.default_rng(7)
    genome = "".join("ACGT"[i] for i in rng.integers(0, 4, 330000))
    chains, strings = [], []
    at = 0
    for m in (2000, 0, 1, 70):
        pos = [at]
        for _ in range(m + 1):
            pos.append(pos[-1] + int(rng.integers(0, 151)))  # 150 = no overlap: an 'N' there
        chains.append(pos)
        at = pos[-1] + 200
    code = np.frombuffer(genome.encode(), dtype=np.uint8)
    lut = np.zeros(256, np.uint64)
    lut[list(b"ACGT")] = [0, 1, 2, 3]
    starts = [p for c in chains for p in c]
    words = np.zeros((len(starts), 5), dtype=np.uint64)
    for i, p in enumerate(starts):
        c = np.zeros(160, np.uint64)
        c[:150] = lut[code[p:p + 150]]
        words[i] = (c.reshape(5, 32) << (np.uint64(62) - np.uint64(2) * np.arange(32, dtype=np.uint64))).sum(axis=1)
    lens = np.full(len(starts), 150, np.uint16)
    e = np.zeros(len(chains), dtype=CONTIG_EDGE_DTYPE)
    reads, offs, rid = [], [], 1
    for k, c in enumerate(chains):
        m = len(c) - 2
        d = np.diff(c)
        e[k] = (rid, rid + m + 1, int(c[-1] - c[0]), len(reads), m, int(d[-1]), 3)
        reads += list(range(rid + 1, rid + 1 + m))
        offs += d[:-1].tolist()
        rid += m + 2
        # the genome itself, with an 'N' before every read that starts where the previous one ends
        s, end = "", c[0]
        for j, p in enumerate(c):
            if j and p == end and j <= m:
                s += "N"
            s += genome[max(p, end) if j else p:p + 150]
            end = p + 150
        strings.append(s)
    args = (e, np.array(reads, np.uint32), np.array(offs, np.uint16), np.ones(len(reads), np.uint8))
    eng = engine_for(words, lens)
    try:
        start, data = assert_same(eng, words, lens, *args)
        assert R.split(start, data) == strings
    finally:
        eng.close()


def test_pieces_around_the_staging_span():
    """With one read length L the bytes a list piece writes equal its offset (L + 1
    with the 'N'), so the sizes below are exact: at the span, one over, one under,
    sub-runs that end exactly at the span, one byte short and one byte over, and
    runs of small pieces whose span limit falls inside a wavefront's 64 pieces."""
    L = 5000
    rng = np.random.default_rng(8)
    words, lens = random_reads(rng, 40, L, L)
    sizes = [SPAN, SPAN + 1, SPAN - 1, 1, SPAN, 0, 2000, 2096, 2000, 2097, 2000, 2095, SPAN + 2, L, L - 1]
    sizes += [100] * 130 + [SPAN - 100, 100, SPAN - 99, 99, 64] + [65] * 64 + [SPAN // 64] * 128 + [SPAN + 1, SPAN]
    e = np.zeros(2, dtype=CONTIG_EDGE_DTYPE)
    e[0] = (1, 2, 7, 0, len(sizes), SPAN, 3)
    e[1] = (3, 4, SPAN + 1, 0, 0, 0, 0)  # a simple edge whose tail is one over the span
    reads = rng.integers(1, 41, len(sizes)).astype(np.uint32)
    ors = rng.integers(0, 2, len(sizes)).astype(np.uint8)
    eng = engine_for(words, lens)
    try:
        start, data = assert_same(eng, words, lens, e, reads, np.array(sizes, np.uint16), ors)
        assert int(start[1]) == L + sum(sizes) + 1 + SPAN  # (one 'N': the piece of L bases)
        assert int(start[2] - start[1]) == L + SPAN + 1
    finally:
        eng.close()


@pytest.mark.parametrize("what", sorted(R.INVALID))
def test_invalid_piece_leaves_the_context_usable(what):
    e, reads, offs, ors = R.INVALID[what]
    good = R.one_edge(1, 2, 3, 10)
    eng = engine_for(R.WORDS, R.LENS)
    try:
        want = host_contigs(R.WORDS, R.LENS, *good)
        got = eng.build_contigs(*good)
        assert got[1] == want[1]
        with pytest.raises(MgError, match=r"edge 1 \(%d, %d\).*\(-2\)" % (e["src"][0], e["dst"][0])):
            eng.build_contigs(np.concatenate([good[0], e]), reads, offs, ors)
        # nothing was copied: the failed build left no strings to fetch
        with pytest.raises(MgError, match="mg_build_contigs must succeed"):
            eng._check(eng_copy(eng), "copy_contigs")
        got = eng.build_contigs(*good)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    finally:
        eng.close()


def eng_copy(eng):
    from metagenomics_amd.overlap import lib

    return lib().mg_copy_contigs(eng._h, None, None, 0, None)


def test_bad_arguments_and_empty_inputs():
    eng = OverlapEngine(0)
    try:
        with pytest.raises(MgError, match="no reads"):
            eng.build_contigs(*R.one_edge(1, 2, 3, 10))
        eng.upload_packed(R.WORDS, R.LENS)
        start, data = eng.build_contigs(np.zeros(0, CONTIG_EDGE_DTYPE), [], [], [])
        assert start.tolist() == [0] and data == b""
        e = R.one_edge(1, 2, 3, 60, [(3, 20, 1)], 0)
        e[0]["first"] = 1
        with pytest.raises(MgError, match="list range"):
            eng.build_contigs(*e)
        # new reads invalidate the strings
        eng.build_contigs(*R.one_edge(1, 2, 3, 10))
        eng.upload_packed(R.WORDS, R.LENS)
        with pytest.raises(MgError, match="mg_build_contigs must succeed"):
            eng._check(eng_copy(eng), "copy_contigs")
    finally:
        eng.close()
