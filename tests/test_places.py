"""Read placements, insert sizes and edge coverage on the device
(metagenomics_amd/csrc/device/mg_places.hip) against the host mirror, which
tests/test_places_host.py pins to the reference's goldens and to the plain-Python
restatement -- so synthetic arrays are fair inputs -- and against the goldens
themselves.

Shapes are the smallest at which each kernel can still go wrong: edges with 0,
1, 63, 64, 65 and 70,000 list entries (the last spans several scan tiles and
starts off a tile boundary); distances above 2^32 from 70,000 offsets of
65,535; reads with 0, 1, 2 and 40 placements; mate lists of 0, 1 and 300
entries; 3 datasets plus dataset 255; insert sizes 999, 1000 and 1001; a
coverage budget that forces several chunks and an edge alone in a chunk; edges
whose counters are no multiple of 64 or 256; both slot layouts; widths 1, 5
and 8 words and the long layout."""
import numpy as np
import pytest

import places_ref as R
from metagenomics_amd.overlap import (MATE_DTYPE, MgError, OverlapEngine, host_edge_coverage, host_insert_size_sums,
                                      host_placements, mean_sd)

pytestmark = pytest.mark.gpu


def packed_reads(rng, lens):
    """packed words [n, W] of random reads with these lengths, zero past the length"""
    lens = np.asarray(lens, dtype=np.uint16)
    wpr = (int(lens.max()) + 31) // 32
    words = rng.integers(0, np.iinfo(np.uint64).max, (lens.shape[0], wpr), dtype=np.uint64, endpoint=True)
    cnt = np.clip(lens[:, None].astype(np.int64) - 32 * np.arange(wpr)[None, :], 0, 32)
    keep = ~np.uint64(0) << np.where(cnt == 0, 0, 64 - 2 * cnt).astype(np.uint64)
    words &= np.where(cnt == 0, np.uint64(0), keep)
    return words, lens


def engine_for(rng, lens, layout=1):
    eng = OverlapEngine(0)
    eng.set_option("layout", layout)
    eng.upload_packed(*packed_reads(rng, lens))
    return eng


def assert_places(eng, n, graph):
    hs, hr, _ = host_placements(n, *graph)
    assert eng.build_placements(*graph) == hr.shape[0]
    ds, dr = eng.placements()
    assert np.array_equal(ds, hs), "start differs"
    assert np.array_equal(dr, hr), "records differ"
    return hs, hr


# ---- the reference's own results: the reads ingested on the device from the fixture's files
@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("name", R.ALL_GOLDENS)
def test_device_equals_reference(name, layout, tmp_path):
    g = R.any_golden(name)
    pe, se = g.write_files(tmp_path)
    eng = OverlapEngine(0)
    try:
        eng.set_option("layout", layout)
        assert eng.ingest_files(pe + se, g.l)["n_unique"] == g.n
        assert np.array_equal(eng.download_packed()[1], g.lens)
        assert np.array_equal(eng.frequency(), g.freq)
        eng.build_placements(*g.graph)
        assert R.sorted_lists(*eng.placements()) == g.locations
        sums = eng.insert_size_sums(len(g.datasets), g.mates)
        assert [mean_sd(*row) for row in sums] == g.datasets
        assert [mean_sd(*row)[:2] for row in eng.edge_coverage()] == g.coverage  # the ingest's resident frequencies
        assert np.array_equal(eng.edge_coverage(g.freq), host_edge_coverage(g.lens, g.freq, *g.graph))
        eng.set_option("cov_budget", 100)
        assert [mean_sd(*row)[:2] for row in eng.edge_coverage()] == g.coverage
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["pair_on_two_edges", "datasets", "non_monotone"])
def test_python_graph_methods_through_the_engine(name, tmp_path):
    """UnitigGraph.insert_sizes / edge_coverage with an engine that holds the reads: the device calls"""
    g = R.hand_cases()[name]
    u = R.case_unitig_graph(g, tmp_path)
    pe, se = g.write_files(tmp_path)
    eng = OverlapEngine(0)
    try:
        assert eng.ingest_files(pe + se, g.l)["n_unique"] == g.n
        assert u.insert_sizes(g.mates, len(g.datasets), engine=eng) == g.datasets
        assert R.coverage_rows_of(u, u.edge_coverage(engine=eng)) == R.golden_coverage_rows(g)
    finally:
        eng.close()


def test_many_edges_per_wavefront():
    """300 edges of one 20-bp read each: a wavefront of the coverage reduction spans several edges, chunks hold many"""
    rng = np.random.default_rng(21)
    n = 700
    lens = rng.integers(20, 33, n).astype(np.uint16)
    freq = rng.integers(1, 4, n).astype(np.uint32)
    graph = R.random_graph(rng, lens, [1] * 300, max_off=8)
    eng = engine_for(rng, lens)
    try:
        assert_places(eng, n, graph)
        want = host_edge_coverage(lens, freq, *graph)
        assert (want[:, 0] > 0).sum() >= 50  # (most one-read edges lie inside their zeroed spans)
        assert np.array_equal(eng.edge_coverage(freq), want)
        eng.set_option("cov_budget", 500)
        assert np.array_equal(eng.edge_coverage(freq), want)
    finally:
        eng.close()


# lengths that give 1, 5 and 8 words per read, and the long layout
WIDTHS = {"w1": (20, 32), "w5": (129, 160), "w8": (230, 256), "long": (1100, 1400)}


@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("width", list(WIDTHS))
def test_device_equals_mirror(width, layout):
    """every call, array for array, with list sizes around the wavefront and mate lists of 0, 1 and 300"""
    rng = np.random.default_rng(11)
    lo, hi = WIDTHS[width]
    n = 1500
    lens = rng.integers(lo, hi + 1, n).astype(np.uint16)
    lens[0], lens[-1] = hi, lo
    freq = rng.integers(1, 6, n).astype(np.uint32)
    graph = R.random_graph(rng, lens, [0, 1, 63, 64, 65, 0, 257, 2, 700], max_off=hi // 4)
    eng = engine_for(rng, lens, layout)
    try:
        start, recs = assert_places(eng, n, graph)
        lists = R.lists_of(start, recs)
        sizes = {a: 1 for a in range(1, n + 1, 3)}
        sizes[next(a for a in range(1, n + 1) if lists[a])] = 300  # (a read that lies on an edge)
        mates = R.random_mates(rng, n, sizes, 3, near=lists)
        want = host_insert_size_sums((start, recs), mates, 3)
        assert want[:, 0].min() > 0  # every dataset has insert sizes
        assert np.array_equal(eng.insert_size_sums(3, mates), want)
        assert eng.insert_ms > 0
        want = host_edge_coverage(lens, freq, *graph)
        assert (want[:, 0] > 0).sum() >= 4
        assert np.array_equal(eng.edge_coverage(freq), want)
        # counters that are no multiple of 64 or 256, and chunks: >= 3 chunks, the largest edge alone in its own
        sizes_ = [int(e["offset"]) + int(lens[int(e["dst"]) - 1]) + 1 for e in graph[0] if e["n"]]
        assert any(s % 64 and s % 256 for s in sizes_)
        eng.set_option("cov_budget", sorted(sizes_)[-2] + 1)
        assert np.array_equal(eng.edge_coverage(freq), want)
        eng.set_option("cov_budget", 1)  # every edge a chunk of its own
        assert np.array_equal(eng.edge_coverage(freq), want)
    finally:
        eng.close()


def test_long_segment_and_distances_above_2_32():
    """one edge of 70,000 entries of offset 65,535 after an edge of 37: its
    segment spans several scan tiles, its base is no tile boundary, and its last
    distances exceed 2^32; a read placed 40 times"""
    rng = np.random.default_rng(5)
    n = 200_000  # (most reads lie nowhere, many once or twice)
    lens = np.full(n, 60, dtype=np.uint16)
    big = 70000
    rs = rng.integers(1, n + 1, big)
    rs[::1750] = 9  # read 9: 40 placements
    lists = [[(int(r), 3, int(q)) for r, q in zip(rng.integers(1, n + 1, 37), rng.integers(0, 2, 37))],
             [(int(r), 65535, int(q)) for r, q in zip(rs, rng.integers(0, 2, big))], []]
    graph = R.make_edges(lists, [(1, 2, 200), (3, 4, 0), (5, 6, 10)])
    eng = engine_for(rng, lens)
    try:
        start, recs = assert_places(eng, n, graph)
        assert int(recs["distance"].max()) == big * 65535 > 1 << 32
        assert int(start[10] - start[9]) >= 40
        counts = np.diff(start.astype(np.int64))
        assert {0, 1, 2} <= set(counts.tolist())
    finally:
        eng.close()


def boundary_case():
    """reads 1..6 of 50 bp on one edge at distances 10, 1009, 1010, 1011, 1011, 5000 and on a second edge"""
    lens = np.full(8, 50, dtype=np.uint16)
    graph = R.make_edges([[(1, 10, 1), (2, 999, 0), (3, 1, 1), (4, 1, 1), (5, 0, 0), (6, 3989, 1)],
                          [(2, 5, 1), (1, 500, 1)], [(7, 10, 1)]],
                         [(7, 8, 5000), (7, 8, 600), (1, 2, 100)])
    mates = [(2, 1, 0), (3, 1, 0), (4, 1, 1),  # x = 999 counts; 1000 and 1001 do not
             (5, 4, 2), (4, 5, 2),             # equal locations: neither direction counts
             (1, 1, 0),                        # a read paired with itself
             (1, 2, 255), (2, 1, 255),         # dataset 255; on edge 1 read 1 lies 500 after read 2
             (6, 1, 1)]                        # far apart
    return lens, graph, mates


def mate_csr(n, triples):
    start = np.zeros(n + 2, dtype=np.uint64)
    recs = np.zeros(len(triples), dtype=MATE_DTYPE)
    order = sorted(range(len(triples)), key=lambda i: triples[i][0])
    for k, i in enumerate(order):
        a, b, d = triples[i]
        recs[k] = (b, 0, d, 0)
        start[a + 1:] += 1
    return start, recs


def test_boundary_distances_and_dataset_255():
    lens, graph, triples = boundary_case()
    rng = np.random.default_rng(1)
    eng = engine_for(rng, lens)
    try:
        start, recs = assert_places(eng, 8, graph)
        mates = mate_csr(8, triples)
        got = eng.insert_size_sums(256, mates)
        assert np.array_equal(got, host_insert_size_sums((start, recs), mates, 256))
        assert np.array_equal(got, R.insert_size_sums(R.lists_of(start, recs), mates[0], mates[1], 256))
        assert got[0].tolist() == [1, 999, 999 * 999]  # (2, 1) on edge 0; (1, 2) on edge 1 is dataset 255
        assert got[1].tolist() == [0, 0, 0] and got[2].tolist() == [0, 0, 0]
        assert got[255].tolist() == [2, 999 + 500, 999 * 999 + 500 * 500]
        assert got[3:255].sum() == 0
        with pytest.raises(MgError, match=r"mate entry 0\b.*\(-2\)"):  # entries sorted by owner: (1, 1, 0) first
            eng.insert_size_sums(0, mates)
        with pytest.raises(MgError, match=r"mate entry \d+.*\(-2\)"):
            eng.insert_size_sums(255, mates)
    finally:
        eng.close()


def test_errors_name_edge_and_entry():
    rng = np.random.default_rng(2)
    lens = np.array([40, 50, 30, 60], dtype=np.uint16)
    freq = np.ones(4, dtype=np.uint32)
    eng = engine_for(rng, lens)
    try:
        ok = [(1, 5, 1), (2, 5, 0)]
        with pytest.raises(MgError, match=r"edge 1 \(2, 3\), list entry 1: read ID 5 outside 1\.\.4 \(-2\)"):
            eng.build_placements(*R.make_edges([ok, [(1, 5, 1), (5, 5, 1)]], [(1, 2, 100), (2, 3, 100)]))
        with pytest.raises(MgError, match=r"edge 0 \(1, 2\), list entry 0: read ID 0 outside"):
            eng.build_placements(*R.make_edges([[(0, 5, 1)]], [(1, 2, 100)]))
        with pytest.raises(MgError, match="copy_placements"):
            eng.placements()  # a failed build leaves no lists
        with pytest.raises(MgError, match="mg_build_placements must succeed"):
            eng.edge_coverage(freq)
        e, r, o, q = R.make_edges([ok], [(1, 2, 100)])
        e["first"][0] = 1
        with pytest.raises(MgError, match="list range lies outside"):
            eng.build_placements(e, r, o, q)
        # coverage: L = offset + len(dst); entry 1 ends at 10 + 50 = 60
        cases = {
            r"edge 1 \(1, 2\), list entry 1: the read ends": ([ok, ok], [(1, 2, 100), (1, 2, 8)]),    # L + 1 = 59 < 60
            r"edge 0 \(4, 3\): the source read is longer": ([[(3, 0, 1)]], [(4, 3, 28)]),           # 60 > L + 1 = 59
            r"edge 1 \(0, 2\): its source or destination": ([ok, [(1, 1, 1)]], [(1, 2, 100), (0, 2, 100)]),
            r"edge 0 \(1, 5\): its source or destination": ([[]], [(1, 5, 100)]),
        }
        for pattern, (lists, sdo) in cases.items():
            graph = R.make_edges(lists, sdo)
            eng.build_placements(*graph)
            with pytest.raises(MgError, match=pattern + r".*\(-2\)"):
                eng.edge_coverage(freq)
            with pytest.raises(MgError, match=pattern):
                host_edge_coverage(lens, freq, *graph)
        # exactly at the bound: the read ends at L + 1
        graph = R.make_edges([ok], [(1, 2, 9)])
        eng.build_placements(*graph)
        assert np.array_equal(eng.edge_coverage(freq), host_edge_coverage(lens, freq, *graph))
        with pytest.raises(MgError, match="no resident frequencies"):
            eng.edge_coverage()
        with pytest.raises(MgError, match="mate lists"):
            eng.insert_size_sums(1)
    finally:
        eng.close()


def test_frequency_sum_limit():
    """32-bit frequency half of a delta word: an edge whose list frequencies sum to 2^32 is refused, 2^32 - 1 is exact"""
    rng = np.random.default_rng(3)
    lens = np.array([40, 40, 40, 40], dtype=np.uint16)
    graph = R.make_edges([[(1, 40, 1), (2, 0, 1), (3, 1, 1)]], [(4, 4, 200)])
    eng = engine_for(rng, lens)
    try:
        eng.build_placements(*graph)
        freq = np.array([1 << 31, (1 << 31) - 2, 1, 7], dtype=np.uint32)
        want = host_edge_coverage(lens, freq, *graph)
        assert int(want[0, 1]) > 0 and np.array_equal(eng.edge_coverage(freq), want)  # the sum is 2^32 - 1
        freq[2] = 2
        with pytest.raises(MgError, match=r"edge 0 \(4, 4\): its list frequencies sum to 2\^32 or more"):
            eng.edge_coverage(freq)
    finally:
        eng.close()


def test_rebuilt_after_second_upload_and_resident_inputs():
    """results belong to the current reads: a new upload invalidates the lists;
    the resident mate lists and ingest frequencies serve when nothing is passed"""
    import mates_ref as M

    g = M.golden("pairs_small")
    eng = OverlapEngine(0)
    try:
        assert not g.se  # the mates are every record of the fixture
        n = eng.ingest_ascii(list(g.raw), g.l)
        assert n == len(g.reads)
        _, lens = eng.download_packed()
        rng = np.random.default_rng(9)
        graph = R.random_graph(rng, lens, [300, 200, 0, 40], max_off=30)
        start, recs = assert_places(eng, n, graph)
        text, off = g.records()
        eng.build_mate_pairs(text, off, g.ppd, g.l, use_super=False)
        mates = eng.mate_lists()
        assert np.array_equal(eng.insert_size_sums(1), host_insert_size_sums((start, recs), mates, 1))
        freq = eng.frequency()
        assert int(freq.max()) > 1
        assert np.array_equal(eng.edge_coverage(), host_edge_coverage(lens, freq, *graph))
        # new reads: everything is rebuilt, nothing stale is served
        lens2 = np.full(50, 45, dtype=np.uint16)
        eng.upload_packed(*packed_reads(rng, lens2))
        for call in (eng.placements, lambda: eng.insert_size_sums(1, mate_csr(50, [])),
                     lambda: eng.edge_coverage(freq[:50])):
            with pytest.raises(MgError, match="mg_build_placements must succeed|copy_placements"):
                call()
        graph2 = R.random_graph(rng, lens2, [30, 3], max_off=20)
        assert_places(eng, 50, graph2)
        with pytest.raises(MgError, match="no resident frequencies"):
            eng.edge_coverage()  # the ingest's frequencies do not belong to uploaded reads
        f2 = np.ones(50, dtype=np.uint32)
        assert np.array_equal(eng.edge_coverage(f2), host_edge_coverage(lens2, f2, *graph2))
    finally:
        eng.close()

