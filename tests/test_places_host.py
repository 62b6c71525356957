"""The host mirrors of the placement calls (metagenomics_amd/csrc/host/mg_places.cpp:
mg::placements_build, mg::insert_sizes, mg::edge_coverage, mg::mean_sd) on the CPU:

  a. the ABI: the device entry points and the mirrors are exported;
  b. the mirrors equal the reference's own results (tests/golden/places.json,
     places_cases.json; make_places_golden.py): every read's four location
     lists, mean / SD / count per dataset, coverageDepth / SD per edge;
  c. the mirror's placements equal the location lists the contraction tracked
     (updateReadLocations / removeReadLocations through every merge), on every
     fixture with a .unitig golden;
  d. the plain-Python restatement (places_ref.py) equals the mirrors on random
     inputs;
  e. every -2 case, with the edge and entry named;
  f. mean_sd's arithmetic, the wrapping variance included."""
import numpy as np
import pytest

import contigs_ref as CR
import places_ref as R
from conftest import FIXTURES
from metagenomics_amd import overlap
from metagenomics_amd.overlap import (MATE_DTYPE, MgError, host_edge_coverage, host_insert_size_sums, host_placements,
                                      mean_sd)


# ---- a. ABI
@pytest.mark.parametrize("symbol", ["mg_build_placements", "mg_copy_placements", "mg_insert_sizes",
                                    "mg_edge_coverage", "mgh_placements_build", "mgh_insert_sizes",
                                    "mgh_edge_coverage", "mgh_mean_sd", "mgh_graph_read_locations"])
def test_abi_symbols(symbol):
    assert getattr(overlap.lib(), symbol) is not None


def test_record_layout():
    assert overlap.PLACE_DTYPE.itemsize == 16
    assert [overlap.PLACE_DTYPE.fields[k][1] for k in ("edge", "flags", "distance")] == [0, 4, 8]


# ---- b. the reference's own results
@pytest.mark.parametrize("name", R.ALL_GOLDENS)
def test_mirror_equals_reference(name):
    g = R.any_golden(name)
    start, recs, fwd = host_placements(g.n, *g.graph)
    assert R.sorted_lists(start, recs) == g.locations  # the four location lists, as sets
    assert fwd.tolist() == [sum(p[1] for p in x) for x in g.locations]
    sums = host_insert_size_sums((start, recs), g.mates, len(g.datasets))
    assert [mean_sd(*row) for row in sums] == g.datasets
    cov = host_edge_coverage(g.lens, g.freq, *g.graph)
    assert [mean_sd(*row)[:2] for row in cov] == g.coverage


def test_goldens_hold_what_the_cases_are_for():
    """the properties the hand cases were written for, read back from the reference's dumps"""
    h = R.hand_cases()
    assert set(R.HAND_CASES) == set(h)
    two = h["pair_on_two_edges"]
    assert max(sum(p[1] for p in x) for x in two.locations) == 2 and two.datasets[0][2] == 4
    assert h["boundaries"].datasets == [(500, 499, 2)]  # x = 999 and, on the twin, x = 1; 1000 and 1001 do not count
    assert [d[2] for d in h["datasets"].datasets] == [4, 4, 0] and h["datasets"].stdout[-1].startswith("No insert-size")
    assert 1 in h["single_and_simple"].graph[0]["n"] and 0 in h["single_and_simple"].graph[0]["n"]
    assert h["all_inside_spans"].coverage == [(0, 0), (0, 0)]
    e, reads, offs, _ = h["non_monotone"].graph
    k = int(np.flatnonzero(e["offset"] == 140000)[0])
    a, m = int(e["first"][k]), int(e["n"][k])
    ends = np.cumsum(offs[a:a + m].astype(np.int64)) + h["non_monotone"].lens[reads[a:a + m] - 1]
    assert ends.tolist() == [120, 85, 129]
    assert int(max(g.freq.max() for g in h.values())) > 1
    b = R.golden("pairs_branchy")
    assert (b.graph[0]["n"] > 0).sum() >= 6 and min(d[2] for d in b.datasets) >= 20 and max(c[1] for c in b.coverage) > 0
    assert [R.golden(n).datasets for n in ("pairs_small", "pairs_mixed", "pairs_long")] == \
        [[(251, 67, 560)], [(378, 294, 94), (388, 217, 44)], [(662, 269, 22)]]


@pytest.mark.parametrize("name", R.HAND_CASES)
def test_cli_insert_lines_on_the_resume_path(name, tmp_path):
    """mg_overlap -s -insert (no device needed): the reference's own stdout lines, and every edge's coverage from
    calculateCoverageOfAllEdges and from getBaseByBaseCoverage(Edge*)"""
    g = R.hand_cases()[name]
    lines, rows = R.run_cli_insert(g, tmp_path, resume=True, env={"MG_DEVICE_PLACES": "0"})
    assert lines == g.stdout
    assert rows == R.golden_coverage_rows(g)


@pytest.mark.parametrize("name", R.HAND_CASES)
def test_python_graph_methods_on_the_host(name, tmp_path):
    """UnitigGraph.insert_sizes / edge_coverage without an engine: the host mirrors"""
    g = R.hand_cases()[name]
    u = R.case_unitig_graph(g, tmp_path)
    assert u.insert_sizes(g.mates, len(g.datasets)) == g.datasets
    assert R.coverage_rows_of(u, u.edge_coverage(g.lens, g.freq)) == R.golden_coverage_rows(g)
    with pytest.raises(MgError, match="needs"):
        u.edge_coverage()


# ---- c. the contraction's own location lists
@pytest.mark.parametrize("name", FIXTURES)
def test_placements_equal_tracked_locations(name):
    ds, g = CR.fixture_graph(name)
    n = ds.num_unique
    tracked = g.read_locations()
    assert tracked is not None and tracked[0].shape[0] == n + 2
    start, recs, fwd = host_placements(n, *g.contig_edges(all_edges=True))
    assert np.array_equal(start, tracked[0])
    key = lambda lst: [sorted(x, key=lambda p: (p[0], p[2], p[1])) for x in lst]
    assert key(R.lists_of(start, recs)) == R.lists_of(*tracked)
    assert fwd.tolist() == [sum(p[1] for p in x) for x in R.lists_of(start, recs)]


@pytest.mark.parametrize("name", [c["name"] for c in CR.hand_cases()])
def test_placements_equal_reread_locations(name, tmp_path):
    """readGraphFromFile's updateReadLocations of both edges of every record"""
    case = next(c for c in CR.hand_cases() if c["name"] == name)
    ds, g = CR.case_graph(case, tmp_path)
    start, recs, _ = host_placements(ds.num_unique, *g.contig_edges(all_edges=True))
    tracked = g.read_locations()
    key = lambda lst: [sorted(x, key=lambda p: (p[0], p[2], p[1])) for x in lst]
    assert key(R.lists_of(start, recs)) == R.lists_of(*tracked)


# ---- d. restatement == mirror on random inputs
@pytest.mark.parametrize("seed", range(6))
def test_restatement_equals_mirror(seed):
    rng = np.random.default_rng(100 + seed)
    n = 60
    lens = rng.integers(20, 90, n).astype(np.uint16)
    freq = rng.integers(0, 5, n).astype(np.uint32)  # (a frequency of 0 adds nothing, but its read can still zero)
    graph = R.random_graph(rng, lens, np.roll([0, 1, 2, 9, 30, 0, 64, 5], seed).tolist(), max_off=25)
    start, recs, fwd = host_placements(n, *graph)
    lists = R.placements(n, *graph)
    want_start, want_recs = R.csr_of(lists)
    assert np.array_equal(start, want_start) and np.array_equal(recs, want_recs)
    assert fwd.tolist() == [sum(p[1] for p in x) for x in lists]
    assert max(fwd) > 1  # some interval is zeroed
    mates = R.random_mates(rng, n, {a: int(rng.integers(0, 4)) for a in range(1, n + 1)}, 3, near=lists)
    got = host_insert_size_sums((start, recs), mates, 3, max_distance=60)
    assert np.array_equal(got, R.insert_size_sums(lists, mates[0], mates[1], 3, max_distance=60))
    assert got[:, 0].sum() > 0
    cov = host_edge_coverage(lens, freq, *graph)
    assert np.array_equal(cov, R.edge_coverage(lens, freq, *graph))
    for row in np.concatenate([got, cov]):
        assert mean_sd(*row) == R.mean_sd(*(int(x) for x in row))


# ---- e. errors
def test_mirror_errors():
    lens = np.array([40, 50, 30, 60], dtype=np.uint16)
    freq = np.ones(4, dtype=np.uint32)
    ok = [(1, 5, 1), (2, 5, 0)]
    with pytest.raises(MgError, match=r"edge 1 \(2, 3\), list entry 1: read ID 5 outside 1\.\.4 \(-2\)"):
        host_placements(4, *R.make_edges([ok, [(1, 5, 1), (5, 5, 1)]], [(1, 2, 100), (2, 3, 100)]))
    with pytest.raises(MgError, match=r"edge 0 \(1, 2\), list entry 0: read ID 0 outside"):
        host_placements(4, *R.make_edges([[(0, 5, 1)]], [(1, 2, 100)]))
    e, r, o, q = R.make_edges([ok], [(1, 2, 100)])
    e["first"][0] = 1
    with pytest.raises(MgError, match=r"list range lies outside.*\(-1\)"):
        host_placements(4, e, r, o, q)
    cases = {
        r"edge 1 \(1, 2\), list entry 1: the read ends": ([ok, ok], [(1, 2, 100), (1, 2, 8)]),
        r"edge 0 \(4, 3\): the source read is longer": ([[(3, 0, 1)]], [(4, 3, 28)]),
        r"edge 1 \(0, 2\): its source or destination": ([ok, [(1, 1, 1)]], [(1, 2, 100), (0, 2, 100)]),
        r"edge 0 \(1, 5\): its source or destination": ([[]], [(1, 5, 100)]),
    }
    for pattern, (lists, sdo) in cases.items():
        graph = R.make_edges(lists, sdo)
        with pytest.raises(MgError, match=pattern + r".*\(-2\)"):
            host_edge_coverage(lens, freq, *graph)
        with pytest.raises(R.Invalid):
            R.edge_coverage(lens, freq, *graph)
    host_edge_coverage(lens, freq, *R.make_edges([ok], [(1, 2, 9)]))  # the read ends exactly at L + 1
    with pytest.raises(MgError, match=r"offset of 2\^40.*\(-1\)"):
        host_edge_coverage(lens, freq, *R.make_edges([ok], [(1, 2, 1 << 40)]))
    # mate entries: dataset, mate ID, owner
    start, recs, _ = host_placements(4, *R.make_edges([ok], [(1, 2, 100)]))
    mstart = np.array([0, 0, 1, 2, 2, 2], dtype=np.uint64)
    for bad, entry in (([(2, 0, 0, 0), (1, 0, 3, 0)], 1), ([(2, 0, 0, 0), (5, 0, 0, 0)], 1),
                       ([(0, 0, 0, 0), (1, 0, 0, 0)], 0)):
        with pytest.raises(MgError, match=r"mate entry %d:.*\(-2\)" % entry):
            host_insert_size_sums((start, recs), (mstart, np.array(bad, dtype=MATE_DTYPE)), 3)
    with pytest.raises(MgError, match=r"mate entry 0:.*\(-2\)"):  # an entry owned by ID 0
        host_insert_size_sums((start, recs), (np.array([0, 1, 1, 1, 1, 1], dtype=np.uint64),
                                              np.array([(1, 0, 0, 0)], dtype=MATE_DTYPE)), 3)


# ---- f. the arithmetic
def test_mean_sd():
    assert mean_sd(0, 0, 0) == (0, 0, 0)
    assert mean_sd(1, 7, 49) == (7, 0, 1)
    xs = [250, 251, 400, 3, 999]
    assert mean_sd(len(xs), sum(xs), sum(x * x for x in xs)) == R.mean_sd(len(xs), sum(xs), sum(x * x for x in xs))
    m = sum(xs) // len(xs)
    assert R.mean_sd(len(xs), sum(xs), sum(x * x for x in xs))[1] == int((sum((m - x) ** 2 for x in xs) // len(xs)) ** 0.5)
    # sums that wrapped: the variance is the reference's wrapping sum of (mean - x)^2
    big = [(1 << 32) - 1, 1 << 31, 5]
    c, s, q = len(big), sum(big), sum(x * x for x in big) & R.M64
    mean = s // c
    var = sum(((mean - x) * (mean - x)) & R.M64 for x in big) & R.M64
    assert mean_sd(c, s, q) == (mean, int(float(var // c) ** 0.5), c) == R.mean_sd(c, s, q)
