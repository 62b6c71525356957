"""The host side of mate-pair path support (metagenomics_amd/csrc/host/mg_paths.cpp:
mg::mate_paths, mg::path_pairs, mg::merge_supported, and the two graph exports)
on the CPU:

  a. the ABI: the device entry points, the mirror and the exports are exported;
  b. the mirror and the plain-Python restatement (paths_ref.py) equal the
     reference's own dump entry for entry on every fixture and hand case
     (tests/golden/paths.json, paths_cases.json.gz; make_paths_golden.py); the
     pair list and the counters equal the reference's summary lines;
  c. on the hand cases (the resume path, which a test can take without a
     device): the location-list export equals the reference's lists in list
     order, the twins equal its twins, and merge_supported leaves the
     reference's merged count, lists and .unitig bytes; the same merge check
     on the four paired fixtures, over the graph their dumps describe;
  d. the goldens hold what the cases are for;
  e. the -2 errors in their order, bad arguments, the refused twin pair;
  f. random small graphs: mirror == restatement, work units included; a budget
     defers exactly the entries above it and `prior` finishes them;
  g. the stand-alone sanitizer program builds and runs clean."""
import os
import subprocess

import numpy as np
import pytest

import paths_ref as R
from conftest import ROOT
from metagenomics_amd import overlap
from metagenomics_amd.overlap import (PAIR_DTYPE, PATH_DEFERRED, PATH_FOUND, PATH_NONE, PATH_SAME_EDGE, PATH_SKIPPED,
                                      MgError, host_mate_paths)

ALL = R.GOLDEN_FIXTURES + R.hand_case_names()


# ---- a. ABI
@pytest.mark.parametrize("symbol", ["mg_mate_paths", "mg_mate_paths_info", "mg_copy_mate_paths", "mg_copy_path_pairs",
                                    "mgh_mate_paths", "mgh_graph_edge_twins", "mgh_graph_location_lists",
                                    "mgh_graph_merge_supported"])
def test_abi_symbols(symbol):
    assert getattr(overlap.lib(), symbol) is not None


def test_record_layout():
    assert PAIR_DTYPE.itemsize == 16
    assert [PAIR_DTYPE.fields[k][1] for k in ("edge1", "edge2", "support")] == [0, 4, 8]
    assert (PATH_SKIPPED, PATH_SAME_EDGE, PATH_NONE, PATH_FOUND, PATH_DEFERRED) == (0, 1, 2, 3, 4)


# ---- b. the reference's own results
@pytest.mark.parametrize("name", ALL)
def test_mirror_and_restatement_equal_reference(name):
    g = R.any_golden(name)
    host = host_mate_paths(*g.args())
    got = R.entries_of(host)
    assert [(st, p, f) for st, _, p, f in got] == g.entries
    assert host.deferred == 0
    pairs, counters = R.pair_list(g.edges, g.twin, got)
    assert R.pairs_of(host) == pairs and host.counters == counters
    s = g.summary()
    if s is not None:  # supported pairs, noPathsFound, pathsFound, mpOnSameEdge
        assert (len(pairs),) + counters == s[1:]
    if name != "pairs_branchy":  # (3,200 entries on a branching graph: minutes in Python; the mirror stands for it)
        assert R.restate(g.edges, g.twin, g.places, g.mates, g.mean, g.sd) == got


# ---- c. the exports and the merge, on the resume path
@pytest.mark.parametrize("name", R.hand_case_names())
def test_exports_and_merge_on_hand_cases(name, tmp_path):
    g = R.hand_cases()[name]
    u = R.unitig_graph(g, tmp_path)
    edges = u.contig_edges(all_edges=True)[0]
    for f in ("src", "dst", "offset", "orient", "n"):
        assert np.array_equal(edges[f], g.edges[f]), f
    assert np.array_equal(u.edge_twins(), g.twin)
    start, recs = u.location_lists()
    assert np.array_equal(start, g.places[0]) and np.array_equal(recs, g.places[1])  # in list order
    ps = u.mate_support(g.mates, g.mean, g.sd)
    assert [(st, p, f) for st, _, p, f in R.entries_of(ps)] == g.entries
    assert u.merge_supported(ps.pairs) == g.merged
    assert_graph_after(u, g, tmp_path)


def assert_graph_after(u, g, tmp_path):
    """the graph's lists and its .unitig bytes equal the reference's after its merge loop"""
    e, st, reads, offs, ors = u.unitig_edges()
    rows = []
    for k, x in enumerate(e):
        a, n = int(st[k]), int(x["n_reads"])
        rows.append(" ".join([str(int(x[f])) for f in ("src", "dst", "orient", "offset", "n_reads")] +
                             [f"{reads[a + i]}:{offs[a + i]}:{ors[a + i]}" for i in range(n)]))
    assert rows == g.graph_after
    out = tmp_path / "after.unitig"
    u.save_unitig(str(out))
    assert out.read_text() == g.unitig_after


@pytest.mark.parametrize("name", R.GOLDEN_FIXTURES)
def test_merge_on_fixtures(name, tmp_path):
    """The merge loop on the four paired fixtures, whose pair lists are long
    enough for std::sort to leave insertion sort (pairs_branchy: 57 records,
    many of equal support, 18 merged): the reference's merged
    count (#X), its lists after the merge (#G) and its .support.unitig bytes.
    The graph is the dump's own edge rows written as a .unitig file and re-read;
    the placements are the dump's, as the re-read lists need not keep the build
    path's order."""
    g = R.golden(name)
    u = R.unitig_graph(g, tmp_path)
    edges = u.contig_edges(all_edges=True)[0]
    for f in ("src", "dst", "offset", "orient", "n"):
        assert np.array_equal(edges[f], g.edges[f]), f
    assert np.array_equal(u.edge_twins(), g.twin)
    host = host_mate_paths(*g.args())
    s = g.summary()
    assert len(host.pairs) == s[1]
    assert u.merge_supported(host.pairs) == g.merged == s[0]
    assert_graph_after(u, g, tmp_path)


@pytest.mark.parametrize("name", R.hand_case_names())
def test_cli_support_on_the_resume_path(name, tmp_path):
    """mg_overlap -s -support by the host mirrors (no device needed):
    OverlapGraph::findSupportByMatepairsAndMerge gives the reference's summary
    lines and .unitig bytes after the merge"""
    g = R.hand_cases()[name]
    lines, unitig = R.run_cli_support(g, tmp_path, resume=True, env={"MG_DEVICE_PATHS": "0", "MG_DEVICE_PLACES": "0"})
    assert lines == R.summary_lines(g)
    assert unitig == g.unitig_after


# ---- d. what the goldens are for
def test_goldens_hold_what_the_cases_are_for():
    h = R.hand_cases()
    assert len(h) == 16
    counts = np.sum([host_counts(R.any_golden(n)) for n in ALL], axis=0)
    assert (counts > 0).all()
    assert [R.golden(n).summary()[2:] for n in ("pairs_small", "pairs_mixed", "pairs_long", "pairs_branchy")] == \
        [(0, 0, 289), (0, 0, 156), (0, 0, 33), (0, 866, 734)]
    b = R.golden("pairs_branchy")
    assert b.merged == 18 and b.summary()[:2] == (18, 57) and sum(f.count(0) for _, _, f in b.entries) == 1539
    assert h["bubble"].entries[path_entry(h["bubble"])][2] == [1, 0, 0, 0, 1]   # cleared inside a combo
    assert h["across"].entries[path_entry(h["across"])][2] == [0, 1]           # cleared across combos
    assert len(h["chain101"].entries[path_entry(h["chain101"])][1]) == 101
    assert (h["wrap"].mean[0], h["wrap"].sd[0]) == (500, 490) and h["mean0"].mean.tolist() == [210, 0]
    m = h["merge3"]  # support 4 = three entries one way and one over the twins; the second pair is freed
    assert [x[3] for x in m.merging()] == [4, 4] and [x[0] for x in m.merging()] == [1, 3] and m.summary()[:2] == (2, 3)
    seen = {(p[k], p[k + 1]) for _, p, f in m.entries for k in range(len(f)) if f[k]}
    assert any((int(m.twin[b]), int(m.twin[a])) in seen for a, b in seen)  # a pair reached in both orientations
    assert sum(st == PATH_FOUND for st, _, _ in h["orient16"].entries) == 8


def host_counts(g):
    return np.array([sum(st == k for st, _, _ in g.entries) for k in (PATH_NONE, PATH_FOUND, PATH_SAME_EDGE)])


def path_entry(g):
    return next(t for t, (st, p, _) in enumerate(g.entries) if st == PATH_FOUND and len(p) > 2)


# ---- e. errors
def test_mirror_errors():
    c = R.random_case(np.random.default_rng(5), 12, 22, 30, 2)

    def refused(match, **change):
        with pytest.raises(MgError, match=match) as e:
            host_mate_paths(*R.host_args({**c, **change}))
        assert "(-2)" in str(e.value)

    edges = c["edges"].copy()
    edges["src"][[5, 9]] = 0
    refused(r"edge 5 \(0, \d+\): its source ID is below", edges=edges)
    twin = c["twin"].copy()
    twin[[7, 3]] = len(twin)
    refused(rf"edge 3 \(\d+, \d+\): its twin {len(twin)} is not below {len(twin)}", twin=twin)
    recs = c["places"][1].copy()
    recs["edge"][[11, 4]] = len(twin) + 2
    refused(rf"placement 4: its edge {len(twin) + 2} is not below", places=(c["places"][0], recs))
    for field, value in (("id", 0), ("id", c["n_reads"] + 1), ("dataset", 2)):
        m = c["mates"][1].copy()
        m[field][[20, 6]] = value
        refused(r"mate entry 6: ", mates=(c["mates"][0], m))
    refused(r"edge 5 ", edges=edges, twin=twin, places=(c["places"][0], recs), mates=(c["mates"][0], m))
    refused(r"edge 3 ", twin=twin, places=(c["places"][0], recs), mates=(c["mates"][0], m))
    refused(r"placement 4", places=(c["places"][0], recs), mates=(c["mates"][0], m))
    bad = c["mates"][0].copy()
    bad[3] = bad[4] + 1
    with pytest.raises(MgError, match=r"bad arguments \(-1\)"):
        host_mate_paths(*R.host_args({**c, "mates": (bad, c["mates"][1])}))
    with pytest.raises(MgError, match="do not fit"):
        host_mate_paths(*R.host_args({**c, "twin": c["twin"][:-1]}))


def test_refused_pairs(tmp_path):
    """a pair that would be merged and is one edge twice, or an edge and its twin, is named and nothing changes"""
    g = R.hand_cases()["merge3"]
    u = R.unitig_graph(g, tmp_path)
    twin = u.edge_twins()
    before = tmp_path / "before.unitig"
    u.save_unitig(str(before))
    for e2, what in ((int(twin[0]), "an edge and its twin"), (0, "one edge twice")):
        pairs = np.array([(2, 4, 5), (0, e2, 3)], dtype=PAIR_DTYPE)
        with pytest.raises(MgError, match=what + r".*\(-5\)"):
            u.merge_supported(pairs)
        after = tmp_path / "after.unitig"
        u.save_unitig(str(after))
        assert after.read_text() == before.read_text()
    assert u.merge_supported(np.array([(2, 4, 5), (0, int(twin[0]), 2)], dtype=PAIR_DTYPE)) == 1  # below min_support
    with pytest.raises(MgError, match="outside the graph"):
        u.merge_supported(np.array([(0, 10 ** 6, 3)], dtype=PAIR_DTYPE))


# ---- f. random graphs
@pytest.mark.parametrize("seed", range(8))
def test_restatement_equals_mirror(seed):
    rng = np.random.default_rng(seed)
    c = R.random_case(rng, 12, 22, 30, 2)
    if seed == 7:  # what the reference cannot produce: orientations above 3 and an offset near 2^64
        c["edges"]["orient"][::5] = 7
        c["edges"]["offset"][3] = (1 << 64) - 5
    host = host_mate_paths(*R.host_args(c))
    want = R.restate(c["edges"], c["twin"], c["places"], c["mates"], c["mean"], c["sd"])
    assert R.entries_of(host) == want
    pairs, counters = R.pair_list(c["edges"], c["twin"], want)
    assert R.pairs_of(host) == pairs and host.counters == counters
    # a budget at the median cost of the searching entries: exactly the entries above it are deferred
    units = np.array([u for _, u, _, _ in want])
    budget = int(np.median(units[units > 0])) if (units > 0).any() else 1
    part = host_mate_paths(*R.host_args(c), budget=budget)
    assert np.array_equal(part.status == PATH_DEFERRED, units > budget) and part.deferred == int((units > budget).sum())
    assert (part.visits[units > budget] == budget + 1).all() and (part.start[1:] >= part.start[:-1]).all()
    done = part.finish()
    assert R.entries_of(done) == want and R.pairs_of(done) == pairs and done.counters == counters


# ---- g. the sanitizer program
def test_paths_check_asan_builds_and_runs_clean():
    """host code only: the mirror, the merge and a stand-alone driver under ASan + UBSan, from its own main"""
    p = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "metagenomics_amd", "csrc"), "paths_check_asan"],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "paths_check: ok" in p.stdout and "ERROR" not in p.stdout + p.stderr
