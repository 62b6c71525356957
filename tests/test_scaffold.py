"""Scaffolder support on the device (metagenomics_amd/csrc/device/mg_scaffold.hip)
array for array against the host mirror, which tests/test_scaffold_host.py pins
to the plain-Python restatement of the reference's loop, and against the lines
the reference's own scaffolder() printed (tests/golden/scaffold.json,
scaffold_cases.json.gz).

Shapes are the smallest at which the kernels can still go wrong: 63, 64 and 65
mate entries (a wavefront and its neighbours); placement segments holding 0, 1,
2, 64 and 65 records of the wanted strand (the count loop stops at 2 across a
wavefront's worth); zero counted entries (no sort), one, and all entries in one
record; 65,535 / 65,536 / 65,537 edges with the pairs on the last ones (the key
crosses 32 bits); a pair first seen in its second orientation; distance sums
above 2^32 and past 2^64; the resident mate lists and placements; every kind of
invalid input, with no score launch behind it; a small call after a larger one
on the same context."""
import numpy as np
import pytest

import paths_ref as P
import scaffold_ref as R
from metagenomics_amd.overlap import SCAF_COUNTED, MgError, OverlapEngine, host_scaffold_pairs, lib

pytestmark = pytest.mark.gpu

F, V = 1, 0
TWIN4 = [1, 0, 3, 2, 5, 4, 7, 6]


def device(c, places=True, mates=True, eng=None):
    """scaffold_pairs over the dict c with the caller's CSRs (or the resident ones of eng)"""
    own = eng is None
    eng = eng or OverlapEngine(0)
    try:
        return eng.scaffold_pairs(c["twin"], len(c["twin"]), c["mean"], c["sd"], places=c["places"] if places else None,
                                  mates=c["mates"] if mates else None, n_reads=c["n_reads"])
    finally:
        if own:
            eng.close()


def host(c):
    return host_scaffold_pairs(*R.host_args(c))


@pytest.fixture(scope="module")
def eng():
    e = OverlapEngine(0)
    yield e
    e.close()


@pytest.mark.parametrize("name", R.GOLDEN_FIXTURES + R.hand_case_names())
def test_reference_scaffolder_runs(name, eng):
    """the reference's own scaffolder() runs: the device explains every line it printed"""
    g = R.any_golden(name)
    c = R.from_golden(g)
    dev = device(c, eng=eng)
    R.assert_explains_reference(dev, g, nothing_freed=name not in ("pairs_branchy", "freed"))
    R.assert_same(dev, host(c))


@pytest.mark.parametrize("name", R.GOLDEN_FIXTURES + R.hand_case_names())
def test_device_support_then_merge_reproduces_the_reference(name, eng, tmp_path):
    """UnitigGraph.scaffold_support through the engine, then the merge: the
    reference's lines character for character, its return value, its lists and
    its .unitig bytes after the merge"""
    g = R.any_golden(name)
    u = P.unitig_graph(g, tmp_path)
    s = u.scaffold_support(g.mates, g.mean, g.sd, engine=eng)
    R.assert_same(s, host(R.from_golden(g)))
    words, lens = R.packed_reads(g, tmp_path)
    merged, lines = u.merge_scaffold(s.pairs, words, lens)
    assert lines == g.raw_lines and merged == g.merged
    R.assert_graph_after(u, g, tmp_path)


@pytest.mark.parametrize("name", P.GOLDEN_FIXTURES + P.hand_case_names())
def test_reference_path_graphs(name, eng):
    """more graphs of the reference's making: the inputs its paths driver dumped"""
    c = R.from_golden(P.any_golden(name))
    R.assert_same(device(c, eng=eng), host(c))


@pytest.mark.parametrize("entries", [63, 64, 65])
def test_wavefront_edges(entries, eng):
    c = R.random_case(np.random.default_rng(entries), 40, 2, entries)
    assert int(c["mates"][0][-1]) == entries
    h = host(c)
    assert all(h.counters) and int(h.pairs["support"].max()) > 1
    R.assert_same(device(c, eng=eng), h)


@pytest.mark.parametrize("wanted", [0, 1, 2, 64, 65])
def test_segment_lengths(wanted, eng):
    """read 1 holds `wanted` forward placements behind 70 reverse ones, read 3 the
    same number of reverse ones between forward ones: unique only for 1"""
    places = {1: [(4, V, 3)] * 70 + [(0, F, 7)] * wanted,
              3: [(6, F, 1)] * 3 + [(2, V, 9)] * wanted + [(6, F, 1)] * 70,
              2: [(0, F, 7)], 4: [(2, V, 9)]}
    mates = {1: [(3, 1, 0), (4, 1, 0)], 2: [(3, 1, 0), (4, 1, 0)]}
    c = R.make_case(4, TWIN4, places, mates, [100], [5])
    h = host(c)
    assert h.counters[SCAF_COUNTED] == (4 if wanted == 1 else 1)
    R.assert_same(device(c, eng=eng), h)


def test_zero_one_and_all_in_one_record(eng):
    none = R.make_case(4, TWIN4, {1: [(0, F, 1)], 2: [(0, V, 1)]}, {1: [(2, 1, 0)] * 3}, [100], [5])
    h = host(none)
    assert h.counters[SCAF_COUNTED] == 0 and len(h.pairs) == 0
    R.assert_same(device(none, eng=eng), h)
    one = R.make_case(4, TWIN4, {1: [(0, F, 1)], 2: [(2, V, 1)]}, {1: [(2, 1, 0)]}, [100], [5])
    h = host(one)
    assert R.pairs_of(h) == [(1, 2, 1, 2)]
    R.assert_same(device(one, eng=eng), h)
    n = 300  # reads 1..150 forward on edge 0, 151..300 reverse on edge 2, read a and read a + 150 in each other's list
    places = {a: [(0, F, a)] if a <= 150 else [(2, V, 1)] for a in range(1, n + 1)}
    mates = {a: [(a + 150, 1, 0)] if a <= 150 else [(a - 150, 2, 0)] for a in range(1, n + 1)}
    c = R.make_case(n, TWIN4, places, mates, [1000], [0])
    h = host(c)
    assert R.pairs_of(h) == [(1, 2, 150, sum(range(1, 151)) + 150)] and h.counters == (150, 0, 0, 0, 150)
    R.assert_same(device(c, eng=eng), h)


@pytest.mark.parametrize("n_edges", [65535, 65536, 65537, 65538])
def test_key_crosses_32_bits(n_edges, eng):
    """pairs on the last edges: twin[L1] * E + L2 passes 2^32 from 65,536 edges
    on (an odd count leaves edge 0 its own twin)"""
    twin = np.arange(n_edges, dtype=np.uint32)
    lo = n_edges & 1
    twin[lo:] = (np.arange(n_edges - lo, dtype=np.uint32) ^ 1) + lo
    e = n_edges - 1
    places = {1: [(e, F, 5)], 2: [(e - 2, V, 6)], 3: [(e - 2, F, 7)], 4: [(e, V, 8)], 5: [(e - 4, F, 1)], 6: [(e, V, 2)],
              7: [(3 + lo, F, 1)], 8: [(e - 1, V, 1)]}
    mates = {1: [(2, 1, 0)], 3: [(4, 1, 0)], 5: [(6, 1, 0)], 7: [(8, 1, 0)]}
    c = R.make_case(8, twin, places, mates, [100], [5])
    h = host(c)
    R.assert_equals_restatement(h, c)
    assert h.pairs["support"].tolist() == [2, 1, 1]
    R.assert_same(device(c, eng=eng), h)


def test_first_seen_in_its_second_orientation(eng):
    places = {1: [(2, F, 7)], 2: [(0, V, 8)], 3: [(0, F, 5)], 4: [(2, V, 6)]}
    c = R.make_case(4, TWIN4, places, {1: [(2, 1, 0)], 3: [(4, 1, 0)]}, [100], [5])
    h = host(c)
    assert R.pairs_of(h) == [(3, 0, 2, 26)]
    R.assert_same(device(c, eng=eng), h)


def test_large_and_wrapping_distance_sums(eng):
    big = (1 << 63) - 3
    places = {1: [(0, F, big)], 2: [(2, V, 10)], 3: [(0, F, big)], 4: [(2, V, 11)], 5: [(0, F, big)], 6: [(2, V, 12)],
              7: [(4, F, 1 << 31)], 8: [(4, F, (1 << 31) + 1)], 9: [(6, V, 1 << 31)]}
    mates = {1: [(2, 1, 0)], 3: [(4, 1, 0)], 5: [(6, 1, 0)], 7: [(9, 1, 0)], 8: [(9, 1, 0)]}
    c = R.make_case(9, TWIN4, places, mates, [1 << 62], [1 << 61])
    h = host(c)
    assert R.pairs_of(h) == [(1, 2, 3, (3 * big + 33) & R.M64), (5, 6, 2, (1 << 33) + 1)]
    R.assert_same(device(c, eng=eng), h)


def test_interleaved_records_keep_first_seen_order(eng):
    """many records, opened in an order that is not the key order, joined later"""
    c = R.random_case(np.random.default_rng(11), 400, 12, 900, p_multi=0.05)
    h = host(c)
    keys = [int(p["edge1"]) * 24 + int(p["edge2"]) for p in h.pairs]
    assert len(keys) > 50 and keys != sorted(keys) and int(h.pairs["support"].max()) > 3
    R.assert_same(device(c, eng=eng), h)


def test_resident_mate_lists_and_placements(tmp_path):
    """ingest -> index -> contained -> mate_pairs -> build_placements on
    pairs_branchy: the resident CSRs give what the caller's CSRs give (only
    lists of one placement are read, so the (edge, position) order is immaterial)"""
    g = R.golden("pairs_branchy")
    c = R.from_golden(g)
    want = host(c)
    assert all(want.counters)
    pe, se = g.write_files(tmp_path)
    e = OverlapEngine(0)
    try:
        assert e.ingest_files(pe + se, g.l)["n_unique"] == g.n
        e.build_index(g.l, 21 if g.l > 21 else 0)
        e.mark_contained()
        e.mate_pairs(pe, g.l)
        R.assert_same(device(c, mates=False, eng=e), want)
        e.build_placements(*g.graph)
        R.assert_same(device(c, places=False, mates=False, eng=e), want)
        R.assert_same(device(c, places=False, eng=e), want)
    finally:
        e.close()


def test_validation_errors():
    c = R.random_case(np.random.default_rng(5), 40, 4, 60)
    e = OverlapEngine(0)
    try:
        def refused(match, **change):
            with pytest.raises(MgError, match=match) as x:
                device({**c, **change}, eng=e)
            assert "(-2)" in str(x.value)
            with pytest.raises(MgError, match="must succeed first"):  # no result of a refused call is left
                e._check(lib().mg_scaffold_info(e._h, None, None), "info")

        twin = c["twin"].copy()
        twin[[7, 3]] = len(twin)
        refused(rf"edge 3: its twin {len(twin)} is not below {len(twin)}", twin=twin)
        recs = c["places"][1].copy()
        recs["edge"][[11, 4]] = len(twin) + 2
        refused(rf"placement 4: its edge {len(twin) + 2} is not below", places=(c["places"][0], recs))
        for field, value in (("id", 0), ("id", c["n_reads"] + 1), ("dataset", 2)):
            m = c["mates"][1].copy()
            m[field][[20, 6]] = value
            refused(r"mate entry 6: ", mates=(c["mates"][0], m))
        # the order of the kinds: a twin before a placement, a placement before a mate
        refused(r"edge 3: ", twin=twin, places=(c["places"][0], recs), mates=(c["mates"][0], m))
        refused(r"placement 4", places=(c["places"][0], recs), mates=(c["mates"][0], m))
        R.assert_same(device(c, eng=e), host(c))  # the context is still good
    finally:
        e.close()


def test_bad_arguments_and_sharded_contexts():
    c = R.random_case(np.random.default_rng(5), 40, 4, 60)
    e = OverlapEngine(0)
    try:
        with pytest.raises(MgError, match="no resident placements"):
            device(c, places=False, eng=e)
        with pytest.raises(MgError, match="no resident mate lists"):
            device(c, mates=False, eng=e)
        bad = c["mates"][0].copy()
        bad[3] = bad[4] + 1
        with pytest.raises(MgError, match="mate_start must not decrease"):
            device({**c, "mates": (bad, c["mates"][1])}, eng=e)
        e.set_shard(0, 2)
        with pytest.raises(MgError, match="sharded"):
            device(c, eng=e)
    finally:
        e.close()


def test_a_small_call_after_a_larger_one():
    big = R.random_case(np.random.default_rng(21), 400, 6, 900)
    small = R.random_case(np.random.default_rng(22), 30, 2, 40)
    e = OverlapEngine(0)
    try:
        R.assert_same(device(big, eng=e), host(big))
        R.assert_same(device(small, eng=e), host(small))
        R.assert_same(device(big, eng=e), host(big))
    finally:
        e.close()
