"""Mate-pair path support on the device (metagenomics_amd/csrc/device/mg_paths.hip)
against the reference's own dumps (tests/golden/paths.json, paths_cases.json.gz)
and, on random graphs, array for array against the host mirror, which
tests/test_paths_host.py pins to the reference and to the plain-Python
restatement.

Shapes are the smallest at which the kernels can still go wrong: 63, 64 and 65
mate entries (a wavefront and its neighbours); 200 entries in batches of 64
(three full batches and a part); a budget of one work unit (every search is
deferred) and a budget one unit below the bubble case's cost (only it is
deferred); the resident mate lists and the resident placements; every kind of
invalid input, with no explore launch behind it."""
import numpy as np
import pytest

import paths_ref as R
from metagenomics_amd.overlap import PATH_DEFERRED, PATH_FOUND, MgError, OverlapEngine, host_mate_paths, lib

pytestmark = pytest.mark.gpu


def device_paths(c, places=True, mates=True, eng=None, **options):
    """mate_paths over the dict c with the caller's CSRs (or the resident ones of eng)"""
    own = eng is None
    eng = eng or OverlapEngine(0)
    try:
        for k, v in options.items():
            eng.set_option(k, v)
        return eng.mate_paths(c["edges"], c["twin"], c["mean"], c["sd"], places=c["places"] if places else None,
                              mates=c["mates"] if mates else None, n_reads=c["n_reads"])
    finally:
        if own:
            eng.close()


def assert_same(dev, host):
    for name in ("status", "visits", "start", "path", "flags", "pairs"):
        assert np.array_equal(getattr(dev, name), getattr(host, name)), name + " differs"
    assert dev.counters == host.counters and dev.deferred == host.deferred


def case_of(g):
    return {"n_reads": g.n, "edges": g.edges, "twin": g.twin, "places": g.places, "mates": g.mates, "mean": g.mean,
            "sd": g.sd}


def want_of(g):
    """the reference's entries, and the pair list and counters the restatement makes of them"""
    want = [(st, p, f) for st, p, f in g.entries]
    pairs, counters = R.pair_list(g.edges, g.twin, [(st, 0, p, f) for st, p, f in g.entries])
    return want, pairs, counters


# ---- the reference's own results
@pytest.mark.parametrize("name", R.GOLDEN_FIXTURES + R.hand_case_names())
def test_device_equals_reference(name):
    g = R.any_golden(name)
    want, pairs, counters = want_of(g)
    dev = device_paths(case_of(g))
    assert dev.deferred == 0
    assert [(st, p, f) for st, _, p, f in R.entries_of(dev)] == want
    assert R.pairs_of(dev) == pairs and dev.counters == counters
    s = g.summary()
    if s is not None:
        assert (len(pairs),) + counters == s[1:]
    assert_same(dev, host_mate_paths(*g.args()))


@pytest.mark.parametrize("name", R.GOLDEN_FIXTURES)
def test_resident_mate_lists_and_placements(name, tmp_path):
    """the reads ingested and the mate lists built on the device: the resident
    mate CSR gives the reference's entries; the resident placements ((edge,
    position) order) give the same statuses and the same supported set"""
    g = R.golden(name)
    want, pairs, counters = want_of(g)
    pe, se = g.write_files(tmp_path)
    eng = OverlapEngine(0)
    try:
        assert eng.ingest_files(pe + se, g.l)["n_unique"] == g.n
        eng.build_index(g.l, 21 if g.l > 21 else 0)
        eng.mark_contained()
        eng.mate_pairs(pe, g.l)
        dev = device_paths(case_of(g), mates=False, eng=eng)
        assert [(st, p, f) for st, _, p, f in R.entries_of(dev)] == want
        assert R.pairs_of(dev) == pairs and dev.counters == counters
        eng.build_placements(*g.graph)
        res = device_paths(case_of(g), places=False, mates=False, eng=eng)
        assert np.array_equal(res.status, dev.status) and res.counters == counters
        canon = lambda ps: {min((a, b), (int(g.twin[b]), int(g.twin[a]))) for a, b, _ in R.pairs_of(ps)}
        assert canon(res) == canon(dev)
        assert_same(res, host_mate_paths(g.n, g.edges, g.twin, eng.placements(), g.mates, g.mean, g.sd))
    finally:
        eng.close()


# ---- random graphs: the device equals the mirror array for array
def exact_mates(total):
    """mates_per_read for random_case: `total` entries over the first reads, three each"""
    return lambda a: 3 if 3 * a <= total else max(0, total - 3 * (a - 1))


@pytest.mark.parametrize("entries,seed", [(63, 3), (64, 4), (65, 3)])  # (seeds whose graphs hold paths and cleared flags)
def test_wavefront_edges(entries, seed):
    c = R.random_case(np.random.default_rng(seed), 12, 22, 30, exact_mates(entries))
    assert int(c["mates"][0][-1]) == entries
    host = host_mate_paths(*R.host_args(c))
    assert (host.status == PATH_FOUND).sum() >= 3 and (host.flags == 0).sum() > (host.status == PATH_FOUND).sum()
    assert_same(device_paths(c), host)


def test_batch_edges():
    """200 entries in batches of 64: the path space and the starts run through four launches"""
    c = R.random_case(np.random.default_rng(1), 14, 26, 60, exact_mates(200))
    host = host_mate_paths(*R.host_args(c))
    assert (host.status == PATH_FOUND).sum() >= 4 and (host.flags == 0).sum() > (host.status == PATH_FOUND).sum()
    assert_same(device_paths(c, path_batch=64), host)
    assert_same(device_paths(c, path_batch=1), host)
    assert_same(device_paths(c), host)


def test_budget_of_one_unit():
    """every entry that searches at all is deferred; the mirror finishes them to the undeferred answer"""
    c = R.random_case(np.random.default_rng(4), 12, 22, 30, 2)
    full = host_mate_paths(*R.host_args(c))
    assert (full.status == PATH_FOUND).sum() >= 3
    dev = device_paths(c, path_budget=1)
    assert dev.deferred == int((full.visits > 1).sum()) > 10
    assert np.array_equal(dev.status == PATH_DEFERRED, full.visits > 1)
    assert_same(dev, host_mate_paths(*R.host_args(c), budget=1))
    done = dev.finish()
    assert done.deferred == 0
    for name in ("status", "start", "path", "flags", "pairs"):
        assert np.array_equal(getattr(done, name), getattr(full, name)), name
    assert done.counters == full.counters
    assert np.array_equal(done.visits[full.visits > 1], full.visits[full.visits > 1])


def test_budget_defers_exactly_the_bubble_case():
    g = R.hand_cases()["bubble"]
    full = host_mate_paths(*g.args())
    t = int(np.argmax(full.visits))
    top = int(full.visits[t])
    assert (full.visits == top).sum() == 1 and full.status[t] == PATH_FOUND and 0 in full.paths()[t][1]
    dev = device_paths(case_of(g), path_budget=top - 1)
    assert dev.deferred == 1 and dev.status[t] == PATH_DEFERRED and dev.visits[t] == top
    assert_same(dev, host_mate_paths(*g.args(), budget=top - 1))
    done = dev.finish()
    for name in ("status", "visits", "start", "path", "flags", "pairs"):
        assert np.array_equal(getattr(done, name), getattr(full, name)), name
    assert done.counters == full.counters
    assert device_paths(case_of(g), path_budget=top).deferred == 0


# ---- validation: the first offender is named and nothing is explored
def test_validation_errors():
    c = R.random_case(np.random.default_rng(5), 12, 22, 30, 2)
    eng = OverlapEngine(0)
    try:
        def refused(match, **change):
            with pytest.raises(MgError, match=match) as e:
                device_paths({**c, **change}, eng=eng)
            assert "(-2)" in str(e.value)
            with pytest.raises(MgError, match="must succeed first"):  # no result of a refused call is left
                eng._check(lib().mg_mate_paths_info(
                    eng._h, None, None), "info")

        edges = c["edges"].copy()
        edges["src"][[5, 9]] = 0  # edges 5 and 9 fall below their predecessors: 5 is named
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
        # the order of the kinds: an unsorted edge before a twin, a twin before a placement, a placement before a mate
        refused(r"edge 5 ", edges=edges, twin=twin, places=(c["places"][0], recs), mates=(c["mates"][0], m))
        refused(r"edge 3 ", twin=twin, places=(c["places"][0], recs), mates=(c["mates"][0], m))
        refused(r"placement 4", places=(c["places"][0], recs), mates=(c["mates"][0], m))
        assert_same(device_paths(c, eng=eng), host_mate_paths(*R.host_args(c)))  # the context is still good
    finally:
        eng.close()


def test_bad_arguments_and_sharded_contexts():
    c = R.random_case(np.random.default_rng(5), 12, 22, 30, 2)
    eng = OverlapEngine(0)
    try:
        with pytest.raises(MgError, match="no resident placements"):
            device_paths(c, places=False, eng=eng)
        with pytest.raises(MgError, match="no resident mate lists"):
            device_paths(c, mates=False, eng=eng)
        bad = c["mates"][0].copy()
        bad[3] = bad[4] + 1
        with pytest.raises(MgError, match="mate_start must not decrease"):
            device_paths({**c, "mates": (bad, c["mates"][1])}, eng=eng)
        eng.set_shard(0, 2)
        with pytest.raises(MgError, match="sharded"):
            device_paths(c, eng=eng)
    finally:
        eng.close()
