"""Safe chains found on the device (mg_build_chains / mg_copy_chains,
metagenomics_amd/csrc/device/mg_chains.hip): list ranking by pointer jumping over
the (node, port) states, two scans, a scatter of the read lists.  Expected
arrays: the host's serial walk (host_chains, mg::chains_build, itself held
against a Python model in tests/test_chain_contract_model.py), array for array,
counters included.  Synthetic graphs of at most a few thousand nodes built by
tests/chains_ref.py; then the fixtures end to end from the device's rows."""
import functools

import numpy as np
import pytest

from chains_ref import GraphBuilder
from conftest import FIXTURES, fixture_input, load_meta
from metagenomics_amd.overlap import (CHAIN_EDGE_DTYPE, CHAIN_INFO, Dataset, MgError, OverlapEngine, UnitigGraph,
                                      host_chains)
from test_unitig import golden_text

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025]


@pytest.fixture(scope="module")
def engine():
    e = OverlapEngine(0)
    yield e
    e.close()


def device_chains(e, start, edges, rounds=0):
    e.set_option("chain_rounds", rounds)
    try:
        n = e.build_chains(start, edges)
    finally:
        e.set_option("chain_rounds", 0)
    ch = e.chains()
    assert ch.chains.shape[0] == n == ch.info["n_chains"] and ch.reads.shape[0] == 2 * ch.info["n_contracted"]
    return ch


def assert_same(got, want):
    assert got.info == want.info
    for g, w in zip(got.arrays(), want.arrays()):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)


def clean_end(g):
    """a fresh end node that is certainly not interior (degree 3 with its chain)"""
    a = g.node()
    g.leaves(a, 2)
    return a


def clean_ends(g):
    return clean_end(g), clean_end(g)


@functools.lru_cache(maxsize=None)
def lengths_graphs():
    """one chain of every length, chain nodes at IDs 1 and N, both port orders"""
    g = GraphBuilder(1)
    mids = {}
    for k in LENGTHS:
        a, b = clean_ends(g)
        mids[k] = g.chain(a, b, k)
    n = len(g.adj) - 1
    pin = {mids[1025][0]: 1, mids[3][1]: n}
    out = []
    for rev in (False, True):
        g.rng = np.random.default_rng(2)  # the same IDs and shuffles, every list then reversed
        start, edges = g.csr(pin=pin, reverse_lists=rev)
        out.append((start, edges, host_chains(start, edges)))
    return out


@pytest.mark.parametrize("flip", [0, 1])
def test_chain_lengths(engine, flip):
    start, edges, want = lengths_graphs()[flip]
    assert sorted(want.chains["n"].tolist()) == LENGTHS and want.info["n_unsafe_chains"] == 0
    assert want.info["n_interior"] == sum(LENGTHS) == want.info["n_contracted"]
    assert want.info["rounds"] == 12  # 1,025 hops: rounds 1..11 find new ends, round 12 none
    reads = set(want.reads.tolist())
    assert 1 in reads and start.shape[0] - 2 in reads
    assert_same(device_chains(engine, start, edges), want)


def test_port_orders_differ():
    (_, e0, a), (_, e1, b) = lengths_graphs()
    assert not np.array_equal(e0["dst"], e1["dst"]) and sorted(a.chains["n"].tolist()) == sorted(b.chains["n"].tolist())


@functools.lru_cache(maxsize=None)
def zoo():
    """every special structure of the definitions in one graph"""
    g = GraphBuilder(3)
    keep = set()
    a = clean_end(g)  # a chain from a node to itself
    g.chain(a, a, 4)
    x = g.node()  # v - x twice: v is interior, its chain runs from x to x
    g.leaves(x, 3)
    v, s = g.node(), g.strand()
    g.edge(v, s, x, g.strand())
    g.edge(v, 1 - s, x, g.strand())
    for lens_ in ((2, 6), (1, 3, 8)):  # two and three parallel chains
        a, b = clean_ends(g)
        for k in lens_:
            g.chain(a, b, k)
    a, b = clean_ends(g)  # a chain beside a direct edge
    g.chain(a, b, 5)
    g.chain(a, b, 0)
    for k in (2, 3, 4, 65):  # pure cycles
        g.cycle(k)
    a, b = clean_ends(g)  # a type mismatch in the middle: two chains
    g.chain(a, b, 7, mismatch_at=3)
    loop, s = g.node(), g.strand()  # a [loop, twin] node
    g.edge(loop, s, loop, s)
    g.chain(clean_end(g), g.node(), 5)  # a chain to a leaf
    m1, m2 = g.nodes(2)  # ends that are mismatched nodes of degree 2
    g.edge(g.node(), g.strand(), m1, 0)
    g.edge(m2, 1, g.node(), g.strand())
    g.chain(m1, m2, 6, sa=1, sb=0)
    for deg, front in ((65, True), (65, False), (300, True), (300, False)):  # hubs, head first / last in the list
        hub, b = g.node(), clean_end(g)
        if front:
            g.chain(hub, b, 6)
        g.leaves(hub, deg - 1)
        if not front:
            g.chain(hub, b, 6)
        keep.add(hub)
    out = []
    for rev in (False, True):
        g.rng = np.random.default_rng(4)
        start, edges = g.csr(reverse_lists=rev, keep_order=keep)
        out.append((start, edges, host_chains(start, edges)))
    return out


@pytest.mark.parametrize("flip", [0, 1])
def test_zoo(engine, flip):
    start, edges, want = zoo()[flip]
    i = want.info
    # a = a, x - x, 2 + 3 parallel, 1 beside an edge are not safe; the cycles' 74 nodes never end
    assert i["n_unsafe_chains"] == 8 and i["n_unresolved_states"] == 2 * (2 + 3 + 4 + 65)
    deg = np.diff(start[1:]).astype(np.int64)
    heads = start[want.chains["a"]].astype(np.int64) + want.chains["pa"]
    assert np.all(np.diff(heads) > 0)  # ascending start[a] + pa
    hubs = want.chains[deg[want.chains["a"] - 1] >= 65]
    hubs_b = want.chains[deg[want.chains["b"] - 1] >= 65]
    at = sorted([(int(deg[c["a"] - 1]), int(c["pa"])) for c in hubs] + [(int(deg[c["b"] - 1]), int(c["pb"])) for c in hubs_b])
    assert at == [(65, 0), (65, 64), (300, 0), (300, 299)]
    assert sorted(want.chains["n"].tolist()) == sorted([3, 3, 5, 6, 6, 6, 6, 6])
    assert_same(device_chains(engine, start, edges), want)


def star():
    g = GraphBuilder(8)
    g.leaves(g.node(), 40)
    return g.csr()


def cycles_only():
    g = GraphBuilder(9)
    g.cycle(3)
    g.cycle(5)
    return g.csr()


@pytest.mark.parametrize("name", ["empty", "no_edges", "no_interior", "cycles_only"])
def test_degenerate_graphs(engine, name):
    empty = np.zeros(0, dtype=CHAIN_EDGE_DTYPE)
    start, edges = {"empty": lambda: (np.zeros(2, dtype=np.uint64), empty),
                    "no_edges": lambda: (np.zeros(7, dtype=np.uint64), empty),
                    "no_interior": star, "cycles_only": cycles_only}[name]()
    want = host_chains(start, edges)
    assert want.info["n_chains"] == 0 and want.chains.shape[0] == 0
    if name == "cycles_only":
        assert (want.info["n_interior"], want.info["n_unresolved_states"], want.info["rounds"]) == (8, 16, 1)
    assert_same(device_chains(engine, start, edges), want)


@functools.lru_cache(maxsize=None)
def capped_graph():
    g = GraphBuilder(10)
    for k in (1, 2, 3, 4, 5, 8, 9, 65):
        g.chain(*clean_ends(g), k)
    a, b = clean_ends(g)  # a short chain beside a long one: unknown ends make the short one unsafe
    g.chain(a, b, 2)
    g.chain(a, b, 20)
    return g.csr()


@pytest.mark.parametrize("rounds", [1, 2, 3])
def test_round_cap(engine, rounds, tmp_path):
    """Chains over 2^rounds nodes are left out, and a half-edge that heads one makes
    its node's chains unsafe; apply + loop still gives the plain loop's graph."""
    start, edges = capped_graph()
    full = host_chains(start, edges)
    want = host_chains(start, edges, rounds)
    kept = [k for k in (1, 2, 3, 4, 5, 8, 9, 65) if k <= 2 ** rounds]
    assert sorted(want.chains["n"].tolist()) == kept and want.info["rounds"] == rounds
    assert sorted(full.chains["n"].tolist()) == [1, 2, 3, 4, 5, 8, 9, 65] and full.info["n_unsafe_chains"] == 2
    assert want.info["n_unresolved_states"] > 0 == full.info["n_unresolved_states"]
    got = device_chains(engine, start, edges, rounds)
    assert_same(got, want)
    texts = []
    for chains in (None, got):
        g = UnitigGraph.from_csr(start, edges, chains=chains)
        g.save_lists(str(tmp_path / "lists"))
        texts.append(((tmp_path / "lists").read_text(), g.nodes, g.edges, g.iterations, g.merged, g.dead_end_nodes))
        g.close()
    assert texts[0] == texts[1]


def test_two_calls_give_identical_arrays(engine):
    start, edges, want = zoo()[0]
    a = device_chains(engine, start, edges)
    small = capped_graph()
    device_chains(engine, *small)  # (another graph in between: buffers are reused)
    b = device_chains(engine, start, edges)
    assert_same(a, b)
    assert_same(b, want)
    assert engine.chains_ms > 0


def test_malformed_csr_is_refused(engine):
    start, edges, _ = zoo()[0]
    n, m = start.shape[0] - 2, edges.shape[0]

    def refused(s, e, pattern):
        with pytest.raises(MgError, match=pattern):
            engine.build_chains(s, e)
        with pytest.raises(MgError, match=pattern):
            host_chains(s, e)
        with pytest.raises(MgError, match="mg_build_chains must succeed"):
            engine.chains()

    for value in (0, n + 1, 2 ** 32 - 1):
        bad = edges.copy()
        bad["dst"][m // 2] = value
        refused(start, bad, r"half-edge %d .*dst %d outside.*\(-2\)" % (m // 2, value))
    for value in (m, 2 ** 32 - 1):
        bad = edges.copy()
        bad["twin"][7] = value
        refused(start, bad, r"half-edge .*twin .*\(-2\)")
    bad = edges.copy()  # two half-edges of one list that both name the same twin
    k = int(np.argmax(np.diff(start[1:]).astype(np.int64) >= 3))
    e0 = int(start[k + 1])
    bad["twin"][e0] = bad["twin"][e0 + 1]
    if bad["dst"][e0] != bad["dst"][e0 + 1]:
        bad["dst"][e0] = bad["dst"][e0 + 1]
    refused(start, bad, r"half-edge %d .*twin\[twin\].*\(-2\)" % e0)
    s = start.copy()
    s[10], s[11] = s[11], s[10] - 1
    refused(s, edges, r"start\[.*\(-2\)")
    s = start.copy()
    s[-1] += 1
    refused(s, edges, r"start\[.*\(-2\)")
    assert_same(device_chains(engine, start, edges), zoo()[0][2])  # the context still works


def test_sharded_context_refuses():
    e = OverlapEngine(0)
    try:
        e.set_shard(0, 2)
        with pytest.raises(MgError, match="sharded"):
            e.build_chains(*star())
    finally:
        e.close()


def device_rows(e, ds, l):
    e.upload(ds)
    e.build_index(l, 0)
    e.mark_contained()
    return e.rows(e.find_overlaps())


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_end_to_end(engine, name, tmp_path):
    """reads -> device rows -> replay -> device chains -> apply + loop: the reference's graph"""
    meta = load_meta(name)
    ds = Dataset.from_files([fixture_input(name)], meta["l"])
    rows = device_rows(engine, ds, meta["l"])
    g = UnitigGraph(rows, ds.packed()[1], meta["l"], chains=engine)
    u = meta["unitig"]
    assert (g.nodes, g.edges, g.iterations) == (u["nodes"], u["edges"], u["iterations"])
    assert set(g.chain_info) == set(CHAIN_INFO)
    if name in ("branchy", "small"):
        assert g.chain_info["n_contracted"] > 0
    g.save_lists(str(tmp_path / "lists"))
    assert (tmp_path / "lists").read_text() == golden_text(name, "lists_file")
    g.sort_edges()
    g.save_unitig(str(tmp_path / "x.unitig"))
    assert (tmp_path / "x.unitig").read_text() == golden_text(name, "file")
    g.close()
