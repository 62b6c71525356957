"""The argument behind the safe chains, checked on a pure-Python
model: contracting the safe chains of a graph first and then running the
reference's contraction loop unchanged (the contracted nodes credited to the
first pass) gives the state the loop alone gives -- every list in list order,
every edge's read list, every read's location lists in list order, the
counters and the iteration count.  tests/chains_ref.py restates the loop
(mg_unitig.cpp) and finds the chains from their definitions; random bidirected
multigraphs with hubs, parallel chains, chains beside a direct edge, a = b
chains, pure cycles, leaf tails, type mismatches, shuffled IDs and list orders
and offsets up to 65,535.  The C++ loop, mirror and apply step are then held
against the same model.  CPU only."""
import numpy as np
import pytest

from chains_ref import LoopModel, python_chains, random_graph
from metagenomics_amd.overlap import UnitigGraph, host_chains

GRAPHS = 300


def test_precontraction_is_exact_on_the_model():
    contracted = chains = several = subsets = 0
    for seed in range(GRAPHS):
        start, edges = random_graph(seed)
        plain = LoopModel(start, edges)
        it_plain = plain.contract()
        table, reads, offs, ors, _, _ = python_chains(start, edges)
        pre = LoopModel(start, edges)
        credit = pre.apply_chains(table, reads, offs, ors)
        assert credit == int(table["n"].sum())
        it_pre = pre.contract(credit)
        assert it_pre == it_plain, seed
        assert pre.state() == plain.state(), seed
        contracted += credit
        chains += table.shape[0]
        several += it_plain > 2
        if table.shape[0] > 1:  # any subset of the safe chains is exact as well
            sub = LoopModel(start, edges)
            credit = sub.apply_chains(table[seed % 2::2], reads, offs, ors)
            assert sub.contract(credit) == it_plain and sub.state() == plain.state(), seed
            subsets += 1
    assert contracted > 3 * GRAPHS and chains > GRAPHS and several > 0 and subsets > GRAPHS // 4


@pytest.mark.parametrize("seed", range(0, GRAPHS, 5))
def test_host_code_matches_the_model(seed, tmp_path):
    start, edges = random_graph(seed)
    table, reads, offs, ors, n_interior, unsafe = python_chains(start, edges)
    got = host_chains(start, edges)
    assert np.array_equal(got.chains, table)
    assert np.array_equal(got.reads, reads) and np.array_equal(got.offs, offs) and np.array_equal(got.ors, ors)
    assert (got.info["n_interior"], got.info["n_chains"], got.info["n_contracted"], got.info["n_unsafe_chains"]) == (
        n_interior, table.shape[0], int(table["n"].sum()), unsafe)
    model = LoopModel(start, edges)
    iterations = model.contract()
    for mode in (None, "host"):
        g = UnitigGraph.from_csr(start, edges, chains=mode)
        g.save_lists(str(tmp_path / "lists"))
        assert (tmp_path / "lists").read_text() == model.lists_text(), mode
        assert (g.nodes, g.edges, g.iterations, g.merged, g.dead_end_nodes) == (
            model.nodes, model.edges, iterations, model.merged_total, model.dead_end_total), mode
        g.close()
