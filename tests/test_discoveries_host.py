"""The host side of the per-read discovery lists D(A): mgh_graph_replay_disc /
mg::Discoveries::from_lists / GraphReplay::build_from take lists already grouped
and ordered (what mg_build_discoveries produces on the device) and give the
graph mgh_graph_replay gives from rows.  The lists here come from numpy
(tests/disc_ref.py) over the golden rows, so this runs without a GPU."""
import ctypes as C

import numpy as np
import pytest

from conftest import FIXTURES, fixture_input, golden_rows, load_meta
from disc_ref import golden_bfs, golden_text, numpy_lists, to_edges, tuples
from metagenomics_amd import overlap
from metagenomics_amd.overlap import (DISC_DTYPE, Dataset, UnitigGraph, check_discoveries, host_discoveries,
                                      replay_discoveries)

_cache = {}


def lists_of(name):
    """(meta, lens, start, disc) of a fixture; computed once, never modified."""
    if name not in _cache:
        meta = load_meta(name)
        ds = Dataset.from_files([fixture_input(name)], meta["l"])
        lens = ds.packed()[1].copy()  # (packed() gives views into ds)
        rows = golden_rows(name)
        rows = rows[np.random.default_rng(0).permutation(rows.shape[0])]  # the device emits rows in any order
        start, disc, _ = numpy_lists(rows, lens, meta["l"])
        for a in (lens, start, disc):
            a.setflags(write=False)
        _cache[name] = (meta, lens, start, disc)
    return _cache[name]


def test_disc_dtype_is_8_bytes():
    assert DISC_DTYPE.itemsize == 8


@pytest.mark.parametrize("name", FIXTURES)
def test_replay_of_lists_matches_reference_graph(name):
    meta, lens, start, disc = lists_of(name)
    nodes, edges, out = replay_discoveries(start, disc, lens, meta["l"])
    assert (nodes, edges) == (meta["bfs"]["nodes"], meta["bfs"]["edges"])
    assert np.array_equal(tuples(out), golden_bfs(name))


@pytest.mark.parametrize("name", FIXTURES)
def test_host_grouping_gives_the_same_lists(name):
    """mg::Discoveries::build (the grouping the device replaces) against numpy, and the checker accepts them."""
    meta, lens, start, disc = lists_of(name)
    rows = to_edges(golden_rows(name))
    s, d = host_discoveries(rows[np.random.default_rng(1).permutation(rows.shape[0])], lens, meta["l"])
    assert np.array_equal(s, start) and np.array_equal(d, disc)
    assert check_discoveries(start, disc, lens, meta["l"]) == 0


@pytest.mark.parametrize("name", ["branchy", "longreads"])
def test_unitig_from_lists_matches_reference(name, tmp_path):
    meta, lens, start, disc = lists_of(name)
    g = UnitigGraph.from_discoveries(start, disc, lens, meta["l"])
    u = meta["unitig"]
    assert (g.replay_nodes, g.replay_edges) == (meta["bfs"]["nodes"], meta["bfs"]["edges"])
    assert (g.nodes, g.edges, g.iterations) == (u["nodes"], u["edges"], u["iterations"])
    g.sort_edges()
    g.save_unitig(str(tmp_path / "x.unitig"))
    assert (tmp_path / "x.unitig").read_text() == golden_text(name, "file")


def status(start, disc, lens, l, n_disc=None):
    start = np.ascontiguousarray(start, dtype=np.uint64)
    disc = np.ascontiguousarray(disc, dtype=DISC_DTYPE)
    lens = np.ascontiguousarray(lens, dtype=np.uint16)
    g = C.c_void_p()
    rc = overlap.lib().mgh_graph_replay_disc(C.c_void_p(start.ctypes.data), C.c_void_p(disc.ctypes.data),
                                             disc.shape[0] if n_disc is None else n_disc,
                                             C.c_void_p(lens.ctypes.data), lens.shape[0], l - 1, C.byref(g))
    if rc == 0:
        overlap.lib().mgh_graph_free(g)
    else:
        assert not g.value
    if n_disc is None:  # the checker alone gives the same verdict
        assert check_discoveries(start, disc, lens, l) == rc
    return rc


def long_list(start):
    """a read with at least two discoveries"""
    deg = np.diff(start.astype(np.int64))
    return int(np.flatnonzero(deg >= 2)[0])


def test_malformed_lists_are_rejected():
    meta, lens, start, disc = lists_of("small")
    l, n = meta["l"], lens.shape[0]
    assert status(start, disc, lens, l) == 0
    a = long_list(start)

    s = start.copy()  # not monotone
    s[a + 1] = s[a] - 1 if s[a] else s[a + 2] + 1
    assert status(s, disc, lens, l) < 0

    assert status(start, disc, lens, l, n_disc=disc.shape[0] - 1) < 0  # start[N + 1] != n_disc
    s = start.copy()
    s[n + 1] -= 1
    assert status(s, disc, lens, l) < 0

    for bad in (0, n + 1):  # dst out of range
        d = disc.copy()
        d["dst"][int(start[a])] = bad
        assert status(start, d, lens, l) < 0

    d = disc.copy()  # j out of range: offset 0 gives j = 0 (o = 0, 2) or j = n1 - h (o = 1, 3)
    d["offset"][int(start[a])] = 0
    assert status(start, d, lens, l) < 0
    d = disc.copy()
    d["offset"][int(start[a])] = 65535
    assert status(start, d, lens, l) < 0

    d = disc.copy()  # two swapped neighbours in one list
    k = int(start[a])
    d[[k, k + 1]] = d[[k + 1, k]]
    assert status(start, d, lens, l) < 0

    d = disc.copy()  # the same record twice
    d[k + 1] = d[k]
    assert status(start, d, lens, l) < 0

    with pytest.raises(overlap.MgError):
        replay_discoveries(start[:-1], disc, lens, l)


def test_large_lists_take_the_threaded_pass():
    """Above 2^20 records from_lists splits the reads over host threads: all 1,801
    windows of 600 bp of a random 2,400-bp genome at l = 30 give 1,727,670 rows
    (CPU oracle).  Same lists as the host grouping, and a fault in any thread's
    range is found with its code."""
    from oracle import OracleDataset, sorted_tuples

    rng = np.random.default_rng(7)
    g = "".join("ACGT"[i] for i in rng.integers(0, 4, 2400))
    od = OracleDataset.from_strings([g[i:i + 600] for i in range(1801)], 30)
    rows = sorted_tuples(od.overlaps(30)[0])
    lens = np.full(od.num_unique, 600, dtype=np.uint16)
    start, disc, _ = numpy_lists(rows, lens, 30)
    assert disc.shape[0] > 1 << 20
    assert check_discoveries(start, disc, lens, 30) == 0
    s, d = host_discoveries(to_edges(rows), lens, 30)
    assert np.array_equal(s, start) and np.array_equal(d, disc)
    n = disc.shape[0]
    for k in (0, n // 3, n // 2, n - 2):  # the first record of the list k falls in, then a swap there
        a = int(np.searchsorted(start, k, side="right")) - 1
        k0 = int(start[a])
        bad = disc.copy()
        bad[[k0, k0 + 1]] = bad[[k0 + 1, k0]]
        assert check_discoveries(start, bad, lens, 30) == -3
        bad = disc.copy()
        bad["dst"][k0] = 0
        assert check_discoveries(start, bad, lens, 30) == -1
        bad = disc.copy()
        bad["offset"][k0] = 0
        assert check_discoveries(start, bad, lens, 30) == -2
    nodes, edges, out = replay_discoveries(start, disc, lens, 30)
    rn, re_, rout = overlap.replay_graph(to_edges(rows), lens, 30)
    assert (nodes, edges) == (rn, re_) and np.array_equal(out, rout)
