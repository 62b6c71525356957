"""The host side of the connected components of the discovery lists:
mg::Components::build (host union-find) against numpy (tests/comp_ref.py), the
validation of a table that arrives through the C ABI (Components::from_device)
and the parallel replay of the components (GraphReplay::build_from with a
table), which must give the serial replay's graph array for array.  The lists
come from numpy over the golden rows, so this runs without a GPU."""
import numpy as np
import pytest

from comp_ref import components_from_lists, components_from_rows
from conftest import FIXTURES, fixture_input, golden_rows, load_meta, rows_sha256
from disc_ref import golden_bfs, golden_text, numpy_lists, tuples
from metagenomics_amd import synth
from metagenomics_amd.overlap import (COMP_DTYPE, Dataset, MgError, UnitigGraph, host_components,
                                      replay_discoveries)
from oracle import OracleDataset, sorted_tuples

THREADS = [1, 2, 4, 16]
# components that hold records (from the golden rows)
N_COMPONENTS = {"small": 7, "mixed": 1, "highdup": 1, "tandem": 1, "tworead": 1, "dirty": 5, "wrapped": 5,
                "branchy": 3, "longreads": 1}

_cache = {}


def lists_of(name):
    """(meta, lens, start, disc, label, comps) of a fixture; computed once, never modified."""
    if name not in _cache:
        meta = load_meta(name)
        ds = Dataset.from_files([fixture_input(name)], meta["l"])
        lens = ds.packed()[1].copy()
        start, disc, _ = numpy_lists(golden_rows(name), lens, meta["l"])
        label, comps = components_from_lists(start, disc)
        for a in (lens, start, disc, label, comps):
            a.setflags(write=False)
        _cache[name] = (meta, lens, start, disc, label, comps)
    return _cache[name]


def many_components():
    """About 4,000 reads of 100 bp over a 200-kb genome (coverage 2), l = 40:
    a thousand components of a few reads each and isolated reads between them."""
    if "many" not in _cache:
        c, L = synth.uniform_read_set(4000, 100, 200000, seed=11)
        od = OracleDataset.from_strings(synth.codes_to_strings(c, L), 40)
        rows = sorted_tuples(od.overlaps(40)[0])
        lens = np.full(od.num_unique, 100, dtype=np.uint16)
        start, disc, _ = numpy_lists(rows, lens, 40)
        label, comps = components_from_lists(start, disc)
        for a in (lens, start, disc, label, comps):
            a.setflags(write=False)
        _cache["many"] = (lens, start, disc, label, comps)
    return _cache["many"]


def test_comp_dtype_is_16_bytes():
    assert COMP_DTYPE.itemsize == 16


def test_reference_agrees_with_itself_from_rows():
    """comp_ref from rows (self rows twice) and from lists (once) is one definition."""
    for name in ("small", "tandem", "branchy"):
        meta, lens, start, disc, label, comps = lists_of(name)
        l2, c2 = components_from_rows(golden_rows(name), lens.shape[0])
        assert np.array_equal(l2, label) and np.array_equal(c2, comps)


@pytest.mark.parametrize("name", FIXTURES)
def test_host_components_match_reference(name):
    meta, lens, start, disc, label, comps = lists_of(name)
    # what the fixtures are here for (preconditions, from the golden rows)
    assert comps.shape[0] == N_COMPONENTS[name]
    if name == "small":
        big = comps[np.argmax(comps["n_disc"])]
        assert (int(big["n_reads"]), int(big["n_disc"])) == (810, 9246)
    if name == "mixed":
        assert (int(comps["n_reads"].sum()), lens.shape[0]) == (939, 2998)
    if name == "tandem":
        assert int(comps["n_self"].sum()) == 461
    if name == "branchy":
        assert int(comps["n_self"].sum()) == 5
    got_label, got_comps = host_components(start, disc)
    assert np.array_equal(got_label, label)
    assert np.array_equal(got_comps, comps)
    assert np.all(np.diff(got_comps["root"].astype(np.int64)) > 0)
    assert int(got_comps["n_disc"].sum()) == disc.shape[0]


@pytest.mark.parametrize("name", FIXTURES)
def test_parallel_replay_matches_reference_graph(name):
    meta, lens, start, disc, label, comps = lists_of(name)
    nodes, edges, serial = replay_discoveries(start, disc, lens, meta["l"])
    assert (nodes, edges) == (meta["bfs"]["nodes"], meta["bfs"]["edges"])
    assert np.array_equal(tuples(serial), golden_bfs(name))
    for t in THREADS:
        n, e, out = replay_discoveries(start, disc, lens, meta["l"], components=(label, comps), threads=t)
        assert (n, e) == (nodes, edges), t
        assert np.array_equal(out, serial), t
    # the table of the host union-find, default thread count
    n, e, out = replay_discoveries(start, disc, lens, meta["l"], components=host_components(start, disc))
    assert (n, e) == (nodes, edges) and np.array_equal(out, serial)


def test_parallel_replay_c1():
    """BASELINE configs[0] (100k x 100 bp, l = 40): oracle multiset -> lists -> parallel replay."""
    meta = load_meta("c1")
    r = meta["recipe"]
    c, L = synth.uniform_read_set(r["n_reads"], r["read_len"], r["genome_len"], r["seed"])
    od = OracleDataset.from_strings(synth.codes_to_strings(c, L), meta["l"])
    rows = sorted_tuples(od.overlaps(meta["l"])[0])
    lens = np.full(od.num_unique, r["read_len"], dtype=np.uint16)
    start, disc, _ = numpy_lists(rows, lens, meta["l"])
    label, comps = components_from_lists(start, disc)
    hl, hc = host_components(start, disc)
    assert np.array_equal(hl, label) and np.array_equal(hc, comps)
    nodes, edges, serial = replay_discoveries(start, disc, lens, meta["l"])
    assert (nodes, edges) == (meta["bfs"]["nodes"], meta["bfs"]["edges"])
    assert rows_sha256(tuples(serial)) == meta["bfs"]["rows_sha256"]
    for t in THREADS:
        n, e, out = replay_discoveries(start, disc, lens, meta["l"], components=(label, comps), threads=t)
        assert (n, e) == (nodes, edges), t
        assert np.array_equal(out, serial), t


def test_many_components():
    lens, start, disc, label, comps = many_components()
    deg = np.diff(start.astype(np.int64))[1:]
    assert comps.shape[0] >= 200 and int((deg == 0).sum()) >= 1  # preconditions
    assert int(np.flatnonzero(deg == 0)[0]) + 1 < lens.shape[0]  # an isolated read inside the ID range
    hl, hc = host_components(start, disc)
    assert np.array_equal(hl, label) and np.array_equal(hc, comps)
    nodes, edges, serial = replay_discoveries(start, disc, lens, 40)
    for t in THREADS:
        n, e, out = replay_discoveries(start, disc, lens, 40, components=(label, comps), threads=t)
        assert (n, e) == (nodes, edges) and np.array_equal(out, serial), t


@pytest.mark.parametrize("name", FIXTURES)
def test_unitig_from_components_matches_reference(name, tmp_path):
    meta, lens, start, disc, label, comps = lists_of(name)
    g = UnitigGraph.from_discoveries(start, disc, lens, meta["l"], components=(label, comps), threads=4)
    u = meta["unitig"]
    assert (g.replay_nodes, g.replay_edges) == (meta["bfs"]["nodes"], meta["bfs"]["edges"])
    assert (g.nodes, g.edges, g.iterations) == (u["nodes"], u["edges"], u["iterations"])
    g.sort_edges()
    g.save_unitig(str(tmp_path / "x.unitig"))
    assert (tmp_path / "x.unitig").read_text() == golden_text(name, "file")


def code_of(start, disc, lens, l, label, comps, threads=4):
    try:
        replay_discoveries(start, disc, lens, l, components=(label, comps), threads=threads)
    except MgError as e:
        msg = str(e)
        assert msg.startswith("graph replay failed (") and msg.endswith(")"), msg
        return int(msg[len("graph replay failed ("):-1])
    return 0


def test_malformed_tables_are_rejected():
    meta, lens, start, disc, label, comps = lists_of("small")
    l, n = meta["l"], lens.shape[0]
    assert comps.shape[0] >= 3
    assert code_of(start, disc, lens, l, label, comps) == 0
    a, b = comps[0], comps[1]
    ra, rb = int(a["root"]), int(b["root"])

    # two components given one label: every static check holds (closure, counts,
    # sums); the replay finds that the walk from the root did not fill the slice
    lab = label.copy()
    lab[label == rb] = ra
    cs = np.delete(comps, 1)
    for k in ("n_reads", "n_disc", "n_self"):
        cs[k][0] = int(a[k]) + int(b[k])
    for t in (2, 4, 16):
        assert code_of(start, disc, lens, l, lab, cs, threads=t) == -4

    # one component split in two: a record joins two labels
    members = np.flatnonzero(label == ra)
    assert members.shape[0] >= 4
    half = members[members.shape[0] // 2:]
    lab = label.copy()
    lab[half] = half[0]
    deg = np.diff(start.astype(np.int64))
    cs = np.zeros(comps.shape[0] + 1, dtype=COMP_DTYPE)
    cs[0] = a
    cs[1] = (int(half[0]), half.shape[0], int(deg[half].sum()), 0)
    cs["n_reads"][0] -= cs["n_reads"][1]
    cs["n_disc"][0] -= cs["n_disc"][1]
    cs[2:] = comps[1:]
    cs = cs[np.argsort(cs["root"], kind="stable")]
    assert code_of(start, disc, lens, l, lab, cs) == -4

    # a root that is not the minimum
    second = int(members[1])
    lab = label.copy()
    lab[members] = second
    cs = comps.copy()
    cs["root"][0] = second
    assert code_of(start, disc, lens, l, lab, cs) == -4

    # roots not ascending
    cs = comps.copy()
    cs[[0, 1]] = cs[[1, 0]]
    assert code_of(start, disc, lens, l, label, cs) == -4
    cs = comps.copy()
    cs[1] = cs[0]
    assert code_of(start, disc, lens, l, label, cs) == -4

    # counts off by one
    for key in ("n_disc", "n_self", "n_reads"):
        for d in (1, -1):
            cs = comps.copy()
            if key == "n_self" and d < 0 and int(cs[key][0]) == 0:
                continue
            cs[key][0] = int(cs[key][0]) + d
            assert code_of(start, disc, lens, l, label, cs) == -4, (key, d)

    # a component missing from the table
    assert code_of(start, disc, lens, l, label, comps[1:]) == -4

    # label[A] > A
    lab = label.copy()
    lab[ra] = int(members[1])
    assert code_of(start, disc, lens, l, lab, comps) == -4

    # IDs out of range
    for bad in (0, n + 1):
        lab = label.copy()
        lab[int(members[2])] = bad
        assert code_of(start, disc, lens, l, lab, comps) == -1
        cs = comps.copy()
        cs["root"][-1] = bad
        assert code_of(start, disc, lens, l, label, cs) == -1

    # a read without records labelled into a component
    meta2, lens2, start2, disc2, label2, comps2 = lists_of("mixed")
    empty = int(np.flatnonzero(np.diff(start2.astype(np.int64))[1:] == 0)[-1]) + 1
    assert empty > int(comps2["root"][0])
    lab = label2.copy()
    lab[empty] = comps2["root"][0]
    assert code_of(start2, disc2, lens2, meta2["l"], lab, comps2) == -4

    # a label array of the wrong length
    with pytest.raises(MgError, match="n_reads \\+ 1"):
        replay_discoveries(start, disc, lens, l, components=(label[:-1], comps))
    with pytest.raises(MgError, match="n_reads \\+ 1"):
        replay_discoveries(start, disc, lens, l, components=(np.append(label, 0), comps))


def test_malformed_tandem_self_count():
    """n_self off by one where self records exist (tandem: 461)."""
    meta, lens, start, disc, label, comps = lists_of("tandem")
    for d in (1, -1):
        cs = comps.copy()
        cs["n_self"][0] = int(cs["n_self"][0]) + d
        assert code_of(start, disc, lens, meta["l"], label, cs) == -4
