"""The device's discovery lists (mg_build_discoveries, metagenomics_amd/csrc/
device/mg_disc.hip) at the list lengths where its three paths and the wavefront
path's packing go wrong, on the sets of tests/disc_sets.py: whole lists packed
into 64 lanes (runs of exactly 64, runs cut at 65, empty lists inside a run, a
list above 64 between small ones, 32 lists in one run, a short last wavefront),
degrees at the wavefront / workgroup bound and at the workgroup path's padding
bounds, block capacities crossed one degree apart (one of them no power of
two), more lists per path than the grid-stride loops have workgroups, all-self
lists on every path, both slot layouts, and read counts around 32 and 64.
tests/test_disc_edges_host.py asserts that the sets reach these cases and pins
the expected arrays with the host mirrors.  Everything is bit-exact."""
import numpy as np
import pytest

import disc_sets as S
from metagenomics_amd.overlap import OverlapEngine, check_discoveries, replay_discoveries, rows_to_tuples

pytestmark = pytest.mark.gpu


def build_lists(e, s):
    e.upload(s.ds)
    e.build_index(s.l, s.k)
    n_rows = e.find_overlaps()
    n_disc = e.build_discoveries()
    start, disc = e.discoveries()
    assert disc.shape[0] == n_disc
    return n_rows, n_disc, start, disc


def assert_lists(s, start, disc):
    assert np.array_equal(start, s.start)
    assert disc.shape == s.disc.shape
    assert np.array_equal(disc, s.disc)


def assert_set(e, s, replay):
    """Rows, lists, components and (replay) the parallel replay of one set on engine e."""
    n_rows, n_disc, start, disc = build_lists(e, s)
    assert np.array_equal(rows_to_tuples(e.rows(n_rows)), s.rows)
    assert n_disc == n_rows - s.n_self // 2
    assert_lists(s, start, disc)
    assert check_discoveries(start, disc, s.lens, s.l) == 0
    n_comp = e.build_components()
    label, comps = e.components()
    assert comps.shape[0] == n_comp
    assert np.array_equal(label, s.comps[0])
    assert comps.shape == s.comps[1].shape and np.array_equal(comps, s.comps[1])
    if replay:
        serial = replay_discoveries(start, disc, s.lens, s.l)
        par = replay_discoveries(start, disc, s.lens, s.l, components=(label, comps), threads=4)
        assert par[:2] == serial[:2] and np.array_equal(par[2], serial[2])


def engine_with(**options):
    e = OverlapEngine(0)
    for name, value in options.items():
        e.set_option(name, value)
    return e


@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("name", ["ladder_low", "ladder_flat", "mixed_small"])
def test_ladder_lists(name, layout):
    """The wavefront path: every degree 0 .. 65 mixed inside the wavefronts' 32
    reads, all-self lists of 16 .. 128 rows and lists that mix self and other
    records among them (ladder_low); 32 lists in one run (ladder_flat); window j
    from each source's own length, in either slot layout (mixed_small)."""
    e = engine_with(layout=layout)
    try:
        assert_set(e, S.disc_set(name), replay=True)
    finally:
        e.close()


@pytest.mark.parametrize("cap,layout", [(0, 1), (100, 1), (128, 1), (512, 1), (64, 1), (0, 0), (64, 0)])
def test_block_ladder(cap, layout):
    """More than 4,096 lists above 64 records, degrees 65, 66, 127 .. 129,
    255 .. 257 and 511 .. 513, all-self lists of 64 .. 1,120 rows.  cap 0: all in
    the workgroup's LDS, padded to 128 .. 2,048 keys, every workgroup more than
    once; cap 100: 65 and 66 there, the rest oversize; cap 128 and 512: the
    capacity itself there, one more oversize; cap 64: one segmented sort of
    more than 4,096 segments."""
    e = engine_with(layout=layout, disc_block_cap=cap)
    try:
        assert_set(e, S.disc_set("ladder_block"), replay=False)
    finally:
        e.close()


@pytest.mark.parametrize("N", S.COUNTS)
def test_read_counts(N):
    s = S.disc_set("count%d" % N)
    e = OverlapEngine(0)
    try:
        n_rows, n_disc, start, disc = build_lists(e, s)
        assert_lists(s, start, disc)
        # N + 2 entries: read 0 has no list, the last entry is the total (the wavefront path's
        # lanes past the last read all load it)
        assert start.shape[0] == N + 2
        assert int(start[0]) == int(start[1]) == 0 and int(start[N + 1]) == n_disc == n_rows - s.n_self // 2
        assert np.all(np.diff(start.astype(np.int64)) >= 0)
    finally:
        e.close()


def test_two_builds_and_a_rerun():
    s = S.disc_set("ladder_low")
    e = OverlapEngine(0)
    try:
        first = build_lists(e, s)
        assert e.build_discoveries() == first[1]
        second = e.discoveries()
        assert_lists(s, first[2], first[3])
        assert_lists(s, *second)
    finally:
        e.close()
    e = engine_with(rows_cap=1)
    try:
        n_rows, n_disc, start, disc = build_lists(e, s)
        assert e.counters()["row_reruns"] > 0
        assert n_disc == n_rows - s.n_self // 2
        assert_lists(s, start, disc)
    finally:
        e.close()
