"""The per-read discovery lists D(A) grouped and ordered on the device
(mg_build_discoveries / mg_copy_discoveries, metagenomics_amd/csrc/device/
mg_disc.hip): for every read the rows with src = A in insertAllEdgesOfRead's
loop order (window j, partner ID, key o), a self row once.  Expected lists:
numpy over the rows (tests/disc_ref.py), array for array."""
import numpy as np
import pytest

from conftest import FIXTURES, fixture_input, golden_rows, load_meta
from disc_ref import golden_bfs, numpy_lists, tuples
from metagenomics_amd.overlap import Dataset, MgError, OverlapEngine, replay_discoveries, rows_to_tuples
from oracle import OracleDataset, sorted_tuples

pytestmark = pytest.mark.gpu

_expected = {}


@pytest.fixture(scope="module")
def engine():
    e = OverlapEngine(0)
    yield e
    e.close()


def expected(name):
    """(meta, ds, lens, start, disc, self rows) from the golden rows; computed once, never modified."""
    if name not in _expected:
        meta = load_meta(name)
        ds = Dataset.from_files([fixture_input(name)], meta["l"])
        lens = ds.packed()[1]
        start, disc, n_self = numpy_lists(golden_rows(name), lens, meta["l"])
        for a in (start, disc):
            a.setflags(write=False)
        _expected[name] = (meta, ds, lens, start, disc, n_self)
    return _expected[name]


def device_lists(e, ds, l):
    e.upload(ds)
    e.build_index(l)
    n_rows = e.find_overlaps()
    n_disc = e.build_discoveries()
    start, disc = e.discoveries()
    assert disc.shape[0] == n_disc
    return n_rows, n_disc, start, disc


def assert_lists(got_start, got_disc, start, disc):
    assert np.array_equal(got_start, start)
    assert got_disc.shape == disc.shape
    assert np.array_equal(got_disc, disc)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_lists(engine, name):
    """highdup crosses the wavefront path's 64 records, tandem has 922 self rows
    and degree 420, longreads offsets up to 7,668 in long mode, mixed empty lists
    inside the ID range, tworead one record per list."""
    meta, ds, lens, start, disc, n_self = expected(name)
    n_rows, n_disc, s, d = device_lists(engine, ds, meta["l"])
    assert n_rows == golden_rows(name).shape[0]
    assert n_disc == n_rows - n_self // 2
    assert_lists(s, d, start, disc)
    # end to end: the lists give the reference's graph
    nodes, edges, out = replay_discoveries(s, d, lens, meta["l"])
    assert (nodes, edges) == (meta["bfs"]["nodes"], meta["bfs"]["edges"])
    assert np.array_equal(tuples(out), golden_bfs(name))


@pytest.mark.parametrize("name", ["highdup", "tandem"])
def test_oversize_path_with_self_rows(name):
    """block capacity 64: every list above the wavefront path takes the segmented sort."""
    meta, ds, lens, start, disc, n_self = expected(name)
    e = OverlapEngine(0)
    try:
        e.set_option("disc_block_cap", 64)
        n_rows, n_disc, s, d = device_lists(e, ds, meta["l"])
        assert n_disc == n_rows - n_self // 2
        assert_lists(s, d, start, disc)
    finally:
        e.close()


@pytest.fixture(scope="module")
def sweep():
    """All 1,801 windows of 600 bp of a random 2,400-bp genome, l = 30: degrees 570..1,140."""
    rng = np.random.default_rng(7)
    g = "".join("ACGT"[i] for i in rng.integers(0, 4, 2400))
    reads = [g[i:i + 600] for i in range(1801)]
    od = OracleDataset.from_strings(reads, 30)
    orows, _, _, _ = od.overlaps(30)
    want = sorted_tuples(orows)
    lens = np.full(od.num_unique, 600, dtype=np.uint16)
    start, disc, n_self = numpy_lists(want, lens, 30)
    deg = np.diff(start.astype(np.int64))[1:]
    # the sweep itself: every degree from 570 to 1,140, both sides of the capacity used below
    assert od.num_unique == 1801 and want.shape[0] == 1727670 and n_self == 0
    assert (int(deg.min()), int(deg.max())) == (570, 1140)
    assert set(deg.tolist()) == set(range(570, 1141))
    assert int((deg > 1024).sum()) == 891
    return Dataset.from_strings(reads, 30), want, start, disc


@pytest.mark.parametrize("cap", [1024, 0])
def test_degree_sweep_across_block_capacity(sweep, cap):
    """cap 1,024: 910 reads sort in the workgroup's LDS, 891 take the oversize
    path; cap 0 (the default 2,048): all take the workgroup path."""
    ds, want, start, disc = sweep
    e = OverlapEngine(0)
    try:
        e.set_option("disc_block_cap", cap)
        e.upload(ds)
        e.build_index(30)
        n = e.find_overlaps()
        assert np.array_equal(rows_to_tuples(e.rows(n)), want)
        assert e.build_discoveries() == n
        assert_lists(*e.discoveries(), start, disc)
    finally:
        e.close()


def test_after_row_capacity_rerun():
    meta, ds, lens, start, disc, n_self = expected("small")
    e = OverlapEngine(0)
    try:
        e.set_option("rows_cap", 1)
        n_rows, n_disc, s, d = device_lists(e, ds, meta["l"])
        assert e.counters()["row_reruns"] > 0
        assert_lists(s, d, start, disc)
    finally:
        e.close()


def test_no_overlaps_at_all():
    rng = np.random.default_rng(3)
    reads = ["".join("ACGT"[i] for i in rng.integers(0, 4, 100)) for _ in range(8)]
    ds = Dataset.from_strings(reads, 90)
    e = OverlapEngine(0)
    try:
        n_rows, n_disc, s, d = device_lists(e, ds, 90)
        assert (n_rows, n_disc, d.shape[0]) == (0, 0, 0)
        assert s.shape[0] == ds.num_unique + 2 and not s.any()
    finally:
        e.close()


def test_lifecycle():
    meta, ds, lens, start, disc, _ = expected("mixed")
    l = meta["l"]
    e = OverlapEngine(0)
    try:
        e.upload(ds)
        e.build_index(l)
        with pytest.raises(MgError, match="mg_find_overlaps"):
            e.build_discoveries()
        e.find_overlaps()
        with pytest.raises(MgError, match="mg_build_discoveries"):
            e.discoveries()
        e.build_discoveries()
        first = e.discoveries()
        e.build_discoveries()
        second = e.discoveries()
        assert_lists(*first, start, disc)
        assert_lists(*second, start, disc)
        # a new index: the lists are stale until find_overlaps and build_discoveries ran again
        e.build_index(l)
        with pytest.raises(MgError):
            e.discoveries()
        with pytest.raises(MgError):
            e.build_discoveries()
        e.find_overlaps()
        with pytest.raises(MgError):
            e.discoveries()
        e.build_discoveries()
        assert_lists(*e.discoveries(), start, disc)
        # rows that are not the whole multiset
        for shard in ((0, 2, 0, 0), (0, 1, 0, ds.num_unique // 2)):
            e.set_shard(*shard)
            with pytest.raises(MgError, match="shard"):
                e.build_discoveries()
            with pytest.raises(MgError, match="shard"):
                e.discoveries()
        e.set_shard(0, 1)
        e.upload(ds)
        e.build_index(l)
        e.find_overlaps()
        e.build_discoveries()
        assert_lists(*e.discoveries(), start, disc)
    finally:
        e.close()


def test_allocation_failure_names_the_list_buffer():
    meta, ds, lens, start, disc, _ = expected("mixed")
    l = meta["l"]
    e = OverlapEngine(0)
    try:
        e.upload(ds)
        e.build_index(l)
        n_rows = e.find_overlaps()
        e.set_option("alloc_cap", n_rows * 8 - 1)  # below the list buffer (8 B per row)
        with pytest.raises(MgError) as exc:
            e.build_discoveries()
        msg = str(exc.value)
        assert "device allocation of " in msg and " B) failed: " in msg and "alloc_cap" in msg, msg
        assert "memory" in msg.lower() and "d_disc (" in msg, msg
        with pytest.raises(MgError):
            e.discoveries()
        e.set_option("alloc_cap", 0)
        e.build_discoveries()
        assert_lists(*e.discoveries(), start, disc)
    finally:
        e.close()
