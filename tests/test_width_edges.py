"""Every instantiated template width and the read-count edges, against the oracle.

Widths: the kernels are instantiated for W = 1, 2, 3, 4, 5, 6, 8, 12, 16, 32
words of 32 bases.  Each W gets an equal-length set at exactly 32 W bases (the
last word full: rc_word, the funnel shifts and overlap_diff's tail mask at a
word boundary) and a mixed-length set with lengths in [32 W - 33, 32 W], which
crosses the word boundary below and drives containment.  Each set runs through
the fused path, a two-way source-range split, the exchange mode at P = 2 and
getListOfReads.

Read counts: N unique reads around the wavefront (64), the block (256), the
window-0 run regions (512) and the flat / exchange regions (1024), fused and
through the exchange mode at P = 3 (ranks that own almost nothing).

Bit-exact: rows as sorted tuples and superReadIDs equal the oracle's."""
import functools

import numpy as np
import pytest

from metagenomics_amd import synth
from metagenomics_amd.overlap import Dataset, OverlapEngine, rows_to_tuples
from oracle import OracleDataset, sorted_tuples
from test_gpu_parity import assert_shard_rows, check_pairs, exchange_rows, gpu_rows

pytestmark = pytest.mark.gpu

# W: (min_overlap l, seed k).  w = l - k covers the register scan (w <= 32, W = 6
# at its largest window), the LDS scan and its 2-wavefront blocks (W = 16: w = 169)
WIDTHS = {1: (12, 6), 2: (40, 21), 3: (50, 31), 4: (50, 17), 5: (60, 31), 6: (64, 32), 8: (50, 31),
          12: (100, 31), 16: (200, 31), 32: (60, 31)}
N_READS, COVERAGE = 600, 17


@pytest.fixture(scope="module")
def engine():
    e = OverlapEngine(0)
    yield e
    e.close()


class ReadSet:
    """A set with its oracle results (computed once per module run)."""

    def __init__(self, seqs, l, k):
        self.seqs, self.l, self.k = seqs, l, k
        self.ds = Dataset.from_strings(seqs, l)
        self.od = OracleDataset.from_strings(seqs, l)
        orows, self.sup, _, _ = self.od.overlaps(l)
        self.rows = sorted_tuples(orows)
        self.lens = self.ds.packed()[1].copy()

    @property
    def n(self):
        return self.ds.num_unique

    def check(self, rows, sup=None):
        if sup is not None:
            assert np.array_equal(np.asarray(sup).astype(np.uint64), self.sup)
        assert np.array_equal(rows_to_tuples(rows), self.rows)


@functools.lru_cache(maxsize=None)
def width_set(W, kind):
    l, k = WIDTHS[W]
    hi = 32 * W
    lo = hi if kind == "equal" else max(l + 1, hi - 33)
    c, L = synth.uniform_read_set(N_READS, 0, max(2 * hi, N_READS * hi // COVERAGE), seed=700 + W, lo=lo, hi=hi)
    s = ReadSet(synth.codes_to_strings(c, L), l, k)
    # the set exercises what it is for (checked on the oracle's output)
    assert s.n == s.od.num_unique and int(s.lens.max()) == hi and int(s.lens.min()) == lo
    assert (int(s.lens.max()) + 31) // 32 == W
    assert s.rows.shape[0] > 0, "no overlaps"
    assert (kind == "mixed") == bool(s.sup.any()), "containment only (and always) in the mixed sets"
    return s


WIDTH_CASES = [pytest.param(W, kind, id=f"W{W}-{kind}") for W in WIDTHS for kind in ("equal", "mixed")]


@pytest.mark.parametrize("W,kind", WIDTH_CASES)
def test_width_fused(engine, W, kind):
    s = width_set(W, kind)
    rows, sup = gpu_rows(engine, s.ds, s.l, k=s.k)
    s.check(rows, sup)
    check_pairs(rows, s.lens)


@pytest.mark.parametrize("W,kind", WIDTH_CASES)
def test_width_source_range_split(engine, W, kind):
    """Two source-range shards (the run-only scans and LaunchIndex): each holds
    its sources' discoveries, the union is the multiset."""
    s = width_set(W, kind)
    parts = []
    for lo, hi in ((0, s.n // 2), (s.n // 2, s.n)):
        rows, sup = gpu_rows(engine, s.ds, s.l, k=s.k, shard=(0, 1, lo, hi))
        assert np.array_equal(sup.astype(np.uint64), s.sup)
        assert_shard_rows(rows, lo, hi)
        parts.append(rows)
    engine.set_shard(0, 1)
    s.check(np.concatenate(parts))


@pytest.mark.parametrize("W,kind", WIDTH_CASES)
def test_width_exchange(W, kind):
    s = width_set(W, kind)
    rows, sup = exchange_rows(s.ds, s.l, 2, k=s.k)
    s.check(rows, sup)


@pytest.mark.parametrize("W,kind", WIDTH_CASES)
def test_width_lookup(engine, W, kind):
    """getListOfReads (HashTable.cpp:202-221) of a prefix, a suffix and a
    reverse-complement prefix of a handful of reads, list order included."""
    s = width_set(W, kind)
    engine.set_option("nb_log2", 0)
    engine.set_shard(0, 1)
    engine.upload(s.ds)
    engine.build_index(s.l, s.k)
    h = s.l - 1
    found = 0
    for rid in range(1, s.n + 1, max(1, s.n // 6)):
        r = s.ds.read(rid)
        for key in (r[:h], r[-h:], synth.revcomp_str(r)[:h]):
            exp = s.od.lookup(s.l, key)
            assert engine.lookup(key) == exp, (rid, key)
            found += len(exp)
    assert found > 0


# ---- read-count edges
COUNTS = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025]
COUNT_L, COUNT_K = 40, 21


@functools.lru_cache(maxsize=None)
def count_pool():
    """One mixed-length high-coverage set; its unique reads in ID order."""
    c, L = synth.uniform_read_set(1400, 0, 1500, seed=731, lo=60, hi=120)
    ds = Dataset.from_codes(c, L, COUNT_L)
    assert ds.num_unique >= max(COUNTS)
    return [ds.read(i) for i in range(1, max(COUNTS) + 1)]


@functools.lru_cache(maxsize=None)
def count_set(N):
    s = ReadSet(count_pool()[:N], COUNT_L, COUNT_K)
    assert s.n == N == s.od.num_unique
    if N >= 255:
        assert s.rows.shape[0] > 0 and s.sup.any()
    return s


@pytest.mark.parametrize("N", COUNTS)
def test_read_count_fused(engine, N):
    s = count_set(N)
    rows, sup = gpu_rows(engine, s.ds, s.l, k=s.k)
    s.check(rows, sup)
    check_pairs(rows, s.lens)


@pytest.mark.parametrize("N", [2, 64, 65, 513, 1025])
def test_read_count_exchange(N):
    s = count_set(N)
    rows, sup = exchange_rows(s.ds, s.l, 3, k=s.k)
    s.check(rows, sup)
