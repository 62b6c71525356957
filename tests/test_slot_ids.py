"""The reference ID that rides in a clustered slot's spare word (slot_id_word,
DESIGN.md §2): k_layout_gather writes it, k_probe's verification reads it
instead of d_id[] at the widths that have the word (template W = 5, 6, 12).

The width tests cover W = 5, 6 and 12 at exactly 32 W bases.  These cover the
rest: template widths that differ from the set's own word count, both slot
arrays after uploads of other sizes and widths, the re-layout of resident reads
for a source range, the ID-order layout beside the clustered one, the device
ingest, and that the word never leaves the device with the reads.

Bit-exact: rows as sorted tuples and superReadIDs equal the oracle's."""
import functools

import numpy as np
import pytest

from metagenomics_amd import synth
from metagenomics_amd.overlap import Dataset, OverlapEngine, rows_to_tuples
from oracle import OracleDataset, sorted_tuples
from test_gpu_parity import assert_shard_rows, check_pairs, exchange_rows, gpu_rows

pytestmark = pytest.mark.gpu

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
def read_set(longest, kind, n=N_READS, seed=0, l=50, k=31):
    """n reads at 17x whose longest read has `longest` bases: all of that
    length ("equal") or lengths down to 33 bases less ("mixed": containment)."""
    lo = longest if kind == "equal" else max(l + 1, longest - 33)
    c, L = synth.uniform_read_set(n, 0, max(2 * longest, n * longest // COVERAGE), seed=900 + longest + seed, lo=lo,
                                  hi=longest)
    s = ReadSet(synth.codes_to_strings(c, L), l, k)
    s.codes = c, L
    # the set exercises what it is for (checked on the oracle's output)
    assert s.n == s.od.num_unique and int(s.lens.max()) == longest and int(s.lens.min()) == lo
    assert s.rows.shape[0] > 0, "no overlaps"
    assert (kind == "mixed") == bool(s.sup.any()), "containment only (and always) in the mixed sets"
    return s


def step(engine, s):
    """One step on the reads the engine holds."""
    engine.build_index(s.l, s.k)
    sup = engine.mark_contained()
    return engine.rows(engine.find_overlaps()), sup


# ---- 1. the template width is not the set's word count: maxw 7 runs the W = 8
# kernels (no ID word), maxw 9 and 11 the W = 12 kernels (ID word 15)
LONGEST = {224: 7, 288: 9, 352: 11}
TEMPLATE_CASES = [pytest.param(b, kind, id=f"{b}bp-{kind}") for b in LONGEST for kind in ("equal", "mixed")]


def template_set(longest, kind):
    s = read_set(longest, kind)
    assert (int(s.lens.max()) + 31) // 32 == LONGEST[longest]
    return s


@pytest.mark.parametrize("longest,kind", TEMPLATE_CASES)
def test_template_width_fused(engine, longest, kind):
    s = template_set(longest, kind)
    rows, sup = gpu_rows(engine, s.ds, s.l, k=s.k)
    s.check(rows, sup)
    check_pairs(rows, s.lens)


@pytest.mark.parametrize("longest,kind", TEMPLATE_CASES)
def test_template_width_source_range_split(engine, longest, kind):
    s = template_set(longest, kind)
    parts = []
    for lo, hi in ((0, s.n // 2), (s.n // 2, s.n)):
        rows, sup = gpu_rows(engine, s.ds, s.l, k=s.k, shard=(0, 1, lo, hi))
        assert np.array_equal(sup.astype(np.uint64), s.sup)
        assert_shard_rows(rows, lo, hi)
        parts.append(rows)
    engine.set_shard(0, 1)
    s.check(np.concatenate(parts))


@pytest.mark.parametrize("longest,kind", TEMPLATE_CASES)
def test_template_width_exchange(longest, kind):
    s = template_set(longest, kind)
    rows, sup = exchange_rows(s.ds, s.l, 2, k=s.k)
    s.check(rows, sup)


# ---- 2. both slot arrays after reuse: the gather writes the array the last
# layout read from, so a stale or missing ID word (a smaller set's tail, another
# width's slots) would surface in the step after the next upload
def test_slot_arrays_after_reuse():
    first = read_set(160, "equal")
    pool = read_set(160, "equal", n=400, seed=1)
    second = ReadSet([pool.ds.read(i) for i in range(1, 258)], pool.l, pool.k)  # one read past a block of 256
    wide = read_set(384, "mixed")
    assert second.n == 257 and second.rows.shape[0] > 0 and not set(second.seqs) & set(first.seqs)
    e = OverlapEngine(0)
    try:
        for s in (first, second, wide, first):
            rows, sup = gpu_rows(e, s.ds, s.l, k=s.k)
            s.check(rows, sup)
            check_pairs(rows, s.lens)
    finally:
        e.close()


# ---- 3. re-layout in place: a source range set on resident reads re-clusters
# them (no upload in between), each time into the other slot array
def test_relayout_in_place(engine):
    s = read_set(160, "mixed")
    n = s.n
    engine.set_option("nb_log2", 0)
    engine.set_shard(0, 1)
    engine.upload(s.ds)
    parts = []
    for lo, hi in ((0, n // 3), (n // 3, n)):
        engine.set_shard(0, 1, lo, hi)
        rows, sup = step(engine, s)
        assert np.array_equal(sup.astype(np.uint64), s.sup)
        assert_shard_rows(rows, lo, hi)
        parts.append(rows)
    s.check(np.concatenate(parts))
    engine.set_shard(0, 1)
    rows, sup = step(engine, s)
    s.check(rows, sup)
    check_pairs(rows, s.lens)


# ---- 4. layout toggled: ID order (no ID map, the words are not read), then clustered
@pytest.mark.parametrize("longest", [160, 192])
@pytest.mark.parametrize("kind", ["equal", "mixed"])
def test_layout_toggled(longest, kind):
    s = read_set(longest, kind)
    e = OverlapEngine(0)
    try:
        for layout in (0, 1, 0, 1):
            e.set_option("layout", layout)
            rows, sup = gpu_rows(e, s.ds, s.l, k=s.k)
            assert bool(np.any(e.slot_of_ids() != np.arange(s.n))) == bool(layout)
            s.check(rows, sup)
    finally:
        e.close()


# ---- 5. device ingest: the Dataset built on the device, then clustered
def test_device_ingest(engine):
    s = read_set(160, "mixed")
    c, L = s.codes
    engine.set_option("nb_log2", 0)
    engine.set_shard(0, 1)
    assert engine.ingest_codes(c, L, s.l) == s.n
    rows, sup = step(engine, s)
    s.check(rows, sup)
    check_pairs(rows, s.lens)


# ---- 6. the ID word stays internal: the reads come back as they went in
@pytest.mark.parametrize("longest", [160, 192, 384])
def test_download_has_no_id_word(engine, longest):
    s = read_set(longest, "mixed")
    engine.set_option("layout", 1)
    engine.set_shard(0, 1)
    engine.upload(s.ds)
    assert np.any(engine.slot_of_ids() != np.arange(s.n)), "the layout is on"
    w, lens = engine.download_packed()
    hw, hl = s.ds.packed()
    assert np.array_equal(lens, hl) and w.shape == hw.shape and np.array_equal(w, hw)
