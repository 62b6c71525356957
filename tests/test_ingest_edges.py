"""The device Dataset ingest (mg_ingest_ascii / mg_ingest_codes, mg_dataset.hip)
at every template width, length and filter edge, against the plain reference
of tests/ingest_ref.py (pinned to the host mirror by test_ingest_ref.py).

  a. every instantiated width W (k_ingest<W>, k_gather_word<W>, k_dedup_*<W>),
     both sources, reads of exactly 32 W bases and lengths across the word
     boundary below, with duplicates on both strands, lower case and dirt; the
     ingested context then gives the oracle's rows and superReadIDs;
  b. a template width chosen by a raw read that the filter drops (Ingest<32>
     and Ingest<0> feeding 3-word slots), and the 1,024 / 1,025 base edge;
  c. order and dedup: reads that pack to equal zero-padded words, pairs that
     differ in one base of one word, palindromes, read counts around the block
     size with runs of equal reads across a block edge, nothing to ingest;
  d. the filter: the 80 % rule at its boundary for each base, the length
     bound, one bad symbol at a word edge, lower case;
  e. one engine ingesting narrower after wider reads.

Bit-exact.  Every precondition is asserted from the reference or the oracle,
never from the device's output."""
import functools
import random

import pytest

from ingest_ref import assert_ingested, ref_dataset
from ingest_sets import EDGE_CASES, EdgeSet, edge_set, majority_read, rand_read, rc
from test_width_edges import WIDTHS, width_set

pytestmark = pytest.mark.gpu

# the widths the ingest is instantiated for (mg_dataset.hip, ingest()), restated
INGEST_WIDTHS = [1, 2, 3, 4, 5, 6, 8, 12, 16, 32]
assert sorted(WIDTHS) == INGEST_WIDTHS
SOURCES = ("ascii", "codes")


@pytest.fixture(scope="module")
def engine():
    from metagenomics_amd.overlap import OverlapEngine

    e = OverlapEngine(0)
    e.set_option("nb_log2", 0)
    e.set_shard(0, 1)
    yield e
    e.close()


def ingest_and_check(engine, s: EdgeSet, source):
    nu = s.ingest(engine, source)
    assert nu == len(s.ref[1])
    assert_ingested(engine, *s.ref)


def step_equals_oracle(engine, ws):
    """The ingested context behaves as an uploaded one: the set's oracle rows and superReadIDs."""
    engine.build_index(ws.l, ws.k)
    sup = engine.mark_contained()
    ws.check(engine.rows(), sup)


# ---- a. every width, both sources
@functools.lru_cache(maxsize=None)
def width_raw(W, kind, source):
    """Raw input whose Dataset is width_set(W, kind)'s: its reads on random
    strands, read i given 1 + i % 4 times, shuffled, a third in lower case
    (ASCII source), plus dirt no longer than 32 W bases."""
    ws = width_set(W, kind)
    rng = random.Random(5000 + 2 * W + (kind == "mixed"))  # (the same raw reads for both sources)
    hi, records, n_given = 32 * W, [], 0
    for i, r in enumerate(ws.seqs):
        b = r.encode()
        records += [rc(b) if rng.random() < .5 else b] * (1 + i % 4)
        n_given += 1 + i % 4
    dirt = [b"", rand_read(rng, ws.l)]
    for j in range(30):
        L = rng.randint(max(ws.l + 1, hi - 33), hi)
        r = bytearray(rand_read(rng, L))
        r[(0, L - 1, rng.randrange(L))[j % 3]] = ord("N")
        dirt.append(bytes(r))  # an N
        dirt.append(rand_read(rng, rng.randint(1, ws.l)))  # length <= l
        dirt.append(majority_read(L, b"ACGT"[j % 4], (9 * L + 9) // 10))  # 90 % one base
    assert max(len(d) for d in dirt) <= hi
    assert ref_dataset(dirt, ws.l) == (0, [], []), "the dirt adds no valid read"
    records += dirt
    rng.shuffle(records)
    if source == "ascii":
        records = [r.lower() if j % 3 == 0 else r for j, r in enumerate(records)]
    s = EdgeSet(records, ws.l)
    # the oracle's IDs still apply
    assert s.ref[1] == [ws.od.read(i) for i in range(1, ws.n + 1)]
    assert s.ref[0] == n_given == sum(s.ref[2])
    return s


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("kind", ["equal", "mixed"])
@pytest.mark.parametrize("W", INGEST_WIDTHS)
def test_ingest_width(engine, W, kind, source):
    ingest_and_check(engine, width_raw(W, kind, source), source)
    if source == "ascii":
        step_equals_oracle(engine, width_set(W, kind))


# ---- b. template width != slot width
def _n_read(rng, L):
    r = bytearray(rand_read(rng, L))
    r[L // 2] = ord("N")
    return bytes(r)


LONG_DIRT = {  # one raw read that picks the template width and then fails the filter
    "N700": lambda rng: _n_read(rng, 700),  # Ingest<32>
    "A85pct700": lambda rng: majority_read(700, ord("A"), 595),
    "N1500": lambda rng: _n_read(rng, 1500),  # Ingest<0>, 47 words per read
    "over65535": lambda rng: rand_read(rng, 70000),  # dropped by the length bound before a width is chosen
}
LONG_DIRT_CASES = [(d, src) for d in LONG_DIRT for src in SOURCES if not (d == "over65535" and src == "codes")]


@pytest.mark.parametrize("dirt,source", LONG_DIRT_CASES)
def test_template_wider_than_slots(engine, dirt, source):
    base = width_raw(3, "mixed", source)
    rng = random.Random(5100)
    records = list(base.records)
    records.insert(len(records) // 3, LONG_DIRT[dirt](rng))
    s = EdgeSet(records, base.l)
    assert s.ref == base.ref, "the long read is dropped"
    assert max(len(x) for x in s.ref[1]) == 96
    ingest_and_check(engine, s, source)
    assert engine.download_packed()[0].shape[1] == 3
    step_equals_oracle(engine, width_set(3, "mixed"))


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("L,wpr", [(1024, 32), (1025, 33)])
def test_longest_kept_read_sets_the_width(engine, L, wpr, source):
    """One valid read of 1,024 bases among 96-base ones: 32 words; of 1,025: the long path, 33."""
    base = width_raw(3, "mixed", source)
    rng = random.Random(5200 + L)
    records = list(base.records)
    records.insert(len(records) // 2, rand_read(rng, L))
    s = EdgeSet(records, base.l)
    assert s.ref[0] == base.ref[0] + 1 and len(s.ref[1]) == len(base.ref[1]) + 1
    ingest_and_check(engine, s, source)
    assert engine.download_packed()[0].shape[1] == wpr


# ---- c, d. order, dedup and filter edges (tests/ingest_sets.py)
@pytest.mark.parametrize("name,source", EDGE_CASES)
def test_ingest_edge_set(engine, name, source):
    ingest_and_check(engine, edge_set(name), source)


@pytest.mark.parametrize("source", SOURCES)
def test_nothing_to_ingest(engine, source):
    """n_raw = 0, then raw reads of which none is valid: an empty Dataset and
    no error; a normal ingest on the same engine straight afterwards is right."""
    ingest_and_check(engine, EdgeSet([]), source)
    assert engine.dataset_counts() == (0, 0)
    ingest_and_check(engine, edge_set("nothing_valid"), source)
    assert engine.dataset_counts() == (0, 0) and engine.n_reads == 0
    ingest_and_check(engine, edge_set("prefix64"), source)
    ws = width_set(2, "mixed")
    ingest_and_check(engine, width_raw(2, "mixed", source), source)
    step_equals_oracle(engine, ws)


# ---- e. one engine, narrower after wider
def test_engine_reuse_narrower_after_wider(engine):
    """W = 16 ingest, W = 2 ingest, W = 5 upload, W = 2 ingest again: the kept
    buffers' wider slots leave no stale words behind."""
    two = width_set(2, "mixed")
    ingest_and_check(engine, width_raw(16, "equal", "ascii"), "ascii")
    ingest_and_check(engine, width_raw(2, "mixed", "codes"), "codes")
    engine.upload(width_set(5, "equal").ds)
    ingest_and_check(engine, width_raw(2, "mixed", "ascii"), "ascii")
    step_equals_oracle(engine, two)
