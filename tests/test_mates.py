"""mg_build_mate_pairs / mg_copy_mate_pairs (mg_mates.hip): the per-read mate
lists built on the device, against the reference's own lists
(tests/golden/pairs_*.mates.gz, matepair_cases.json), the host mirror
(mg::MatePairs::build) and the restatement of tests/mates_ref.py.

  a. every fixture and hand case, with the superReadID redirect (after
     mg_mark_contained) and without it, array for array;
  b. random paired sets of 5,000 pairs at 150 bp and at mixed lengths with
     planted containments;
  c. the refusals and the not-found error, their codes and messages;
  d. the lists survive mg_find_overlaps and are invalidated by a new ingest;
  e. the drop-in: Read::getMatePairList() after new OverlapGraph(ht)
     (test_mates_dropin.py);
  f. the word edges of the redirected-mate substring test (mates of 11-65 bp
     at the first, last and word-edge offsets of containers of every slot
     width, forward near-misses), 256 datasets, a 3,000-entry list, runs of
     1,000 equal records and the pair counts 0 .. 257: test_mate_edges.py on
     the sets of mate_sets.py, whose host mirror test_mate_edges_host.py pins."""
import numpy as np
import pytest

import mates_ref as R

pytestmark = pytest.mark.gpu

ALL = R.FIXTURES + R.HAND_CASES


@pytest.fixture(scope="module")
def engine():
    from metagenomics_amd.overlap import OverlapEngine

    e = OverlapEngine(0)
    yield e
    e.close()


def fixture(name):
    return R.golden(name) if name in R.FIXTURES else R.hand_cases()[name]


def assert_lists(got, want):
    assert np.array_equal(got[0], want[0]), "start differs"
    assert got[1].dtype == want[1].dtype and np.array_equal(got[1], want[1]), "records differ"


# ---- a. the fixtures
@pytest.mark.parametrize("path", ["ingest", "upload"])
@pytest.mark.parametrize("name", ALL)
def test_fixture_lists(engine, name, path, tmp_path):
    from metagenomics_amd.overlap import Dataset, host_mate_pairs

    g = fixture(name)
    pe, se = g.write_files(tmp_path)
    engine.set_option("layout", 1 if path == "ingest" else 0)
    if path == "ingest":
        assert engine.ingest_files(pe + se, g.l)["n_unique"] == len(g.reads)
    else:
        engine.upload(Dataset.from_files(pe + se, g.l))
    words, lens = engine.download_packed()
    engine.build_index(g.l, 21 if g.l > 21 else 0)
    sup = engine.mark_contained()
    assert np.array_equal(sup, g.super_ids)
    text, off = g.records()
    for block, use_super in ((1, True), (0, False)):
        start, recs = engine.mate_pairs(pe, g.l, use_super)
        assert_lists((start, recs), g.blocks[block])
        host = host_mate_pairs(words, lens, text, off, g.ppd, g.l, sup if use_super else None)
        assert_lists((start, recs), host[:2])
        assert (engine.good_pairs, engine.bad_pairs) == host[2:]
        assert engine.mates_ms > 0


# ---- b. random sets
@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("kind", ["150", "mixed"])
def test_random_pairs(engine, kind, layout):
    raw, ppd, l = R.random_pairs(kind, 5000, 23)
    reads = R.dataset_of(raw, l)
    engine.set_option("layout", layout)
    assert engine.ingest_ascii(list(raw), l) == len(reads)
    engine.build_index(l, 21)
    sup = engine.mark_contained()  # (pinned to the reference by the parity tests; here an input of both sides)
    text, off = R.records_of(raw)
    if kind == "mixed":
        assert np.count_nonzero(sup) > 500
    else:
        assert not sup.any()
    for use_super in (True, False):
        want = R.mate_lists(reads, list(raw), ppd, l, sup if use_super else None)
        n = engine.build_mate_pairs(text, off, ppd, l, use_super)
        got = engine.mate_lists()
        assert n == len(want[1])
        assert_lists(got, want[:2])
        assert (engine.good_pairs, engine.bad_pairs) == want[2:]
    # duplicates were dropped and some mates were redirected into a read where they do not occur
    assert len(want[1]) < 2 * want[2]


# ---- c. refusals
def test_refusals_and_not_found(engine):
    from metagenomics_amd.overlap import MgError, OverlapEngine

    raw, ppd, l = R.random_pairs("mixed", 300, 5)
    raw = list(raw)
    text, off = R.records_of(raw)
    engine.set_option("layout", 1)
    engine.ingest_ascii(raw, l)
    with pytest.raises(MgError, match="mg_build_mate_pairs must run for the current reads first"):
        engine.mate_lists()
    with pytest.raises(MgError, match="use_super needs a completed mg_mark_contained"):
        engine.build_mate_pairs(text, off, ppd, l, True)
    engine.build_mate_pairs(text, off, ppd, l, False)  # no redirect: needs no index
    with pytest.raises(MgError, match="n_raw must be even"):
        engine.build_mate_pairs(text, off[:-1], (ppd[0], ppd[1] - 1), l, False)
    with pytest.raises(MgError, match="mg_build_mate_pairs must run"):  # a refused build leaves no lists
        engine.mate_lists()
    with pytest.raises(MgError, match="does not add up"):
        engine.build_mate_pairs(text, off, (ppd[0], ppd[1] + 1), l, False)
    with pytest.raises(MgError, match="does not add up"):
        engine.build_mate_pairs(text, off, (ppd[0],), l, False)
    with pytest.raises(MgError, match="more than 256 datasets"):
        engine.build_mate_pairs(text, off, [1] * 300, l, False)
    # a good mate without a resident read: the first such raw index
    k = next(i for i in range(len(raw)) if R.passes(raw[i], l) and R.passes(raw[i ^ 1], l))
    gone = min(raw[k].upper(), R.rc(raw[k].upper()))
    rest = [r for r in raw if min(r.upper(), R.rc(r.upper())) != gone]
    with pytest.raises(KeyError) as e:
        R.mate_lists(R.dataset_of(rest, l), raw, ppd, l)
    engine.ingest_ascii(rest, l)
    with pytest.raises(MgError, match=f"String not found in Dataset: raw record {e.value.args[0]} "):
        engine.build_mate_pairs(text, off, ppd, l, False)
    with pytest.raises(MgError, match="mg_build_mate_pairs must run"):
        engine.mate_lists()
    # sharded, source-range and exchange-mode contexts: no redirect
    e2 = OverlapEngine(0)
    try:
        e2.ingest_ascii(raw, l)
        e2.build_index(l, 21)
        e2.mark_contained()
        e2.set_shard(0, 2)
        with pytest.raises(MgError, match="the context is sharded"):
            e2.build_mate_pairs(text, off, ppd, l, True)
        e2.set_shard(0, 1, 10, 50)
        with pytest.raises(MgError, match="the context is sharded"):
            e2.build_mate_pairs(text, off, ppd, l, True)
        assert e2.build_mate_pairs(text, off, ppd, l, False) > 0
        e2.set_shard(0, 1)
        e2.xchg_begin(l, 21)
        with pytest.raises(MgError, match="exchange-mode build"):
            e2.build_mate_pairs(text, off, ppd, l, True)
    finally:
        e2.close()


# ---- d. lifetime
def test_lists_survive_discovery_and_die_with_the_reads(engine):
    from metagenomics_amd.overlap import MgError

    g = R.golden("pairs_mixed")
    raw_all = g.raw + [r for d in g.se for r in [b"".join(x.split(b"\n")[1:]).decode() for x in d.split(b">")[1:]]]
    engine.set_option("layout", 1)
    assert engine.ingest_ascii(raw_all, g.l) == len(g.reads)
    engine.build_index(g.l, 21)
    engine.mark_contained()
    text, off = g.records()
    engine.build_mate_pairs(text, off, g.ppd, g.l, True)
    before = engine.mate_lists()
    assert_lists(before, g.blocks[1])
    assert engine.find_overlaps() > 0
    engine.build_discoveries()
    assert_lists(engine.mate_lists(), before)
    engine.ingest_ascii(raw_all, g.l)
    with pytest.raises(MgError, match="mg_build_mate_pairs must run for the current reads first"):
        engine.mate_lists()
