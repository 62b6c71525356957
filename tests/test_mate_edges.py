"""mg_build_mate_pairs (mg_mates.hip) at the word edges of the redirected-mate
substring test and at the order, dedup and count edges of the list build,
against the restatement of tests/mates_ref.py (pinned to the reference by the
goldens) and the host mirror (pinned at these shapes by
tests/test_mate_edges_host.py).  The sets are those of tests/mate_sets.py.

  a. per container class (slot widths 1, 2, 5, 8, 32 words, the long layout
     up to 60 kb), by both load paths: mates of 11 .. 65 bp cut from either
     strand of a container at the first, the last and the word-edge offsets,
     and containers with forward near-misses in front of the true occurrence.
     mg_mark_contained must equal the oracle's superReadIDs (l = 10), then the
     lists with the redirect and without it equal both expected values;
  b. 256 datasets of which three hold pairs, a 3,000-entry list in input
     order, runs of 1,000 equal records, two orientations alternating;
  c. pair counts 0 .. 257 around the wavefront and workgroup edges of the good
     pair count, and contexts without reads.

Not reachable here: "redirect once, not transitively".  mg_mark_contained
assigns the longest container, which is itself uncontained; the mirror's
test_host_mirror_random keeps that case."""
import numpy as np
import pytest

import mate_sets as M
import mates_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from metagenomics_amd.overlap import OverlapEngine

    e = OverlapEngine(0)
    yield e
    e.close()


def assert_lists(got, want, what=""):
    assert np.array_equal(got[0], want[0]), "start differs" + what
    assert got[1].dtype == want[1].dtype and np.array_equal(got[1], want[1]), "records differ" + what


def load(engine, s, path):
    """The set's Dataset on the device, by the ingest (clustered slots) or as an
    upload of the host Dataset (slots in ID order).  Returns (words, lens)."""
    from metagenomics_amd.overlap import Dataset

    engine.set_option("layout", 1 if path == "ingest" else 0)
    if path == "ingest":
        assert engine.ingest_ascii(s.records, s.l) == len(s.reads)
    else:
        engine.upload(Dataset.from_strings([r for r in s.records if R.passes(r, s.l)], s.l))
    words, lens = engine.download_packed()
    assert lens.tolist() == [len(r) for r in s.reads]
    return words, lens


def check_build(engine, s, words, lens, raw, ppd, use_super, want):
    """One build against the restatement and the mirror, array for array."""
    from metagenomics_amd.overlap import host_mate_pairs

    text, off = R.records_of(raw)
    n = engine.build_mate_pairs(text, off, ppd, s.l, use_super)
    got = engine.mate_lists()
    counts = (engine.good_pairs, engine.bad_pairs)
    host = host_mate_pairs(words, lens, text, off, ppd, s.l, s.super_ids if use_super else None)
    print("%s use_super=%d: %d records, good/bad %s" % (s.name, use_super, n, counts))
    what = ""
    if use_super and s.cases:
        first = s.first_difference(*got)
        what = "; first differing planted case (class, kind, L, s, strand): %s" % first
        print(what)
    assert n == len(want[1]), "list length" + what
    assert_lists(got, want[:2], what)
    assert_lists(got, host[:2], what)
    assert counts == want[2:] == host[2:]


# ---- a. the container classes
@pytest.mark.parametrize("path", ["ingest", "upload"])
@pytest.mark.parametrize("cls", list(M.CLASSES))
def test_class_lists(engine, cls, path):
    s = M.class_set(cls)
    words, lens = load(engine, s, path)
    assert words.shape[1] == (max(M.CLASSES[cls]) + 31) // 32  # the slot's last word is the container's
    engine.build_index(s.l, 0)
    sup = engine.mark_contained()
    diff = np.flatnonzero(sup != s.super_ids)
    assert diff.size == 0, "superReadID of read %d (%d bp): device %d, oracle %d" % (
        diff[0], len(s.reads[diff[0] - 1]), sup[diff[0]], s.super_ids[diff[0]])
    for use_super in (True, False):
        check_build(engine, s, words, lens, s.raw, s.ppd, use_super, s.want(use_super))


# ---- b. order and dedup
@pytest.mark.parametrize("path", ["ingest", "upload"])
def test_order_and_dedup(engine, path):
    s = M.order_set()
    words, lens = load(engine, s, path)
    engine.build_index(s.l, 0)
    assert np.array_equal(engine.mark_contained(), s.super_ids)
    for use_super in (True, False):
        check_build(engine, s, words, lens, s.raw, s.ppd, use_super, s.want(use_super))
    start, recs = engine.mate_lists()
    assert int(np.diff(start[1:].astype(np.int64)).max()) == M.HUB_MATES
    assert set(np.unique(recs["dataset"]).tolist()) == {0, 3, 255}


# ---- c. counts
@pytest.mark.parametrize("path", ["ingest", "upload"])
def test_pair_counts(engine, path):
    s = M.count_pool()
    words, lens = load(engine, s, path)
    for n_pairs in M.COUNTS:
        raw, ppd, want = M.count_want(n_pairs)
        check_build(engine, s, words, lens, raw, ppd, False, want)
        assert (engine.good_pairs, engine.bad_pairs) == (n_pairs - n_pairs // 5, n_pairs // 5)


def test_no_resident_reads(engine):
    from metagenomics_amd.overlap import MgError

    s = M.count_pool()
    bad = [r for p in range(4, len(s.raw) // 2, 5) for r in s.raw[2 * p:2 * p + 2]][:12]
    assert not any(R.passes(a, s.l) and R.passes(b, s.l) for a, b in zip(bad[::2], bad[1::2]))
    engine.set_option("layout", 1)
    assert engine.ingest_ascii(["ACGTNACGTACGTACGTACGT", "ACGT"], s.l) == 0
    text, off = R.records_of(bad)
    assert engine.build_mate_pairs(text, off, (len(bad) // 2,), s.l, False) == 0
    start, recs = engine.mate_lists()
    assert start.tolist() == [0, 0] and len(recs) == 0
    assert (engine.good_pairs, engine.bad_pairs) == (0, len(bad) // 2)
    assert_lists((start, recs), R.mate_lists([], bad, (len(bad) // 2,), s.l)[:2])
    good = s.raw[:2]
    assert R.passes(good[0], s.l) and R.passes(good[1], s.l)
    text, off = R.records_of(bad[:2] + good)
    with pytest.raises(KeyError) as e:
        R.mate_lists([], bad[:2] + good, (2,), s.l)
    assert e.value.args[0] == 2
    with pytest.raises(MgError, match="String not found in Dataset: raw record 2 "):
        engine.build_mate_pairs(text, off, (2,), s.l, False)
    assert (engine.good_pairs, engine.bad_pairs) == (1, 1)
    text, off = R.records_of(good)
    with pytest.raises(MgError, match="String not found in Dataset: raw record 0 "):
        engine.build_mate_pairs(text, off, (1,), s.l, False)
    with pytest.raises(MgError, match="mg_build_mate_pairs must run"):
        engine.mate_lists()
