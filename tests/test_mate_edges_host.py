"""The host mirror of the mate lists (mg::MatePairs::build) at the shapes of
tests/mate_sets.py, against the restatement of tests/mates_ref.py, which the
goldens pin to the reference.  CPU only.  The device test
(tests/test_mate_edges.py) uses the mirror as its second expected value, so
this module keeps it pinned where no fixture reaches:

  a. the generators' preconditions, checked once more from outside them:
     every class holds every planted case, the oracle's superReadID of each
     planted mate is its container, found / not found is what str.find says;
  b. per container class (slot widths 1, 2, 5, 8, 32 words and the long
     layout up to 60 kb): the mirror equals the restatement with the oracle's
     superReadIDs and with none;
  c. the order and dedup set (256 datasets, a 3,000-entry list, runs of 1,000
     equal records) and the pair counts 0 .. 257."""
import numpy as np
import pytest

import mate_sets as M
import mates_ref as R


def assert_lists(got, want):
    assert np.array_equal(got[0], want[0]), "start differs"
    assert got[1].dtype == want[1].dtype and np.array_equal(got[1], want[1]), "records differ"


def host_lists(s, raw, ppd, sup):
    """host_mate_pairs over the mirror's own Dataset of the set's records."""
    from metagenomics_amd.overlap import Dataset, host_mate_pairs

    ds = Dataset.from_strings([r for r in s.records if R.passes(r, s.l)], s.l)
    assert [ds.read(i) for i in range(1, ds.num_unique + 1)] == s.reads
    words, lens = ds.packed()
    text, off = R.records_of(raw)
    return host_mate_pairs(np.array(words), np.array(lens), text, off, ppd, s.l, sup)


# ---- a. the generators
@pytest.mark.parametrize("cls", list(M.CLASSES))
def test_class_preconditions(cls):
    s = M.class_set(cls)
    M.check_class(s)
    assert 0 <= s.redraws <= M.MAX_REDRAWS
    assert len(s.cases) == M.expected_cases(cls)
    sweep_L = M.SWEEP_L_64K if cls == "long64k" else M.SWEEP_L
    for n in M.CLASSES[cls]:  # every (container length, L, offset, strand) of the sweep is there once
        for L in (x for x in sweep_L if x < n):
            for off in M.sweep_offsets(n, L):
                for strand in "+-":
                    assert sum(1 for c in s.cases if c.kind == "sweep" and (len(c.cont), c.L, c.s, c.strand)
                               == (n, L, off, strand)) == 1
    # the orientation bit the restatement gives the partner's record is the planted answer
    start, recs = s.want(True)[:2]
    for c in s.cases:
        a = s.read_id(s.raw[2 * c.pair + 1 - c.side])
        (rec,) = recs[int(start[a]):int(start[a + 1])]
        assert int(rec["id"]) == s.read_id(c.cont)
        assert int(rec["orient"]) & 1 == int(c.found), c.label()  # bit 0: the owner's mate, here the planted one


def test_classes_reach_every_edge():
    """What the sets were made for, over all classes."""
    cases = [c for cls in M.CLASSES for c in M.class_set(cls).cases]
    assert len(cases) == sum(M.expected_cases(cls) for cls in M.CLASSES) > 1100
    for cls, lengths in M.CLASSES.items():
        top = max(lengths)
        mine = [c for c in cases if c.cls == cls and c.kind == "sweep" and len(c.cont) == top and c.strand == "+"]
        assert top % 32 == 0 or cls == "long"  # the widest container fills the slot's last word (3,000 bp: 94 words)
        assert any(c.s == top - c.L for c in mine)  # the last offset of the class's widest container
        assert any(c.L < 32 for c in mine)
    assert {c.L for c in cases if c.kind == "sweep"} == set(M.SWEEP_L)
    assert {c.L for c in cases if c.kind == "decoy"} == set(M.DECOY_L)
    assert {c.L for c in cases if c.cls == "long64k"} == set(M.SWEEP_L_64K)


# ---- b. the classes
@pytest.mark.parametrize("cls", list(M.CLASSES))
def test_host_mirror_classes(cls):
    s = M.class_set(cls)
    for use_super in (True, False):
        want = s.want(use_super)
        got = host_lists(s, s.raw, s.ppd, s.super_ids if use_super else None)
        assert_lists(got[:2], want[:2])
        assert got[2:] == want[2:]


# ---- c. order, dedup and counts
def test_host_mirror_order_set():
    s = M.order_set()
    assert len(s.ppd) == 256 and [d for d, n in enumerate(s.ppd) if n] == [0, 3, 255]
    for use_super in (True, False):
        want = s.want(use_super)
        got = host_lists(s, s.raw, s.ppd, s.super_ids if use_super else None)
        assert_lists(got[:2], want[:2])
        assert got[2:] == want[2:]


@pytest.mark.parametrize("n_pairs", M.COUNTS)
def test_host_mirror_counts(n_pairs):
    s = M.count_pool()
    raw, ppd, want = M.count_want(n_pairs)
    got = host_lists(s, raw, ppd, None)
    assert_lists(got[:2], want[:2])
    assert got[2:] == want[2:] == (n_pairs - n_pairs // 5, n_pairs // 5)
