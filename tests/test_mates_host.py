"""The host mirror of the mate-pair path (mg::read_pairs_*, mg::MatePairs::build,
csrc/host/mg_mates.cpp) against the reference's own lists
(tests/golden/pairs_*.mates.gz and matepair_cases.json, dumped from the
reference's readMatePairsFromFile() by tests/golden/make_matepair_golden.py)
and against the plain restatement of tests/mates_ref.py.  CPU only.

  a. the pair reader: storeMatePairInformation's loop with getline's rules
     (a trailing newline's extra empty pair, an odd FASTA record count, CRLF,
     a truncated last record), record for record against the restatement;
  b. the lists: both golden blocks (with the reference's superReadIDs, and with
     none: the setDataset case) entry for entry, mirror and restatement;
  c. the good / bad pair counts, mirror against restatement;
  d. random paired sets with planted containments, mirror against restatement;
  e. the refusals and the not-found error;
  f. the stand-alone ASan + UBSan check (make mates_check_asan) on every fixture."""
import os
import random
import subprocess

import numpy as np
import pytest

import mates_ref as R
from conftest import ROOT

ALL = R.FIXTURES + R.HAND_CASES


def fixture(name):
    return R.golden(name) if name in R.FIXTURES else R.hand_cases()[name]


def host_dataset(g, tmp_path):
    """The host Dataset mirror of the fixture's files: (words, lens, strings in ID order)."""
    from metagenomics_amd.overlap import Dataset

    pe, se = g.write_files(tmp_path)
    ds = Dataset.from_files(pe + se, g.l)
    words, lens = ds.packed()
    return ds, np.array(words), np.array(lens), [ds.read(i) for i in range(1, ds.num_unique + 1)]


def assert_lists(got, want):
    assert np.array_equal(got[0], want[0]), "start differs"
    assert got[1].dtype == want[1].dtype and np.array_equal(got[1], want[1]), "records differ"


# ---- a. the reader
@pytest.mark.parametrize("name", ALL)
def test_reader_equals_restatement(name):
    from metagenomics_amd.overlap import read_pairs

    g = fixture(name)
    for data in g.pe:
        text, off, ppf, _ = read_pairs(data=data)
        want = R.read_pairs(data)
        got = [text[int(off[i]):int(off[i + 1])].decode("latin-1") for i in range(len(off) - 1)]
        assert got == want
        assert int(ppf[0]) * 2 == len(want)


def test_reader_files_and_quirks(tmp_path):
    from metagenomics_amd.overlap import MgError, read_pairs

    g = R.golden("pairs_mixed")
    pe, _ = g.write_files(tmp_path)
    text, off, ppf, _ = read_pairs(pe)
    assert [int(x) for x in ppf] == g.ppd
    assert [text[int(off[i]):int(off[i + 1])].decode() for i in range(len(off) - 1)] == g.raw
    # an odd FASTA record count pairs the last sequence with itself
    assert g.raw[-1] == g.raw[-2] and len(R.read_pairs(g.pe[1])) % 2 == 0
    # a FASTQ file ending in a newline gives one more pair of two empty mates
    s = R.golden("pairs_small")
    assert s.pe[0].endswith(b"\n") and s.raw[-2:] == ["", ""] and s.pe[0].count(b"\n") // 8 + 1 == s.ppd[0]
    # CRLF leaves '\r' in
    c = R.hand_cases()["crlf_fastq"]
    assert c.raw[2].endswith("\r") and c.raw[3].endswith("\r") and not c.raw[0].endswith("\r")
    # a truncated last record repeats its last text
    t = R.hand_cases()["truncated_fastq"]
    assert t.raw[2] == t.raw[3] and R.passes(t.raw[2], t.l)
    with pytest.raises(MgError, match="Unknown input file format"):
        read_pairs(data=b"ACGT\n")
    with pytest.raises(MgError, match="Unknown input file format"):
        read_pairs(data=b"")
    with pytest.raises(MgError, match="Unable to open"):
        read_pairs([str(tmp_path / "missing.fq")])


# ---- b, c. the lists
@pytest.mark.parametrize("name", ALL)
def test_restatement_equals_reference(name):
    g = fixture(name)
    assert g.reads == R.dataset_of(g.raw + sum((se_records(d) for d in g.se), []), g.l)
    assert set(g.blocks) == {0, 1}
    assert_lists(R.mate_lists(g.reads, g.raw, g.ppd, g.l, g.super_ids)[:2], g.blocks[1])
    assert_lists(R.mate_lists(g.reads, g.raw, g.ppd, g.l, None)[:2], g.blocks[0])


def se_records(data):
    """readDataset's records of a single-end FASTA fixture file (one '>' per header line)."""
    return [b"".join(r.split(b"\n")[1:]).decode() for r in data.split(b">")[1:]]


@pytest.mark.parametrize("name", ALL)
def test_host_mirror_equals_reference(name, tmp_path):
    from metagenomics_amd.overlap import host_mate_pairs

    g = fixture(name)
    _, words, lens, strings = host_dataset(g, tmp_path)
    assert strings == g.reads
    text, off = g.records()
    for block, sup in ((1, g.super_ids), (0, None)):
        start, recs, good, bad = host_mate_pairs(words, lens, text, off, g.ppd, g.l, sup)
        assert_lists((start, recs), g.blocks[block])
        _, _, rgood, rbad = R.mate_lists(g.reads, g.raw, g.ppd, g.l, sup)
        assert (good, bad) == (rgood, rbad) and good + bad == len(g.raw) // 2


def test_fixtures_hold_their_cases():
    """What the fixtures were made to show is in them (from the reference's dump)."""
    s = R.golden("pairs_small")
    start, recs = s.blocks[1]
    deg = np.diff(start[1:].astype(np.int64))
    assert deg.max() >= 4                                    # one read with several different mates
    own = np.repeat(np.arange(1, len(s.reads) + 1), deg)
    assert np.any(recs["id"] == own)                         # a read paired with itself
    pal = [i + 1 for i, r in enumerate(s.reads) if r == R.rc(r)]
    assert pal and start[pal[0] + 1] > start[pal[0]]         # the palindrome has mates
    assert any(x != x.upper() for x in s.raw) and any("N" in x for x in s.raw)
    assert any(len(x) == s.l for x in s.raw)
    m = R.golden("pairs_mixed")
    assert np.count_nonzero(m.super_ids) >= 10
    # (A in B in C: markContainedReads keeps the longest container, so the reference's own
    # superReadIDs never point at a contained read; test_host_mirror_random plants such chains)
    assert not np.array_equal(m.blocks[0][1], m.blocks[1][1])
    assert set(np.unique(m.blocks[1][1]["dataset"])) == {0, 1}
    assert set(np.unique(m.blocks[1][1]["orient"])) == {0, 1, 2, 3}
    # a redirected mate that is found in its super read and one that is not
    found = set()
    for i in range(0, len(m.raw)):
        line = m.raw[i].upper()
        if not R.passes(line, m.l):
            continue
        rid = m.reads.index(min(line, R.rc(line))) + 1
        if m.super_ids[rid]:
            found.add(line in m.reads[m.super_ids[rid] - 1])
    assert found == {True, False}
    lg = R.golden("pairs_long")
    assert max(len(r) for r in lg.reads) > 1024 and min(len(r) for r in lg.reads) == 150


# ---- d. random sets
@pytest.mark.parametrize("kind,n_pairs", [("150", 600), ("mixed", 400)])
def test_host_mirror_random(kind, n_pairs):
    from metagenomics_amd.overlap import Dataset, host_mate_pairs

    raw, ppd, l = R.random_pairs(kind, n_pairs, 11)
    reads = R.dataset_of(raw, l)
    ds = Dataset.from_strings([r for r in raw if R.passes(r, l)], l)
    words, lens = ds.packed()
    assert [ds.read(i) for i in range(1, ds.num_unique + 1)] == reads
    text, off = R.records_of(raw)
    sup = R.contained_super(reads, random.Random(5))
    assert kind == "150" or np.count_nonzero(sup) > 20
    # a super read that is contained itself: the redirect must stop after one step
    assert kind == "150" or any(sup[i] and sup[sup[i]] for i in range(1, len(reads) + 1))
    for s in (sup, None):
        want = R.mate_lists(reads, list(raw), ppd, l, s)
        got = host_mate_pairs(words, lens, text, off, ppd, l, s)
        assert_lists(got[:2], want[:2])
        assert got[2:] == want[2:]


# ---- e. refusals
def test_host_mirror_refusals():
    from metagenomics_amd.overlap import Dataset, MgError, host_mate_pairs

    raw, ppd, l = R.random_pairs("150", 50, 3)
    ds = Dataset.from_strings([r for r in raw if R.passes(r, l)], l)
    words, lens = ds.packed()
    text, off = R.records_of(raw)
    with pytest.raises(MgError, match="bad arguments"):
        host_mate_pairs(words, lens, text, off[:-1], ppd, l)          # an odd n_raw
    with pytest.raises(MgError, match="bad arguments"):
        host_mate_pairs(words, lens, text, off, (ppd[0], ppd[1] + 1), l)  # counts that do not add up
    with pytest.raises(MgError, match="bad arguments"):
        host_mate_pairs(words, lens, text, off, (ppd[0],), l)
    # a good mate that is in no read: the first such raw index is named
    k = next(i for i, r in enumerate(raw) if R.passes(raw[i], l) and R.passes(raw[i ^ 1], l))
    gone = min(raw[k].upper(), R.rc(raw[k].upper()))
    ds2 = Dataset.from_strings([r for r in raw if R.passes(r, l) and min(r.upper(), R.rc(r.upper())) != gone], l)
    w2, l2 = ds2.packed()
    with pytest.raises(KeyError) as e:
        R.mate_lists(R.dataset_of([r for r in raw if min(r.upper(), R.rc(r.upper())) != gone], l), list(raw), ppd, l)
    with pytest.raises(MgError, match=f"String not found in Dataset: raw record {e.value.args[0]}$"):
        host_mate_pairs(w2, l2, text, off, ppd, l)


# ---- f. the sanitizer build of the host code, from its own main
@pytest.fixture(scope="module")
def mates_check():
    csrc = os.path.join(ROOT, "metagenomics_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "mates_check_asan"], check=True)
    return os.path.join(ROOT, "metagenomics_amd", "lib", "asan", "mg_mates_check")


@pytest.mark.parametrize("name", ALL)
def test_mates_check_asan(name, mates_check, tmp_path):
    g = fixture(name)
    pe, _ = g.write_files(tmp_path)
    dump = tmp_path / "dump.txt"
    lines = ["#N %d" % len(g.reads)] + ["#R %d %s" % (i + 1, r) for i, r in enumerate(g.reads)]
    lines += ["#S %d %d" % (i, s) for i, s in enumerate(g.super_ids) if s]
    for b in (1, 0):
        start, recs = g.blocks[b]
        lines.append("#B %d" % b)
        for a in range(1, len(g.reads) + 1):
            lines += ["#M %d %d %d %d" % (a, r["id"], r["orient"], r["dataset"])
                      for r in recs[int(start[a]):int(start[a + 1])]]
    dump.write_text("\n".join(lines) + "\n")
    r = subprocess.run([mates_check, str(g.l), str(dump)] + pe, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mg_mates_check: ok" in r.stdout and "runtime error" not in r.stderr
