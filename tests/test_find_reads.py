"""mg_find_reads (mg_mates.hip: k_ingest / k_ingest_long + k_find_reads): the
batched Dataset::getReadFromString on the device, at every slot width and
across the word boundaries, after a host upload and after the device ingest,
with the clustered layout on and off.

Per length: a 2,000-read set given on random strands, partly in lower case and
with duplicates.  Every raw record must map to the ID whose canonical string it
is (the ID -> string map is the sorted set of canonical strings, Dataset.cpp:
197-202, 316-345) with the right strand bit; strings that are not in the set
must give 0: the reverse complement of an absent string, a read with one base
changed, a proper prefix, a read extended by 'A's (the same packed words: only
the length tiebreak rejects it), a read extended by one 'C', invalid records."""
import functools

import numpy as np
import pytest

from mates_ref import passes, rc

pytestmark = pytest.mark.gpu

L_MIN = 15
LENGTHS = list(range(20, 33)) + [33, 64, 65, 150, 1024, 1025, "mixed"]
N_READS = 2000


@pytest.fixture(scope="module")
def engine():
    from metagenomics_amd.overlap import OverlapEngine

    e = OverlapEngine(0)
    yield e
    e.close()


def rand_strings(rng, n, lens):
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [acgt[rng.integers(0, 4, int(lens[k]))].tobytes().decode() for k in range(n)]


class FindSet:
    def __init__(self, length):
        rng = np.random.default_rng(900 + (length if length != "mixed" else 7))
        if length == "mixed":
            lens = rng.integers(20, 301, N_READS)
        else:
            lens = np.full(N_READS, length)
        base = [s for s in rand_strings(rng, N_READS, lens) if passes(s, L_MIN)]
        if length == "mixed":
            # a read, a proper prefix of it and the read extended by 'A's, all in the set
            for s in base[:40]:
                if len(s) > 40:
                    base += [s[:len(s) // 2], s + "AAA", s[:32]]
            base = [s for s in base if passes(s, L_MIN)]
        self.raw = []
        for k, s in enumerate(base):
            t = rc(s) if rng.integers(0, 2) else s
            if k % 3 == 0:
                t = t.lower()
            self.raw.append(t)
            if k % 7 == 0:
                self.raw.append(rc(t))  # a duplicate on the other strand
        canon = {min(s.upper(), rc(s.upper())) for s in self.raw}
        self.reads = sorted(canon)  # ID - 1 -> string (std::string order)
        self.ids = {s: i + 1 for i, s in enumerate(self.reads)}
        # strings that are not in the set
        neg = []

        def add(s, why):
            c = min(s.upper(), rc(s.upper()))
            if c not in canon:
                neg.append((s, why))

        pick = [self.reads[0], self.reads[-1]] + [self.reads[int(i)] for i in rng.integers(0, len(self.reads), 120)]
        for j, s in enumerate(pick):
            p = int(rng.integers(0, len(s)))
            add(s[:p] + "ACGT"[("ACGT".index(s[p]) + 1 + j % 3) % 4] + s[p + 1:], "one base changed")
            add(s[:-1], "proper prefix")
            add(s[1:], "proper suffix")
            add(s + "A", "extended by A")
            add(s + "A" * (1 + (32 - len(s) % 32) % 32), "extended by As across the word edge")
            add(s + "A" * 33, "extended by more than a word of As")
            add(s + "C", "extended by C")
            add(rc(s + "C"), "reverse complement of an absent string")
        absent = rand_strings(rng, 60, np.full(60, len(pick[0])))
        for s in absent:
            add(rc(s), "reverse complement of an absent string")
        self.neg = [(s, w) for s, w in neg]
        self.invalid = [pick[2][:5] + "N" + pick[2][6:], pick[3][:L_MIN], "", "A" * len(pick[4]), pick[5] + "n",
                        pick[6][:-1] + "\r"]

    def queries(self):
        q = list(self.raw) + [s for s, _ in self.neg] + self.invalid
        want_id = np.zeros(len(q), dtype=np.uint32)
        want_fl = np.zeros(len(q), dtype=np.uint8)
        for i, s in enumerate(q):
            if not passes(s, L_MIN):
                continue
            u = s.upper()
            c = min(u, rc(u))
            want_fl[i] = 1
            if c in self.ids:
                want_id[i] = self.ids[c]
                want_fl[i] |= 2 if u == c else 0
        return q, want_id, want_fl


@functools.lru_cache(maxsize=None)
def find_set(length):
    return FindSet(length)


def load(engine, s, path, layout):
    from metagenomics_amd.overlap import Dataset

    engine.set_option("layout", layout)
    if path == "upload":
        ds = Dataset.from_strings(s.raw, L_MIN)
        assert ds.num_unique == len(s.reads)
        engine.upload(ds)
    else:
        assert engine.ingest_ascii(s.raw, L_MIN) == len(s.reads)


@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("path", ["upload", "ingest"])
@pytest.mark.parametrize("length", LENGTHS)
def test_find_reads(engine, length, path, layout):
    s = find_set(length)
    load(engine, s, path, layout)
    q, want_id, want_fl = s.queries()
    # the set holds what the test is about
    assert np.count_nonzero(want_id) >= len(s.raw) and len(s.neg) > 300
    assert want_id.max() == len(s.reads) and want_id[want_id > 0].min() == 1  # the first and the last ID
    assert np.any(want_fl == 3) and np.any(want_fl == 1)
    ids, flags = engine.find_reads(q, L_MIN)
    bad = np.flatnonzero(ids != want_id)
    why = [w for _, w in s.neg]
    assert bad.size == 0, [(int(i), int(ids[i]), int(want_id[i]),
                            why[i - len(s.raw)] if len(s.raw) <= i < len(s.raw) + len(why) else "raw / invalid")
                           for i in bad[:5]]
    assert np.array_equal(flags, want_fl)
    if layout and path == "upload" and max(map(len, s.reads)) <= 1024:  # (long reads keep ID order)
        assert not np.array_equal(engine.slot_of_ids(), np.arange(len(s.reads)))  # (the search went through d_phys)


def test_find_reads_palindrome_and_single_read(engine):
    h = "ACGGTCATTGCAGGCTAAGCTTACG"
    pal = h + rc(h)
    assert pal == rc(pal)
    engine.set_option("layout", 1)
    assert engine.ingest_ascii([pal.lower()], 10) == 1
    assert rc(h)[0] != "A"
    ids, flags = engine.find_reads([pal, pal.lower(), pal[:-1], pal + "A", h + "A" + rc(h)[1:], "ACGN" * 12], 10)
    assert ids.tolist() == [1, 1, 0, 0, 0, 0]
    assert flags.tolist() == [3, 3, 1, 1, 1, 0]  # a read that is its own reverse complement sets bit 1
    # no records, and no reads
    ids, flags = engine.find_reads([], 10)
    assert ids.shape == (0,) and flags.shape == (0,)
    assert engine.ingest_ascii(["ACGN" * 12], 10) == 0
    ids, flags = engine.find_reads([pal], 10)
    assert ids.tolist() == [0] and flags.tolist() == [1]


def test_find_reads_query_wider_than_the_slots(engine):
    """Records longer than every resident read (more words than a slot) are not found."""
    s = find_set(33)
    load(engine, s, "ingest", 1)
    r = s.reads[5]
    long_q = [r + "AAC" * 70, r + "ACGT" * 300, rc(r + "ACGT" * 300), r]
    assert all(passes(q, L_MIN) for q in long_q)
    ids, flags = engine.find_reads(long_q, L_MIN)
    assert ids.tolist() == [0, 0, 0, 6]
    assert flags.tolist()[:3] == [1, 1, 1] and flags[3] == 3


def test_find_reads_in_a_sharded_and_an_exchange_context():
    """Every rank holds all reads: the lookup does not refuse such contexts."""
    from metagenomics_amd.overlap import OverlapEngine

    s = find_set(64)
    e = OverlapEngine(0)
    try:
        e.set_shard(1, 2)
        assert e.ingest_ascii(s.raw, L_MIN) == len(s.reads)
        q, want_id, want_fl = s.queries()
        ids, flags = e.find_reads(q, L_MIN)
        assert np.array_equal(ids, want_id) and np.array_equal(flags, want_fl)
        e.set_shard(0, 1)
        e.xchg_begin(40, 21)
        ids, flags = e.find_reads(q, L_MIN)
        assert np.array_equal(ids, want_id) and np.array_equal(flags, want_fl)
    finally:
        e.close()
