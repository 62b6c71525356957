"""Plain restatement of the reference's mate-pair path for the tests
(storeMatePairInformation Dataset.cpp:208-310, getReadFromString :421-455,
Read::addMatePair Read.cpp:132-166) on Python strings and dicts, plus the
loaders of the fixtures that pin it to the reference itself
(tests/golden/pairs_*.mates.gz, matepair_cases.json; made by
tests/golden/make_matepair_golden.py).  No native code."""
import functools
import gzip
import json
import os
import random

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MATE_DTYPE = np.dtype([("id", "<u4"), ("orient", "u1"), ("dataset", "u1"), ("pad", "<u2")])
FIXTURES = ("pairs_small", "pairs_mixed", "pairs_long")
_COMP = str.maketrans("ACGT", "TGCA")


def rc(s):
    return s.translate(_COMP)[::-1]


def test_read(s):
    """Dataset::testRead (Dataset.cpp:398-413)."""
    if any(c not in "ACGT" for c in s):
        return False
    thr = int(len(s) * .8)
    return all(s.count(c) < thr for c in "ACGT")


test_read.__test__ = False  # (a helper, not a test)


def passes(raw, l):
    """The ingest's filter on a raw record (any case)."""
    return l < len(raw) <= 65535 and test_read(raw.upper())


# ---- the pair reader (storeMatePairInformation's loop with getline's rules)
class _Stream:
    def __init__(self, data):
        self.d, self.pos, self.eof, self.fail, self.text = data, 0, False, False, b""

    def getline(self, delim=b"\n"):
        if self.eof or self.fail:  # not good: the string keeps its text
            self.fail = True
            return self.text
        e = self.d.find(delim, self.pos)
        if e >= 0:
            self.text, self.pos = self.d[self.pos:e], e + 1
        else:
            self.text, self.pos, self.eof = self.d[self.pos:], len(self.d), True
            if not self.text:
                self.fail = True
        return self.text


def read_pairs(data):
    """The raw mates [line1, line2, line1, ...] of one paired-end file's bytes."""
    f = _Stream(data)
    first = f.getline()
    if first[:1] not in (b">", b"@"):
        raise ValueError("Unknown input file format.")
    fasta = first[:1] == b">"
    f.pos, f.eof = 0, False
    out = []
    while not f.eof:
        if fasta:
            f.getline()
            a = f.getline(b">")
            f.getline()
            b = f.getline(b">")
            out += [a.replace(b"\n", b""), b.replace(b"\n", b"")]
        else:
            lines = [f.getline() for _ in range(8)]
            out += [lines[1], lines[5]]
    return [x.decode("latin-1") for x in out]


# ---- the lists
def mate_lists(reads, raw, pairs_per_dataset, l, super_ids=None):
    """reads: the unique canonical strings in ID order; raw: the mates, 2 per
    pair; super_ids: superReadID per ID (index 0 unused) or None.  Returns
    (start uint64[n + 2], records MATE_DTYPE, good pairs, bad pairs); raises
    KeyError(raw index) for a good mate without a read."""
    ids = {s: i + 1 for i, s in enumerate(reads)}
    lists = [[] for _ in range(len(reads) + 1)]
    good = bad = 0
    p = 0
    assert len(raw) == 2 * sum(int(x) for x in pairs_per_dataset)
    for d, npairs in enumerate(pairs_per_dataset):
        for _ in range(int(npairs)):
            m = [raw[2 * p], raw[2 * p + 1]]
            p += 1
            if not (passes(m[0], l) and passes(m[1], l)):
                bad += 1
                continue
            good += 1
            r, o = [0, 0], [0, 0]
            for k in range(2):
                line = m[k].upper()
                canon = min(line, rc(line))
                if canon not in ids:
                    raise KeyError(2 * (p - 1) + k)
                r[k] = ids[canon]
                if super_ids is not None and super_ids[r[k]]:
                    r[k] = int(super_ids[r[k]])
                o[k] = 1 if line in reads[r[k] - 1] else 0
            for owner, rec in ((r[0], (r[1], o[0] * 2 + o[1], d)), (r[1], (r[0], o[0] + o[1] * 2, d))):
                if rec not in lists[owner]:
                    lists[owner].append(rec)
    return (*to_csr(lists), good, bad)


def to_csr(lists):
    n = len(lists) - 1
    start = np.zeros(n + 2, dtype=np.uint64)
    for a in range(1, n + 1):
        start[a + 1] = start[a] + len(lists[a])
    recs = np.zeros(int(start[n + 1]), dtype=MATE_DTYPE)
    k = 0
    for a in range(1, n + 1):
        for mid, o, d in lists[a]:
            recs[k] = (mid, o, d, 0)
            k += 1
    return start, recs


# ---- goldens
def parse_dump(text):
    """The reference driver's dump -> (reads in ID order, super_ids uint32[n + 1],
    {1: (start, recs), 0: (start, recs)})."""
    n, reads, sup, blocks, cur = 0, {}, {}, {}, None
    for line in text.splitlines():
        t = line.split()
        if t[0] == "#N":
            n = int(t[1])
        elif t[0] == "#R":
            reads[int(t[1])] = t[2] if len(t) > 2 else ""
        elif t[0] == "#S":
            sup[int(t[1])] = int(t[2])
        elif t[0] == "#B":
            cur = blocks.setdefault(int(t[1]), [[] for _ in range(n + 1)])
        elif t[0] == "#M":
            cur[int(t[1])].append((int(t[2]), int(t[3]), int(t[4])))
    super_ids = np.zeros(n + 1, dtype=np.uint32)
    for i, s in sup.items():
        super_ids[i] = s
    return [reads[i] for i in range(1, n + 1)], super_ids, {b: to_csr(v) for b, v in blocks.items()}


class Golden:
    """One fixture: the files' bytes (paired-end first), l and the reference's dump."""

    def __init__(self, name, l, pe, se, dump):
        self.name, self.l, self.pe, self.se = name, l, pe, se
        self.reads, self.super_ids, self.blocks = parse_dump(dump)
        self.raw, self.ppd = [], []
        for data in pe:
            m = read_pairs(data)
            self.raw += m
            self.ppd.append(len(m) // 2)

    def write_files(self, d):
        """The files under directory d; returns (pe paths, se paths)."""
        out = ([], [])
        for k, (lst, datas) in enumerate(((out[0], self.pe), (out[1], self.se))):
            for i, data in enumerate(datas):
                p = os.path.join(str(d), "%s.%s%d" % (self.name, "ps"[k], i))
                with open(p, "wb") as f:
                    f.write(data)
                lst.append(p)
        return out

    def records(self):
        """(text bytes, offsets) of the raw mates, as the C-ABI takes them."""
        return records_of(self.raw)


def records_of(raw):
    b = [x.encode("latin-1") for x in raw]
    off = np.zeros(len(b) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in b])
    return b"".join(b), off


@functools.lru_cache(maxsize=None)
def golden(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        meta = json.load(f)

    def gz(fn):
        with gzip.open(os.path.join(GOLDEN, fn), "rb") as f:
            return f.read()

    return Golden(name, meta["l"], [gz(f) for f in meta["pe"]], [gz(f) for f in meta["se"]], gz(meta["mates"]).decode())


@functools.lru_cache(maxsize=None)
def hand_cases():
    with open(os.path.join(GOLDEN, "matepair_cases.json")) as f:
        cases = json.load(f)
    return {c["name"]: Golden(c["name"], c["l"], [x.encode("latin-1") for x in c["pe"]],
                              [x.encode("latin-1") for x in c["se"]], c["dump"]) for c in cases}


HAND_CASES = ("crlf_fastq", "gt_in_fasta_header", "truncated_fastq", "truncated_fastq_header_only", "odd_fasta",
              "two_trailing_newlines")


# ---- random paired sets
def dataset_of(raw, l):
    """Dataset(pe, se, l)'s unique canonical strings in ID order for raw records."""
    return sorted({min(s.upper(), rc(s.upper())) for s in raw if passes(s, l)})


def contained_super(reads, rng):
    """A superReadID vector for the tests of the redirect: every read that is a
    substring of a longer read (either strand) points at one such container,
    chosen at random.  (Any vector is a legal input of the mate-list build; the
    reference's own choice is pinned by the goldens.)"""
    sup = np.zeros(len(reads) + 1, dtype=np.uint32)
    by_len = sorted(range(len(reads)), key=lambda i: -len(reads[i]))
    for i, s in enumerate(reads):
        r = rc(s)
        c = [j + 1 for j in by_len if len(reads[j]) > len(s) and (s in reads[j] or r in reads[j])]
        if c:
            sup[i + 1] = rng.choice(c)
    return sup


@functools.lru_cache(maxsize=None)
def random_pairs(kind, n_pairs, seed):
    """(raw mates, pairs_per_dataset, l).  kind "150": n_pairs of 150 bp from
    both strands of a genome short enough that mates repeat, in two datasets,
    with some dirt; kind "mixed": lengths 60-300 with planted containments."""
    rng = random.Random(seed)
    g = "".join(rng.choice("ACGT") for _ in range(max(400, n_pairs // 3)))
    raw = []

    def piece(n):
        p = rng.randrange(0, len(g) - n)
        s = g[p:p + n]
        return rc(s) if rng.random() < .5 else s

    for k in range(n_pairs):
        if kind == "150":
            a, b = piece(150), piece(150)
        else:
            a, b = piece(rng.randrange(60, 301)), piece(rng.randrange(60, 301))
            if k % 5 == 0:  # a mate contained in the other one, either strand
                n = rng.randrange(60, len(a)) if len(a) > 61 else len(a)
                q = rng.randrange(0, len(a) - n + 1)
                b = a[q:q + n] if k % 10 else rc(a[q:q + n])
        if k % 97 == 0:
            a = a[:10] + "N" + a[11:]
        if k % 101 == 0:
            b = b.lower()
        if k % 89 == 0 and raw:
            a, b = raw[-1], raw[-2]  # the previous pair in the other order
        raw += [a, b]
    first = n_pairs // 2 + 1
    return tuple(raw), (first, n_pairs - first), 40
