"""Hand-built inputs for the Dataset ingest's order, dedup and filter edges,
shared by tests/test_ingest_ref.py (host mirror, CPU) and
tests/test_ingest_edges.py (device).  Every set asserts from the plain
reference (ingest_ref) that it still exercises its edge, so a set that stops
doing so fails instead of passing vacuously."""
import functools
import random

import numpy as np

from ingest_ref import ref_dataset

L_EDGE = 20  # min_overlap of the hand-built sets
_COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
_CODE = np.full(256, 4, dtype=np.uint8)
for _ch, _v in zip(b"ACGTacgt", [0, 1, 2, 3, 0, 1, 2, 3]):
    _CODE[_ch] = _v


def rc(s: bytes) -> bytes:
    return s.translate(_COMPLEMENT)[::-1]


def rand_read(rng, n) -> bytes:
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def to_codes(records):
    """(codes [n, longest] uint8, lens [n] uint16) of byte records: A, C, G, T
    in either case are 0..3, every other byte and the padding 4."""
    stride = max((len(r) for r in records), default=1) or 1
    codes = np.full((len(records), stride), 4, dtype=np.uint8)
    lens = np.zeros(len(records), dtype=np.uint16)
    for i, r in enumerate(records):
        codes[i, : len(r)] = _CODE[np.frombuffer(r, dtype=np.uint8)]
        lens[i] = len(r)
    return codes, lens


def to_text(records):
    """(text, offsets uint64 [n + 1]): the records back to back."""
    off = np.zeros(len(records) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in records])
    return b"".join(records), off


def strands(rng, read, copies):
    """`copies` copies of a read, the strands alternating, in random order."""
    out = [read if (j + copies) % 2 else rc(read) for j in range(copies)]
    rng.shuffle(out)
    return out


class EdgeSet:
    """Raw records with their reference Dataset.  code_values: {(record, position):
    code} written over the codes source's matrix (bad code values other than 4)."""

    def __init__(self, records, l=L_EDGE, sources=("ascii", "codes"), code_values=None):
        self.records, self.l, self.sources = [bytes(r) for r in records], l, sources
        self.code_values = code_values or {}
        self.ref = ref_dataset(self.records, l)

    def codes(self):
        c, L = to_codes(self.records)
        for (i, p), v in self.code_values.items():
            assert c[i, p] == 4  # only over a symbol the reference drops the read for
            c[i, p] = v
        return c, L

    def text(self):
        return to_text(self.records)

    def ingest(self, engine, source):
        """Run the set through one of the device's two sources."""
        assert source in self.sources
        if source == "ascii":
            text, off = self.text()
            return engine.ingest_ascii(min_overlap=self.l, text=text, offsets=off)
        return engine.ingest_codes(*self.codes(), self.l)


# ---- order and dedup
def prefix_set(n):
    """R (n bases), R + A, R + 32 A, R + 33 A: A is code 0, so all four pack to
    the same zero-padded words wherever they end in the same word, and only the
    length separates them, in the sort and in the dedup."""
    rng = random.Random(4100 + n)
    # R starts with A and ends with C: R + A..A < its reverse complement T..T.., R < G..
    R = b"A" + rand_read(rng, n - 2) + b"C"
    four = [R, R + b"A", R + b"A" * 32, R + b"A" * 33]
    counts = [3, 5, 2, 4]
    for x in four:
        assert ref_dataset([x], L_EDGE) == (1, [x.decode()], [1]), "not its own canonical strand"
    records = [y for x, c in zip(four, counts) for y in strands(rng, x, c)]
    rng.shuffle(records)
    s = EdgeSet(records)
    assert s.ref == (sum(counts), [x.decode() for x in four], counts)  # four IDs in length order
    return s


def single_base_set(W):
    """A read of 32 W bases and its copies with one base changed, at the first
    and the last base of every word: each LSD pass decides an order, and a
    dedup that skips a word merges a pair."""
    rng = random.Random(4200 + W)
    X = b"A" + rand_read(rng, 32 * W - 2) + b"A"  # stays canonical (the other strand starts with T or G)
    variants = [X]
    for p in sorted({q for k in range(W) for q in (32 * k, 32 * k + 31)}):
        new = b"ACGT"[(b"ACGT".index(X[p]) + 1) % 4]
        variants.append(X[:p] + bytes([new]) + X[p + 1:])
    counts = [1 + i % 3 for i in range(len(variants))]
    records = [y for x, c in zip(variants, counts) for y in strands(rng, x, c)]
    rng.shuffle(records)
    s = EdgeSet(records)
    order = sorted(range(len(variants)), key=lambda i: variants[i])
    assert s.ref == (sum(counts), [variants[i].decode() for i in order], [counts[i] for i in order])
    return s


def palindrome_set():
    """Reads equal to their reverse complement, several copies each: one ID each."""
    rng = random.Random(4300)
    pal = []
    for half in (20, 32, 33, 64):
        h = rand_read(rng, half)
        pal.append(h + rc(h))
    counts = [3, 4, 5, 6]
    assert all(p == rc(p) for p in pal)
    records = [p for p, c in zip(pal, counts) for _ in range(c)]
    rng.shuffle(records)
    s = EdgeSet(records)
    order = sorted(range(4), key=lambda i: pal[i])
    assert s.ref == (sum(counts), [pal[i].decode() for i in order], [counts[i] for i in order])
    return s


COUNTS = [1, 2, 255, 256, 257, 1025]


def count_set(N):
    """N unique reads, repeated so that a run of equal reads lies across a
    multiple of 256 in sorted order (the 256-thread kernels' block edge in the
    dedup flags, the scan and the frequencies)."""
    from test_width_edges import COUNT_L, count_pool

    pool = [p.encode() for p in count_pool()[:N]]
    rng = random.Random(4400 + N)
    counts = [300 if N <= 2 else 1 + (7 * i) % 5 for i in range(N)]
    records = [y for x, c in zip(pool, counts) for y in strands(rng, x, c)]
    rng.shuffle(records)
    s = EdgeSet(records, COUNT_L)
    assert s.ref == (sum(counts), [p.decode() for p in pool], counts)
    first = np.concatenate([[0], np.cumsum(s.ref[2])])  # run u: sorted positions [first[u], first[u + 1])
    assert np.any(first[:-1] // 256 != (first[1:] - 1) // 256), "no run of equal reads across a block edge"
    return s


def nothing_valid_set():
    """Records of which none passes the filter."""
    rng = random.Random(4500)
    good = rand_read(rng, 60)
    s = EdgeSet([good[:L_EDGE], b"", good[:30] + b"N" + good[31:], b"A" * 55 + good[:5], b"acgt"])
    assert s.ref == (0, [], [])
    return s


# ---- filter
MAJORITY_LENGTHS = (41, 45, 50, 64, 99)


def majority_read(L, b, count):
    """L bases of which exactly `count` are b (one block in the middle), the
    rest cycling through the other three."""
    others = [x for x in b"ACGT" if x != b]
    fill = bytes(others[i % 3] for i in range(L - count))
    at = len(fill) // 2
    r = fill[:at] + bytes([b]) * count + fill[at:]
    assert len(r) == L and r.count(bytes([b])) == count
    return r


def majority_set():
    """The 80 % rule at its boundary for every base, and the length bound:
    count int(.8 L) - 1 is kept, int(.8 L) dropped; length l dropped, l + 1 kept."""
    rng = random.Random(4600)
    kept, dropped = [], []
    for L in MAJORITY_LENGTHS:
        thr = int(L * .8)
        for b in b"ACGT":
            kept.append(majority_read(L, b, thr - 1))
            dropped.append(majority_read(L, b, thr))
    kept.append(rand_read(rng, L_EDGE + 1))
    dropped.append(rand_read(rng, L_EDGE))
    for r in kept:
        assert ref_dataset([r], L_EDGE)[0] == 1, r
    for r in dropped:
        assert ref_dataset([r], L_EDGE)[0] == 0, r
    records = kept + dropped + [rc(r) for r in kept + dropped]
    rng.shuffle(records)
    s = EdgeSet(records)
    assert s.ref[0] == 2 * len(kept)
    return s


BAD_POSITIONS = (0, 31, 32, 69)
BAD_CODES = (4, 5, 255)
BAD_BYTES = (b"N", b"n", b"!", b"[", b"{", b"@", b"\x01", b"\x14", b"\xc1", b"\xe1")


def _bad_symbol_records(symbols):
    rng = random.Random(4700)
    base = rand_read(rng, 70)
    records, where = [base], []
    for p in BAD_POSITIONS:
        for sym in symbols:
            where.append((len(records), p))
            records.append(base[:p] + sym + base[p + 1:])
    return base, records, where


def bad_code_set():
    """One bad code value in an otherwise valid 70-base read (codes source)."""
    symbols = [b"N"] * len(BAD_CODES)
    base, records, where = _bad_symbol_records(symbols)
    values = {w: BAD_CODES[j % len(BAD_CODES)] for j, w in enumerate(where)}
    s = EdgeSet(records, sources=("codes",), code_values=values)
    assert s.ref[0] == 1 and s.ref[2] == [1]  # the clean read alone
    return s


def bad_byte_set():
    """One bad byte in an otherwise valid 70-base read (ASCII source): bytes
    that clearing bit 5 maps onto or near a base letter must stay invalid."""
    base, records, where = _bad_symbol_records(BAD_BYTES)
    s = EdgeSet(records, sources=("ascii",))
    assert s.ref[0] == 1 and s.ref[2] == [1]
    return s


def lowercase_set():
    """Lower-case and mixed-case reads are kept and are duplicates of their
    upper-case twins (ASCII source)."""
    rng = random.Random(4800)
    records, reads = [], [rand_read(rng, n) for n in (21, 32, 33, 64, 70)]
    for r in reads:
        mixed = bytes(c | 0x20 if rng.random() < .5 else c for c in r)
        records += [r, r.lower(), mixed, rc(r).lower()]
    rng.shuffle(records)
    s = EdgeSet(records, sources=("ascii",))
    assert s.ref[0] == 4 * len(reads) and s.ref[2] == [4] * len(reads)
    return s


EDGE_SETS = {
    "prefix63": lambda: prefix_set(63), "prefix64": lambda: prefix_set(64), "prefix65": lambda: prefix_set(65),
    "single_base_w2": lambda: single_base_set(2), "single_base_w5": lambda: single_base_set(5),
    "palindromes": palindrome_set,
    **{f"count{N}": functools.partial(count_set, N) for N in COUNTS},
    "nothing_valid": nothing_valid_set,
    "majority": majority_set, "bad_codes": bad_code_set, "bad_bytes": bad_byte_set, "lowercase": lowercase_set,
}


@functools.lru_cache(maxsize=None)
def edge_set(name) -> EdgeSet:
    return EDGE_SETS[name]()


# every (set, source) the set is meant for
EDGE_CASES = [(name, src) for name in EDGE_SETS for src in ("ascii", "codes")
              if not (name in ("bad_bytes", "lowercase") and src == "codes")
              and not (name == "bad_codes" and src == "ascii")]
