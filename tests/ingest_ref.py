"""A plain reference for the Dataset ingest, and the comparison of an engine
with it.  No project code in here: the reference restates Dataset.cpp:158-167
(upper-case, testRead, canonical strand), :398-413 (testRead) and :316-345
(sort, dedup, frequencies, IDs 1..N) in Python, to be checked by eye.

tests/test_ingest_ref.py pins it to the host mirror (which test_host_dataset.py
pins to the reference's ID map); tests/test_ingest_edges.py compares the device
ingest with it."""
from collections import Counter

import numpy as np

_COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")
# the word counts the kernels are instantiated for (mg_ctx.hpp, supported_maxw)
WIDTHS = (1, 2, 3, 4, 5, 6, 8, 12, 16, 32)


def _record_bytes(r) -> bytes:
    return r.encode("latin-1") if isinstance(r, str) else bytes(r)


def canonical(s: bytes) -> bytes:
    """The strand the Dataset stores (Dataset.cpp:163-167)."""
    rc = s.translate(_COMPLEMENT)[::-1]
    return s if s < rc else rc


def passes_filter(s: bytes, l: int) -> bool:
    """Dataset.cpp:160 and testRead (:398-413) on an upper-cased record."""
    if not l < len(s) <= 65535:  # Read::getReadLength is UINT16
        return False
    if any(c not in b"ACGT" for c in s):
        return False
    return max(s.count(b) for b in b"ACGT") < int(len(s) * .8)


def ref_dataset(raw, l):
    """(n_good, [unique canonical strings in ID order], [frequencies]) of raw
    records given as str or bytes.  Python's order on ASCII strings is
    std::string's: first differing byte, a proper prefix first."""
    good = Counter()
    for r in raw:
        s = _record_bytes(r).upper()  # bytes.upper: ASCII letters only (toupper in the C locale)
        if passes_filter(s, l):
            good[canonical(s).decode("ascii")] += 1
    seqs = sorted(good)
    return sum(good.values()), seqs, [good[s] for s in seqs]


def pack(strings, wpr) -> np.ndarray:
    """uint64 [N, wpr]: 2 bits per base (A, C, G, T = 0..3), the first base in
    the top bits of word 0, zero padded."""
    codes = np.zeros((len(strings), 32 * wpr), dtype=np.uint64)
    lut = np.zeros(256, dtype=np.uint64)
    for ch, v in zip(b"ACGT", range(4)):
        lut[ch] = v
    for i, s in enumerate(strings):
        assert len(s) <= 32 * wpr
        codes[i, : len(s)] = lut[np.frombuffer(s.encode("ascii"), dtype=np.uint8)]
    shifts = np.arange(62, -2, -2).astype(np.uint64)
    return (codes.reshape(len(strings), wpr, 32) << shifts).sum(axis=2, dtype=np.uint64)


def slot_maxw(need: int) -> int:
    """Words per downloaded read for a longest kept read of `need` words: the
    next instantiated width up to 32, the exact count beyond (long reads)."""
    need = max(1, need)
    return need if need > 32 else next(w for w in WIDTHS if w >= need)


def assert_ingested(engine, n_good, seqs, freqs):
    """The engine holds exactly the reference's Dataset after an ingest."""
    assert engine.n_reads == len(seqs)
    assert engine.dataset_counts() == (n_good, len(seqs))
    words, lens = engine.download_packed()
    assert np.array_equal(lens, np.array([len(s) for s in seqs], dtype=np.uint16))
    if seqs:
        assert np.array_equal(engine.frequency(), np.array(freqs, dtype=np.uint32))
    wpr = slot_maxw((max((len(s) for s in seqs), default=0) + 31) // 32)  # the longest *kept* read
    assert words.shape == (len(seqs), wpr)
    assert np.array_equal(words, pack(seqs, wpr))
