"""An independent numpy restatement of the per-read discovery lists D(A), for
tests/test_discoveries*.py: from rows (src, dst, orient, offset) map orient to
the key o, compute the window j from the read lengths, lexsort by (src, j, dst,
o), drop every second copy of a self row and bincount into start.  It calls
neither mg::Discoveries::build nor the device grouping."""
import gzip
import os

import numpy as np

from conftest import GOLDEN, load_meta
from metagenomics_amd.overlap import DISC_DTYPE, EDGE_DTYPE

KEY_OF_ORIENT = np.array([1, 3, 2, 0], dtype=np.int64)  # orient 3 -> 0, 0 -> 1, 2 -> 2, 1 -> 3


def numpy_lists(rows: np.ndarray, lens: np.ndarray, l: int):
    """rows: int64 [n, 4] (src, dst, orient, offset), any order.  Returns
    (start uint64[N + 2], disc DISC_DTYPE, number of self rows)."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    n_reads, h = int(len(lens)), l - 1
    src, dst, orient, off = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    o = KEY_OF_ORIENT[orient]
    n1 = np.asarray(lens, dtype=np.int64)[src - 1]
    j = np.where((o == 0) | (o == 2), off, n1 - h - off)
    assert ((j >= 1) & (j < n1 - h)).all()
    order = np.lexsort((o, dst, j, src))
    src, dst, orient, off, o, j = (x[order] for x in (src, dst, orient, off, o, j))
    self_idx = np.flatnonzero(src == dst)
    assert self_idx.size % 2 == 0
    first, second = self_idx[0::2], self_idx[1::2]
    assert np.array_equal(second, first + 1)  # the two copies are identical, hence adjacent
    for x in (src, dst, o, j):
        assert np.array_equal(x[first], x[second])
    keep = np.ones(src.shape[0], dtype=bool)
    keep[second] = False
    disc = np.zeros(int(keep.sum()), dtype=DISC_DTYPE)
    disc["dst"], disc["offset"], disc["orient"], disc["o"] = dst[keep], off[keep], orient[keep], o[keep]
    counts = np.bincount(src[keep], minlength=n_reads + 2)
    start = np.zeros(n_reads + 2, dtype=np.uint64)
    start[1:] = np.cumsum(counts[: n_reads + 1])
    return start, disc, int(self_idx.size)


def to_edges(t: np.ndarray) -> np.ndarray:
    r = np.zeros(t.shape[0], dtype=EDGE_DTYPE)
    r["src"], r["dst"], r["orient"], r["offset"] = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
    return r


def tuples(rows: np.ndarray) -> np.ndarray:
    return np.stack([rows["src"], rows["dst"], rows["orient"], rows["offset"]], axis=1).astype(np.int64)


def golden_bfs(name):
    meta = load_meta(name)
    with gzip.open(os.path.join(GOLDEN, meta["bfs"]["file"]), "rt") as f:
        txt = f.read().split()
    return np.array(txt, dtype=np.int64).reshape(-1, 4) if txt else np.zeros((0, 4), np.int64)


def golden_text(name, key):
    meta = load_meta(name)
    with gzip.open(os.path.join(GOLDEN, meta["unitig"][key]), "rt") as f:
        return f.read()
