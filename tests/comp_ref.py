"""An independent numpy restatement of the connected components of the
discovery lists, for tests/test_components*.py.  Two reads are connected when a
record joins them.  Every read starts with its own ID as label and repeatedly
takes the minimum label among itself and its partners, hands that minimum to
the read its own label names (a read of the same component) and follows labels
of labels, until nothing changes: every label is then equal across every record
and names a read of the component no greater than any member, which is the
smallest read ID of the component.  The table is np.unique / bincount
over the reads that have records.  It calls neither the host union-find
(mg::Components::build) nor the device."""
import numpy as np

from metagenomics_amd.overlap import COMP_DTYPE


def _labels(n_reads: int, src: np.ndarray, dst: np.ndarray) -> np.ndarray:
    label = np.arange(n_reads + 1, dtype=np.int64)
    # every pair in both directions, grouped by the read that takes the minimum
    to = np.concatenate([src, dst])
    other = np.concatenate([dst, src])
    order = np.argsort(to, kind="stable")
    to, other = to[order], other[order]
    if to.size == 0:
        return label
    firsts = np.flatnonzero(np.r_[True, to[1:] != to[:-1]])
    reads = to[firsts]
    while True:
        low = np.minimum.reduceat(label[other], firsts)  # per read: the smallest label among its partners
        new = label.copy()
        np.minimum.at(new, label[reads], low)  # the read's label (a read of its component) takes it too
        new[reads] = np.minimum(new[reads], low)
        while True:  # every label to the label of its label
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, label):
            return label
        label = new


def _table(n_reads: int, label: np.ndarray, src: np.ndarray, dst: np.ndarray):
    """src / dst: one entry per list record (a self record once)."""
    deg = np.bincount(src, minlength=n_reads + 1)
    has = np.flatnonzero(deg > 0)
    roots = np.unique(label[has])
    n_reads_of = np.bincount(label[has], minlength=n_reads + 1)
    n_disc_of = np.bincount(label[src], minlength=n_reads + 1)
    n_self_of = np.bincount(label[src[src == dst]], minlength=n_reads + 1)
    comps = np.zeros(roots.shape[0], dtype=COMP_DTYPE)
    comps["root"], comps["n_reads"] = roots, n_reads_of[roots]
    comps["n_disc"], comps["n_self"] = n_disc_of[roots], n_self_of[roots]
    return label.astype(np.uint32), comps


def components_from_lists(start: np.ndarray, disc: np.ndarray):
    """(label uint32[n_reads + 1], comps COMP_DTYPE) of the lists D(A) = disc[start[A]:start[A + 1]]."""
    n_reads = start.shape[0] - 2
    src = np.repeat(np.arange(n_reads + 1, dtype=np.int64), np.diff(start.astype(np.int64)))
    dst = disc["dst"].astype(np.int64)
    return _table(n_reads, _labels(n_reads, src, dst), src, dst)


def components_from_rows(rows: np.ndarray, n_reads: int):
    """The same from rows int64 [n, 4] (src, dst, orient, offset); a self row comes twice and counts once."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    order = np.lexsort((rows[:, 3], rows[:, 2], rows[:, 1], rows[:, 0]))
    rows = rows[order]
    self_idx = np.flatnonzero(rows[:, 0] == rows[:, 1])
    assert self_idx.size % 2 == 0 and np.array_equal(rows[self_idx[0::2]], rows[self_idx[1::2]])
    keep = np.ones(rows.shape[0], dtype=bool)
    keep[self_idx[1::2]] = False
    src, dst = rows[keep, 0], rows[keep, 1]
    return _table(n_reads, _labels(n_reads, src, dst), src, dst)
