"""Read sets with exact list lengths for the device's discovery lists
(mg_build_discoveries, metagenomics_amd/csrc/device/mg_disc.hip), shared by
tests/test_disc_edges_host.py (host mirror, CPU) and tests/test_disc_edges.py
(device).  Every set carries its Dataset, the C oracle's rows and the expected
arrays (tests/disc_ref.py, tests/comp_ref.py), computed once and read-only.

Two building blocks:

  clique   all m windows of length L, step 1, of a random genome of L + m - 1
           bases, L - l >= m - 1: m reads of degree exactly m - 1 (m = 1: an
           isolated read with an empty list).  Read IDs follow string order, so
           the cliques of different genomes interleave at random along the ID
           axis: that mixes degrees inside the 32 reads of one wavefront.
  tandem   one read that repeats a random unit of u bases: 4 * ((L - l) // u)
           rows before the second copy of every self row is dropped, all of
           them self rows.  Several phases of one unit give lists that mix self
           and other records.

wave_runs restates k_disc_wave's packing rule (not its sort), so that the host
file can assert that a set reaches the runs it was made for."""
import collections
import functools
import time

import numpy as np

from comp_ref import components_from_rows
from disc_ref import numpy_lists
from metagenomics_amd import synth
from metagenomics_amd.overlap import Dataset
from oracle import OracleDataset, sorted_tuples

SEED = 46  # (chosen so that ladder_low holds a list with self rows between two others of one run)
WAVE, WAVE_READS = 64, 32  # lanes, and consecutive reads, of one wavefront of k_disc_wave

LOW_L, LOW_l = 100, 35
LOW_SIZES = range(1, 67)  # clique sizes: degrees 0 .. 65
LOW_UNITS = {2: 128, 3: 84, 4: 64, 5: 52, 7: 36, 16: 16}  # unit length: rows of the all-self read
PHASES, PHASE_UNIT, PHASE_ROWS, PHASE_SELF = 4, 13, 50, 20

BLOCK_L, BLOCK_l = 600, 40
BLOCK_DEGREES = (65, 66, 127, 128, 129, 255, 256, 257, 511, 512, 513)
BLOCK_MORE = {65: 10, 66: 10}  # further cliques of these degrees
BLOCK_UNITS = {2: 1120, 3: 744, 5: 448, 8: 280, 17: 128, 18: 124, 32: 68, 33: 64, 35: 64}
ACGT_ROWS = 1120  # ACGT is its own reverse complement: self rows in every orientation

COUNTS = (31, 32, 33, 63, 64, 65)

_COMPLEMENT = str.maketrans("ACGT", "TGCA")


def low_copies(m):
    return max(3, 200 // m)


def rc(s):
    return s.translate(_COMPLEMENT)[::-1]


def genome(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def clique(rng, m, L):
    g = genome(rng, L + m - 1)
    return [g[i:i + L] for i in range(m)]


def unit(rng, u):
    """A random unit that is no repeat of a shorter one, of which no rotation is
    its own reverse complement, and no base of which fills 80 % of a read."""
    while True:
        s = genome(rng, u)
        rot = {s[i:] + s[:i] for i in range(u)}
        if len(rot) == u and rc(s) not in rot and max(s.count(b) for b in "ACGT") <= 0.6 * u:
            return s


def tandem(s, L, phase=0):
    return (s * (L // len(s) + 2))[phase:phase + L]


Run = collections.namedtuple("Run", "first total lists nonempty at_end cut")


def wave_runs(deg):
    """k_disc_wave's packing rule over list lengths deg[0 .. N) of the reads 1 .. N
    (both copies of a self row counted: the lengths it packs).  Per block of 32
    consecutive IDs: a list of 0 or more than 64 records is skipped, otherwise the
    longest run of consecutive lists that totals at most 64 is taken.  One Run
    per run: the ID of its first read, its total, the number of lists and of
    non-empty lists in it, whether it reached the block's end, and the length
    of the list that cut it (None at the block's end)."""
    deg = [int(d) for d in deg]
    runs = []
    for b0 in range(0, len(deg), WAVE_READS):
        blk = deg[b0:b0 + WAVE_READS]
        cur = 0
        while cur < len(blk):
            if blk[cur] == 0 or blk[cur] > WAVE:
                cur += 1
                continue
            k, total = cur, 0
            while k < len(blk) and total + blk[k] <= WAVE:
                total += blk[k]
                k += 1
            runs.append(Run(b0 + cur + 1, total, k - cur, sum(1 for d in blk[cur:k] if d), k == len(blk),
                            blk[k] if k < len(blk) else None))
            cur = k
    return runs


def run_of(runs, a):
    """The run read a lies in, and its position there."""
    for r in runs:
        if r.first <= a < r.first + r.lists:
            return r, a - r.first
    return None, None


class DiscSet:
    """Reads with the oracle's rows and the expected lists and components."""

    def __init__(self, l, seqs=None, codes=None, k=0, marks=None):
        self.l, self.k = l, k
        if seqs is not None:
            self.ds = Dataset.from_strings(seqs, l)
            od = OracleDataset.from_strings(seqs, l)
        else:
            self.ds = Dataset.from_codes(*codes, l)
            od = OracleDataset.from_codes(*codes, l)
        self.n = self.ds.num_unique
        assert od.num_unique == self.n
        t0 = time.perf_counter()
        rows = od.overlaps(l)[0]
        self.oracle_s = time.perf_counter() - t0
        self.rows = sorted_tuples(rows)
        self.lens = self.ds.packed()[1].copy()
        self.start, self.disc, self.n_self = numpy_lists(self.rows, self.lens, l)
        self.comps = components_from_rows(self.rows, self.n)
        # list lengths as the sort sees them (a self row twice), reads 1 .. N
        self.raw = np.bincount(self.rows[:, 0], minlength=self.n + 1)[1:]
        self.self_raw = np.bincount(self.rows[self.rows[:, 0] == self.rows[:, 1], 0], minlength=self.n + 1)[1:]
        for a in (self.rows, self.lens, self.start, self.disc, self.raw, self.self_raw, *self.comps):
            a.setflags(write=False)
        # marks: {name: read ID} of the planted reads
        self.marks = {}
        for name, s in (marks or {}).items():
            self.marks[name] = self.ds.find(s) or self.ds.find(rc(s))
            assert 1 <= self.marks[name] <= self.n, name
        assert len(set(self.marks.values())) == len(self.marks)

    def clique_raw(self):
        """The list lengths of the reads that are no planted tandem read."""
        keep = np.ones(self.n, dtype=bool)
        keep[np.array(list(self.marks.values()), dtype=np.int64) - 1] = False
        return self.raw[keep]


def _ladder_low():
    rng = np.random.default_rng(SEED)
    seqs = [r for m in LOW_SIZES for _ in range(low_copies(m)) for r in clique(rng, m, LOW_L)]
    assert len(seqs) == 12316
    marks = {"u%d" % u: tandem(unit(rng, u), LOW_L) for u in LOW_UNITS}
    s13 = unit(rng, PHASE_UNIT)
    marks.update({"phase%d" % p: tandem(s13, LOW_L, p) for p in range(PHASES)})
    s = DiscSet(LOW_l, seqs + list(marks.values()), marks=marks)
    assert s.n == len(seqs) + len(marks)
    return s


def _ladder_flat():
    rng = np.random.default_rng(SEED + 1)
    seqs = [r for m in (1, 2, 3) for _ in range(300) for r in clique(rng, m, LOW_L)]
    s = DiscSet(LOW_l, seqs)
    assert (s.n, s.rows.shape[0]) == (1800, 2400)
    return s


def _ladder_block():
    rng = np.random.default_rng(SEED + 2)
    degrees = list(BLOCK_DEGREES) + [d for d, c in BLOCK_MORE.items() for _ in range(c)]
    seqs = [r for d in degrees for r in clique(rng, d + 1, BLOCK_L)]
    assert len(seqs) == 4160
    marks = {"u%d" % u: tandem(unit(rng, u), BLOCK_L) for u in BLOCK_UNITS}
    marks["acgt"] = tandem("ACGT", BLOCK_L)
    s = DiscSet(BLOCK_l, seqs + list(marks.values()), marks=marks)
    assert s.n == len(seqs) + len(marks)
    return s


def _mixed_small():
    return DiscSet(50, codes=synth.metagenome_read_set(5000, 100, 250, n_genomes=8, total_len=100000, seed=SEED + 3))


def _count(N):
    from test_width_edges import COUNT_K, COUNT_L, count_pool

    s = DiscSet(COUNT_L, count_pool()[:N], k=COUNT_K)
    assert s.n == N
    return s


SETS = {"ladder_low": _ladder_low, "ladder_flat": _ladder_flat, "ladder_block": _ladder_block,
        "mixed_small": _mixed_small, **{"count%d" % N: functools.partial(_count, N) for N in COUNTS}}


@functools.lru_cache(maxsize=None)
def disc_set(name) -> DiscSet:
    return SETS[name]()


@functools.lru_cache(maxsize=None)
def runs_of(name):
    return tuple(wave_runs(disc_set(name).raw))
