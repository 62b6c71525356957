"""The window scan's two run recorders against each other and the oracle.

Option run_masks = 1 (default) records a read's minimizer positions in a per-lane
bit set and emits its runs after the read (k_scan<..., MASKS>, for W <= 8 words
and w = l - k <= 32); run_masks = 0 stages every closed run in LDS.  Both must give
the same run records up to their order, so for every set here the rows, the
superReadIDs and the device's rows digest are equal between the two settings
and equal to the reference's, and counters()["scan_runs"] is equal between them.

m = k and J = n - l, so the read lengths below put n - m and J on the edges of
the 32-bit chunks and of pairs of them (1, 2, 63, 64, 65, 127, 128, 129 and the
width's maximum); n - m = 1, 2 would need n < l and cannot exist."""
import functools

import numpy as np
import pytest

import digest
from metagenomics_amd import synth
from metagenomics_amd.overlap import Dataset, rows_to_tuples
from refsets import engine_with, fixture_reference, from_oracle, super_dict
from test_gpu_parity import exchange_rows, gpu_rows

pytestmark = pytest.mark.gpu

SETTINGS = (0, 1)


def rows_digest_of(t):
    return digest.rows_digest(t[:, 0], t[:, 1], t[:, 2], t[:, 3])


def both(ref, k, nb_log2=0, opts=None, shards=((0, 1, 0, 0),), want_run_reruns=False):
    """Run the set with run_masks = 0 and 1 (a fresh engine each, one step per
    shard); rows of the shards are united.  Asserts everything the module's
    docstring lists and returns the two settings' counters."""
    ds, l, want, want_sup = ref
    out = {}
    for masks in SETTINGS:
        parts, runs, dig = [], [], []
        for shard in shards:
            e = engine_with(dict(opts or {}, run_masks=masks))
            try:
                rows, sup = gpu_rows(e, ds, l, k=k, nb_log2=nb_log2, shard=shard)
                c = e.counters()
                if len(shards) == 1:
                    dig.append(e.rows_digest())
            finally:
                e.close()
            assert super_dict(sup) == want_sup, (masks, shard)
            if want_run_reruns:
                assert c["run_reruns"] >= 1, c
            parts.append(rows)
            runs.append(c["scan_runs"])
        t = rows_to_tuples(np.concatenate(parts))
        assert np.array_equal(t, want), masks
        if dig:
            assert dig[0] == rows_digest_of(want), masks
        out[masks] = runs
    assert out[0] == out[1], out
    if want.shape[0]:
        assert sum(out[1]) > 0
    return out


def sampled(lengths, per_length, genome_len, seed):
    """per_length reads of each length at random offsets of one random genome, shuffled."""
    rng = np.random.default_rng(seed)
    g = "".join("ACGT"[c] for c in synth.random_genome(genome_len, seed))
    seqs = []
    for n in lengths:
        for _ in range(per_length):
            at = int(rng.integers(0, genome_len - n + 1))
            s = g[at:at + n]
            seqs.append(synth.revcomp_str(s) if rng.integers(0, 2) else s)
    rng.shuffle(seqs)
    return seqs


# ---- every template width, equal and mixed lengths.  (l, k): w <= 32 everywhere
WIDTHS = {1: (12, 6), 2: (40, 21), 3: (50, 31), 4: (50, 31), 5: (50, 31), 6: (64, 32), 7: (50, 31), 8: (50, 31)}


@functools.lru_cache(maxsize=None)
def width_ref(W, kind):
    l, k = WIDTHS[W]
    hi = 32 * W
    lo = hi if kind == "equal" else max(l + 1, hi - 33)
    c, L = synth.uniform_read_set(400, 0, max(2 * hi, 400 * hi // 17), seed=900 + W, lo=lo, hi=hi)
    ref = from_oracle(synth.codes_to_strings(c, L), l)
    assert ref[2].shape[0] > 0
    return ref


@pytest.mark.parametrize("kind", ["equal", "mixed"])
@pytest.mark.parametrize("W", sorted(WIDTHS))
def test_widths(W, kind):
    both(width_ref(W, kind), WIDTHS[W][1])


# ---- read counts: idle lanes, exactly full groups, group remainders
@functools.lru_cache(maxsize=None)
def count_pool():
    c, L = synth.uniform_read_set(300, 0, 400, seed=941, lo=60, hi=120)
    ds = Dataset.from_codes(c, L, 40)
    assert ds.num_unique >= 130
    return [ds.read(i) for i in range(1, 131)]


@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
def test_read_counts(N):
    both(from_oracle(count_pool()[:N], 40), 21)


# ---- n - m and J on the chunk edges
EDGE_L, EDGE_K = 40, 21
EDGE_LENGTHS = sorted({EDGE_L + j for j in (1, 2, 63, 64, 65, 127, 128, 129)} |
                      {EDGE_K + x for x in (63, 64, 65, 127, 128, 129)} | {255, 256})


def test_mixed_edge_lengths_in_one_wavefront():
    """Every edge length among 64 neighbours: lanes past their read beside lanes
    that go on (the length-ranked windows of the index scan, the plain scan)."""
    assert max(EDGE_LENGTHS) == 256
    both(from_oracle(sampled(EDGE_LENGTHS, 8, 700, 951), EDGE_L), EDGE_K)


@pytest.mark.parametrize("n", [EDGE_L + 1, EDGE_L + 64, EDGE_K + 128, 160, 256])
def test_equal_edge_lengths(n):
    """One length per set (one group per window, no length ranking); n = l + 1 has one window."""
    both(from_oracle(sampled([n], 150, 3 * n, 960 + n), EDGE_L), EDGE_K)


def test_homopolymers():
    """Every window's minimizer is its leftmost m-mer: J runs, the maximum count."""
    seqs = [b * n for b in "AC" for n in range(41, 161, 3)] + sampled([90, 150], 20, 300, 971)
    both(from_oracle(seqs, 40), 21)


def test_tandem_repeats():
    """Self rows."""
    both(fixture_reference("tandem"), 0)
    both(fixture_reference("tandem"), 8)


@pytest.mark.parametrize("l,k", [(30, 29), (33, 32), (72, 40 - 8), (60, 21)], ids=["w1", "w1-m32", "w40", "w39"])
def test_window_lengths(l, k):
    """w = 1 (every window its own run) and w > 32 (no mask path: both settings stage)."""
    both(from_oracle(sampled([l + 1, 100, 131, 160], 40, 500, 980 + l), l), k)


@pytest.mark.parametrize("name", ["mixed", "highdup"])
def test_tiny_directory(name):
    """2^10 buckets: long cell chains (the inserts' chained path)."""
    both(fixture_reference(name), 0, nb_log2=10)


@pytest.mark.parametrize("name", ["small", "mixed"])
def test_run_capacity_rerun(name):
    """run_cap = 8: the scan is cut and repeated with larger regions."""
    both(fixture_reference(name), 0, opts={"run_cap": 8}, want_run_reruns=True)


@pytest.mark.parametrize("which", ["small", "W5"])
def test_bucket_range_shards(which):
    """Both ranks of a two-way bucket split: the runs each keeps (the owned() filter
    in the emission) verify to a partition of the unsharded rows.  (Sets without
    containment: a bucket shard alone cannot mark contained reads.)"""
    ref, k = (fixture_reference("small"), 0) if which == "small" else (width_ref(5, "equal"), WIDTHS[5][1])
    assert not ref[3]
    both(ref, k, shards=((0, 2, 0, 0), (1, 2, 0, 0)))


@pytest.mark.parametrize("lds_scan", [0, 1], ids=["default", "xchg_scan_lds"])
@pytest.mark.parametrize("name", ["small", "mixed"])
def test_exchange_two_ranks(name, lds_scan):
    """sharded_step over LocalExchange at P = 2: the receiver scan and, with option
    xchg_scan_lds, the key-record scan, with their per-destination run counts."""
    ds, l, want, want_sup = fixture_reference(name)
    runs = {}
    for masks in SETTINGS:
        rows, sup = exchange_rows(ds, l, 2, opts={"run_masks": masks, "xchg_scan_lds": lds_scan})
        assert np.array_equal(rows_to_tuples(rows), want), masks
        assert super_dict(sup) == want_sup, masks
        runs[masks] = [c["scan_runs"] for c in exchange_rows.counters]
    assert runs[0] == runs[1], runs
