"""The sets of tests/disc_sets.py without a GPU: what each set was made for,
asserted from its expected arrays (conditions, not measurements), and the
expected arrays themselves pinned a second, independent way by the host
mirrors: mg::Discoveries::build and the checker of mg::Discoveries::from_lists
against numpy (tests/disc_ref.py), mg::Components::build against numpy
(tests/comp_ref.py).  The device test (tests/test_disc_edges.py) compares with
the same arrays."""
import collections

import numpy as np
import pytest

import disc_sets as S
from disc_ref import to_edges
from metagenomics_amd.overlap import check_discoveries, host_components, host_discoveries


def degrees(s):
    return np.diff(s.start.astype(np.int64))[1:]


# ---- the packing rule's restatement, on hand-made lengths
def test_wave_runs_by_hand():
    R = S.Run
    assert S.wave_runs([]) == []
    assert S.wave_runs([0, 65, 0]) == []
    assert S.wave_runs([64]) == [R(1, 64, 1, 1, True, None)]
    assert S.wave_runs([30, 34, 1]) == [R(1, 64, 2, 2, False, 1), R(3, 1, 1, 1, True, None)]
    assert S.wave_runs([60, 0, 4, 0, 1]) == [R(1, 64, 4, 2, False, 1), R(5, 1, 1, 1, True, None)]
    assert S.wave_runs([0, 3, 70, 2]) == [R(2, 3, 1, 1, False, 70), R(4, 2, 1, 1, True, None)]
    # the 33rd read starts another wavefront, whatever is left of the 64 lanes
    assert S.wave_runs([1] * 33) == [R(1, 32, 32, 32, True, None), R(33, 1, 1, 1, True, None)]
    assert S.wave_runs([2] * 32 + [0, 5]) == [R(1, 64, 32, 32, True, None), R(34, 5, 1, 1, True, None)]


# ---- preconditions
def test_ladder_low_reaches_every_packing_case():
    s, runs = S.disc_set("ladder_low"), S.runs_of("ladder_low")
    assert s.n % S.WAVE_READS != 0
    assert set(degrees(s).tolist()) >= set(range(66))
    # the planted all-self reads: both copies of every row, and nothing else
    for u, raw in S.LOW_UNITS.items():
        a = s.marks["u%d" % u]
        assert (int(s.raw[a - 1]), int(s.self_raw[a - 1]), int(degrees(s)[a - 1])) == (raw, raw, raw // 2), u
    for p in range(S.PHASES):
        a = s.marks["phase%d" % p]
        assert (int(s.raw[a - 1]), int(s.self_raw[a - 1])) == (S.PHASE_ROWS, S.PHASE_SELF), p
    assert s.n_self == sum(S.LOW_UNITS.values()) + S.PHASES * S.PHASE_SELF
    # every other read is a clique's: degree d copies(d + 1) x (d + 1) times
    count = collections.Counter(s.clique_raw().tolist())
    assert count == {m - 1: S.low_copies(m) * m for m in S.LOW_SIZES}
    assert s.rows.shape[0] - s.n_self - S.PHASES * (S.PHASE_ROWS - S.PHASE_SELF) == 391592

    assert sum(1 for r in runs if r.total == S.WAVE and r.nonempty >= 2) >= 50
    assert sum(1 for r in runs if r.total == S.WAVE and r.nonempty == 1) >= 50
    assert sum(1 for r in runs if r.nonempty >= 2 and r.cut is not None and r.total + r.cut == S.WAVE + 1) >= 20
    assert sum(1 for r in runs if r.cut is not None and r.cut > S.WAVE) >= 50
    assert sum(1 for r in runs if r.lists > r.nonempty) >= 50
    assert sum(1 for r in runs if r.at_end) >= 100
    # a list with self rows inside a run, and one whose last pair lies at lanes 62 and 63
    inside = 0
    for name, a in s.marks.items():
        if s.raw[a - 1] <= S.WAVE:
            r, at = S.run_of(runs, a)
            assert r is not None, name
            inside += 0 < at < r.lists - 1
    assert inside >= 1
    r, at = S.run_of(runs, s.marks["u4"])
    assert (r.total, r.nonempty) == (S.WAVE, 1)


def test_ladder_flat_fills_wavefronts_with_lists():
    s, runs = S.disc_set("ladder_flat"), S.runs_of("ladder_flat")
    assert s.n % S.WAVE_READS != 0
    assert collections.Counter(degrees(s).tolist()) == {0: 300, 1: 600, 2: 900} and s.n_self == 0
    assert sum(1 for r in runs if r.lists >= 31) >= 10
    assert any(r.lists == S.WAVE_READS for r in runs)  # lane 32's start is the run's end


def test_ladder_block_degrees_and_strides():
    s = S.disc_set("ladder_block")
    count = collections.Counter(s.clique_raw().tolist())
    assert count == {d: (1 + S.BLOCK_MORE.get(d, 0)) * (d + 1) for d in S.BLOCK_DEGREES}
    assert int((s.raw > S.WAVE).sum()) > 4096  # two full strides of 8 x 256 workgroups
    for name, raw in [("u%d" % u, r) for u, r in S.BLOCK_UNITS.items()] + [("acgt", S.ACGT_ROWS)]:
        a = s.marks[name]
        assert (int(s.raw[a - 1]), int(s.self_raw[a - 1]), int(degrees(s)[a - 1])) == (raw, raw, raw // 2), name
    assert s.n_self == sum(S.BLOCK_UNITS.values()) + S.ACGT_ROWS
    assert s.rows.shape[0] - s.n_self == 1130718
    # at every block capacity of the device test an all-self list on either side of it
    # (the wavefront path below the capacity 64, nothing above the default 2,048)
    planted = [int(s.raw[a - 1]) for a in s.marks.values()]
    for cap in (64, 100, 128, 512):
        assert any((r <= cap if cap == S.WAVE else S.WAVE < r <= cap) for r in planted), cap
        assert any(r > cap for r in planted), cap
    assert any(S.WAVE < r <= 2048 for r in planted)


def test_mixed_small_has_mixed_lengths_and_empty_lists():
    s = S.disc_set("mixed_small")
    assert len(set(s.lens.tolist())) > 100 and (int(s.lens.min()), int(s.lens.max())) == (100, 250)
    d = degrees(s)
    assert int((d == 0).sum()) > 0 and int(np.flatnonzero(d == 0)[0]) + 1 < s.n
    odd = (s.disc["o"] & 1) == 1  # the keys whose window j comes from the source's own length
    assert int(odd.sum()) > 0 and s.n <= 5000


@pytest.mark.parametrize("N", S.COUNTS)
def test_count_sets(N):
    s = S.disc_set("count%d" % N)
    assert s.n == N and s.start.shape[0] == N + 2
    assert int(s.start[N]) <= int(s.start[N + 1]) == s.disc.shape[0]


# ---- the host mirrors on the same sets
@pytest.mark.parametrize("name", list(S.SETS))
def test_host_mirrors_agree_with_numpy(name):
    s = S.disc_set(name)
    rows = to_edges(s.rows)
    start, disc = host_discoveries(rows[np.random.default_rng(1).permutation(rows.shape[0])], s.lens, s.l)
    assert np.array_equal(start, s.start)
    assert disc.shape == s.disc.shape and np.array_equal(disc, s.disc)
    assert disc.shape[0] == s.rows.shape[0] - s.n_self // 2
    assert check_discoveries(s.start, s.disc, s.lens, s.l) == 0
    label, comps = host_components(s.start, s.disc)
    assert np.array_equal(label, s.comps[0])
    assert comps.shape == s.comps[1].shape and np.array_equal(comps, s.comps[1])
