"""The persistent probe's region walk, its virtual region split, and the
options that results must not depend on.  Bit-exact against the reference's
goldens or the oracle.

Region walk: a probe wavefront that owns several run regions moves on with
reg_of(rg + 1) / open_region(++rg) and prefetches across the switch.  On small
sets the probe grid covers the scan's regions one to one; option max_blocks
caps the grid.  Set before the build it caps scan and probe alike: the block's
four wavefronts then share four regions (probe_share) or, on mixed lengths,
walk the four window groups of each scan wavefront.  Set after the build it
caps the probe alone, so every probe wavefront walks several of the uncapped
scan's regions whatever the sharing.

Virtual split (LaunchProbe::run): with R run regions and nwp probe wavefronts,
R < 4 nwp, the host takes the smallest k <= min(probe_split_max, run_cap / 4096)
that minimises ceil(R k / nwp) nwp / (R k); each region is then walked as k
parts of per = ceil(ceil(c / k) / st) st records (st = 64, or 256 with
probe_share).  R = (scan blocks) x (scan wavefronts per block: 4, or 2 once
w = l - k needs more than 40 KB of LDS per wavefront, w >= 154) x (4 window
groups on mixed lengths); scan blocks = min(ceil(ceil(n / 64) / wavefronts per
block), max_blocks), probe blocks = min(ceil(ceil(n / 64) / 4), max_blocks).
The cases below work R, nwp and k out from that; counters().probe_vsplit
says whether the launch took the split."""
import functools

import numpy as np
import pytest

from metagenomics_amd import synth
from metagenomics_amd.overlap import OverlapEngine, rows_to_tuples
from refsets import first_unique_reads, fixture_reference, from_oracle, super_dict
from test_gpu_parity import check_pairs, exchange_rows, gpu_rows, prefix_reads

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def reference(name):
    """(Dataset, l, rows as sorted tuples, {id: superReadID}), computed once."""
    if name == "prefixes":
        return from_oracle(prefix_reads(), 40)
    if name == "metagenome":
        c, L = synth.metagenome_read_set(20000, 100, 250, n_genomes=20, total_len=400000, seed=51)
        return from_oracle(synth.codes_to_strings(c, L), 50)
    if name == "wide_window_mixed":
        # 560 unique reads (9 scan groups) of 300-500 bp at l = 200, k = 31: w = 169, two scan
        # wavefronts per block; the first 560 reads in ID order of a 25x set of one genome
        c, L = synth.uniform_read_set(700, 0, 11000, seed=741, lo=300, hi=500)
        ref = from_oracle(first_unique_reads(c, L, 200, 560), 200)
        assert ref[0].num_unique == 560 and ref[2].shape[0] > 0 and ref[3]
        return ref
    if name == "wide_window_short":
        # 300 unique reads (5 scan groups) of 232 bp at l = 200, k = 31: w = 169 again, and only
        # 232 - 199 - 1 = 32 windows per read, so a read leaves one or two runs
        c, L = synth.uniform_read_set(600, 232, 900, seed=743)
        ref = from_oracle(first_unique_reads(c, L, 200, 300), 200)
        assert ref[0].num_unique == 300 and ref[2].shape[0] > 0 and not ref[3]
        return ref
    return fixture_reference(name)


def step(e, ds, l, k=0, probe_opts=None, shard=(0, 1, 0, 0)):
    """One fused step; probe_opts are set after the build (they reach the probe alone)."""
    e.set_shard(*shard)
    e.upload(ds)
    e.build_index(l, k)
    sup = e.mark_contained()
    for kk, v in (probe_opts or {}).items():
        e.set_option(kk, v)
    n = e.find_overlaps()
    rows = e.rows(n)
    assert rows.shape[0] == n
    return rows, sup


@pytest.mark.parametrize("share,compact", [(1, 1), (0, 1), (1, 0)])
@pytest.mark.parametrize("when", ["build", "probe"])
@pytest.mark.parametrize("max_blocks", [1, 2])
@pytest.mark.parametrize("name", ["small", "highdup", "mixed", "prefixes"])
def test_many_regions_per_wavefront(name, max_blocks, when, share, compact):
    """max_blocks = 1, 2 (4 or 8 probe wavefronts for 24-47 groups of 64 reads;
    prefixes: 2 groups, 8 window-group regions for one block): set before the
    build or only for the probe.  mixed and prefixes also take the containment
    probe and the window-0 runs through the capped grid."""
    ds, l, want, want_sup = reference(name)
    cap = {"max_blocks": max_blocks}
    e = OverlapEngine(0)
    try:
        e.set_option("probe_share", share)
        e.set_option("probe_compact", compact)
        if when == "build":
            e.set_option("max_blocks", max_blocks)
        rows, sup = step(e, ds, l, probe_opts=cap if when == "probe" else None)
    finally:
        e.close()
    assert super_dict(sup) == want_sup
    assert np.array_equal(rows_to_tuples(rows), want)
    check_pairs(rows, ds.packed()[1])


# name, options before the build, options for the probe alone, the split the rule gives, and
# whether the trailing parts are certainly empty with probe_share (asserted from scan_runs).
# run_cap = 32768 records per region lifts the rule's bound k <= run_cap / 4096 to 8.
SPLIT_CASES = {
    # highdup: 1,530 reads = 24 groups, 6 scan blocks x 4 = 24 regions; 4 probe blocks = 16
    # wavefronts: k = 1 gives 2 rounds for 1.5 (ratio 4/3), k = 2 gives 48 = 3 x 16
    "highdup_k2": ("highdup", {"run_cap": 32768}, {"max_blocks": 4}, 2, False),
    # small: 1,913 reads = 30 groups, 8 scan blocks x 4 = 32 regions; 3 probe blocks = 12
    # wavefronts: k = 1 and 2 leave 9/8, k = 3 gives 96 = 8 x 12
    "small_k3": ("small", {"run_cap": 32768}, {"max_blocks": 3}, 3, False),
    # small scanned by one block (4 regions of ~480 reads' runs), probed by all 8 blocks = 32
    # wavefronts: only k = 8 gives every wavefront a part (of about 6,100 / 8 records, rounded
    # up to whole batch strides: every part holds records)
    "small_k8": ("small", {"run_cap": 32768, "max_blocks": 1}, {"max_blocks": 8192}, 8, False),
    # mixed lengths, w = 169: 9 groups, 5 scan blocks x 2 wavefronts x 4 window groups = 40
    # regions of a few hundred records; 3 probe blocks = 12 wavefronts: k = 1 gives 48/40,
    # k = 2 gives 84/80, k = 3 gives 120 = 10 x 12.  Discovery runs after containment on the
    # live runs
    "wide_window_mixed_k3": ("wide_window_mixed", {"run_cap": 32768}, {}, 3, False),
    # one length, w = 169: 5 groups, 3 scan blocks x 2 wavefronts = 6 regions (one group of 64
    # reads each, the last empty); 2 probe blocks = 8 wavefronts: k = 1, 2, 3 leave 4/3, k = 4
    # gives 24 = 3 x 8.  Empty trailing parts: with probe_share a part is a multiple of 256
    # records, so once ALL the scan's runs are at most 3 x 256, three parts cover any region
    # and every region's fourth part starts at its end (lo == rcnt)
    "wide_window_short_k4": ("wide_window_short", {"run_cap": 32768}, {}, 4, True),
}


@pytest.mark.parametrize("share", [0, 1])
@pytest.mark.parametrize("case", sorted(SPLIT_CASES))
def test_virtual_region_split(case, share):
    name, build_opts, probe_opts, vsplit, empty_tail = SPLIT_CASES[case]
    ds, l, want, want_sup = reference(name)
    e = OverlapEngine(0)
    try:
        e.set_option("probe_share", share)
        for kk, v in build_opts.items():
            e.set_option(kk, v)
        rows, sup = step(e, ds, l, k=31 if name.startswith("wide_window") else 0, probe_opts=probe_opts)
        c = e.counters()
    finally:
        e.close()
    print(case, share, {x: c[x] for x in ("probe_vsplit", "scan_runs", "row_reruns", "run_reruns")})
    assert c["probe_vsplit"] >= 2 and c["probe_vsplit"] == vsplit, c
    assert c["run_reruns"] == 0, c  # (the regions the rule was worked out for)
    if empty_tail and share:  # per >= 256 records, so parts 0 .. k - 2 hold every record of any region
        assert 0 < c["scan_runs"] <= (vsplit - 1) * 256, c
    assert super_dict(sup) == want_sup
    assert np.array_equal(rows_to_tuples(rows), want)
    check_pairs(rows, ds.packed()[1])


def test_virtual_split_wider_bound():
    """probe_split_max = 64 with run_cap = 64 x 4096: small scanned by one block
    and probed by all 8 still takes k = 8 (the smallest that evens the rounds),
    and probe_split_max = 1 switches the split off."""
    ds, l, want, _ = reference("small")
    for split_max, vsplit in ((64, 8), (1, 1)):
        e = OverlapEngine(0)
        try:
            for kk, v in (("run_cap", 64 * 4096), ("max_blocks", 1), ("probe_split_max", split_max)):
                e.set_option(kk, v)
            rows, _ = step(e, ds, l, probe_opts={"max_blocks": 8192})
            assert e.counters()["probe_vsplit"] == vsplit, e.counters()
        finally:
            e.close()
        assert np.array_equal(rows_to_tuples(rows), want)


# ---- options that results never depend on (include/mg_overlap.h)
def fused_case(name, opts, steps=1, shard=(0, 1, 0, 0)):
    ds, l, want, want_sup = reference(name)
    e = OverlapEngine(0)
    try:
        for kk, v in opts.items():
            e.set_option(kk, v)
        for _ in range(steps):
            rows, sup = gpu_rows(e, ds, l, shard=shard)
            assert super_dict(sup) == want_sup, opts
            if shard == (0, 1, 0, 0):
                assert np.array_equal(rows_to_tuples(rows), want), opts
        packed = e.download_packed()
    finally:
        e.close()
    return ds, rows, packed


@pytest.mark.parametrize("name", ["tandem", "mixed"])
def test_option_halving(name):
    """halving = 1: the lower ID's side of a self-symmetric pair discovers it."""
    fused_case(name, {"halving": 1})


@pytest.mark.parametrize("name", ["small", "mixed"])
def test_option_layout_hash(name):
    """layout_hash = 1: another slot permutation; rows, superReadIDs and the
    downloaded reads (back in ID order) are unchanged."""
    ds, _, (w, lens) = fused_case(name, {"layout_hash": 1})
    hw, hl = ds.packed()
    assert np.array_equal(lens, hl) and np.array_equal(w[:, :hw.shape[1]], hw) and not np.any(w[:, hw.shape[1]:])


@pytest.mark.parametrize("name", ["small", "mixed"])
def test_option_cells_double(name):
    """cells_double = 1 over three steps of one engine: both tables serve, each
    cleared on the side stream while the other is in use."""
    fused_case(name, {"cells_double": 1}, steps=3)


@pytest.mark.parametrize("index_keys", [0, 1])
def test_option_index_keys_source_range(index_keys):
    """A source-range shard builds its index without a scan (LaunchIndex):
    index_keys = 0 takes k_index_build, 1 (default) k_index_keys."""
    ds, l, want, _ = reference("mixed")
    n = ds.num_unique
    parts = [fused_case("mixed", {"index_keys": index_keys}, shard=(0, 1, lo, hi))[1]
             for lo, hi in ((0, n // 2), (n // 2, n))]
    assert np.array_equal(rows_to_tuples(np.concatenate(parts)), want)


@pytest.mark.parametrize("opts", [{"live_runs": 0}, {"live_overlap": 0}, {"live_runs": 0, "live_overlap": 0}],
                         ids=["live_runs0", "live_overlap0", "both0"])
@pytest.mark.parametrize("name", ["mixed", "metagenome"])
def test_option_live_runs(name, opts):
    """live_runs = 0: the probe drops the runs of contained sources itself;
    live_overlap = 0: k_live_runs in line instead of beside the live index build."""
    fused_case(name, opts)


@pytest.mark.parametrize("name,world,opts", [
    ("small", 2, {"xchg_keys_first": 0, "check_cells": 1}), ("small", 3, {"xchg_keys_first": 0, "check_cells": 1}),
    ("highdup", 2, {"xchg_keys_first": 0, "check_cells": 1}), ("highdup", 3, {"xchg_keys_first": 0, "check_cells": 1}),
    ("small", 2, {"xchg_scan_lds": 0}), ("highdup", 3, {"xchg_scan_lds": 0}),
    ("small", 2, {"xchg_split_max": 0}), ("highdup", 2, {"xchg_split_max": 0}),
    ("small", 8, {"xchg_split_max": 8}), ("highdup", 8, {"xchg_split_max": 8}),
    ("small", 3, {"xchg_region": 64}), ("small", 3, {"xchg_region": 4096}),
    ("mixed", 3, {"xchg_region": 64}), ("mixed", 3, {"xchg_region": 4096})],
    ids=lambda x: "-".join(f"{k}{v}" for k, v in x.items()) if isinstance(x, dict) else str(x))
def test_exchange_option_sweep(name, world, opts):
    """Exchange mode: the sorted key build of one read length walked by
    check_cells (xchg_keys_first = 0), the register scan (xchg_scan_lds = 0), the
    discovery probe unsplit at P = 2 and split at P = 8 (xchg_split_max), and
    probe regions of 64 and 4,096 records (xchg_region)."""
    ds, l, want, want_sup = reference(name)
    rows, sup = exchange_rows(ds, l, world, opts=opts)
    assert np.array_equal(rows_to_tuples(rows), want)
    assert super_dict(sup) == want_sup
