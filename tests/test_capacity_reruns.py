"""Row-capacity reruns (option rows_cap), alone and with run-region reruns
(run_cap), on every host loop that has one: probe_shared (fused), run_discover
(source-range shards), the long-read loop and mg_xchg_probe (split and whole).

The kernels refuse a store past a region's capacity and keep counting; the
host reads the counts, grows the row buffer and reruns the probe.  Two caps:

  zero     rows_cap = 1: the per-region capacity is 0, every store is refused;
  partial  max_blocks = 1 with rows_cap = 4 * 50: one block's four regions of
           50 rows fill partway and a ballot-compacted batch straddles the cap.

Every test asserts that the reference has more rows than the capacity (so an
overflow must occur) and that counters().row_reruns saw it; the second step of
the same engine starts from the grown buffer and reruns nothing.  Bit-exact
against the reference's goldens or the oracle."""
import functools

import numpy as np
import pytest

from metagenomics_amd.overlap import rows_to_tuples
from refsets import engine_with as capped_engine
from refsets import fixture_reference, from_oracle, super_dict
from test_gpu_parity import assert_shard_rows, check_pairs, gpu_rows
from test_long_reads import LONG_CASES, long_set

pytestmark = pytest.mark.gpu

CAPS = {"zero": {"rows_cap": 1}, "partial": {"max_blocks": 1, "rows_cap": 4 * 50}}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(Dataset, l, k, rows as sorted tuples, {id: superReadID}) of a fixture or a long-read case."""
    if name in LONG_CASES:
        n, lo, hi, G, l, k, seed = LONG_CASES[name]
        ds, l, rows, sup = from_oracle(long_set(n, lo, hi, G, seed), l)
        return ds, l, k, rows, sup
    ds, l, rows, sup = fixture_reference(name)
    return ds, l, 0, rows, sup


def two_steps(e, name, rows_cap, shard=(0, 1, 0, 0), want_runs=False):
    """Two steps on one engine: the first overflows and reruns, the second does
    not.  Returns the rows of each step (a shard's rows are compared by the
    caller, as the union over the shards, for each step) and the counters."""
    ds, l, k, want, want_sup = reference(name)
    lens = ds.packed()[1]
    out, step_rows = [], []
    for step in range(2):
        rows, sup = gpu_rows(e, ds, l, k=k, shard=shard)
        c = e.counters()
        print(name, shard, "step", step, "rows", rows.shape[0], {x: c[x] for x in ("row_reruns", "run_reruns")})
        assert super_dict(sup) == want_sup
        if shard == (0, 1, 0, 0):
            assert np.array_equal(rows_to_tuples(rows), want)
        assert rows.shape[0] > rows_cap  # (this context's own rows overflow its capacity)
        if step == 0:
            assert c["row_reruns"] >= 1, c
            if want_runs:
                assert c["run_reruns"] >= 1, c
        else:
            assert c["row_reruns"] == 0, c
        check_pairs(rows, lens)
        out.append(c)
        step_rows.append(rows)
    return step_rows, out


@pytest.mark.parametrize("cap", sorted(CAPS))
@pytest.mark.parametrize("name", ["small", "highdup", "tandem", "mixed", "branchy", "longreads", "1025_1500"])
def test_row_overflow_reruns(name, cap):
    """Fused path: one read length (probe_shared as the scan's first reader;
    tandem's four-row self hits at the cap), mixed lengths (discovery after
    containment on the live runs) and reads over 1,024 bp (k_probe_long's loop)."""
    opts = CAPS[cap]
    assert reference(name)[3].shape[0] > opts["rows_cap"]
    e = capped_engine(opts)
    try:
        two_steps(e, name, opts["rows_cap"])
    finally:
        e.close()


@pytest.mark.parametrize("cap", sorted(CAPS))
def test_row_overflow_source_range_shard(cap):
    """run_discover's loop: the source-range shards [0, n/3) and [n/3, n) of
    mixed, each on its own capped engine; the union is the multiset."""
    opts = CAPS[cap]
    ds, l, _, want, _ = reference("mixed")
    n = ds.num_unique
    assert want.shape[0] > 2 * opts["rows_cap"]
    parts = ([], [])  # per step: the step that reran, the step that did not
    for lo, hi in ((0, n // 3), (n // 3, n)):
        e = capped_engine(opts)
        try:
            step_rows, _ = two_steps(e, "mixed", opts["rows_cap"], shard=(0, 1, lo, hi))
        finally:
            e.close()
        for step, rows in enumerate(step_rows):
            assert_shard_rows(rows, lo, hi)
            parts[step].append(rows)
    for step in range(2):
        assert np.array_equal(rows_to_tuples(np.concatenate(parts[step])), want), step


@pytest.mark.parametrize("cap", sorted(CAPS))
def test_row_overflow_bucket_shards(cap):
    """Bucket-range shards (r, 3, 0, 0) of small, one capped engine per rank."""
    opts = CAPS[cap]
    want = reference("small")[3]
    assert want.shape[0] > 3 * opts["rows_cap"]
    parts = ([], [])  # per step: the step that reran, the step that did not
    for r in range(3):
        e = capped_engine(opts)
        try:
            step_rows, _ = two_steps(e, "small", opts["rows_cap"], shard=(r, 3, 0, 0))
        finally:
            e.close()
        for step, rows in enumerate(step_rows):
            parts[step].append(rows)
    for step in range(2):
        assert np.array_equal(rows_to_tuples(np.concatenate(parts[step])), want), step


@pytest.mark.parametrize("name", ["small", "mixed"])
def test_run_and_row_overflow_together(name):
    """run_cap = 8 with rows_cap = 1: the cut scan, the rescan, the row overflow
    and the success all fit probe_shared's attempts."""
    opts = {"run_cap": 8, "rows_cap": 1}
    assert reference(name)[3].shape[0] > opts["rows_cap"]
    e = capped_engine(opts)
    try:
        two_steps(e, name, opts["rows_cap"], want_runs=True)
    finally:
        e.close()


# ---- exchange mode
def exchange_steps(ds, l, world, opts, route_rows, steps=2):
    """test_gpu_parity.exchange_rows with the engines kept over `steps` steps:
    per step (the ranks' rows, superReadIDs, the ranks' counters)."""
    import torch

    from metagenomics_amd.sharded import LocalExchange, sharded_step, source_range

    engines = []
    out = []
    try:
        for r in range(world):
            e = capped_engine(opts)
            engines.append(e)
            e.set_shard(r, world, 0, 0)
            e.upload(ds)
        xchg = LocalExchange(world, torch.device("cuda:0"))
        for _ in range(steps):
            res = sharded_step(engines, xchg, l, 0, want_super=True, route_rows=route_rows)
            assert res.reruns == 0  # (no stream was cut: a rerun of the whole step would hide the probe's)
            parts = [res.rows_numpy(r) for r in range(world)]
            if route_rows:
                for r, rows in enumerate(parts):
                    lo, hi = source_range(ds.num_unique, r, world)
                    assert np.all((rows["src"] >= lo + 1) & (rows["src"] <= hi)), "row at a rank that does not own its src"
            out.append((parts, res.super_read_id, [e.counters() for e in engines]))
    finally:
        for e in engines:
            e.close()
    return out


@pytest.mark.parametrize("cap", sorted(CAPS))
@pytest.mark.parametrize("name,world,route,extra", [
    ("small", 2, 0, {}), ("small", 2, 1, {}), ("highdup", 4, 0, {}),  # the split probe: own part, appended peers' part
    ("mixed", 3, 0, {}), ("small", 2, 0, {"xchg_split_max": 0}),       # one probe over every stream
])
def test_exchange_row_overflow_reruns(name, world, route, extra, cap):
    """mg_xchg_probe's loop.  After mg_xchg_probe_own a row overflow drops the
    own part's rows with the buffer, recomputes the region counts for every
    stream and probes them all in one launch; mixed lengths and
    xchg_split_max = 0 never split."""
    opts = dict(CAPS[cap], **extra)
    ds, l, _, want, want_sup = reference(name)
    assert want.shape[0] > world * opts["rows_cap"]
    lens = ds.packed()[1]
    steps = exchange_steps(ds, l, world, opts, bool(route))
    for step, (parts, sup, counters) in enumerate(steps):
        reruns = [c["row_reruns"] for c in counters]
        print(name, world, route, "step", step, [p.shape[0] for p in parts], reruns)
        assert np.array_equal(rows_to_tuples(np.concatenate(parts)), want)
        assert super_dict(sup) == want_sup
        if step == 0:
            assert max(reruns) >= 1, reruns
            if not route:  # each rank holds what it verified: its own overflow is known
                assert all(x >= 1 for x, p in zip(reruns, parts) if p.shape[0] > opts["rows_cap"]), reruns
        else:
            assert not any(reruns), reruns
        if not route:
            for p in parts:
                check_pairs(p, lens)


# ---- work counters after a rerun
@pytest.mark.parametrize("cap", ["rows_zero", "rows_partial", "runs"])
@pytest.mark.parametrize("name", ["small", "highdup"])
def test_counters_after_rerun(name, cap):
    """Option stats: a rerun's work counters replace the cut attempt's (the
    accumulators are cleared before every attempt that starts from scratch), so
    they equal those of the same step without a rerun.

    `rows`, `sources` and `runs` are compared with a fresh engine that has no
    cap (same max_blocks).  `entries` and `verified` depend on where the index
    build's CAS inserts happened to land (entries of other minimizers in a
    walked cell or chain), so two builds of the same index differ in them with
    no rerun anywhere (figures in DESIGN.md §7a); they are compared with a
    second discovery over the same index on the same engine, which starts from
    the grown buffers, reruns nothing and must count exactly the same."""
    base = {"stats": 1, **({"max_blocks": 1} if cap == "rows_partial" else {})}
    opts = dict(base, **{"rows_zero": {"rows_cap": 1}, "rows_partial": {"rows_cap": 4 * 50},
                         "runs": {"run_cap": 8}}[cap])
    ds, l, k, want, _ = reference(name)
    assert want.shape[0] > opts.get("rows_cap", 0)
    got = {}
    for which, o in (("plain", base), ("capped", opts)):
        e = capped_engine(o)
        try:
            rows, _ = gpu_rows(e, ds, l, k=k)
            got[which] = e.counters()
            if which == "capped":  # the same index again: nothing overflows now
                assert e.find_overlaps() == want.shape[0]
                got["again"] = e.counters()
        finally:
            e.close()
        assert np.array_equal(rows_to_tuples(rows), want)
    print(name, cap, got)
    plain, capped, again = got["plain"], got["capped"], got["again"]
    assert plain["row_reruns"] == 0 and plain["run_reruns"] == 0 and again["row_reruns"] == 0
    assert capped["run_reruns" if cap == "runs" else "row_reruns"] >= 1, capped
    for c in (plain, capped, again):
        assert c["rows"] == want.shape[0], c
        assert c["sources"] == ds.num_unique, c
    assert capped["runs"] == plain["runs"] > 0, (plain, capped)
    for key in ("runs", "entries", "verified"):
        assert capped[key] == again[key] > 0, (key, capped, again)


def test_copy_rows_below_count_after_rerun():
    """mg_copy_rows with cap < the row count, after a rerun (settle_rows' new
    buffer, k_compact_rows' clamp): exactly cap rows, each one of the reference's."""
    from collections import Counter

    ds, l, k, want, _ = reference("small")
    assert want.shape[0] > 1
    e = capped_engine({"rows_cap": 1})
    try:
        e.upload(ds)
        e.build_index(l, k)
        e.mark_contained()
        n = e.find_overlaps()
        assert n == want.shape[0] and e.counters()["row_reruns"] >= 1
        part = e.rows(n // 2)
    finally:
        e.close()
    assert part.shape[0] == n // 2
    have, ref = Counter(map(tuple, rows_to_tuples(part).tolist())), Counter(map(tuple, want.tolist()))
    assert all(ref[t] >= c for t, c in have.items())
