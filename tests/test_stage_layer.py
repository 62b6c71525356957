"""What the device stage files share (metagenomics_amd/csrc/device/mg_stage.hpp
and the per-stage structs of mg_ctx.hpp), seen through the calls:

  a. a failed allocation of call-lifetime scratch names its buffer and its
     bytes in every call that allocates some, option alloc_cap reaches it, and
     the same call on the same engine succeeds once the cap is lifted;
  b. one engine running the whole chain for a smaller, a larger and the smaller
     set again: the resident arrays grow, are reused and, on the tandem-repeat
     path of the discovery lists, are swapped with their capacities;
  c. the CSR starts of sorted owners (k_csr_starts) at their edges: no records,
     records of read 1 and of read N, a read without records between two that
     have some;
  d. the core context (mg_kernels.hip: upload, index, containment, discovery,
     rows, lookup, exchange) under the same model: its call-lifetime scratch is
     named and capped like the stages', and under a ladder of caps every chain
     either completes with the golden results or fails at a named allocation
     larger than the cap, and completes on the same engine once the cap is lifted.

Each cap sits one byte below the scratch buffer it names; the buffers the call
allocates before it are listed with their sizes, restated from the call's code,
and asserted to fit under the cap.  The temporary storage of the device-wide
sorts and scans (a few KiB at these sizes) is the one size that is not
restated; the named buffers are chosen far above it.  Expected results: the
plain references of ingest_ref.py and mates_ref.py, the golden files, and the
host mirrors that test_places_host.py and test_mates_host.py pin."""
import re

import numpy as np
import pytest

import contigs_ref
import mates_ref
import places_ref
from comp_ref import components_from_rows
from conftest import fixture_input, golden_rows, load_meta
from ingest_ref import assert_ingested, pack, ref_dataset
from metagenomics_amd.overlap import (CONTIG_EDGE_DTYPE, MATE_DTYPE, PLACE_DTYPE, Dataset, MgError, OverlapEngine,
                                      host_edge_coverage, host_insert_size_sums, host_mate_pairs, host_placements,
                                      rows_to_tuples)
from test_discoveries import assert_lists, expected
from test_gpu_parity import exchange_rows
from test_places import boundary_case, engine_for, mate_csr

pytestmark = pytest.mark.gpu

L_MIN = 15
LONG = 1000  # one record of 32 words among records of 2: the canonical words outweigh the text


def skewed_records():
    """150 pairs of 40-bp records, the first mate of pair 0 a 1,000-bp record; every record is a read."""
    rng = np.random.default_rng(41)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    raw = [acgt[rng.integers(0, 4, LONG if k == 0 else 40)].tobytes().decode() for k in range(300)]
    raw[7], raw[8] = mates_ref.rc(raw[5]), raw[5].lower()  # a read given three times, either strand and case
    assert all(mates_ref.passes(s, L_MIN) for s in raw)
    return raw


def expect_named_failure(eng, cap, name, call):
    """`call` fails at the buffer `name` of cap + 1 bytes; with the cap lifted the same call returns its result"""
    eng.set_option("alloc_cap", cap)
    with pytest.raises(MgError) as exc:
        call()
    msg = str(exc.value)
    print(msg)
    for part in ("device allocation of ", f"{name} ({cap + 1} B) failed: ", "alloc_cap"):
        assert part in msg, msg
    eng.set_option("alloc_cap", 0)
    return call()


# ---- a. allocation failures

def test_find_reads_names_its_scratch():
    raw = skewed_records()
    _, seqs, _ = ref_dataset(raw, L_MIN)
    ids = {s: i + 1 for i, s in enumerate(seqs)}
    absent = [raw[1][:-1] + "ACGT"["ACGT".index(raw[1][-1]) - 1], raw[2] + "C", "ACGN" * 10]
    q = raw + absent
    want_id = np.array([ids.get(min(s.upper(), mates_ref.rc(s.upper())), 0) for s in q], dtype=np.uint32)
    want_fl = np.array([(1 | (2 if i and s.upper() == seqs[i - 1] else 0)) if mates_ref.passes(s, L_MIN) else 0
                        for s, i in zip(q, want_id)], dtype=np.uint8)
    assert want_id[:300].all() and not want_id[300:].any() and want_fl[-1] == 0
    n, total = len(q), sum(map(len, q))
    before = {"mate records": total, "mate record offsets": (n + 1) * 8}
    target = n * 32 * 8  # "mate canonical words": 32 words per record
    assert max(before.values()) < target
    eng = OverlapEngine(0)
    try:
        assert eng.ingest_ascii(raw, L_MIN) == len(seqs)
        got_id, got_fl = expect_named_failure(eng, target - 1, "mate canonical words",
                                              lambda: eng.find_reads(q, L_MIN))
        assert np.array_equal(got_id, want_id) and np.array_equal(got_fl, want_fl)
    finally:
        eng.close()


def test_build_mate_pairs_names_its_scratch():
    raw = skewed_records()
    _, seqs, _ = ref_dataset(raw, L_MIN)
    ppd = (100, 50)
    text, off = mates_ref.records_of(raw)
    want = mates_ref.mate_lists(seqs, raw, ppd, L_MIN)
    n_raw, N = len(raw), len(seqs)
    # resident lists first, then the sort's scratch (4 or 8 B per record), then the lookup's
    before = {"d_mate_start": (N + 2) * 8, "d_mates": n_raw * MATE_DTYPE.itemsize, "mate pair keys": n_raw * 8,
              "mate records": len(text), "mate record offsets": (n_raw + 1) * 8}
    target = n_raw * 32 * 8  # "mate canonical words"
    assert max(before.values()) < target
    eng = OverlapEngine(0)
    try:
        assert eng.ingest_ascii(raw, L_MIN) == N
        words, lens = eng.download_packed()

        def call():
            n = eng.build_mate_pairs(text, off, ppd, L_MIN, use_super=False)
            return n, eng.mate_lists()

        n, got = expect_named_failure(eng, target - 1, "mate canonical words", call)
        assert n == want[1].shape[0] > 0
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert (eng.good_pairs, eng.bad_pairs) == want[2:] == (150, 0)
        host = host_mate_pairs(words, lens, text, off, ppd, L_MIN)
        assert np.array_equal(got[0], host[0]) and np.array_equal(got[1], host[1])
    finally:
        eng.close()


def test_ingest_ascii_names_its_scratch():
    raw = skewed_records()
    ref = ref_dataset(raw, L_MIN)
    n, total = len(raw), sum(map(len, raw))
    before = {"ingest records": total, "ingest record offsets": (n + 1) * 8}
    target = n * 32 * 8  # "ingest canonical words": the 32-word template
    assert max(before.values()) < target
    eng = OverlapEngine(0)
    try:
        nu = expect_named_failure(eng, target - 1, "ingest canonical words", lambda: eng.ingest_ascii(raw, L_MIN))
        assert nu == len(ref[1])
        assert_ingested(eng, *ref)
    finally:
        eng.close()


PAD = 1 << 16  # list entries no edge refers to: they make the uploaded lists the largest buffers


def padded(reads, offs, ors):
    return (np.concatenate([reads, np.ones(PAD, dtype=reads.dtype)]), np.concatenate([offs, np.zeros(PAD, offs.dtype)]),
            np.concatenate([ors, np.zeros(PAD, ors.dtype)]))


def test_build_contigs_names_its_scratch():
    ds, g = contigs_ref.fixture_graph("small")
    want = contigs_ref.parse_estrings(contigs_ref.golden_file("small", "estrings").decode())
    e, reads, offs, ors = g.contig_edges(all_edges=True)
    e = e[np.array([w[5] != "!" for w in want], dtype=bool)]
    reads, offs, ors = padded(reads, offs, ors)
    P = int(e["n"].sum()) + 2 * e.shape[0]
    before = {"d_ctg_desc": P * 8, "d_ctg_len": (P + 1) * 8, "d_ctg_pos": (P + 1) * 8,
              "d_ctg_pbase": (e.shape[0] + 1) * 8, "contig edges": e.shape[0] * CONTIG_EDGE_DTYPE.itemsize}
    target = reads.shape[0] * 4  # "contig list reads"
    assert max(before.values()) < target
    eng = OverlapEngine(0)
    try:
        eng.upload(ds)
        start, data = expect_named_failure(eng, target - 1, "contig list reads",
                                           lambda: eng.build_contigs(e, reads, offs, ors))
        assert contigs_ref.split(start, data) == [w[5] for w in want if w[5] != "!"]
    finally:
        eng.close()


def test_build_placements_names_its_scratch():
    lens, graph, _ = boundary_case()
    edges, reads, offs, ors = graph
    reads, offs, ors = padded(reads, offs, ors)
    N, E = lens.shape[0], int(edges["n"].sum())
    before = {"d_pl_start": (N + 2) * 8, "d_places": E * PLACE_DTYPE.itemsize, "d_pl_edges": edges.nbytes,
              "d_pl_edist": E * 8, "placement offset sums": E * 8}
    target = reads.shape[0] * 4  # "placement list reads"
    assert max(before.values()) < target
    hs, hr, _ = host_placements(N, *graph)  # (the mirror ignores what no edge refers to: checked below)
    hp = host_placements(N, edges, reads, offs, ors)
    assert np.array_equal(hp[0], hs) and np.array_equal(hp[1], hr)
    eng = engine_for(np.random.default_rng(1), lens)
    try:
        def call():
            n = eng.build_placements(edges, reads, offs, ors)
            return n, eng.placements()

        n, (ds, dr) = expect_named_failure(eng, target - 1, "placement list reads", call)
        assert n == hr.shape[0] == E
        assert np.array_equal(ds, hs) and np.array_equal(dr, hr)
    finally:
        eng.close()


def test_insert_sizes_names_its_scratch():
    lens, graph, triples = boundary_case()
    triples = triples + [(7, 1, 0), (8, 2, 1), (3, 2, 0)]  # more entries than reads + 2
    N = lens.shape[0]
    mates = mate_csr(N, triples)
    before = {"caller's mate list starts": (N + 2) * 8}
    target = len(triples) * MATE_DTYPE.itemsize  # "caller's mate lists"
    assert max(before.values()) < target
    eng = engine_for(np.random.default_rng(1), lens)
    try:
        eng.build_placements(*graph)
        places = eng.placements()
        hs, hr, _ = host_placements(N, *graph)
        assert np.array_equal(places[0], hs) and np.array_equal(places[1], hr)
        got = expect_named_failure(eng, target - 1, "caller's mate lists", lambda: eng.insert_size_sums(256, mates))
        assert np.array_equal(got, host_insert_size_sums((hs, hr), mates, 256))
        assert np.array_equal(got, places_ref.insert_size_sums(places_ref.lists_of(hs, hr), mates[0], mates[1], 256))
        assert got[:, 0].sum() > 0
    finally:
        eng.close()


def test_edge_coverage_names_its_scratch():
    lens, graph, _ = boundary_case()
    N, n_edges = lens.shape[0], graph[0].shape[0]
    freq = np.arange(1, N + 1, dtype=np.uint32)
    before = {"caller's read frequencies": N * 4}
    target = n_edges * 24  # "coverage edge records": 24 B per edge (EdgeInfo of mg_places.hip)
    assert max(before.values()) < target
    want = host_edge_coverage(lens, freq, *graph)
    assert want[:, 0].min() > 0
    eng = engine_for(np.random.default_rng(1), lens)
    try:
        eng.build_placements(*graph)
        got = expect_named_failure(eng, target - 1, "coverage edge records", lambda: eng.edge_coverage(freq))
        assert np.array_equal(got, want)
    finally:
        eng.close()


# ---- b. grow, shrink and swap on one context

def test_chain_on_one_engine_tandem_small_tandem():
    """tandem's self rows take the duplicate-free copy (the lists and their starts swap with their
    twins); small, the larger set, then has to grow whatever the swap left too small, and tandem
    again runs in arrays larger than it needs and swaps them once more"""
    eng = OverlapEngine(0)
    try:
        sizes = []
        for name in ("tandem", "small", "tandem"):
            meta, ds, lens, start, disc, n_self = expected(name)
            eng.upload(ds)
            eng.build_index(meta["l"])
            n_rows = eng.find_overlaps()
            assert n_rows == golden_rows(name).shape[0]
            assert eng.build_discoveries() == n_rows - n_self // 2
            assert_lists(*eng.discoveries(), start, disc)
            n_comp = eng.build_components()
            label, comps = eng.components()
            want = components_from_rows(golden_rows(name), ds.num_unique)
            assert comps.shape[0] == n_comp
            assert np.array_equal(label, want[0]) and np.array_equal(comps, want[1])
            sizes.append((ds.num_unique, n_rows, n_self))
        assert sizes[0][2] > 0 and sizes[1][2] == 0  # only tandem drops copies of self rows
        assert sizes[1][0] > sizes[0][0] and sizes[1][1] > sizes[0][1]  # the middle set has more reads and rows
    finally:
        eng.close()


# ---- c. the CSR starts at their edges

def csr_reads():
    rng = np.random.default_rng(43)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    seqs = sorted({min(s, mates_ref.rc(s)) for s in (acgt[rng.integers(0, 4, 50)].tobytes().decode() for _ in range(9))})
    assert len(seqs) == 9 and all(mates_ref.passes(s, L_MIN) for s in seqs)
    return seqs


def assert_edges_of_starts(start, n, owners):
    """the expected starts show what the case is about: N + 2 entries, start[0] = start[1] = 0, exactly `owners` have records"""
    assert start.shape[0] == n + 2 and start[0] == 0 and start[1] == 0
    assert {a for a in range(1, n + 1) if start[a + 1] > start[a]} == set(owners)


@pytest.mark.parametrize("pairs, owners", [((), ()), (((1, 9), (3, 9)), (1, 3, 9)), (((9, 9), (5, 4)), (4, 5, 9))],
                         ids=["none", "first_gap_last", "last_only_self"])
def test_mate_list_starts(pairs, owners):
    seqs = csr_reads()
    n = len(seqs)
    raw = [seqs[i - 1] for p in pairs for i in p]
    ppd = (len(pairs),) if pairs else ()
    text, off = mates_ref.records_of(raw)
    wpr = 2
    want = host_mate_pairs(pack(seqs, wpr), np.array([len(s) for s in seqs], np.uint16), text, off, ppd, L_MIN)
    ref = mates_ref.mate_lists(seqs, raw, ppd, L_MIN)
    assert np.array_equal(want[0], ref[0]) and np.array_equal(want[1], ref[1])
    assert_edges_of_starts(want[0], n, owners)
    eng = OverlapEngine(0)
    try:
        assert eng.ingest_ascii(seqs, L_MIN) == n
        assert eng.build_mate_pairs(text, off, ppd, L_MIN, use_super=False) == want[1].shape[0]
        start, recs = eng.mate_lists()
        assert np.array_equal(start, want[0]) and np.array_equal(recs, want[1])
    finally:
        eng.close()


@pytest.mark.parametrize("lists, owners", [([], ()), ([[], []], ()), ([[(1, 3, 1), (9, 0, 0)], [(3, 2, 1), (1, 1, 0)]], (1, 3, 9)),
                                           ([[(9, 5, 1)], [], [(8, 0, 1), (9, 1, 1)]], (8, 9))],
                         ids=["no_edges", "empty_lists", "first_gap_last", "last_two"])
def test_placement_starts(lists, owners):
    n = 9
    lens = np.full(n, 50, dtype=np.uint16)
    graph = places_ref.make_edges(lists, [(1, 2, 100)] * len(lists))
    hs, hr, _ = host_placements(n, *graph)
    assert_edges_of_starts(hs, n, owners)
    eng = engine_for(np.random.default_rng(2), lens)
    try:
        assert eng.build_placements(*graph) == hr.shape[0]
        start, recs = eng.placements()
        assert np.array_equal(start, hs) and np.array_equal(recs, hr)
    finally:
        eng.close()


# ---- d. the core context's buffers

def core_fixture(name):
    """(meta, Dataset, the h-base key at the start of read 1) of a golden fixture"""
    meta = load_meta(name)
    ds = Dataset.from_files([fixture_input(name)], meta["l"])
    return meta, ds, ds.read(1)[: meta["l"] - 1]


def super_of(sup):
    return {str(i): int(s) for i, s in enumerate(sup) if s}


def test_lookup_names_its_scratch():
    meta, ds, key = core_fixture("small")
    before = {"lookup key": ((len(key) + 31) // 32 + 1) * 8}
    target = 1024 * 8  # "lookup results": the binding's first buffer of 1,024 entries
    assert max(before.values()) < target
    eng = OverlapEngine(0)
    try:
        eng.set_option("nb_log2", 10)
        eng.upload(ds)
        eng.build_index(meta["l"])
        want = eng.lookup(key)  # (the first lookup after a build files the lookup table, far above the cap)
        assert (1, 0) in want
        assert expect_named_failure(eng, target - 1, "lookup results", lambda: eng.lookup(key)) == want
    finally:
        eng.close()


def test_upload_ascii_names_its_scratch():
    meta, ds, _ = core_fixture("small")
    seqs = [ds.read(i) for i in range(1, ds.num_unique + 1)]
    total = sum(map(len, seqs))  # "upload records": the call's first allocation on a fresh context
    eng = OverlapEngine(0)
    try:
        expect_named_failure(eng, total - 1, "upload records", lambda: eng.upload_ascii(seqs))
        eng.build_index(meta["l"])
        eng.mark_contained()
        assert np.array_equal(rows_to_tuples(eng.rows()), golden_rows("small"))
    finally:
        eng.close()


LADDER = [1 << s for s in (8, 12, 16, 20, 24)]
ALLOC_FAILURE = re.compile(r"device allocation of (.+) \((\d+) B\) failed: ")


def assert_capped(err, cap):
    """the failure names a buffer larger than the cap and the option that refused it"""
    msg = str(err)
    print(cap, msg)
    m = ALLOC_FAILURE.search(msg)
    assert m and "alloc_cap" in msg, msg
    assert int(m.group(2)) > cap, msg


@pytest.mark.parametrize("name", ["small", "mixed"])
def test_core_allocation_ladder(name):
    meta, ds, key = core_fixture(name)
    want_rows = golden_rows(name)

    def chain(eng):
        eng.upload(ds)
        eng.build_index(meta["l"])
        sup = eng.mark_contained()
        rows = eng.rows(eng.find_overlaps())
        assert (1, 0) in eng.lookup(key)
        assert np.array_equal(rows_to_tuples(rows), want_rows) and super_of(sup) == meta["super"]

    failed = []
    for cap in LADDER:
        eng = OverlapEngine(0)
        try:
            eng.set_option("alloc_cap", cap)
            try:
                chain(eng)
            except MgError as e:
                assert_capped(e, cap)
                failed.append(cap)
            eng.set_option("alloc_cap", 0)
            chain(eng)
        finally:
            eng.close()
    assert failed and len(failed) < len(LADDER), failed  # some cap refuses an allocation, some cap lets the chain through


def test_exchange_allocation_ladder():
    """the same ladder through the exchange step of two ranks, the caps set once the reads are resident"""
    meta, ds, _ = core_fixture("small")
    want_rows = golden_rows("small")
    failed = []
    for cap in LADDER:
        try:
            rows, sup = exchange_rows(ds, meta["l"], 2, opts_after_upload={"alloc_cap": cap})
        except MgError as e:
            assert_capped(e, cap)
            failed.append(cap)
        else:
            assert np.array_equal(rows_to_tuples(rows), want_rows) and super_of(sup) == meta["super"]
    assert failed and len(failed) < len(LADDER), failed
