#!/usr/bin/env python3
"""Scaffolder support (mg_scaffold_pairs) against its host mirror at two shapes.

  chain       the C3-shaped chain set of tools/paths_bench.py: 9.36M reads on 24
              unitig edges, 5M mate pairs (10M entries), both mates on one edge:
              every processed entry ends in the same-edge test, no record
              exists.  The scoring pass and the transfers alone.
  fragmented  --contigs disjoint contigs (16,384: an edge of offset 1,000 and
              its twin each, 32,768 edges); --frag-reads reads (2M), each once
              on a contig (forward on the edge at p, reverse on the twin at
              1,000 - p); --frag-pairs pairs (1M, 2M entries) joining a read to
              one on the next contig or the one after, mean 400, SD 100 (bound
              700): tens of thousands of records, supports of a few dozen.

Per shape, as medians of --repeats alternating repeats after one warm-up:
  score_ms / aggregate_ms  HIP-event time of k_sc_score and of the aggregate
                           (scans, sorts, head kernels)
  call_ms                  wall time of OverlapEngine.scaffold_pairs: adds the
                           H2D of twins and CSRs, the validation kernels, and the
                           D2H of the statuses and the records
  mirror_ms                wall time of host_scaffold_pairs (one thread)
device == mirror is checked array for array on the first repeat.  Writes the JSON
to --out with the library's sha256 as tools/pmc_summary.py records it."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from metagenomics_amd.overlap import MATE_DTYPE, PLACE_DTYPE, OverlapEngine, host_scaffold_pairs  # noqa: E402
from paths_bench import chain_case  # noqa: E402
from pmc_summary import library_provenance  # noqa: E402


def fragmented_case(a):
    rng = np.random.default_rng(31)
    C, R, Pn, O = a.contigs, a.frag_reads, a.frag_pairs, 1000
    contig = np.sort(rng.integers(0, C, R))  # read IDs ascend with the contig, so A < B for a pair looking ahead
    p = rng.integers(0, O, R)
    recs = np.zeros(2 * R, dtype=PLACE_DTYPE)
    recs["edge"][0::2], recs["flags"][0::2], recs["distance"][0::2] = 2 * contig, 1, p
    recs["edge"][1::2], recs["flags"][1::2], recs["distance"][1::2] = 2 * contig + 1, 0, O - p
    start = np.zeros(R + 2, dtype=np.uint64)
    start[1:] = 2 * np.arange(R + 1, dtype=np.uint64)
    first_of = np.searchsorted(contig, np.arange(C + 1))
    A = rng.integers(0, R, Pn)
    tc = np.minimum(contig[A] + rng.integers(1, 3, Pn), C - 1)
    lo, hi = first_of[tc], np.maximum(first_of[tc + 1], first_of[tc] + 1)
    B = np.minimum(lo + (rng.random(Pn) * (hi - lo)).astype(np.int64), R - 1)
    ida, idb = A + 1, B + 1
    owner, mate = np.concatenate([ida, idb]), np.concatenate([idb, ida])
    orient = np.concatenate([np.full(Pn, 2, np.uint8), np.full(Pn, 1, np.uint8)])
    order = np.argsort(owner, kind="stable")
    mrecs = np.zeros(owner.shape[0], dtype=MATE_DTYPE)
    mrecs["id"], mrecs["orient"] = mate[order], orient[order]
    mstart = np.zeros(R + 2, dtype=np.uint64)
    mstart[1:] = np.cumsum(np.bincount(owner, minlength=R + 1))
    twin = np.arange(2 * C, dtype=np.uint32) ^ 1
    return R, twin, (start, recs), (mstart, mrecs), np.array([400], np.uint64), np.array([100], np.uint64)


def measure(name, case, a):
    n, twin, places, mates, mean, sd = case
    eng = OverlapEngine(0)

    def timed(f):
        t0 = time.perf_counter()
        r = f()
        return r, (time.perf_counter() - t0) * 1e3

    run = lambda: eng.scaffold_pairs(twin, twin.shape[0], mean, sd, places=places, mates=mates, n_reads=n)
    run()  # warm-up: buffers sized
    dev, mir, got = [], [], None
    for rep in range(a.repeats):
        got, t = timed(run)
        dev.append((eng.scaffold_ms[0], eng.scaffold_ms[1], t))
        host, m = timed(lambda: host_scaffold_pairs(n, twin, places, mates, mean, sd))
        mir.append(m)
        if rep == 0:
            assert np.array_equal(got.status, host.status), name + ": device != mirror in status"
            assert np.array_equal(got.pairs, host.pairs), name + ": device != mirror in pairs"
            assert got.counters == host.counters
    eng.close()
    med = statistics.median
    sup = got.pairs["support"]
    return {
        "shape": name, "reads": int(n), "edges": int(twin.shape[0]), "mate_entries": int(mates[1].shape[0]),
        "placements": int(places[1].shape[0]), "repeats": a.repeats,
        "counters": dict(zip(("skipped", "not_unique", "far", "same_edge", "counted"), got.counters)),
        "records": int(got.pairs.shape[0]), "records_support_ge_3": int((sup >= 3).sum()),
        "max_support": int(sup.max()) if sup.size else 0,
        "score_ms": med([d[0] for d in dev]), "aggregate_ms": med([d[1] for d in dev]),
        "call_ms": med([d[2] for d in dev]), "mirror_ms": med(mir), "all_device": dev, "all_mirror": mir,
        "checked_equal": True,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=9_360_000)
    ap.add_argument("--edges", type=int, default=24)
    ap.add_argument("--pairs", type=int, default=5_000_000)
    ap.add_argument("--coverage", type=int, default=20)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--contigs", type=int, default=16_384)
    ap.add_argument("--frag-reads", type=int, default=2_000_000)
    ap.add_argument("--frag-pairs", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default="chain,fragmented")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"shapes": [], "library": library_provenance()}
    for name in a.shapes.split(","):
        if name == "chain":
            n, _, twin, places, mates, mean, sd = chain_case(a)
            case = (n, twin, places, mates, mean, sd)
        else:
            case = fragmented_case(a)
        res["shapes"].append(measure(name, case, a))
        print(json.dumps(res["shapes"][-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
