#!/usr/bin/env python3
"""Mate-pair path support (mg_mate_paths) against its host mirror at two shapes.

  chain   the C3-shaped chain set of tools/places_bench.py: --reads 150-bp reads
          (default 9.36M) on 24 unitig edges, --pairs mate pairs (5M, 10M mate
          entries), both mates on one edge.  The set lists every edge once, so
          twin[k] = k.  Every entry ends in the same-edge test (one work unit):
          the shape measures the per-entry fixed cost, the transfers and the
          batch loop, not the search.
  ladder  a branching shape: --layers layers (4096) of two nodes, each node
          joined to both nodes of the next layer (offset 40, orientation 0) and
          back (orientation 3, the twins): 4 * layers * 2 edges.  --ladder-reads
          reads (2M) lie on one forward edge each; --ladder-pairs pairs (1M, 2M
          entries) join a read to one 1-4 layers ahead, mean 120, SD 20 (window
          60..180), so a search walks a binary tree 2-5 edges deep.

Per shape, as medians of --repeats alternating repeats after one warm-up:
  explore_ms / aggregate_ms  HIP-event time of the explore kernels and of the
                             aggregate (scans, sorts, pair kernels)
  call_ms                    wall time of OverlapEngine.mate_paths: adds the H2D
                             of edges, CSRs, the per-batch host synchronisation,
                             any regrowth of the path space, and the D2H of the
                             per-entry results and the pair list
  mirror_ms                  wall time of host_mate_paths (one thread)
and the distribution of work units per searching entry (the quantity option
path_budget bounds), the deferred count, and the explore workspace in bytes.
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

from contig_bench import chain_set  # noqa: E402
from metagenomics_amd.overlap import (CONTIG_EDGE_DTYPE, MATE_DTYPE, PLACE_DTYPE, OverlapEngine, host_mate_paths,  # noqa: E402
                                      host_placements)
from places_bench import mate_set  # noqa: E402
from pmc_summary import library_provenance  # noqa: E402

LEVELS, BYTES_PER_LEVEL = 101, 26  # the explore workspace per lane


def chain_case(a):
    words, lens, edges, reads, offs, ors = chain_set(a.reads, a.edges, a.coverage, a.read_len, 11)
    n = lens.shape[0]
    start, recs, _ = host_placements(n, edges, reads, offs, ors)
    mates = mate_set(edges, reads, n, a.pairs, 12)
    order = np.argsort(edges["src"], kind="stable")
    assert np.array_equal(order, np.arange(edges.shape[0])), "the chain set's edges ascend in src"
    twin = np.arange(edges.shape[0], dtype=np.uint32)
    return n, edges, twin, (start, recs), mates, np.array([400], np.uint64), np.array([100], np.uint64)


def ladder_case(a):
    rng = np.random.default_rng(21)
    L = a.layers
    rows = []  # (src, dst, orient); node of layer i, side s = 2 i + s + 1
    for i in range(L):
        for s in range(2):
            u = 2 * i + s + 1
            if i + 1 < L:
                rows += [(u, 2 * (i + 1) + t + 1, 0) for t in range(2)]
            if i > 0:
                rows += [(u, 2 * (i - 1) + t + 1, 3) for t in range(2)]
    rows.sort(key=lambda r: (r[0], r[1]))
    index = {(r[0], r[1]): k for k, r in enumerate(rows)}
    edges = np.zeros(len(rows), dtype=CONTIG_EDGE_DTYPE)
    edges["src"], edges["dst"], edges["orient"] = (np.array(c) for c in zip(*rows))
    edges["offset"] = 40
    twin = np.array([index[(r[1], r[0])] for r in rows], dtype=np.uint32)
    fwd = np.flatnonzero(edges["orient"] == 0)
    layer_of = (edges["src"][fwd].astype(np.int64) - 1) // 2
    by_layer = [fwd[layer_of == i] for i in range(L - 1)]
    n_nodes, R = 2 * L, a.ladder_reads
    n = n_nodes + R
    # read n_nodes + 1 + r lies on one forward edge; IDs ascend with the layer, so A < B for a pair looking ahead
    lay = np.sort(rng.integers(0, L - 1, R))
    pick = rng.integers(0, 4, R)
    e = np.array([by_layer[i][p] for i, p in zip(lay, pick)], dtype=np.uint32)
    recs = np.zeros(R, dtype=PLACE_DTYPE)
    recs["edge"], recs["flags"], recs["distance"] = e, 1, rng.integers(0, 40, R)
    start = np.zeros(n + 2, dtype=np.uint64)
    start[n_nodes + 1:] = np.arange(R + 1, dtype=np.uint64)
    first_of = np.searchsorted(lay, np.arange(L))  # first read of each layer
    A = rng.integers(0, R, a.ladder_pairs)
    tl = np.minimum(lay[A] + rng.integers(1, 5, a.ladder_pairs), L - 2)
    lo, hi = first_of[tl], np.maximum(first_of[np.minimum(tl + 1, L - 1)], first_of[tl] + 1)
    B = np.minimum(lo + (rng.random(a.ladder_pairs) * (hi - lo)).astype(np.int64), R - 1)
    ida, idb = A + n_nodes + 1, B + n_nodes + 1
    owner, mate = np.concatenate([ida, idb]), np.concatenate([idb, ida])
    order = np.argsort(owner, kind="stable")
    mrecs = np.zeros(owner.shape[0], dtype=MATE_DTYPE)
    mrecs["id"], mrecs["orient"] = mate[order], 2  # both mates' forward lists
    mstart = np.zeros(n + 2, dtype=np.uint64)
    mstart[1:] = np.cumsum(np.bincount(owner, minlength=n + 1))
    return n, edges, twin, (start, recs), (mstart, mrecs), np.array([120], np.uint64), np.array([20], np.uint64)


def measure(name, case, a):
    n, edges, twin, places, mates, mean, sd = case
    eng = OverlapEngine(0)

    def timed(f):
        t0 = time.perf_counter()
        r = f()
        return r, (time.perf_counter() - t0) * 1e3

    run = lambda: eng.mate_paths(edges, twin, mean, sd, places=places, mates=mates, n_reads=n)
    run()  # warm-up: buffers sized
    dev, mir, got = [], [], None
    for rep in range(a.repeats):
        got, t = timed(run)
        dev.append((eng.paths_ms[0], eng.paths_ms[1], t))
        if a.no_mirror:
            continue
        host, m = timed(lambda: host_mate_paths(n, edges, twin, places, mates, mean, sd))
        mir.append(m)
        if rep == 0:
            full = got.finish()
            for f in ("status", "start", "path", "flags", "pairs"):
                assert np.array_equal(getattr(full, f), getattr(host, f)), name + ": device != mirror in " + f
            assert full.counters == host.counters
    eng.close()
    med = lambda v: statistics.median(v) if v else None
    M = int(mates[1].shape[0])
    units = got.visits[got.visits > 0].astype(np.int64)
    pct = lambda q: int(np.percentile(units, q)) if units.size else 0
    batch = min(1 << 18, max(M, 1))
    return {
        "shape": name, "reads": int(n), "edges": int(edges.shape[0]), "mate_entries": M,
        "placements": int(places[1].shape[0]), "repeats": a.repeats,
        "counters": {"no_path": got.counters[0], "path": got.counters[1], "same_edge": got.counters[2]},
        "pairs": int(got.pairs.shape[0]), "path_positions": int(got.path.shape[0]), "deferred": got.deferred,
        "explore_ms": med([d[0] for d in dev]), "aggregate_ms": med([d[1] for d in dev]),
        "call_ms": med([d[2] for d in dev]), "mirror_ms": med(mir), "all_device": dev, "all_mirror": mir,
        "checked_equal": not a.no_mirror,
        "work_units": {"searching_entries": int(units.size), "median": pct(50), "p90": pct(90), "p99": pct(99),
                       "p999": pct(99.9), "max": int(units.max()) if units.size else 0,
                       "above_2^16": int((units > (1 << 16)).sum())},
        "workspace_bytes": batch * LEVELS * BYTES_PER_LEVEL, "batches": -(-M // batch),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=9_360_000)
    ap.add_argument("--edges", type=int, default=24)
    ap.add_argument("--pairs", type=int, default=5_000_000)
    ap.add_argument("--coverage", type=int, default=20)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--layers", type=int, default=4096)
    ap.add_argument("--ladder-reads", type=int, default=2_000_000)
    ap.add_argument("--ladder-pairs", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default="chain,ladder")
    ap.add_argument("--no-mirror", action="store_true", help="device only (profiler runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"shapes": [], "library": library_provenance()}
    for name in a.shapes.split(","):
        case = chain_case(a) if name == "chain" else ladder_case(a)
        res["shapes"].append(measure(name, case, a))
        print(json.dumps(res["shapes"][-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
