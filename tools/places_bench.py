#!/usr/bin/env python3
"""Read placements, insert sizes and edge coverage at C3 shape: the three device
calls (mg_build_placements, mg_insert_sizes, mg_edge_coverage) against their
host mirrors.

The C3-shaped chain set of tools/contig_bench.py: --reads 150-bp reads (default
9.36M) on --edges unitig edges (24), the reads of an edge at starts drawn
uniformly at --coverage (20x) over the edge's stretch of genome; and --pairs
mate pairs (5M): both mates on one edge, the second 20-110 list positions after
the first (insert sizes of 150-830 bases on average), both directions listed, as
Read::addMatePair leaves them.  Frequencies are 1-3.  Only lengths, offsets and
IDs matter to the kernels, so the packed words are zeros.

Reports, as medians of --repeats alternating repeats after one warm-up:
  *_device_ms  the call's HIP-event time (kernels, scans, sort; no transfers of
               the inputs and results)
  *_call_ms    wall time of the call (adds the H2D of its inputs, the host
               reads between kernels and the D2H of its results)
  *_mirror_ms  wall time of the host mirror on the same box
and the bytes each call's work implies.  device == mirror is checked array for
array on the first repeat.  Writes the JSON to --out with the library's sha256
as tools/pmc_summary.py records it.
"""
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
from metagenomics_amd.overlap import (MATE_DTYPE, OverlapEngine, host_edge_coverage, host_insert_size_sums,  # noqa: E402
                                      host_placements)
from pmc_summary import library_provenance  # noqa: E402


def mate_set(edges, reads, n_reads, n_pairs, seed):
    """a mate CSR of 2 * n_pairs entries: pairs of list reads of one edge, 20-110 positions apart"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, edges.shape[0], n_pairs)
    first, m = edges["first"][k].astype(np.int64), edges["n"][k].astype(np.int64)
    gap = rng.integers(20, 111, n_pairs)
    i = (rng.random(n_pairs) * (m - gap)).astype(np.int64)
    a, b = reads[first + i], reads[first + i + gap]
    owner = np.concatenate([a, b])
    mate = np.concatenate([b, a])
    order = np.argsort(owner, kind="stable")
    recs = np.zeros(2 * n_pairs, dtype=MATE_DTYPE)
    recs["id"] = mate[order]
    recs["orient"] = rng.integers(0, 4, 2 * n_pairs)
    start = np.zeros(n_reads + 2, dtype=np.uint64)
    start[1:] = np.cumsum(np.bincount(owner, minlength=n_reads + 1))
    return start, recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=9_360_000)
    ap.add_argument("--edges", type=int, default=24)
    ap.add_argument("--pairs", type=int, default=5_000_000)
    ap.add_argument("--coverage", type=int, default=20)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--layout", type=int, default=1)
    ap.add_argument("--no-mirror", action="store_true", help="device only (profiler runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    words, lens, edges, reads, offs, ors = chain_set(a.reads, a.edges, a.coverage, a.read_len, 11)
    words[:] = 0
    n = lens.shape[0]
    mates = mate_set(edges, reads, n, a.pairs, 12)
    freq = np.random.default_rng(13).integers(1, 4, n).astype(np.uint32)
    eng = OverlapEngine(0)
    eng.set_option("layout", a.layout)
    eng.upload_packed(words, lens)

    def timed(f):
        t0 = time.perf_counter()
        r = f()
        return r, (time.perf_counter() - t0) * 1e3

    eng.build_placements(edges, reads, offs, ors)  # warm-up: buffers sized
    eng.insert_size_sums(1, mates)
    eng.edge_coverage(freq)
    dev, mir = [], []
    for rep in range(a.repeats):
        _, t_b = timed(lambda: eng.build_placements(edges, reads, offs, ors))
        d_b = eng.places_ms
        sums, t_i = timed(lambda: eng.insert_size_sums(1, mates))
        d_i = eng.insert_ms
        cov, t_c = timed(lambda: eng.edge_coverage(freq))
        d_c = eng.coverage_ms
        dev.append((d_b, t_b, d_i, t_i, d_c, t_c))
        if a.no_mirror:
            continue
        (hs, hr, _), m_b = timed(lambda: host_placements(n, edges, reads, offs, ors))
        hsum, m_i = timed(lambda: host_insert_size_sums((hs, hr), mates, 1))
        hcov, m_c = timed(lambda: host_edge_coverage(lens, freq, edges, reads, offs, ors))
        mir.append((m_b, m_i, m_c))
        if rep == 0:
            ds, dr = eng.placements()
            assert np.array_equal(ds, hs) and np.array_equal(dr, hr), "placements: device != mirror"
            assert np.array_equal(sums, hsum) and int(sums[0, 0]) > 0, "insert sizes: device != mirror"
            assert np.array_equal(cov, hcov) and int(cov[:, 0].min()) > 0, "coverage: device != mirror"
    med = lambda v: statistics.median(v) if v else None
    E, M = int(reads.shape[0]), int(mates[1].shape[0])
    bases = int((edges["offset"].astype(np.int64) + a.read_len + 1).sum())
    res = {
        "reads": n, "edges": a.edges, "list_entries": E, "mate_entries": M, "coverage_counters": bases,
        "read_len": a.read_len, "layout": a.layout, "repeats": a.repeats,
        "insert_sizes": int(sums[0, 0]),
        "placements_device_ms": med([d[0] for d in dev]), "placements_call_ms": med([d[1] for d in dev]),
        "insert_device_ms": med([d[2] for d in dev]), "insert_call_ms": med([d[3] for d in dev]),
        "coverage_device_ms": med([d[4] for d in dev]), "coverage_call_ms": med([d[5] for d in dev]),
        "placements_mirror_ms": med([m[0] for m in mir]), "insert_mirror_ms": med([m[1] for m in mir]),
        "coverage_mirror_ms": med([m[2] for m in mir]),
        "all_device": dev, "all_mirror": mir, "checked_equal": not a.no_mirror,
        # what each call's work implies (bytes): per list entry the three list arrays, the entry-space arrays
        # written and read again, the scan, three sort passes of 8-B pairs and the 16-B record; per mate entry
        # its 8-B record, two starts and about two 16-B placement records per side; per counter the delta word
        # zeroed, scanned (read + write) and reduced, plus two atomics per list entry
        "implied_bytes": {"placements": E * (7 + 17 + 16 + 16 + 3 * 16 + 16) + 8 * (n + 2),
                          "insert_sizes": M * (8 + 4 * 16 + 32), "coverage": bases * 8 * 4 + E * (16 + 16)},
        "library": library_provenance(),
    }
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
