#!/usr/bin/env python3
"""Contig strings at C3 shape: mg_build_contigs against the host mirror.

A C3-shaped chain set: --reads 150-bp reads (default 9.36M) on --edges unitig
edges (24), the reads of an edge at starts drawn uniformly at --coverage (20x)
over the edge's stretch of genome, so a list piece contributes ~7.5 bases.  The
packed words are random: the work of every kernel depends on lengths and
offsets only, and device == mirror is checked byte for byte on the first repeat.

Reports, as medians of --repeats alternating repeats after one warm-up:
  device_ms    mg_build_contigs' HIP-event time (length kernel, scan, starts, copy kernel)
  build_ms     wall time of mg_build_contigs (adds the lists' H2D and two host reads)
  copy_out_ms  wall time of mg_copy_contigs (the strings' D2H)
  mirror_ms    wall time of the host mirror (mgh_contigs_build, sizes + bases)
and the bytes the copy kernel's work implies: one 64-B slot line per piece plus
the output stream.  Writes the JSON to --out.  (The reference's own string
building is quadratic in the contig length and is not timed.)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metagenomics_amd.overlap import CONTIG_EDGE_DTYPE, OverlapEngine, _ptr, lib  # noqa: E402


def chain_set(n_reads, n_edges, coverage, rl, seed):
    rng = np.random.default_rng(seed)
    per = n_reads // n_edges
    span = per * rl // coverage
    edges = np.zeros(n_edges, dtype=CONTIG_EDGE_DTYPE)
    offs = np.zeros(n_edges * (per - 2), dtype=np.uint16)
    reads = np.zeros(n_edges * (per - 2), dtype=np.uint32)
    for k in range(n_edges):
        s = np.sort(rng.integers(0, span, per))
        d = np.minimum(np.diff(s), rl)
        a, m = k * (per - 2), per - 2
        ids = k * per + 1 + rng.permutation(per)  # the edge's reads lie anywhere among its IDs
        edges[k] = (ids[0], ids[-1], int(d.sum()), a, m, int(d[-1]), int(rng.integers(0, 4)))
        reads[a:a + m] = ids[1:-1]
        offs[a:a + m] = d[:-1]
    ors = rng.integers(0, 2, reads.shape[0]).astype(np.uint8)
    n = per * n_edges
    wpr = (rl + 31) // 32
    words = rng.integers(0, np.iinfo(np.uint64).max, (n, wpr), dtype=np.uint64, endpoint=True)
    if rl % 32:
        words[:, -1] &= ~np.uint64(0) << np.uint64(64 - 2 * (rl % 32))
    return words, np.full(n, rl, np.uint16), edges, reads, offs, ors


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=9_360_000)
    ap.add_argument("--edges", type=int, default=24)
    ap.add_argument("--coverage", type=int, default=20)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--layout", type=int, default=1)
    ap.add_argument("--no-mirror", action="store_true", help="device only (profiler runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = lib()
    words, lens, edges, reads, offs, ors = chain_set(a.reads, a.edges, a.coverage, a.read_len, 11)
    n = lens.shape[0]
    eng = OverlapEngine(0)
    eng.set_option("layout", a.layout)
    eng.upload_packed(words, lens)
    start_d = np.zeros(a.edges + 1, np.uint64)
    start_h = np.zeros(a.edges + 1, np.uint64)
    total, ms, got = C.c_uint64(), C.c_float(), C.c_uint64()

    def device(out):
        t0 = time.perf_counter()
        eng._check(L.mg_build_contigs(eng._h, _ptr(edges), a.edges, _ptr(reads), _ptr(offs), _ptr(ors),
                                      reads.shape[0], C.byref(total), C.byref(ms)), "build_contigs")
        t1 = time.perf_counter()
        eng._check(L.mg_copy_contigs(eng._h, _ptr(start_d), _ptr(out), out.shape[0], C.byref(got)), "copy_contigs")
        t2 = time.perf_counter()
        return float(ms.value), (t1 - t0) * 1e3, (t2 - t1) * 1e3

    def mirror(out):
        t0 = time.perf_counter()
        rc = L.mgh_contigs_build(_ptr(words), _ptr(lens), n, words.shape[1], _ptr(edges), a.edges, _ptr(reads),
                                 _ptr(offs), _ptr(ors), reads.shape[0], _ptr(start_h), _ptr(out), out.shape[0],
                                 C.byref(got), None, 0)
        assert rc == 0, rc
        return (time.perf_counter() - t0) * 1e3

    eng._check(L.mg_build_contigs(eng._h, _ptr(edges), a.edges, _ptr(reads), _ptr(offs), _ptr(ors), reads.shape[0],
                                  C.byref(total), C.byref(ms)), "build_contigs")  # warm-up: buffers sized
    nbytes = int(total.value)
    out_d = np.zeros(nbytes, np.uint8)
    out_h = np.zeros(nbytes, np.uint8)
    dev, mir = [], []
    for rep in range(a.repeats):
        dev.append(device(out_d))
        if not a.no_mirror:
            mir.append(mirror(out_h))
            if rep == 0:
                assert np.array_equal(start_d, start_h) and np.array_equal(out_d, out_h), "device != mirror"
                assert int(start_d[-1]) == nbytes and np.isin(out_d, np.frombuffer(b"ACGTN", np.uint8)).all()
    pieces = reads.shape[0] + 2 * a.edges
    med = lambda v: statistics.median(v) if v else None
    res = {
        "reads": n, "edges": a.edges, "pieces": pieces, "read_len": a.read_len, "coverage": a.coverage,
        "layout": a.layout, "total_bases": nbytes, "bases_per_piece": nbytes / pieces, "repeats": a.repeats,
        "device_ms": med([d[0] for d in dev]), "build_ms": med([d[1] for d in dev]),
        "copy_out_ms": med([d[2] for d in dev]), "end_to_end_ms": med([d[1] + d[2] for d in dev]),
        "mirror_ms": med(mir), "all_device_ms": [d[0] for d in dev], "all_mirror_ms": mir,
        "checked_equal": not a.no_mirror,
        # what the copy kernel's work implies: a 64-B slot line per piece, 17 B of piece records, the output
        "implied_bytes": {"slot_lines": 64 * pieces, "piece_records": 17 * pieces + 8, "output": nbytes},
    }
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
