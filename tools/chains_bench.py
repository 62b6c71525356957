#!/usr/bin/env python3
"""The contraction of a freshly replayed graph with and without the safe chains
contracted first, at a bench.py configuration, on one GPU, in one process.

From an uncontracted graph handle to the contracted one:
  (a) loop:   mgh_graph_contract (the reference's loop alone);
  (b) host:   mgh_graph_simple_csr, mgh_chains_build (the host's serial walk),
              mgh_graph_contract_chains (validation, apply, loop);
  (c) device: mgh_graph_simple_csr, mg_build_chains (upload + kernels),
              mg_copy_chains, mgh_graph_contract_chains; split into export,
              the build call with its device_ms (the rest of the call is the
              upload and the round trips), the copy, and apply + loop.
--repeats alternating runs of each after one warm-up of each.  The graph is
replayed once from the device's lists and components; every run gets a handle of
its own rebuilt from that graph's CSR (mgh_graph_from_csr, outside the times).
Every run's contracted graph (edges in list order, read lists, location lists,
counters, iterations) must be identical.  Writes one JSON document (--out).
Not part of bench.py."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metagenomics_amd import overlap, synth  # noqa: E402
from metagenomics_amd.overlap import (Dataset, OverlapEngine, UnitigGraph, _graph_csr, _ptr, _replay_disc,  # noqa: E402
                                      host_chains)

CONFIGS = {  # bench.py's: (n_reads, lo, hi, genome_len, l, k, seed, genomes (0 = one uniform genome))
    "c1": (100_000, 100, 100, 500_000, 40, 21, 7, 0),
    "c2": (1_000_000, 150, 150, 7_500_000, 50, 31, 21, 0),
    "c3": (10_000_000, 150, 150, 75_000_000, 50, 31, 31, 0),
    "c5s": (5_000_000, 100, 250, 43_750_000, 50, 31, 55, 100),
}


def log(*a):
    print(*a, file=sys.stderr, flush=True)


class Run(UnitigGraph):
    """a handle rebuilt from the CSR, contracted by one of the three ways"""

    def __init__(self, start, edges):
        self._L = overlap.lib()
        self._g = C.c_void_p()
        rc = self._L.mgh_graph_from_csr(_ptr(start), _ptr(edges), start.shape[0] - 2, edges.shape[0],
                                        C.byref(self._g))
        if rc:
            raise SystemExit(f"chains_bench: mgh_graph_from_csr failed ({rc})")
        self.n_reads = start.shape[0] - 2
        self.parts = {}

    def _timed(self, key, f):
        t0 = time.perf_counter()
        r = f()
        self.parts[key] = time.perf_counter() - t0
        return r

    def _finish(self, chains):
        it, merged, dead = C.c_uint64(), C.c_uint64(), C.c_uint64()
        if chains is None:
            rc = self._L.mgh_graph_contract(self._g, 1, C.byref(it), C.byref(merged), C.byref(dead))
        else:
            t, r, o, d = chains.arrays()
            rc = self._L.mgh_graph_contract_chains(self._g, _ptr(t), t.shape[0], _ptr(r), _ptr(o), _ptr(d), r.shape[0],
                                                   1, C.byref(it), C.byref(merged), C.byref(dead))
        if rc:
            raise SystemExit(f"chains_bench: contraction failed ({rc})")
        self.iterations, self.merged, self.dead_end_nodes = it.value, merged.value, dead.value

    def loop(self):
        self._timed("loop_s", lambda: self._finish(None))

    def host(self):
        csr = self._timed("export_s", lambda: _graph_csr(self._g, self.n_reads))
        ch = self._timed("mirror_s", lambda: host_chains(*csr))
        self._timed("apply_loop_s", lambda: self._finish(ch))
        return ch

    def device(self, e):
        csr = self._timed("export_s", lambda: _graph_csr(self._g, self.n_reads))
        self._timed("build_call_s", lambda: e.build_chains(*csr))
        self.parts["device_ms"] = e.chains_ms
        ch = self._timed("copy_s", e.chains)
        self._timed("apply_loop_s", lambda: self._finish(ch))
        return ch

    def digest(self):
        h = hashlib.sha256()
        for a in self.unitig_edges():
            h.update(np.ascontiguousarray(a).tobytes())
        for a in self.location_lists() or ():
            h.update(np.ascontiguousarray(a).tobytes())
        h.update(repr((self.nodes, self.edges, self.iterations, self.merged, self.dead_end_nodes)).encode())
        return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c5s", choices=sorted(CONFIGS))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the Dataset build and the replay")
    ap.add_argument("--device-only", action="store_true", help="one (c) run and nothing else (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or os.path.join(ROOT, "profiles", f"chains_{args.config}.json")
    if overlap.device_count() < 1:
        sys.exit("chains_bench: no HIP device (there is no CPU path to measure)")
    n, lo, hi, G, l, k, seed, genomes = CONFIGS[args.config]
    if genomes:
        codes, L = synth.metagenome_read_set(n, lo, hi, genomes, G, seed)
    else:
        codes, L = synth.uniform_read_set(n, 0, G, seed=seed, lo=lo, hi=hi)
    ds = Dataset.from_codes(codes, L, l, nthreads=args.threads)
    del codes
    lens = ds.packed()[1]
    e = OverlapEngine(0)
    e.upload(ds)
    e.build_index(l, k)
    e.mark_contained(copy=False)
    e.find_overlaps()
    e.build_discoveries()
    e.build_components()
    t0 = time.perf_counter()
    g = _replay_disc(*e.discoveries(), lens, l, components=e.components(), threads=args.threads)
    replay_s = time.perf_counter() - t0
    start, edges = _graph_csr(g, lens.shape[0])
    overlap.lib().mgh_graph_free(g)
    log(f"[chains_bench] {args.config}: {ds.num_unique} reads, {edges.shape[0]} directed edges, replay {replay_s:.2f} s")

    if args.device_only:
        r = Run(start, edges)
        ch = r.device(e)
        log(f"[chains_bench] device only: {ch.info} {r.parts}")
        return
    ways = {"loop": lambda r: r.loop(), "host": lambda r: r.host(), "device": lambda r: r.device(e)}
    samples = {w: [] for w in ways}
    digests, info = set(), {}
    for rep in range(args.repeats + 1):  # the first round warms up
        for w, f in ways.items():
            r = Run(start, edges)
            t0 = time.perf_counter()
            ch = f(r)
            total = time.perf_counter() - t0
            if ch is not None:
                info[w] = ch.info
            digests.add(r.digest())
            counters = (r.nodes, r.edges, r.iterations, r.merged, r.dead_end_nodes)
            r.close()
            log(f"[chains_bench] round {rep} {w}: {total:.3f} s {r.parts}")
            if rep:
                samples[w].append(dict(r.parts, total_s=total))
    med = {w: statistics.median(s["total_s"] for s in samples[w]) for w in ways}
    loop_min = min(s["total_s"] for s in samples["loop"])
    dev = [s["total_s"] for s in samples["device"]]
    res = {
        "tool": "tools/chains_bench.py", "config": args.config, "repeats": args.repeats,
        "unique_reads": int(ds.num_unique), "directed_edges": int(edges.shape[0]), "replay_s": replay_s,
        "contracted": dict(zip(("nodes", "edges", "iterations", "merged", "dead_end_nodes"), map(int, counters))),
        "identical": len(digests) == 1, "chain_info": info, "median_total_s": med, "loop_min_s": loop_min,
        "device_below_loop_min": med["device"] < loop_min,
        "host_inside_device_spread": min(dev) <= med["host"] <= max(dev),
        "device_parts_median": {key: statistics.median(s[key] for s in samples["device"])
                                for key in samples["device"][0]},
        "host_parts_median": {key: statistics.median(s[key] for s in samples["host"]) for key in samples["host"][0]},
        "samples": samples,
    }
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k_: res[k_] for k_ in ("config", "identical", "median_total_s", "loop_min_s",
                                             "device_below_loop_min", "host_inside_device_spread",
                                             "device_parts_median", "host_parts_median", "chain_info")}))
    if not res["identical"]:
        sys.exit("chains_bench: the contracted graphs differ")


if __name__ == "__main__":
    main()
