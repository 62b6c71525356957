#!/usr/bin/env python3
"""Component labelling on the device and the parallel replay of the components
against the serial replay, at a bench.py configuration, on one GPU.

  device:     mg_build_components' device_ms beside mg_build_discoveries' from
              the same run, and the device memory the component buffers add;
  end to end, from the lists on the device to the replayed graph:
    (a) serial:   mg_copy_discoveries, mgh_graph_replay_disc;
    (b) parallel: mg_copy_discoveries, mg_build_components, mg_copy_components,
                  mgh_graph_replay_comp (validation + replay on --replay-threads
                  host threads);
each timed up to the graph handle (copying the list rows out for the comparison
and releasing the handle are the same code after either and stay outside), a
median over --repeats runs after one warm-up, (a) and (b) alternating in one
process, with np.array_equal of the two graphs' list rows, the component
count, the largest component's share s of the records, the bound
1 / max(s, 1 / threads) on the speed-up and the fraction of it achieved.
Writes one JSON document (--out).  Not part of bench.py."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metagenomics_amd import overlap, synth  # noqa: E402
from metagenomics_amd.overlap import Dataset, OverlapEngine, _ptr, _replay_disc, check_discoveries  # noqa: E402

CONFIGS = {  # bench.py's: (n_reads, lo, hi, genome_len, l, k, seed, genomes (0 = one uniform genome))
    "c1": (100_000, 100, 100, 500_000, 40, 21, 7, 0),
    "c2": (1_000_000, 150, 150, 7_500_000, 50, 31, 21, 0),
    "c3": (10_000_000, 150, 150, 75_000_000, 50, 31, 31, 0),
    "c5s": (5_000_000, 100, 250, 43_750_000, 50, 31, 55, 100),
    "c5": (50_000_000, 100, 250, 437_500_000, 50, 31, 55, 100),
}


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return r, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c5s", choices=sorted(CONFIGS))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the Dataset build")
    ap.add_argument("--replay-threads", type=int, default=16, help="host threads of the parallel replay")
    ap.add_argument("--no-replay", action="store_true", help="device part only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or os.path.join(ROOT, "profiles", f"comp_{args.config}.json")
    if overlap.device_count() < 1:
        sys.exit("comp_bench: no HIP device (there is no CPU path to measure)")
    import torch

    n, lo, hi, G, l, k, seed, genomes = CONFIGS[args.config]
    if genomes:
        codes, L = synth.metagenome_read_set(n, lo, hi, genomes, G, seed)
    else:
        codes, L = synth.uniform_read_set(n, 0, G, seed=seed, lo=lo, hi=hi)
    ds = Dataset.from_codes(codes, L, l, nthreads=args.threads)
    del codes
    lens = ds.packed()[1]
    log(f"[comp_bench] {args.config}: {ds.num_unique} unique reads")

    e = OverlapEngine(0)
    e.upload(ds)
    e.build_index(l, k)
    e.mark_contained(copy=False)
    n_rows = e.find_overlaps()
    n_disc = e.build_discoveries()
    torch.cuda.synchronize(0)
    free0 = torch.cuda.mem_get_info(0)[0]
    n_comp = e.build_components()  # warm-up: allocates the component buffers, loads the kernels
    torch.cuda.synchronize(0)
    extra_bytes = free0 - torch.cuda.mem_get_info(0)[0]
    _, comps = e.components()
    share = float(comps["n_disc"].max()) / n_disc if n_comp else 1.0
    bound = 1.0 / max(share, 1.0 / args.replay_threads)
    log(f"[comp_bench] rows {n_rows}, list records {n_disc}, components {n_comp}, largest share {share:.4f}, "
        f"device ms (first) {e.comp_ms:.2f}")

    dev = {"disc_device_ms": [], "comp_device_ms": [], "comp_call_s": []}
    for _ in range(args.repeats):
        e.build_discoveries()
        dev["disc_device_ms"].append(e.disc_ms)
        _, t = timed(e.build_components)
        dev["comp_call_s"].append(t)
        dev["comp_device_ms"].append(e.comp_ms)
    med = statistics.median
    res = {
        "tool": "tools/comp_bench.py", "config": args.config, "repeats": args.repeats,
        "unique_reads": int(ds.num_unique), "rows": int(n_rows), "list_records": int(n_disc),
        "components": int(n_comp), "largest_component_records": int(comps["n_disc"].max()) if n_comp else 0,
        "largest_component_reads": int(comps["n_reads"][np.argmax(comps["n_disc"])]) if n_comp else 0,
        "largest_share": share, "replay_threads": args.replay_threads, "speedup_bound": bound,
        "device": {"discoveries_device_ms": med(dev["disc_device_ms"]), "components_device_ms": med(dev["comp_device_ms"]),
                   "components_call_s": med(dev["comp_call_s"]), "samples": dev},
        "extra_device_bytes": int(extra_bytes),
    }
    ok = True
    if not args.no_replay:
        parts = {"copy_lists_s": [], "comp_build_copy_s": [], "replay_s": []}

        def graph_of(g):
            """(nodes, edges, list rows) of a handle, and its release: the same code after either replay, not timed"""
            L = overlap.lib()
            cnt = int(L.mgh_graph_rows(g, None, 0))
            out = np.zeros(cnt, dtype=overlap.EDGE_DTYPE)
            L.mgh_graph_rows(g, _ptr(out), cnt)
            r = int(L.mgh_graph_nodes(g)), int(L.mgh_graph_edges(g)), out
            L.mgh_graph_free(g)
            return r

        def serial():
            def run():
                s, d = e.discoveries()
                return _replay_disc(s, d, lens, l)

            g, t = timed(run)
            return graph_of(g), t

        def parallel():
            (s, d), t0 = timed(e.discoveries)

            def table():
                e.build_components()
                return e.components()

            c, t1 = timed(table)
            g, t2 = timed(lambda: _replay_disc(s, d, lens, l, c, args.replay_threads))
            parts["copy_lists_s"].append(t0)
            parts["comp_build_copy_s"].append(t1)
            parts["replay_s"].append(t2)
            return graph_of(g), t0 + t1 + t2

        def split(components, threads):
            """One replay taken apart: the lists' validation pass alone, the replay call (that pass, the
            table's validation and the replay), the copy of the list rows out, the release of the graph."""
            L = overlap.lib()
            s, d = e.discoveries()
            _, t_lists = timed(lambda: check_discoveries(s, d, lens, l))
            g, t_call = timed(lambda: _replay_disc(s, d, lens, l, components, threads))
            cnt = int(L.mgh_graph_rows(g, None, 0))
            out = np.zeros(cnt, dtype=overlap.EDGE_DTYPE)
            _, t_rows = timed(lambda: L.mgh_graph_rows(g, _ptr(out), cnt))
            _, t_free = timed(lambda: L.mgh_graph_free(g))
            return {"from_lists_s": t_lists, "replay_call_s": t_call, "rows_out_s": t_rows, "free_s": t_free}

        g_ser, _ = serial()  # warm-up (pages touched)
        g_par, _ = parallel()
        for v in parts.values():
            v.clear()
        same = g_ser[:2] == g_par[:2] and bool(np.array_equal(g_ser[2], g_par[2]))
        nodes_edges = list(g_ser[:2])
        del g_ser, g_par
        t_ser, t_par = [], []
        for r in range(args.repeats):
            g, t = serial()
            t_ser.append(t)
            same = same and g[:2] == tuple(nodes_edges)
            del g
            g, t = parallel()
            t_par.append(t)
            same = same and g[:2] == tuple(nodes_edges)
            del g
            log(f"[comp_bench] repeat {r}: serial {t_ser[-1]:.3f} s, parallel {t_par[-1]:.3f} s (lists "
                f"{parts['copy_lists_s'][-1]:.3f} + table {parts['comp_build_copy_s'][-1]:.3f} + validation and "
                f"replay {parts['replay_s'][-1]:.3f})")
        speedup = med(t_ser) / med(t_par)
        res["end_to_end"] = {
            "serial_s": med(t_ser), "parallel_s": med(t_par), "serial_spread_s": max(t_ser) - min(t_ser),
            "speedup": speedup, "fraction_of_bound": speedup / bound,
            "parallel_parts_s": {k2: med(v) for k2, v in parts.items()},
            "nodes_edges": nodes_edges, "same_graph": same,
            "samples": {"serial_s": t_ser, "parallel_s": t_par, **parts},
        }
        # where the time goes: the serial replay and the parallel one at 2 .. replay-threads threads, once each
        table = e.components()
        res["split"] = {"serial": split(None, 0)}
        t = 2 if share < 0.9 else args.replay_threads  # (one giant component: the thread count changes nothing)
        while t <= args.replay_threads:
            res["split"][f"threads_{t}"] = split(table, t)
            t *= 2
        for k2, v in res["split"].items():
            log(f"[comp_bench] {k2}: " + ", ".join(f"{a} {b:.3f}" for a, b in v.items()))
        ok = same
        log(f"[comp_bench] end to end: serial {med(t_ser):.2f} s, parallel {med(t_par):.2f} s, speed-up {speedup:.2f} "
            f"of a bound of {bound:.2f}; same graph {same}")
    e.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
