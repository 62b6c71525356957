#!/usr/bin/env python3
"""Host grouping against device grouping of the discovery rows into the
per-read lists D(A), at a bench.py configuration (default C3), on one GPU.

  (a) host:   mg_copy_rows, then mg::Discoveries::build (mgh_discoveries_build),
              timed separately;
  (b) device: mg_build_discoveries (device_ms = its HIP-event time),
              mg_copy_discoveries, then mg::Discoveries::from_lists
              (mgh_discoveries_check);
each a median over --repeats runs after one warm-up, (a) and (b) alternating;
then, once each, end to end through GraphReplay (rows -> mgh_graph_replay
against lists -> mgh_graph_replay_disc: the two positions of the drop-in's
switch), the device memory mg_build_discoveries adds, and np.array_equal of the
device lists against the host-built ones.  Writes one JSON document (--out).
Not part of bench.py."""
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

from metagenomics_amd import overlap, synth  # noqa: E402
from metagenomics_amd.overlap import (Dataset, OverlapEngine, check_discoveries, host_discoveries,  # noqa: E402
                                      replay_discoveries, replay_graph)

CONFIGS = {  # bench.py's: (n_reads, read_len, genome_len, l, k, seed)
    "c1": (100_000, 100, 500_000, 40, 21, 7),
    "c2": (1_000_000, 150, 7_500_000, 50, 31, 21),
    "c3": (10_000_000, 150, 75_000_000, 50, 31, 31),
}


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return r, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the Dataset build")
    ap.add_argument("--no-replay", action="store_true", help="skip the two end-to-end GraphReplay runs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disc_c3.json"))
    args = ap.parse_args()
    if overlap.device_count() < 1:
        sys.exit("disc_bench: no HIP device (there is no CPU path to measure)")
    import torch

    n, rl, G, l, k, seed = CONFIGS[args.config]
    codes, L = synth.uniform_read_set(n, 0, G, seed=seed, lo=rl, hi=rl)
    ds = Dataset.from_codes(codes, L, l, nthreads=args.threads)
    del codes
    lens = ds.packed()[1]
    log(f"[disc_bench] {args.config}: {ds.num_unique} unique reads")

    e = OverlapEngine(0)
    e.upload(ds)
    e.build_index(l, k)
    e.mark_contained(copy=False)
    n_rows = e.find_overlaps()
    torch.cuda.synchronize(0)
    free0 = torch.cuda.mem_get_info(0)[0]
    n_disc = e.build_discoveries()  # warm-up: allocates the list buffers, loads the kernels
    torch.cuda.synchronize(0)
    extra_bytes = free0 - torch.cuda.mem_get_info(0)[0]
    log(f"[disc_bench] rows {n_rows}, list records {n_disc}, device ms (first) {e.disc_ms:.2f}")

    rows = np.zeros(n_rows, dtype=overlap.EDGE_DTYPE)
    e.copy_rows_to(rows.ctypes.data, n_rows)  # warm-up (pages touched, the gather buffer allocated)
    host = {"copy_rows_s": [], "build_s": []}
    dev = {"device_ms": [], "build_call_s": [], "copy_s": [], "from_lists_s": []}
    h_start = h_disc = d_start = d_disc = None
    for r in range(args.repeats):
        _, t = timed(lambda: e.copy_rows_to(rows.ctypes.data, n_rows))
        host["copy_rows_s"].append(t)
        (h_start, h_disc), t = timed(lambda: host_discoveries(rows, lens, l))
        host["build_s"].append(t)
        _, t = timed(e.build_discoveries)
        dev["build_call_s"].append(t)
        dev["device_ms"].append(e.disc_ms)
        (d_start, d_disc), t = timed(e.discoveries)
        dev["copy_s"].append(t)
        rc, t = timed(lambda: check_discoveries(d_start, d_disc, lens, l))
        if rc:
            sys.exit(f"disc_bench: the device lists fail from_lists ({rc})")
        dev["from_lists_s"].append(t)
        log(f"[disc_bench] repeat {r}: host copy {host['copy_rows_s'][-1]:.3f} s + build {host['build_s'][-1]:.3f} s; "
            f"device {dev['device_ms'][-1]:.2f} ms (call {dev['build_call_s'][-1]:.3f} s) + copy "
            f"{dev['copy_s'][-1]:.3f} s + from_lists {dev['from_lists_s'][-1]:.3f} s")
    equal = bool(np.array_equal(h_start, d_start) and np.array_equal(h_disc, d_disc))
    log(f"[disc_bench] device lists == host lists: {equal}")
    del h_start, h_disc

    med = statistics.median
    res = {
        "tool": "tools/disc_bench.py", "config": args.config, "repeats": args.repeats,
        "unique_reads": int(ds.num_unique), "rows": int(n_rows), "list_records": int(n_disc),
        "host_grouping": {"copy_rows_s": med(host["copy_rows_s"]), "discoveries_build_s": med(host["build_s"]),
                          "total_s": med([a + b for a, b in zip(host["copy_rows_s"], host["build_s"])]),
                          "samples": host},
        "device_grouping": {"device_ms": med(dev["device_ms"]), "build_call_s": med(dev["build_call_s"]),
                            "copy_discoveries_s": med(dev["copy_s"]), "from_lists_s": med(dev["from_lists_s"]),
                            "total_s": med([a + b + c for a, b, c in
                                            zip(dev["build_call_s"], dev["copy_s"], dev["from_lists_s"])]),
                            "samples": dev},
        "extra_device_bytes": int(extra_bytes),
        "lists_equal_host": equal,
    }
    if not args.no_replay:
        # the drop-in's two switch positions, end to end from the rows on the device to the replayed graph
        def via_host():
            r = e.rows(n_rows)
            return replay_graph(r, lens, l)[:2]

        def via_device():
            e.build_discoveries()
            s, d = e.discoveries()
            return replay_discoveries(s, d, lens, l)[:2]

        del rows, d_start, d_disc
        g_dev, t_dev = timed(via_device)
        g_host, t_host = timed(via_host)
        res["graph_replay_end_to_end"] = {"host_grouping_s": t_host, "device_grouping_s": t_dev,
                                          "nodes_edges_host": list(g_host), "nodes_edges_device": list(g_dev),
                                          "same_graph": g_host == g_dev, "runs": 1}
        log(f"[disc_bench] end to end: host {t_host:.2f} s, device {t_dev:.2f} s, same graph {g_host == g_dev}")
    e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k2: v for k2, v in res.items() if k2 != "samples"}))
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
