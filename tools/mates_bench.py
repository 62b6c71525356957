#!/usr/bin/env python3
"""The mate-pair path on the device against its host mirror, on C3-shaped
paired input (bench.py's c3 reads taken two by two as pairs, one FASTQ file),
on one GPU.  Reported separately, each a median over --repeats runs after one
warm-up, device and host alternating in one process:

  reader           mgh_read_pairs (serial, storeMatePairInformation's loop)
  h2d              the records' bytes and offsets, pageable host memory -> device
  find_reads       mg_find_reads device_ms (filter + pack + binary search) and
                   the call's wall time (with its transfers)
  build            mg_build_mate_pairs device_ms and the call's wall time
  download         mg_copy_mate_pairs
  host_mirror      mgh_mate_pairs_build on one thread over the same parsed pairs

and np.array_equal of the two results in the same run.  Writes one JSON
document (--out).  Not part of bench.py."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metagenomics_amd import overlap, synth  # noqa: E402
from metagenomics_amd.overlap import OverlapEngine, host_mate_pairs, read_pairs  # noqa: E402

C3 = (10_000_000, 150, 150, 75_000_000, 50, 31, 31)  # bench.py's c3: n_reads, lo, hi, genome, l, k, seed


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return r, time.perf_counter() - t0


def write_fastq(path, codes, lens, chunk=500_000):
    """Reads 2p, 2p + 1 = pair p; fixed-width records written in chunks."""
    n, w = codes.shape
    assert int(lens.min()) == int(lens.max()) == w
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(path, "wb") as f:
        for a in range(0, n, chunk):
            b = min(n, a + chunk)
            rec = np.empty((b - a, 2 * w + 7), dtype=np.uint8)
            rec[:, 0], rec[:, 1], rec[:, 2] = ord("@"), ord("r"), ord("\n")
            rec[:, 3:3 + w] = acgt[codes[a:b]]
            rec[:, 3 + w:6 + w] = np.frombuffer(b"\n+\n", dtype=np.uint8)
            rec[:, 6 + w:6 + 2 * w] = ord("I")
            rec[:, 6 + 2 * w] = ord("\n")
            f.write(rec.tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=C3[0] // 2, help="pairs (default: c3's 5M)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="device part only (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or os.path.join(ROOT, "profiles", "mates_c3.json")
    if overlap.device_count() < 1:
        sys.exit("mates_bench: no HIP device (there is no CPU path to measure)")
    import torch

    n, lo, hi, G, l, k, seed = C3
    scale = 2 * args.pairs / n
    n, G = 2 * args.pairs, max(10_000, int(G * scale))
    codes, L = synth.uniform_read_set(n, 0, G, seed=seed, lo=lo, hi=hi)
    tmp = tempfile.mkdtemp(prefix="mates_bench_")
    fq = os.path.join(tmp, "pairs.fq")
    write_fastq(fq, codes, L)
    del codes
    size = os.path.getsize(fq)
    log(f"[mates_bench] {args.pairs} pairs, {size / 1e9:.2f} GB FASTQ")

    med = statistics.median
    t_reader = []
    for _ in range(args.repeats):
        (text, off, ppd, _), t = timed(lambda: read_pairs([fq]))
        t_reader.append(t)
    os.unlink(fq)
    os.rmdir(tmp)
    n_raw = off.shape[0] - 1
    log(f"[mates_bench] reader {med(t_reader):.2f} s, {n_raw} raw mates ({int(ppd[0])} pairs: the trailing newline adds one)")

    e = OverlapEngine(0)
    nu = e.ingest_ascii(text=text, offsets=off, min_overlap=l)
    e.build_index(l, k)
    e.mark_contained(copy=False)
    words, lens = e.download_packed()
    log(f"[mates_bench] {nu} unique reads resident")

    def h2d():
        a = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy())
        b = torch.from_numpy(off.view(np.int64))
        torch.cuda.synchronize(0)
        t0 = time.perf_counter()
        a.cuda()
        b.cuda()
        torch.cuda.synchronize(0)
        return time.perf_counter() - t0

    S = {k2: [] for k2 in ("h2d_s", "find_device_ms", "find_call_s", "build_device_ms", "build_call_s", "download_s",
                          "host_mirror_s")}
    same = True

    def device(record):
        t_h = h2d()
        _, t_f = timed(lambda: e.find_reads(text=text, offsets=off, min_overlap=l))
        _, t_b = timed(lambda: e.build_mate_pairs(text, off, ppd, l, True))
        r, t_d = timed(e.mate_lists)
        if record:
            S["h2d_s"].append(t_h)
            S["find_device_ms"].append(e.find_ms)
            S["find_call_s"].append(t_f)
            S["build_device_ms"].append(e.mates_ms)
            S["build_call_s"].append(t_b)
            S["download_s"].append(t_d)
        return r

    def host(record):
        r, t = timed(lambda: host_mate_pairs(words, lens, text, off, ppd, l, None))  # (one length: superReadIDs all 0)
        if record:
            S["host_mirror_s"].append(t)
        return r

    dev = device(False)  # warm-up: kernels loaded, buffers sized, pages touched
    for r in range(args.repeats):
        dev = device(True)
        log(f"[mates_bench] repeat {r}: h2d {S['h2d_s'][-1]:.3f} s, find {S['find_device_ms'][-1]:.1f} ms device / "
            f"{S['find_call_s'][-1]:.3f} s call, build {S['build_device_ms'][-1]:.1f} ms device / "
            f"{S['build_call_s'][-1]:.3f} s call, download {S['download_s'][-1]:.3f} s")
        if not args.no_host:
            h = host(True)
            same = same and bool(np.array_equal(dev[0], h[0]) and np.array_equal(dev[1], h[1]))
            same = same and (e.good_pairs, e.bad_pairs) == h[2:]
            log(f"[mates_bench] repeat {r}: host mirror {S['host_mirror_s'][-1]:.2f} s, equal {same}")
    res = {
        "tool": "tools/mates_bench.py", "pairs": int(ppd[0]), "raw_mates": int(n_raw), "fastq_bytes": int(size),
        "read_length": lo, "l": l, "unique_reads": int(nu), "list_records": int(dev[1].shape[0]),
        "good_pairs": e.good_pairs, "bad_pairs": e.bad_pairs, "repeats": args.repeats,
        "reader_s": med(t_reader),
        **{k2: med(v) for k2, v in S.items() if v},
        "same_lists": same if not args.no_host else None,
        "samples": {"reader_s": t_reader, **S},
    }
    if S["host_mirror_s"]:
        res["device_path_s"] = res["build_call_s"] + res["download_s"]
        res["speedup_over_host_mirror"] = res["host_mirror_s"] / res["device_path_s"]
    e.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
