// mg_scaffold.hip — scaffolder support: for every mate entry whether its two
// reads lie uniquely on two different edges close enough to each other, and the
// list of edge pairs so supported with their support and summed distance.  The
// definitions are in include/mg_overlap.h ("scaffolder"); csrc/host/mg_scaffold.cpp
// is the mirror.
//
// Reference path replaced (relative to the reference's MetaGenomics directory):
//   OverlapGraph::scaffolder   OverlapGraph.cpp:2120-2195 (up to the sort)
//
// mg_scaffold_pairs (one stream):
//   k_sc_twins / k_check_places / k_mate_owners (the last two from mg_stage.hpp,
//                 shared with mg_mate_paths): validation, the first offender of
//                 each kind kept by atomicMin; per mate entry its owner;
//   k_sc_score  : lane per mate entry.  Counts the placements of the wanted
//                 strand in A's and B's segments and stops at 2 (a repeat read
//                 can have a long segment), applies the bound and the same-edge
//                 test, leaves status, canonical key, dist and the record the
//                 entry would open.  The five status counters: ballot +
//                 popcount per wavefront, one integer atomic each;
//   aggregate   : ExclusiveSum of the counted flags -> k_sc_emit (counted
//                 entries compacted in entry order: index c ascends with t) ->
//                 stable SortPairs (key, c) over the bits E^2 needs ->
//                 k_run_heads -> ExclusiveSum -> k_sc_dist (dist in sorted
//                 order) -> 64-bit InclusiveSum -> k_sc_headrec (first index,
//                 run length by an upper bound, distance = difference of the
//                 scan at the run's ends, exact modulo 2^64) -> SortPairs of the
//                 heads by first index -> k_sc_pairs.  The sort is stable and c
//                 ascends, so a run's first element is where the reference
//                 first saw the pair; its edges are taken from that entry.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <string>

#include "mg_overlap.h"
#include "mg_stage.hpp"

namespace {

typedef unsigned long long ull;

__global__ __launch_bounds__(kThreads) void k_sc_twins(const uint32_t* __restrict__ twin, uint64_t n,
                                                       ull* __restrict__ bad) {
  const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k < n && twin[k] >= n) atomicMin(bad, (ull)k);
}

// the only placement of the wanted strand in [p0, p1): its count, capped at 2
__device__ __forceinline__ uint32_t only_place(const mg_place* __restrict__ places, uint64_t p0, uint64_t p1,
                                               uint32_t want, mg_place& out) {
  uint32_t n = 0;
  for (uint64_t p = p0; p < p1 && n < 2; ++p) {
    const mg_place pl = places[p];
    if ((pl.flags & 1u) != want) continue;
    if (!n) out = pl;
    ++n;
  }
  return n;
}

// Lane per mate entry t in [0, M]; lane M only closes the scan's input.
__global__ __launch_bounds__(kThreads) void k_sc_score(const uint32_t* __restrict__ twin, uint64_t n_edges,
                                                       const uint64_t* __restrict__ pstart,
                                                       const mg_place* __restrict__ places,
                                                       const mg_mate* __restrict__ mates,
                                                       const uint32_t* __restrict__ owner,
                                                       const uint64_t* __restrict__ mean,
                                                       const uint64_t* __restrict__ sd, uint64_t M,
                                                       uint8_t* __restrict__ status, uint32_t* __restrict__ sel,
                                                       uint64_t* __restrict__ key, uint64_t* __restrict__ dist,
                                                       uint64_t* __restrict__ rec, ull* __restrict__ counters) {
  const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  uint32_t st = 255;
  if (t < M) {
    const mg_mate mt = mates[t];
    const uint64_t a = owner[t];
    if (a > mt.id) {  // :2137
      st = MG_SCAF_SKIPPED;
    } else {
      const uint32_t want1 = (mt.orient == 0 || mt.orient == 1) ? 1u : 0u;  // :2149
      const uint32_t want2 = (mt.orient == 0 || mt.orient == 2) ? 1u : 0u;  // :2153
      mg_place pa{0, 0, 0}, pb{0, 0, 0};
      const uint32_t n1 = only_place(places, pstart[a], pstart[a + 1], want1, pa);
      const uint32_t n2 = only_place(places, pstart[mt.id], pstart[mt.id + 1], want2, pb);
      const uint64_t d = pa.distance + pb.distance;
      if (n1 != 1 || n2 != 1) {
        st = MG_SCAF_NOT_UNIQUE;
      } else if (!(d < mean[mt.dataset] + 3 * sd[mt.dataset])) {  // :2157 (mod 2^64)
        st = MG_SCAF_FAR;
      } else {
        const uint64_t t1 = twin[pa.edge], t2 = twin[pb.edge];
        if (pa.edge == pb.edge || pa.edge == t2) {  // :2161
          st = MG_SCAF_SAME_EDGE;
        } else {
          st = MG_SCAF_COUNTED;
          const uint64_t k1 = t1 * n_edges + pb.edge, k2 = t2 * n_edges + pa.edge;  // :2168, :2174
          key[t] = k1 < k2 ? k1 : k2;
          dist[t] = d;
          rec[t] = (t1 << 32) | pb.edge;  // :2185-2186
        }
      }
    }
    status[t] = (uint8_t)st;
  }
  if (t <= M) sel[t] = st == MG_SCAF_COUNTED;
#pragma unroll
  for (uint32_t i = 0; i < 5; ++i) {
    const ull n = (ull)__popcll(__ballot(st == i));
    if ((threadIdx.x & (kWave - 1)) == 0 && n) atomicAdd(&counters[i], n);
  }
}

__global__ __launch_bounds__(kThreads) void k_sc_emit(uint64_t M, const uint32_t* __restrict__ sel,
                                                      const uint32_t* __restrict__ idx,
                                                      const uint64_t* __restrict__ key,
                                                      const uint64_t* __restrict__ dist,
                                                      const uint64_t* __restrict__ rec, uint64_t* __restrict__ keys,
                                                      uint32_t* __restrict__ vals, uint64_t* __restrict__ cdist,
                                                      uint64_t* __restrict__ crec) {
  const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= M || !sel[t]) return;
  const uint32_t c = idx[t];
  keys[c] = key[t];
  vals[c] = c;
  cdist[c] = dist[t];
  crec[c] = rec[t];
}

__global__ __launch_bounds__(kThreads) void k_sc_dist(const uint32_t* __restrict__ vals,
                                                      const uint64_t* __restrict__ cdist, uint64_t C,
                                                      uint64_t* __restrict__ sdist) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < C) sdist[i] = cdist[vals[i]];
}

__global__ __launch_bounds__(kThreads) void k_sc_headrec(const uint64_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ vals, uint64_t C,
                                                         const uint32_t* __restrict__ head,
                                                         const uint32_t* __restrict__ hidx,
                                                         const uint64_t* __restrict__ cum, uint32_t* __restrict__ hseq,
                                                         uint32_t* __restrict__ hord, uint64_t* __restrict__ hsup,
                                                         uint64_t* __restrict__ hdist) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= C || !head[i]) return;
  const uint64_t key = keys[i];
  uint64_t lo = i + 1, hi = C;  // first index past the run
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (keys[mid] <= key) lo = mid + 1;
    else hi = mid;
  }
  const uint32_t h = hidx[i];
  hseq[h] = vals[i];  // the sort is stable and indices were emitted ascending: the run's first
  hord[h] = h;
  hsup[h] = lo - i;
  hdist[h] = cum[lo - 1] - (i ? cum[i - 1] : 0);  // (mod 2^64)
}

__global__ __launch_bounds__(kThreads) void k_sc_pairs(const uint32_t* __restrict__ hseq,
                                                       const uint32_t* __restrict__ hord,
                                                       const uint64_t* __restrict__ hsup,
                                                       const uint64_t* __restrict__ hdist,
                                                       const uint64_t* __restrict__ crec, uint64_t H,
                                                       mg_scaffold_pair* __restrict__ out) {
  const uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= H) return;
  const uint64_t e = crec[hseq[r]];
  const uint32_t h = hord[r];
  out[r] = mg_scaffold_pair{(uint32_t)(e >> 32), (uint32_t)e, hsup[h], hdist[h]};
}

}  // namespace

extern "C" {

int mg_scaffold_pairs(mg_ctx* ctx, const uint32_t* twin, uint64_t n_edges, uint64_t n_reads,
                      const uint64_t* place_start, const mg_place* places, const uint64_t* mate_start,
                      const mg_mate* mates, const uint64_t* mean, const uint64_t* sd, uint32_t n_datasets,
                      uint64_t* counters, uint64_t* n_pairs, float* device_ms) {
  if (!ctx) return -1;
  ctx->err.clear();
  if (n_pairs) *n_pairs = 0;
  if (device_ms) *device_ms = 0.f;
  if (counters) std::fill(counters, counters + 5, 0);
  ScaffoldStage& ss = ctx->scaffold;
  ss.ready = false;
  if ((n_edges && !twin) || (n_datasets && (!mean || !sd))) return set_err(ctx, "mg_scaffold_pairs: null argument");
  if (n_datasets > 256) return set_err(ctx, "mg_scaffold_pairs: more than 256 datasets (datasetNumber is UINT8)");
  if (n_edges >> 31) return set_err(ctx, "mg_scaffold_pairs: 2^31 or more edges are not supported");
  MG_TRY(hipSetDevice(ctx->device));
  if (whole_multiset(ctx, "mg_scaffold_pairs")) return -1;
  const uint64_t N = n_reads;
  hipStream_t st = ctx->stream;

  PairCsrs csr;
  if (const int rc = csr.take(ctx, "mg_scaffold_pairs", N, n_edges, place_start, places, mate_start, mates)) return rc;
  const uint64_t P = csr.P, M = csr.M;

  Scratch<uint32_t> d_twin, d_owner;
  Scratch<uint64_t> d_mean, d_sd;
  Scratch<ull> ctl;  // [0..2] first offenders, [3..7] the status counters
  MG_SCRATCH(d_twin, n_edges, "scaffold edge twins");
  MG_SCRATCH(d_owner, M, "mate entry owners");
  MG_SCRATCH(d_mean, n_datasets, "insert-size means");
  MG_SCRATCH(d_sd, n_datasets, "insert-size deviations");
  MG_SCRATCH(ctl, 8, "scaffold control words");
  if (n_edges) MG_TRY(hipMemcpyAsync(d_twin.p, twin, n_edges * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  if (n_datasets) {
    MG_TRY(hipMemcpyAsync(d_mean.p, mean, n_datasets * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    MG_TRY(hipMemcpyAsync(d_sd.p, sd, n_datasets * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  }
  MG_TRY(ctl_fill(st, ctl.p, 3, ~0ull));
  MG_TRY(ctl_fill(st, ctl.p + 3, 5, 0));

  // --- validation: nothing below indexes with an unchecked value
  if (n_edges) {
    hipLaunchKernelGGL(k_sc_twins, dim3(blocks_for(n_edges)), dim3(kThreads), 0, st, d_twin.p, n_edges, ctl.p);
    MG_TRY(hipGetLastError());
  }
  if (P) {
    hipLaunchKernelGGL(k_check_places<ull>, dim3(blocks_for(P)), dim3(kThreads), 0, st, csr.prec, P, n_edges, ctl.p + 1);
    MG_TRY(hipGetLastError());
  }
  if (M) {
    hipLaunchKernelGGL(k_mate_owners<ull>, dim3(blocks_for(M)), dim3(kThreads), 0, st, csr.mstart, csr.mrec, M, N,
                       n_datasets, d_owner.p, ctl.p + 2);
    MG_TRY(hipGetLastError());
  }
  ull bad[3] = {~0ull, ~0ull, ~0ull};
  MG_TRY(ctl_read(st, ctl.p, 3, bad));
  if (bad[0] != ~0ull) {
    ctx->err = "mg_scaffold_pairs: edge " + std::to_string(bad[0]) + ": its twin " + std::to_string(twin[bad[0]]) +
               " is not below " + std::to_string(n_edges) + " (-2)";
    return -2;
  }
  if (bad[1] != ~0ull) return bad_place(ctx, "mg_scaffold_pairs", csr.prec, bad[1], n_edges);
  if (bad[2] != ~0ull) return bad_mate(ctx, "mg_scaffold_pairs", bad[2], n_datasets, N);

  // --- score
  Scratch<uint32_t> sel, idx;
  Scratch<uint64_t> key, dist, rec;
  Scratch<uint8_t> tmp;
  MG_GROW(ss.status, M, "d_scaffold_status");
  MG_SCRATCH(sel, M + 1, "scaffold counted flags");
  MG_SCRATCH(idx, M + 1, "scaffold counted indices");
  MG_SCRATCH(key, M, "scaffold entry keys");
  MG_SCRATCH(dist, M, "scaffold entry distances");
  MG_SCRATCH(rec, M, "scaffold entry records");
  size_t tb = 0;
  MG_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, sel.p, idx.p, (int64_t)(M + 1), st));
  MG_SCRATCH(tmp, tb, "scaffold scan storage");
  MG_TRY(ss.ev.start(st));
  hipLaunchKernelGGL(k_sc_score, dim3(blocks_for(M + 1)), dim3(kThreads), 0, st, d_twin.p, n_edges, csr.pstart, csr.prec,
                     csr.mrec, d_owner.p, d_mean.p, d_sd.p, M, ss.status.p, sel.p, key.p, dist.p, rec.p, ctl.p + 3);
  MG_TRY(hipGetLastError());
  MG_TRY(ss.ev.end(st));
  MG_TRY(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, sel.p, idx.p, (int64_t)(M + 1), st));
  uint32_t C32 = 0;
  MG_TRY(hipMemcpyAsync(&C32, idx.p + M, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  MG_TRY(hipStreamSynchronize(st));
  MG_TRY(ss.ev.elapsed(&ss.score_ms));
  const uint64_t C = C32;

  // --- aggregate
  uint64_t H = 0;
  ss.aggregate_ms = 0.f;
  if (C) {
    Scratch<uint64_t> keys_a, keys_b, cdist, crec, sdist, cum, hsup, hdist;
    Scratch<uint32_t> vals_a, vals_b, head, hidx, hseq_a, hseq_b, hord_a, hord_b;
    Scratch<uint8_t> tmp2;
    MG_SCRATCH(keys_a, C, "scaffold pair keys");
    MG_SCRATCH(keys_b, C, "scaffold pair keys");
    MG_SCRATCH(vals_a, C, "scaffold pair indices");
    MG_SCRATCH(vals_b, C, "scaffold pair indices");
    MG_SCRATCH(cdist, C, "scaffold counted distances");
    MG_SCRATCH(crec, C, "scaffold counted records");
    MG_SCRATCH(sdist, C, "scaffold sorted distances");
    MG_SCRATCH(cum, C, "scaffold distance sums");
    MG_SCRATCH(head, C + 1, "scaffold run heads");
    MG_SCRATCH(hidx, C + 1, "scaffold run indices");
    const int key_bits = bits_of(n_edges * n_edges - 1), idx_bits = bits_of(C);
    size_t b1 = 0, b2 = 0, b3 = 0, b4 = 0;
    MG_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, b1, keys_a.p, keys_b.p, vals_a.p, vals_b.p, (int)C, 0, key_bits,
                                              st));
    MG_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b2, head.p, hidx.p, (int64_t)(C + 1), st));
    MG_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, b3, sdist.p, cum.p, (int64_t)C, st));
    MG_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, b4, hseq_a.p, hseq_b.p, hord_a.p, hord_b.p, (int)C, 0, idx_bits,
                                              st));
    const size_t tb2 = std::max(std::max(b1, b2), std::max(b3, b4));
    MG_SCRATCH(tmp2, tb2, "scaffold sort storage");
    // the head buffers at their upper bound C (H <= C), so no allocation falls between the two events
    MG_SCRATCH(hseq_a, C, "scaffold pair first indices");
    MG_SCRATCH(hseq_b, C, "scaffold pair first indices");
    MG_SCRATCH(hord_a, C, "scaffold pair run numbers");
    MG_SCRATCH(hord_b, C, "scaffold pair run numbers");
    MG_SCRATCH(hsup, C, "scaffold pair supports");
    MG_SCRATCH(hdist, C, "scaffold pair distances");
    MG_GROW(ss.pairs, C, "d_scaffold_pairs");
    MG_TRY(ss.ev.start(st));
    hipLaunchKernelGGL(k_sc_emit, dim3(blocks_for(M)), dim3(kThreads), 0, st, M, sel.p, idx.p, key.p, dist.p, rec.p,
                       keys_a.p, vals_a.p, cdist.p, crec.p);
    MG_TRY(hipGetLastError());
    size_t t2 = tb2;
    MG_TRY(hipcub::DeviceRadixSort::SortPairs(tmp2.p, t2, keys_a.p, keys_b.p, vals_a.p, vals_b.p, (int)C, 0, key_bits,
                                              st));
    hipLaunchKernelGGL(k_run_heads<uint64_t>, dim3(blocks_for(C + 1)), dim3(kThreads), 0, st, keys_b.p, C, head.p);
    MG_TRY(hipGetLastError());
    t2 = tb2;
    MG_TRY(hipcub::DeviceScan::ExclusiveSum(tmp2.p, t2, head.p, hidx.p, (int64_t)(C + 1), st));
    uint32_t H32 = 0;
    MG_TRY(hipMemcpyAsync(&H32, hidx.p + C, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    hipLaunchKernelGGL(k_sc_dist, dim3(blocks_for(C)), dim3(kThreads), 0, st, vals_b.p, cdist.p, C, sdist.p);
    MG_TRY(hipGetLastError());
    t2 = tb2;
    MG_TRY(hipcub::DeviceScan::InclusiveSum(tmp2.p, t2, sdist.p, cum.p, (int64_t)C, st));
    MG_TRY(hipStreamSynchronize(st));
    H = H32;
    hipLaunchKernelGGL(k_sc_headrec, dim3(blocks_for(C)), dim3(kThreads), 0, st, keys_b.p, vals_b.p, C, head.p, hidx.p,
                       cum.p, hseq_a.p, hord_a.p, hsup.p, hdist.p);
    MG_TRY(hipGetLastError());
    t2 = tb2;
    MG_TRY(hipcub::DeviceRadixSort::SortPairs(tmp2.p, t2, hseq_a.p, hseq_b.p, hord_a.p, hord_b.p, (int)H, 0, idx_bits,
                                              st));
    hipLaunchKernelGGL(k_sc_pairs, dim3(blocks_for(H)), dim3(kThreads), 0, st, hseq_b.p, hord_b.p, hsup.p, hdist.p,
                       crec.p, H, ss.pairs.p);
    MG_TRY(hipGetLastError());
    MG_TRY(ss.ev.end(st));
    MG_TRY(hipStreamSynchronize(st));  // the scratch above is released here
    MG_TRY(ss.ev.elapsed(&ss.aggregate_ms));
  }
  ull cnt[5] = {0, 0, 0, 0, 0};
  MG_TRY(ctl_read(st, ctl.p + 3, 5, cnt));
  ss.n_entries = M;
  ss.n_counted = C;
  ss.n_pairs = H;
  ss.ready = true;
  if (counters) std::copy(cnt, cnt + 5, counters);
  if (n_pairs) *n_pairs = H;
  if (device_ms) *device_ms = ss.score_ms + ss.aggregate_ms;
  return 0;
}

int mg_scaffold_info(mg_ctx* ctx, uint64_t* out, float* ms) {
  if (!ctx) return -1;
  ctx->err.clear();
  if (!ctx->scaffold.ready) return set_err(ctx, "mg_scaffold_info: mg_scaffold_pairs must succeed first");
  const ScaffoldStage& ss = ctx->scaffold;
  if (out) {
    out[0] = ss.n_entries;
    out[1] = ss.n_counted;
    out[2] = ss.n_pairs;
  }
  if (ms) {
    ms[0] = ss.score_ms;
    ms[1] = ss.aggregate_ms;
  }
  return 0;
}

int mg_copy_scaffold_entries(mg_ctx* ctx, uint8_t* status) {
  if (!ctx) return -1;
  ctx->err.clear();
  MG_TRY(hipSetDevice(ctx->device));
  if (!ctx->scaffold.ready) return set_err(ctx, "mg_copy_scaffold_entries: mg_scaffold_pairs must succeed first");
  const ScaffoldStage& ss = ctx->scaffold;
  if (status && ss.n_entries)
    MG_TRY(hipMemcpyAsync(status, ss.status.p, ss.n_entries, hipMemcpyDeviceToHost, ctx->stream));
  MG_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}

int mg_copy_scaffold_pairs(mg_ctx* ctx, mg_scaffold_pair* out, uint64_t cap, uint64_t* n_copied) {
  if (!ctx) return -1;
  ctx->err.clear();
  if (n_copied) *n_copied = 0;
  MG_TRY(hipSetDevice(ctx->device));
  if (!ctx->scaffold.ready) return set_err(ctx, "mg_copy_scaffold_pairs: mg_scaffold_pairs must succeed first");
  const uint64_t c = out ? std::min(cap, ctx->scaffold.n_pairs) : 0;
  if (c)
    MG_TRY(hipMemcpyAsync(out, ctx->scaffold.pairs.p, c * sizeof(mg_scaffold_pair), hipMemcpyDeviceToHost, ctx->stream));
  MG_TRY(hipStreamSynchronize(ctx->stream));
  if (n_copied) *n_copied = c;
  return 0;
}

}  // extern "C"
