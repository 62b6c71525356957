// mg_places.hip — where every read lies on the edges, and the two statistics
// that are joins over it: insert sizes per dataset and per-edge coverage.
//
// Reference paths replaced (paths relative to the reference's MetaGenomics directory):
//   OverlapGraph::updateReadLocations              OverlapGraph.cpp:1048-1071
//   OverlapGraph::calculateMeanAndSdOfInsertSize   OverlapGraph.cpp:1124-1211 (the sums; the host divides)
//   OverlapGraph::getBaseByBaseCoverage            OverlapGraph.cpp:2722-2792 (the sums; the host divides)
//
// "Entry space": the list entries of all edges laid end to end, edge k at
// ebase[k]; entry e = (edge k, list position i) with e ascending in (k, i).
//
// mg_build_placements (one stream):
//   k_pl_entry  : thread per entry: its edge (binary search over ebase), read,
//                 strand and offset; the smallest entry with a read ID outside
//                 1..N is kept by atomicMin;
//   InclusiveSum: 64-bit, over the offsets of all entries (a segment can be
//                 millions of entries long: device-wide, not per workgroup);
//   k_pl_dist   : distance = the scan minus the scan before the edge's first
//                 entry; forward placements counted per read (integer atomics);
//   SortPairs   : stable radix sort of (read ID, entry) over the bits of N: a
//                 read's records come out in ascending entry = (edge, position),
//                 whatever the read's degree, so no per-read sort follows;
//   k_pl_write  : the 16-byte records;  k_csr_starts (mg_stage.hpp): start[A] by binary search.
// mg_insert_sizes: thread per mate entry, the k x l loop of :1162-1175 over the
//   two reads' records; count / sum / sum of squares reduced across the
//   wavefront per dataset, then one 64-bit atomic per counter.
// mg_edge_coverage: per chunk of edges a 64-bit delta word per base (high half:
//   zeroing entries, low half: frequency), atomics at interval starts and ends,
//   one InclusiveSum, one reduction pass keyed by edge.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "mg_overlap.h"
#include "mg_stage.hpp"

namespace {

constexpr uint64_t kCovBudget = 1ull << 25;  // per-base counters per chunk (two 8-B words each)
constexpr uint64_t kMaxOffset = 1ull << 40;  // an edge's overlapOffset mg_edge_coverage accepts

typedef unsigned long long ull;

// last k in [lo, hi) with base[k] <= x (base[lo] <= x)
__device__ __forceinline__ uint64_t last_le(const uint64_t* __restrict__ base, uint64_t lo, uint64_t hi, uint64_t x) {
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (base[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Every lane of the wavefront calls this.  The lanes with `has` add their NV
// values to out[NV * key ..]: per distinct key one butterfly reduction and one
// 64-bit atomic per non-zero counter from lane 0.
template <int NV>
__device__ __forceinline__ void wave_add_by_key(uint32_t key, bool has, const ull (&v)[NV], ull* __restrict__ out) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  ull todo = __ballot(has);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const uint32_t k0 = (uint32_t)__shfl((int)key, leader);
    const bool mine = has && key == k0;
    ull s[NV];
#pragma unroll
    for (int t = 0; t < NV; ++t) s[t] = mine ? v[t] : 0ull;
#pragma unroll
    for (int o = kWave / 2; o; o >>= 1) {
#pragma unroll
      for (int t = 0; t < NV; ++t) s[t] += __shfl_xor(s[t], o);
    }
    if (lane == 0) {
#pragma unroll
      for (int t = 0; t < NV; ++t)
        if (s[t]) atomicAdd(&out[(uint64_t)NV * k0 + t], s[t]);
    }
    todo &= ~__ballot(mine);
  }
}

__global__ __launch_bounds__(kThreads) void k_pl_entry(const mg_contig_edge* __restrict__ edges,
                                                       const uint64_t* __restrict__ ebase, uint64_t n_edges,
                                                       const uint32_t* __restrict__ reads,
                                                       const uint16_t* __restrict__ offs, const uint8_t* __restrict__ ors,
                                                       uint64_t E, uint64_t N, uint32_t* __restrict__ eread,
                                                       uint32_t* __restrict__ eedge, uint8_t* __restrict__ efwd,
                                                       uint64_t* __restrict__ val, ull* __restrict__ ctl) {
  const uint64_t e = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= E) return;
  const uint64_t k = last_le(ebase, 0, n_edges, e);
  const uint64_t q = edges[k].first + (e - ebase[k]);
  const uint32_t id = reads[q];
  if (id < 1 || id > N) atomicMin(&ctl[0], (ull)e);
  eread[e] = id;
  eedge[e] = (uint32_t)k;
  efwd[e] = ors[q] == 1 ? 1 : 0;
  val[e] = offs[q];
}

__global__ __launch_bounds__(kThreads) void k_pl_dist(uint64_t E, const uint32_t* __restrict__ eedge,
                                                      const uint64_t* __restrict__ ebase,
                                                      const uint64_t* __restrict__ incl,
                                                      const uint32_t* __restrict__ eread,
                                                      const uint8_t* __restrict__ efwd, uint64_t* __restrict__ edist,
                                                      uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                      uint32_t* __restrict__ fwdcnt) {
  const uint64_t e = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= E) return;
  const uint64_t b = ebase[eedge[e]];
  edist[e] = incl[e] - (b ? incl[b - 1] : 0);
  const uint32_t id = eread[e];  // (validated: 1..N)
  keys[e] = id;
  vals[e] = (uint32_t)e;
  if (efwd[e]) atomicAdd(&fwdcnt[id], 1u);
}

__global__ __launch_bounds__(kThreads) void k_pl_write(uint64_t E, const uint32_t* __restrict__ sorted,
                                                       const uint32_t* __restrict__ eedge,
                                                       const uint8_t* __restrict__ efwd,
                                                       const uint64_t* __restrict__ edist, mg_place* __restrict__ out) {
  const uint64_t s = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (s >= E) return;
  const uint32_t e = sorted[s];
  mg_place p;
  p.edge = eedge[e];
  p.flags = efwd[e];
  p.distance = edist[e];
  out[s] = p;
}

// Thread per mate entry: the quadruple loop of :1140-1179 for one (read1, j).
__global__ __launch_bounds__(kThreads) void k_insert_sizes(const uint64_t* __restrict__ mstart,
                                                           const mg_mate* __restrict__ mates, uint64_t M, uint64_t N,
                                                           uint32_t n_datasets, uint64_t max_distance,
                                                           const uint64_t* __restrict__ pstart,
                                                           const mg_place* __restrict__ places, ull* __restrict__ sums,
                                                           ull* __restrict__ ctl) {
  const uint64_t m = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  ull v[3] = {0, 0, 0};
  uint32_t d = 0;
  if (m < M) {
    const uint64_t a = last_le(mstart, 0, N + 2, m);  // mstart[a] <= m < mstart[a + 1]
    const mg_mate mt = mates[m];
    d = mt.dataset;
    if (a < 1 || a > N || mt.id < 1 || mt.id > N || d >= n_datasets) {
      atomicMin(&ctl[0], (ull)m);
    } else {
      const uint64_t p0 = pstart[a], p1 = pstart[a + 1], q0 = pstart[mt.id], q1 = pstart[mt.id + 1];
      for (uint64_t p = p0; p < p1; ++p) {
        const mg_place pa = places[p];
        for (uint64_t q = q0; q < q1; ++q) {
          const mg_place pb = places[q];
          if (pa.edge == pb.edge && pa.distance > pb.distance) {
            const uint64_t x = pa.distance - pb.distance;
            if (x < max_distance) {
              v[0] += 1;
              v[1] += x;
              v[2] += x * x;
            }
          }
        }
      }
    }
  }
  wave_add_by_key<3>(d, v[0] != 0, v, sums);
}

struct EdgeInfo {
  uint64_t L;  // offset + len(dst)
  uint32_t lsrc, ldst;
  uint32_t bad;  // 1: src or dst outside 1..N; 2: len(src) > L + 1
  uint32_t pad;
};

__global__ __launch_bounds__(kThreads) void k_cov_edges(ReadView v, const mg_contig_edge* __restrict__ edges,
                                                        uint64_t n_edges, EdgeInfo* __restrict__ info,
                                                        ull* __restrict__ ctl) {
  const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k >= n_edges) return;
  const mg_contig_edge e = edges[k];
  EdgeInfo f{0, 0, 0, 0, 0};
  if (e.src < 1 || e.src > v.n || e.dst < 1 || e.dst > v.n) {
    f.bad = 1;
    atomicMin(&ctl[1], (ull)k);
  } else {
    f.lsrc = len_of(v, e.src);
    f.ldst = len_of(v, e.dst);
    f.L = e.offset + f.ldst;  // (offset < 2^40: checked by the host)
    if (f.lsrc > f.L + 1) {
      f.bad = 2;
      atomicMin(&ctl[2], (ull)k);
    }
  }
  info[k] = f;
}

// Thread per entry: D + len(read) <= L + 1, and the edge's frequency sum.
__global__ __launch_bounds__(kThreads) void k_cov_entries(ReadView v, uint64_t E, const uint32_t* __restrict__ eread,
                                                          const uint32_t* __restrict__ eedge,
                                                          const uint64_t* __restrict__ edist,
                                                          const EdgeInfo* __restrict__ info,
                                                          const uint32_t* __restrict__ freq, ull* __restrict__ fsum,
                                                          ull* __restrict__ ctl) {
  const uint64_t e = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  ull f[1] = {0};
  uint32_t k = 0;
  if (e < E) {
    k = eedge[e];
    const uint32_t id = eread[e];
    const EdgeInfo in = info[k];
    if (in.bad != 1 && edist[e] + len_of(v, id) > in.L + 1) atomicMin(&ctl[0], (ull)e);
    f[0] = freq[id - 1];
  }
  wave_add_by_key<1>(k, f[0] != 0, f, fsum);
}

// Entries [e0, e1) of one chunk: +word at the interval's start, -word one past its end.
__global__ __launch_bounds__(kThreads) void k_cov_delta(ReadView v, uint64_t e0, uint64_t e1,
                                                        const uint32_t* __restrict__ eread,
                                                        const uint32_t* __restrict__ eedge,
                                                        const uint64_t* __restrict__ edist,
                                                        const uint64_t* __restrict__ cbase, uint64_t chunk_base,
                                                        const uint32_t* __restrict__ freq,
                                                        const uint32_t* __restrict__ fwdcnt, ull* __restrict__ delta) {
  const uint64_t e = e0 + (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= e1) return;
  const uint32_t id = eread[e];
  const uint32_t len = len_of(v, id);
  const ull word = ((fwdcnt[id] > 1) ? 1ull << 32 : 0ull) | freq[id - 1];
  if (!len || !word) return;
  const uint64_t pos = cbase[eedge[e]] - chunk_base + edist[e];  // pos + len <= the chunk's counters (validated)
  atomicAdd(&delta[pos], word);
  atomicAdd(&delta[pos + len], 0ull - word);
}

// Thread per counter of the chunk (edges [k0, k1), n == 0 edges own none).
__global__ __launch_bounds__(kThreads) void k_cov_reduce(const uint64_t* __restrict__ cov, uint64_t B, uint64_t k0,
                                                         uint64_t k1, const uint64_t* __restrict__ cbase,
                                                         uint64_t chunk_base, const EdgeInfo* __restrict__ info,
                                                         ull* __restrict__ out) {
  const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  ull v[3] = {0, 0, 0};
  uint32_t k = 0;
  if (j < B) {
    k = (uint32_t)last_le(cbase, k0, k1, j + chunk_base);
    const uint64_t x = j + chunk_base - cbase[k];
    const EdgeInfo in = info[k];
    const uint64_t w = cov[j];
    ull c = (w >> 32) ? 0ull : (w & 0xFFFFFFFFull);
    if (x < in.lsrc || x + in.ldst > in.L) c = 0;
    v[0] = c ? 1 : 0;
    v[1] = c;
    v[2] = c * c;
  }
  wave_add_by_key<3>(k, v[0] != 0, v, out);
}

}  // namespace

extern "C" {

int mg_build_placements(mg_ctx* ctx, const mg_contig_edge* edges, uint64_t n_edges, const uint32_t* reads,
                        const uint16_t* offs, const uint8_t* ors, uint64_t n_list, uint64_t* n_places,
                        float* device_ms) {
  if (!ctx) return -1;
  ctx->err.clear();
  if (n_places) *n_places = 0;
  if (device_ms) *device_ms = 0.f;
  ctx->places.ready = false;
  if ((n_edges && !edges) || (n_list && (!reads || !offs || !ors)))
    return set_err(ctx, "mg_build_placements: null argument");
  MG_TRY(hipSetDevice(ctx->device));
  if (whole_multiset(ctx, "mg_build_placements")) return -1;
  if (ctx->n && !ctx->d_len.p) return set_err(ctx, "mg_build_placements: no reads on the device");
  if (n_edges >> 31) return set_err(ctx, "mg_build_placements: 2^31 or more edges are not supported");
  std::vector<uint64_t> ebase;
  if (edge_bases(ctx, "mg_build_placements", edges, n_edges, n_list, 0, ebase)) return -1;
  const uint64_t E = ebase[n_edges], N = ctx->n, entries = N + 2;
  if (E >> 31) return set_err(ctx, "mg_build_placements: 2^31 or more list entries are not supported");
  hipStream_t st = ctx->stream;
  PlaceStage& pl = ctx->places;
  MG_GROW(pl.start, entries, "d_pl_start");
  MG_GROW(pl.recs, E, "d_places");
  MG_GROW(pl.fwd, entries, "d_pl_fwd");
  MG_GROW(pl.d_edges, n_edges, "d_pl_edges");
  MG_GROW(pl.d_ebase, n_edges + 1, "d_pl_ebase");
  MG_GROW(pl.eread, E, "d_pl_eread");
  MG_GROW(pl.eedge, E, "d_pl_eedge");
  MG_GROW(pl.edist, E, "d_pl_edist");
  EdgeLists lists;
  Scratch<uint32_t> keys_a, keys_b, vals_a, vals_b;
  Scratch<uint8_t> efwd, tmp;
  Scratch<uint64_t> val, incl;
  Scratch<ull> ctl;
  MG_SCRATCH(efwd, E, "placement strands");
  MG_SCRATCH(val, E, "placement offsets");
  MG_SCRATCH(incl, E, "placement offset sums");
  MG_SCRATCH(keys_a, E, "placement sort keys");
  MG_SCRATCH(keys_b, E, "placement sort keys");
  MG_SCRATCH(vals_a, E, "placement sort values");
  MG_SCRATCH(vals_b, E, "placement sort values");
  MG_SCRATCH(ctl, 1, "placement control word");
  int end_bit = 1;
  while (end_bit < 32 && (N >> end_bit)) ++end_bit;
  size_t scan_bytes = 0, sort_bytes = 0;
  MG_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, val.p, incl.p, (int64_t)E, st));
  MG_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, keys_a.p, keys_b.p, vals_a.p, vals_b.p, (int)E, 0,
                                            end_bit, st));
  const size_t tmp_bytes = std::max(scan_bytes, sort_bytes);
  MG_SCRATCH(tmp, tmp_bytes, "placement scan and sort storage");
  if (n_edges) MG_TRY(hipMemcpyAsync(pl.d_edges.p, edges, n_edges * sizeof(mg_contig_edge), hipMemcpyHostToDevice, st));
  if (lists.upload(ctx, "placement", reads, offs, ors, n_list)) return -1;
  MG_TRY(hipMemcpyAsync(pl.d_ebase.p, ebase.data(), (n_edges + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  MG_TRY(ctl_fill(st, ctl.p, 1, ~0ull));
  MG_TRY(hipMemsetAsync(pl.fwd.p, 0, entries * sizeof(uint32_t), st));

  MG_TRY(pl.ev.start(st));
  if (E) {
    hipLaunchKernelGGL(k_pl_entry, dim3(blocks_for(E)), dim3(kThreads), 0, st, pl.d_edges.p, pl.d_ebase.p, n_edges,
                       lists.reads.p, lists.offs.p, lists.ors.p, E, N, pl.eread.p, pl.eedge.p, efwd.p, val.p, ctl.p);
    MG_TRY(hipGetLastError());
    size_t tb = tmp_bytes;
    MG_TRY(hipcub::DeviceScan::InclusiveSum(tmp.p, tb, val.p, incl.p, (int64_t)E, st));
  }
  // the read IDs index the forward counts from here on: the error word decides first
  ull bad = ~0ull;
  MG_TRY(ctl_read(st, ctl.p, 1, &bad));
  if (bad != ~0ull) {
    const uint64_t k = (uint64_t)(std::upper_bound(ebase.begin(), ebase.end(), (uint64_t)bad) - ebase.begin()) - 1;
    ctx->err = "mg_build_placements: " + edge_name(edges, k) + ", list entry " + std::to_string(bad - ebase[k]) + ": read ID " +
               std::to_string(reads[edges[k].first + (bad - ebase[k])]) + " outside 1.." + std::to_string(N) + " (-2)";
    return -2;
  }
  if (E) {
    hipLaunchKernelGGL(k_pl_dist, dim3(blocks_for(E)), dim3(kThreads), 0, st, E, pl.eedge.p, pl.d_ebase.p, incl.p,
                       pl.eread.p, efwd.p, pl.edist.p, keys_a.p, vals_a.p, pl.fwd.p);
    MG_TRY(hipGetLastError());
    size_t tb = tmp_bytes;
    MG_TRY(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, keys_a.p, keys_b.p, vals_a.p, vals_b.p, (int)E, 0, end_bit,
                                              st));
    hipLaunchKernelGGL(k_pl_write, dim3(blocks_for(E)), dim3(kThreads), 0, st, E, vals_b.p, pl.eedge.p, efwd.p,
                       pl.edist.p, pl.recs.p);
    MG_TRY(hipGetLastError());
  }
  MG_TRY(csr_starts(st, keys_b.p, E, entries, pl.start.p));
  MG_TRY(pl.ev.end(st));
  MG_TRY(hipStreamSynchronize(st));
  MG_TRY(pl.ev.elapsed(device_ms));
  pl.edges.assign(edges, edges + n_edges);
  pl.ebase.swap(ebase);
  pl.n = E;
  ctx->places.ready = true;
  if (n_places) *n_places = E;
  return 0;
}

int mg_copy_placements(mg_ctx* ctx, uint64_t* start, mg_place* out, uint64_t cap, uint64_t* n_copied) {
  if (!ctx) return -1;
  ctx->err.clear();
  MG_TRY(hipSetDevice(ctx->device));
  if (n_copied) *n_copied = 0;
  if (!ctx->places.ready)
    return set_err(ctx, "mg_copy_placements: mg_build_placements must succeed for the current reads first");
  return copy_csr(ctx, ctx->places.start.p, ctx->n + 2, start, ctx->places.recs.p, ctx->places.n, out, cap, n_copied);
}

int mg_insert_sizes(mg_ctx* ctx, const uint64_t* mate_start, const mg_mate* mates, uint32_t n_datasets,
                    uint64_t max_distance, uint64_t* sums, float* device_ms) {
  if (!ctx) return -1;
  ctx->err.clear();
  if (device_ms) *device_ms = 0.f;
  if (n_datasets > 256) return set_err(ctx, "mg_insert_sizes: more than 256 datasets (datasetNumber is UINT8)");
  if (n_datasets && !sums) return set_err(ctx, "mg_insert_sizes: null argument");
  for (uint32_t i = 0; i < 3 * n_datasets; ++i) sums[i] = 0;
  MG_TRY(hipSetDevice(ctx->device));
  if (!ctx->places.ready)
    return set_err(ctx, "mg_insert_sizes: mg_build_placements must succeed for the current reads first");
  const uint64_t N = ctx->n, entries = N + 2;
  hipStream_t st = ctx->stream;
  Scratch<uint64_t> d_ms;
  Scratch<mg_mate> d_m;
  Scratch<ull> d_sums, ctl;
  const uint64_t* ms = ctx->mates.start.p;
  const mg_mate* mm = ctx->mates.recs.p;
  uint64_t M = ctx->mates.n;
  if (mate_start) {
    if (mate_start[0] != 0) return set_err(ctx, "mg_insert_sizes: mate_start[0] must be 0");
    for (uint64_t a = 0; a + 1 < entries; ++a)
      if (mate_start[a + 1] < mate_start[a]) return set_err(ctx, "mg_insert_sizes: mate_start must not decrease");
    M = mate_start[entries - 1];
    if (M && !mates) return set_err(ctx, "mg_insert_sizes: null argument");
    MG_SCRATCH(d_ms, entries, "caller's mate list starts");
    MG_SCRATCH(d_m, M, "caller's mate lists");
    MG_TRY(hipMemcpyAsync(d_ms.p, mate_start, entries * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (M) MG_TRY(hipMemcpyAsync(d_m.p, mates, M * sizeof(mg_mate), hipMemcpyHostToDevice, st));
    ms = d_ms.p;
    mm = d_m.p;
  } else if (!ctx->mates.ready) {
    return set_err(ctx, "mg_insert_sizes: no resident mate lists: mg_build_mate_pairs must run for the current reads "
                        "first, or pass a CSR");
  }
  MG_SCRATCH(d_sums, 3 * (uint64_t)std::max<uint32_t>(n_datasets, 1), "insert-size sums");
  MG_SCRATCH(ctl, 1, "insert-size control word");
  MG_TRY(hipMemsetAsync(d_sums.p, 0, 3 * (size_t)std::max<uint32_t>(n_datasets, 1) * sizeof(ull), st));
  MG_TRY(ctl_fill(st, ctl.p, 1, ~0ull));
  MG_TRY(ctx->places.ev.start(st));
  if (M) {
    hipLaunchKernelGGL(k_insert_sizes, dim3(blocks_for(M)), dim3(kThreads), 0, st, ms, mm, M, N, n_datasets, max_distance,
                       ctx->places.start.p, ctx->places.recs.p, d_sums.p, ctl.p);
    MG_TRY(hipGetLastError());
  }
  MG_TRY(ctx->places.ev.end(st));
  ull bad = ~0ull;
  std::vector<ull> h(3 * (size_t)n_datasets, 0);
  if (n_datasets) MG_TRY(hipMemcpyAsync(h.data(), d_sums.p, h.size() * sizeof(ull), hipMemcpyDeviceToHost, st));
  MG_TRY(ctl_read(st, ctl.p, 1, &bad));
  MG_TRY(ctx->places.ev.elapsed(device_ms));
  if (bad != ~0ull) {
    ctx->err = "mg_insert_sizes: mate entry " + std::to_string(bad) +
               ": its dataset is not below " + std::to_string(n_datasets) + " or its owner or mate ID lies outside 1.." +
               std::to_string(N) + " (-2)";
    return -2;
  }
  for (size_t i = 0; i < h.size(); ++i) sums[i] = h[i];
  return 0;
}

int mg_edge_coverage(mg_ctx* ctx, const uint32_t* freq, uint64_t* out, float* device_ms) {
  if (!ctx) return -1;
  ctx->err.clear();
  if (device_ms) *device_ms = 0.f;
  MG_TRY(hipSetDevice(ctx->device));
  if (!ctx->places.ready)
    return set_err(ctx, "mg_edge_coverage: mg_build_placements must succeed for the current reads first");
  PlaceStage& pl = ctx->places;
  const uint64_t n_edges = pl.edges.size(), E = pl.n, N = ctx->n;
  if (n_edges && !out) return set_err(ctx, "mg_edge_coverage: null argument");
  if (!freq && !(ctx->freq_ready && ctx->d_freq.p))
    return set_err(ctx, "mg_edge_coverage: no resident frequencies (the reads were not ingested on the device): "
                        "pass freq");
  for (uint64_t k = 0; k < n_edges; ++k)
    if (pl.edges[k].offset >= kMaxOffset)
      return set_err(ctx, "mg_edge_coverage: " + edge_name(pl.edges.data(), k) + ": an offset of 2^40 or more is not supported");
  hipStream_t st = ctx->stream;
  const ReadView v = view_of(ctx);
  Scratch<uint32_t> d_f;
  Scratch<EdgeInfo> d_info;
  Scratch<ull> d_fsum, ctl, d_out, delta;
  Scratch<uint64_t> d_cbase, cov;
  Scratch<uint8_t> tmp;
  const uint32_t* fp = ctx->d_freq.p;
  if (freq) {
    MG_SCRATCH(d_f, N, "caller's read frequencies");
    if (N) MG_TRY(hipMemcpyAsync(d_f.p, freq, N * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    fp = d_f.p;
  }
  MG_SCRATCH(d_info, n_edges, "coverage edge records");
  MG_SCRATCH(d_fsum, n_edges, "coverage frequency sums");
  MG_SCRATCH(d_out, 3 * n_edges, "coverage sums");
  MG_SCRATCH(d_cbase, n_edges + 1, "coverage counter bases");
  MG_SCRATCH(ctl, 3, "coverage control words");
  MG_TRY(hipMemsetAsync(d_fsum.p, 0, std::max<uint64_t>(n_edges, 1) * sizeof(ull), st));
  MG_TRY(hipMemsetAsync(d_out.p, 0, std::max<uint64_t>(3 * n_edges, 1) * sizeof(ull), st));
  MG_TRY(ctl_fill(st, ctl.p, 3, ~0ull));
  MG_TRY(pl.ev.start(st));
  if (n_edges) {
    hipLaunchKernelGGL(k_cov_edges, dim3(blocks_for(n_edges)), dim3(kThreads), 0, st, v, pl.d_edges.p, n_edges, d_info.p,
                       ctl.p);
    MG_TRY(hipGetLastError());
  }
  if (E) {
    hipLaunchKernelGGL(k_cov_entries, dim3(blocks_for(E)), dim3(kThreads), 0, st, v, E, pl.eread.p, pl.eedge.p,
                       pl.edist.p, d_info.p, fp, d_fsum.p, ctl.p);
    MG_TRY(hipGetLastError());
  }
  ull bad[3] = {~0ull, ~0ull, ~0ull};
  std::vector<EdgeInfo> info(n_edges);
  std::vector<ull> fsum(n_edges, 0);
  if (n_edges) {
    MG_TRY(hipMemcpyAsync(info.data(), d_info.p, n_edges * sizeof(EdgeInfo), hipMemcpyDeviceToHost, st));
    MG_TRY(hipMemcpyAsync(fsum.data(), d_fsum.p, n_edges * sizeof(ull), hipMemcpyDeviceToHost, st));
  }
  MG_TRY(ctl_read(st, ctl.p, 3, bad));
  if (bad[0] != ~0ull || bad[1] != ~0ull || bad[2] != ~0ull) {
    // the first invalid edge; within it: its IDs, then its first entry, then its source span
    const uint64_t ke =
        bad[0] == ~0ull ? ~0ull
                        : (uint64_t)(std::upper_bound(pl.ebase.begin(), pl.ebase.end(), (uint64_t)bad[0]) -
                                     pl.ebase.begin()) - 1;
    const uint64_t k = std::min<uint64_t>(ke, std::min<uint64_t>(bad[1], bad[2]));
    std::string why;
    if (k == bad[1]) why = ": its source or destination read ID lies outside 1.." + std::to_string(N);
    else if (k == ke)
      why = ", list entry " + std::to_string(bad[0] - pl.ebase[k]) +
            ": the read ends beyond the edge's counters (vector::at would throw)";
    else why = ": the source read is longer than the edge's counters (vector::at would throw)";
    ctx->err = "mg_edge_coverage: " + edge_name(pl.edges.data(), k) + why + " (-2)";
    return -2;
  }
  for (uint64_t k = 0; k < n_edges; ++k)
    if (fsum[k] >> 32)
      return set_err(ctx, "mg_edge_coverage: " + edge_name(pl.edges.data(), k) +
                              ": its list frequencies sum to 2^32 or more (the per-base counters are 32 bits wide)");
  // counters of edge k at cbase[k]; an edge without list reads owns none
  std::vector<uint64_t> cbase(n_edges + 1, 0);
  for (uint64_t k = 0; k < n_edges; ++k) cbase[k + 1] = cbase[k] + (pl.edges[k].n ? info[k].L + 1 : 0);
  MG_TRY(hipMemcpyAsync(d_cbase.p, cbase.data(), (n_edges + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  const uint64_t budget = pl.cov_budget ? pl.cov_budget : kCovBudget;
  uint64_t chunk_cap = 0;
  for (uint64_t k0 = 0; k0 < n_edges;) {  // sizes first: one allocation serves every chunk
    uint64_t k1 = k0 + 1;
    while (k1 < n_edges && cbase[k1 + 1] - cbase[k0] <= budget) ++k1;
    chunk_cap = std::max(chunk_cap, cbase[k1] - cbase[k0]);
    k0 = k1;
  }
  size_t tmp_bytes = 0;
  MG_SCRATCH(delta, chunk_cap + 1, "coverage delta words");
  MG_SCRATCH(cov, chunk_cap + 1, "coverage counters");
  MG_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, tmp_bytes, delta.p, cov.p, (int64_t)std::max<uint64_t>(chunk_cap, 1),
                                          st));
  MG_SCRATCH(tmp, tmp_bytes, "coverage scan storage");
  for (uint64_t k0 = 0; k0 < n_edges;) {
    uint64_t k1 = k0 + 1;
    while (k1 < n_edges && cbase[k1 + 1] - cbase[k0] <= budget) ++k1;
    const uint64_t B = cbase[k1] - cbase[k0], e0 = pl.ebase[k0], e1 = pl.ebase[k1];
    if (B) {
      MG_TRY(hipMemsetAsync(delta.p, 0, (B + 1) * sizeof(ull), st));
      if (e1 > e0) {
        hipLaunchKernelGGL(k_cov_delta, dim3(blocks_for(e1 - e0)), dim3(kThreads), 0, st, v, e0, e1, pl.eread.p,
                           pl.eedge.p, pl.edist.p, d_cbase.p, cbase[k0], fp, pl.fwd.p, delta.p);
        MG_TRY(hipGetLastError());
      }
      size_t tb = tmp_bytes;
      MG_TRY(hipcub::DeviceScan::InclusiveSum(tmp.p, tb, delta.p, cov.p, (int64_t)B, st));
      hipLaunchKernelGGL(k_cov_reduce, dim3(blocks_for(B)), dim3(kThreads), 0, st, cov.p, B, k0, k1, d_cbase.p, cbase[k0],
                         d_info.p, d_out.p);
      MG_TRY(hipGetLastError());
    }
    k0 = k1;
  }
  MG_TRY(pl.ev.end(st));
  if (n_edges) MG_TRY(hipMemcpyAsync(out, d_out.p, 3 * n_edges * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  MG_TRY(hipStreamSynchronize(st));
  MG_TRY(pl.ev.elapsed(device_ms));
  return 0;
}

}  // extern "C"
