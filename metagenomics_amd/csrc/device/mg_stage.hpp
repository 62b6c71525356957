// mg_stage.hpp — INTERNAL: what the derived-stage translation units share
// beyond the context (mg_dataset.hip, mg_disc.hip, mg_comp.hip, mg_mates.hip,
// mg_contigs.hip, mg_places.hip, mg_paths.hip, mg_scaffold.hip, mg_chains.hip): the view
// of the resident reads, the launch grid, the CSR starts of sorted owners,
// control words, the copy tail of the mg_copy_* calls, the edge lists that
// mg_build_contigs and mg_build_placements both take, and the CSR inputs and
// validation kernels that mg_mate_paths and mg_scaffold_pairs both take.
// (DevArray, Scratch and their growth macros
// are in mg_ctx.hpp.)  mg_kernels.hip does not include it.
#ifndef MG_STAGE_HPP_
#define MG_STAGE_HPP_
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "mg_ctx.hpp"
#include "mg_overlap.h"

constexpr int kThreads = 256;
constexpr int kWave = 64;

// blocks of kThreads for a thread per item; 1 for no items, so a launch over
// an empty range is still a valid one
inline uint32_t blocks_for(uint64_t items) { return (uint32_t)std::max<uint64_t>(1, (items + kThreads - 1) / kThreads); }

// the resident reads
struct ReadView {
  const uint64_t* words;
  const uint16_t* len;
  const uint32_t* phys;  // slot of ID - 1, or nullptr (slots in ID order)
  uint64_t n;
  uint32_t maxw, stride;
};

inline ReadView view_of(const mg_ctx* ctx) {
  return ReadView{ctx->d_words.p, ctx->d_len.p, ctx->d_phys, ctx->n, ctx->maxw, ctx->stride};
}

// slot of the read with ID idx + 1
__device__ __forceinline__ uint64_t slot_of(const ReadView& v, uint64_t idx) { return v.phys ? v.phys[idx] : idx; }
// length of the read with this ID
__device__ __forceinline__ uint32_t len_of(const ReadView& v, uint32_t id) {
  return v.len[v.phys ? v.phys[id - 1] : id - 1];
}

// start[a] = first index in the ascending keys whose key is >= a, for a in
// [0, entries): the CSR starts of records sorted by owner ID
template <typename Start>
__global__ __launch_bounds__(kThreads) void k_csr_starts(const uint32_t* __restrict__ sorted_keys, uint64_t n,
                                                         uint64_t entries, Start* __restrict__ start) {
  const uint64_t a = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (a >= entries) return;
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if ((uint64_t)sorted_keys[mid] < a) lo = mid + 1;
    else hi = mid;
  }
  start[a] = lo;
}

// (a template as well: only the files that call it carry the kernel)
template <typename Start>
hipError_t csr_starts(hipStream_t st, const uint32_t* sorted_keys, uint64_t n, uint64_t entries, Start* start) {
  hipLaunchKernelGGL(k_csr_starts<Start>, dim3(blocks_for(entries)), dim3(kThreads), 0, st, sorted_keys, n, entries,
                     start);
  return hipGetLastError();
}

// Control words: a stage sets a few 64-bit words to 0 or ~0 on its stream, its
// kernels atomicMin / atomicAdd into them (the first bad item, a count), and
// the host reads them back.
typedef unsigned long long ctl_word;
inline hipError_t ctl_fill(hipStream_t st, ctl_word* d, size_t n, ctl_word value /* 0 or ~0 */) {
  return hipMemsetAsync(d, value ? 0xFF : 0, n * sizeof(ctl_word), st);
}
// copies them to the host and waits for the stream
inline hipError_t ctl_read(hipStream_t st, const ctl_word* d, size_t n, ctl_word* host) {
  const hipError_t e = hipMemcpyAsync(host, d, n * sizeof(ctl_word), hipMemcpyDeviceToHost, st);
  return e != hipSuccess ? e : hipStreamSynchronize(st);
}

// The tail of the mg_copy_* calls: `entries` starts (or labels) and the first
// min(cap, n) records to the host, either only where its pointer is given;
// *n_copied = records copied.  The callers check readiness first.
template <typename S, typename T>
int copy_csr(mg_ctx* ctx, const S* d_start, uint64_t entries, S* start, const void* d_recs, uint64_t n, T* out,
             uint64_t cap, uint64_t* n_copied) {
  if (start) MG_TRY(hipMemcpyAsync(start, d_start, entries * sizeof(S), hipMemcpyDeviceToHost, ctx->stream));
  const uint64_t c = out ? std::min(cap, n) : 0;
  if (c) MG_TRY(hipMemcpyAsync(out, d_recs, c * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
  MG_TRY(hipStreamSynchronize(ctx->stream));
  if (n_copied) *n_copied = c;
  return 0;
}

// --- the edge lists of mg_build_contigs and mg_build_placements ---

inline std::string edge_name(const mg_contig_edge* edges, uint64_t k) {
  return "edge " + std::to_string(k) + " (" + std::to_string(edges[k].src) + ", " + std::to_string(edges[k].dst) + ")";
}

// base[k] = items of the edges before k, an edge counting its list entries plus
// `extra` (base has n_edges + 1 entries); every list range must lie inside the lists
inline int edge_bases(mg_ctx* ctx, const char* who, const mg_contig_edge* edges, uint64_t n_edges, uint64_t n_list,
                      uint64_t extra, std::vector<uint64_t>& base) {
  base.assign(n_edges + 1, 0);
  for (uint64_t k = 0; k < n_edges; ++k) {
    if (edges[k].first > n_list || edges[k].n > n_list - edges[k].first)
      return set_err(ctx, std::string(who) + ": " + edge_name(edges, k) + ": its list range lies outside the " +
                              std::to_string(n_list) + " list entries");
    base[k + 1] = base[k] + edges[k].n + extra;
  }
  return 0;
}

// the caller's reads / offs / ors lists in scratch
struct EdgeLists {
  Scratch<uint32_t> reads;
  Scratch<uint16_t> offs;
  Scratch<uint8_t> ors;
  // `stage` ("contig", "placement") starts the buffers' names
  int upload(mg_ctx* ctx, const std::string& stage, const uint32_t* h_reads, const uint16_t* h_offs,
             const uint8_t* h_ors, uint64_t n_list) {
    MG_SCRATCH(reads, n_list, (stage + " list reads").c_str());
    MG_SCRATCH(offs, n_list, (stage + " list offsets").c_str());
    MG_SCRATCH(ors, n_list, (stage + " list orientations").c_str());
    if (!n_list) return 0;
    MG_TRY(hipMemcpyAsync(reads.p, h_reads, n_list * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    MG_TRY(hipMemcpyAsync(offs.p, h_offs, n_list * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
    MG_TRY(hipMemcpyAsync(ors.p, h_ors, n_list, hipMemcpyHostToDevice, ctx->stream));
    return 0;
  }
};

// --- what mg_mate_paths and mg_scaffold_pairs share: the two CSRs they read,
// the validation of placements and mate entries, run heads of sorted keys ---

// last k in [lo, hi) with base[k] <= x (base[lo] <= x)
__device__ __forceinline__ uint64_t last_le(const uint64_t* __restrict__ base, uint64_t lo, uint64_t hi, uint64_t x) {
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (base[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// (templates, as k_csr_starts: only the files that launch them carry them)
// *bad = the first placement whose edge is not below n
template <typename Ctl>
__global__ __launch_bounds__(kThreads) void k_check_places(const mg_place* __restrict__ places, uint64_t P, uint64_t n,
                                                           Ctl* __restrict__ bad) {
  const uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p < P && places[p].edge >= n) atomicMin(bad, (Ctl)p);
}

// owner[m] = the read whose list holds mate entry m; *bad = the first entry
// whose owner or mate ID lies outside 1..N or whose dataset is not below n_datasets
template <typename Ctl>
__global__ __launch_bounds__(kThreads) void k_mate_owners(const uint64_t* __restrict__ mstart,
                                                          const mg_mate* __restrict__ mates, uint64_t M, uint64_t N,
                                                          uint32_t n_datasets, uint32_t* __restrict__ owner,
                                                          Ctl* __restrict__ bad) {
  const uint64_t m = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (m >= M) return;
  const uint64_t a = last_le(mstart, 0, N + 2, m);  // mstart[a] <= m < mstart[a + 1]
  const mg_mate mt = mates[m];
  if (a < 1 || a > N || mt.id < 1 || mt.id > N || mt.dataset >= n_datasets) atomicMin(bad, (Ctl)m);
  owner[m] = (uint32_t)a;
}

// head[i] = 1 where sorted key i starts a run, for i in [0, F]; head[F] = 0 (the scan's total slot)
template <typename Key>
__global__ __launch_bounds__(kThreads) void k_run_heads(const Key* __restrict__ keys, uint64_t F,
                                                        uint32_t* __restrict__ head) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i > F) return;
  head[i] = i < F && (i == 0 || keys[i] != keys[i - 1]);
}

inline int bits_of(uint64_t x) {  // bits that hold every value <= x (at least 1)
  int b = 1;
  while (b < 64 && (x >> b)) ++b;
  return b;
}

// the -2 messages of the two checks above (`who` = the entry point's name)
inline int bad_place(mg_ctx* ctx, const char* who, const mg_place* d_places, uint64_t p, uint64_t n_edges) {
  mg_place pl{0, 0, 0};
  MG_TRY(hipMemcpy(&pl, d_places + p, sizeof(mg_place), hipMemcpyDeviceToHost));
  ctx->err = std::string(who) + ": placement " + std::to_string(p) + ": its edge " + std::to_string(pl.edge) +
             " is not below " + std::to_string(n_edges) + " (-2)";
  return -2;
}
inline int bad_mate(mg_ctx* ctx, const char* who, uint64_t m, uint32_t n_datasets, uint64_t n_reads) {
  ctx->err = std::string(who) + ": mate entry " + std::to_string(m) + ": its dataset is not below " +
             std::to_string(n_datasets) + " or its owner or mate ID lies outside 1.." + std::to_string(n_reads) + " (-2)";
  return -2;
}

// The placement CSR and the mate CSR of one call: the caller's, uploaded to
// scratch and checked (starts from 0, never decreasing), or, for a NULL start
// array, the resident ones of mg_build_placements (for n_edges edges) and
// mg_build_mate_pairs.  Fewer than 2^31 records each.
struct PairCsrs {
  Scratch<uint64_t> d_ps, d_ms;
  Scratch<mg_place> d_pl;
  Scratch<mg_mate> d_mt;
  const uint64_t* pstart = nullptr;
  const mg_place* prec = nullptr;
  uint64_t P = 0;
  const uint64_t* mstart = nullptr;
  const mg_mate* mrec = nullptr;
  uint64_t M = 0;

  int take(mg_ctx* ctx, const std::string& who, uint64_t n_reads, uint64_t n_edges, const uint64_t* place_start,
           const mg_place* places, const uint64_t* mate_start, const mg_mate* mates) {
    const uint64_t N = n_reads, entries = N + 2;
    hipStream_t st = ctx->stream;
    pstart = ctx->places.start.p;
    prec = ctx->places.recs.p;
    P = ctx->places.n;
    if (place_start) {
      if (place_start[0] != 0) return set_err(ctx, who + ": place_start[0] must be 0");
      for (uint64_t a = 0; a + 1 < entries; ++a)
        if (place_start[a + 1] < place_start[a]) return set_err(ctx, who + ": place_start must not decrease");
      P = place_start[entries - 1];
      if (P && !places) return set_err(ctx, who + ": null argument");
      MG_SCRATCH(d_ps, entries, "caller's placement starts");
      MG_SCRATCH(d_pl, P, "caller's placements");
      MG_TRY(hipMemcpyAsync(d_ps.p, place_start, entries * sizeof(uint64_t), hipMemcpyHostToDevice, st));
      if (P) MG_TRY(hipMemcpyAsync(d_pl.p, places, P * sizeof(mg_place), hipMemcpyHostToDevice, st));
      pstart = d_ps.p;
      prec = d_pl.p;
    } else if (!ctx->places.ready || ctx->n != N || ctx->places.edges.size() != n_edges) {
      return set_err(ctx, who + ": no resident placements of n_reads reads on n_edges edges: "
                                "mg_build_placements must run for these edges first, or pass a CSR");
    }
    mstart = ctx->mates.start.p;
    mrec = ctx->mates.recs.p;
    M = ctx->mates.n;
    if (mate_start) {
      if (mate_start[0] != 0) return set_err(ctx, who + ": mate_start[0] must be 0");
      for (uint64_t a = 0; a + 1 < entries; ++a)
        if (mate_start[a + 1] < mate_start[a]) return set_err(ctx, who + ": mate_start must not decrease");
      M = mate_start[entries - 1];
      if (M && !mates) return set_err(ctx, who + ": null argument");
      MG_SCRATCH(d_ms, entries, "caller's mate list starts");
      MG_SCRATCH(d_mt, M, "caller's mate lists");
      MG_TRY(hipMemcpyAsync(d_ms.p, mate_start, entries * sizeof(uint64_t), hipMemcpyHostToDevice, st));
      if (M) MG_TRY(hipMemcpyAsync(d_mt.p, mates, M * sizeof(mg_mate), hipMemcpyHostToDevice, st));
      mstart = d_ms.p;
      mrec = d_mt.p;
    } else if (!ctx->mates.ready || ctx->n != N) {
      return set_err(ctx, who + ": no resident mate lists of n_reads reads: mg_build_mate_pairs must run for "
                                "the current reads first, or pass a CSR");
    }
    if ((P >> 31) || (M >> 31)) return set_err(ctx, who + ": 2^31 or more placements or mate entries are not supported");
    return 0;
  }
};

#endif  // MG_STAGE_HPP_
