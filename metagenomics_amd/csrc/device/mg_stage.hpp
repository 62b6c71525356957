// mg_stage.hpp — INTERNAL: what the derived-stage translation units share
// beyond the context (mg_dataset.hip, mg_disc.hip, mg_comp.hip, mg_mates.hip,
// mg_contigs.hip, mg_places.hip, mg_chains.hip): the view of the resident reads, the launch
// grid, the CSR starts of sorted owners, control words, the copy tail of the
// mg_copy_* calls and the edge lists that mg_build_contigs and
// mg_build_placements both take.  (DevArray, Scratch and their growth macros
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

#endif  // MG_STAGE_HPP_
