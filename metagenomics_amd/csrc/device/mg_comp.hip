// mg_comp.hip — connected components of the per-read discovery lists on the
// device (mg_build_components / mg_copy_components, include/mg_overlap.h).
//
// Why: the reference's outer loop (OverlapGraph.cpp:144-204) explores one
// component at a time from its smallest read ID, and nothing it touches
// meanwhile belongs to another component.  With the components known the host
// replays them in parallel (GraphReplay::build_from with a table,
// host/mg_graph.cpp) and gets the same pool and lists.  Host counterpart of
// this file: mg::Components::build.
//
// Input: the CSR lists of mg_build_discoveries (d_disc_start, d_disc), already
// resident.  Pipeline (one stream):
//   k_comp_init    : parent[v] = v, self counts = 0;
//   k_comp_hook    : union-find.  A wavefront takes 32 consecutive reads (their
//                    records are contiguous) and strides over the records with
//                    its 64 lanes, whatever the degrees; the lane finds its
//                    record's read A by a search over the 33 list starts held
//                    in the lanes.  dst == A counts a self record; dst < A is a
//                    union (every non-self pair is in both lists, so dst > A is
//                    the other list's work);
//   k_comp_flatten : a launch of its own, so the kernel boundary has made every
//                    hook visible: label[A] = the root of A's tree;
//   k_comp_sums    : per read, reads / records / self records added to its
//                    root's counters.  A workgroup sums its 4,096 consecutive
//                    reads per root in an LDS table first and adds each table
//                    entry with one global atomic per counter (a few large
//                    components would otherwise put every read's atomics on a
//                    handful of addresses: C3, 12 components, 29 ms that way);
//   table          : flag the roots that hold records, exclusive scan
//                    (rocprim), scatter: ascending root falls out.
//
// THE INVARIANT of the union-find: parent[v] <= v at all times, and an entry
// only ever decreases.  The per-XCD L2s are not coherent with each other and a
// CU's L1 is never refreshed by another CU's stores, so a plain load of
// parent[] may return an old value.  Under the invariant an old value is an
// older ancestor of v in the same tree, nothing worse.  Every write to parent[]
// is an atomic, which executes at the memory side:
//   * a hook is atomicCAS(&parent[big], big, small) with small < big: it
//     succeeds only when big is a root in memory, and a failed one returns
//     big's parent in memory, from where the union continues.  small may be a
//     non-root member of its tree (a stale find): hooking under any member of
//     the right tree is still a correct union;
//   * path halving is atomicMin(&parent[v], grandparent): it only lowers, and
//     to an ancestor.
// Nothing here relies on a plain load being fresh; staleness costs extra steps
// only.  A union ends: the larger of its two candidates strictly decreases with
// every failed hook.  The labels are the minimum of each tree (roots are
// minima, since parent[v] <= v), so they do not depend on the order of the
// atomics.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>  // (brings rocprim in, as in mg_disc.hip)

#include <algorithm>
#include <cstdint>
#include <string>

#include "mg_overlap.h"
#include "mg_stage.hpp"

namespace {

constexpr int kWaveReads = 32;   // consecutive reads one wavefront of k_comp_hook takes
constexpr int kSumReads = 4096;  // consecutive reads one workgroup of k_comp_sums takes
constexpr int kSumSlotsLog2 = 9;
constexpr int kSumSlots = 1 << kSumSlotsLog2;  // roots it sums in LDS (8 KiB)

static_assert(sizeof(mg_comp) == 16, "mg_comp is 16 bytes");

__global__ __launch_bounds__(kThreads) void k_comp_init(uint32_t* __restrict__ parent,
                                                        uint32_t* __restrict__ self_cnt, uint64_t entries) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= entries) return;
  parent[i] = (uint32_t)i;
  self_cnt[i] = 0;
}

// an ancestor of v that looked like a root (plain loads: see the header)
__device__ __forceinline__ uint32_t find_root(uint32_t* parent, uint32_t v) {
  for (;;) {
    const uint32_t p = parent[v];
    if (p == v) return v;
    const uint32_t g = parent[p];
    if (g == p) return p;
    atomicMin(&parent[v], g);  // path halving
    v = g;
  }
}

__device__ __forceinline__ void unite(uint32_t* parent, uint32_t a, uint32_t b) {
  uint32_t ra = find_root(parent, a), rb = find_root(parent, b);
  while (ra != rb) {
    const uint32_t big = ra > rb ? ra : rb, small = ra > rb ? rb : ra;
    const uint32_t old = atomicCAS(&parent[big], big, small);
    if (old == big || old == small) return;
    // big has a parent in memory: old < big.  max(ra, rb) strictly decreases.
    ra = find_root(parent, old);
    rb = small;
  }
}

__global__ __launch_bounds__(kThreads) void k_comp_hook(const uint64_t* __restrict__ disc,
                                                        const uint64_t* __restrict__ start, uint32_t n,
                                                        uint32_t* parent, uint32_t* __restrict__ self_cnt) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint64_t wave = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) / kWave;
  const uint64_t a0 = 1 + wave * kWaveReads;
  if (a0 > n) return;  // (whole wavefront)
  const uint64_t s0 = start[a0];
  const uint64_t at = a0 + (uint64_t)lane;
  // lanes 0..32: the list starts relative to s0 (clamped past the last read, so monotone over all lanes)
  const uint32_t rel = (uint32_t)(start[at <= (uint64_t)n + 1 ? at : (uint64_t)n + 1] - s0);
  const uint32_t total = __shfl(rel, kWaveReads);
  for (uint32_t base = 0; base < total; base += kWave) {  // (uniform: every lane runs the shuffles)
    const bool active = base + (uint32_t)lane < total;
    const uint32_t p = active ? base + (uint32_t)lane : base;
    int lo = 0, hi = kWaveReads - 1;  // the last t with rel[t] <= p
#pragma unroll
    for (int it = 0; it < 5; ++it) {
      const int mid = (lo + hi + 1) >> 1;
      const uint32_t sm = __shfl(rel, mid);
      if (lo < hi) {
        if (sm <= p) lo = mid;
        else hi = mid - 1;
      }
    }
    if (!active) continue;
    const uint32_t a = (uint32_t)(a0 + (uint64_t)lo);  // <= n: a clamped start is never <= p
    const uint32_t dst = (uint32_t)disc[s0 + p];       // mg_disc::dst
    if (dst == a)
      atomicAdd(&self_cnt[a], 1u);
    else if (dst >= 1 && dst < a)
      unite(parent, a, dst);
  }
}

__global__ __launch_bounds__(kThreads) void k_comp_flatten(const uint32_t* __restrict__ parent, uint32_t n,
                                                           uint32_t* __restrict__ label) {
  const uint64_t a = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (a > n) return;
  uint32_t v = (uint32_t)a;
  for (uint32_t p = parent[v]; p != v; p = parent[v]) v = p;  // (p < v: ends)
  label[a] = v;
}

// reads / records / self records per root.  acc_reads, acc_disc, acc_self are
// indexed by root and zero on entry.  A workgroup takes kSumReads consecutive
// reads and sums per root in a small LDS table first (slot = hash of the root,
// claimed by the first root that comes; a root that finds its slot taken by
// another adds to global memory directly), then adds every claimed slot with
// one global atomic per counter.
__global__ __launch_bounds__(kThreads) void k_comp_sums(const uint32_t* __restrict__ label,
                                                        const uint64_t* __restrict__ start,
                                                        const uint32_t* __restrict__ self_cnt, uint32_t n,
                                                        uint32_t* __restrict__ acc_reads,
                                                        uint32_t* __restrict__ acc_disc,
                                                        uint32_t* __restrict__ acc_self) {
  __shared__ uint32_t s_root[kSumSlots], s_reads[kSumSlots], s_disc[kSumSlots], s_self[kSumSlots];
  for (int i = threadIdx.x; i < kSumSlots; i += kThreads) s_root[i] = s_reads[i] = s_disc[i] = s_self[i] = 0;
  __syncthreads();
  const uint64_t a0 = 1 + (uint64_t)blockIdx.x * kSumReads;
  for (int i = threadIdx.x; i < kSumReads; i += kThreads) {
    const uint64_t a = a0 + (uint64_t)i;
    if (a > n) break;
    const uint32_t d = (uint32_t)(start[a + 1] - start[a]);
    if (!d) continue;  // (a read without records is a component without records: not in the table)
    const uint32_t r = label[a], s = self_cnt[a];
    const uint32_t slot = (r * 2654435761u) >> (32 - kSumSlotsLog2);
    const uint32_t owner = atomicCAS(&s_root[slot], 0u, r);  // (roots are >= 1)
    if (owner == 0 || owner == r) {
      atomicAdd(&s_reads[slot], 1u);
      atomicAdd(&s_disc[slot], d);
      if (s) atomicAdd(&s_self[slot], s);
    } else {
      atomicAdd(&acc_reads[r], 1u);
      atomicAdd(&acc_disc[r], d);
      if (s) atomicAdd(&acc_self[r], s);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kSumSlots; i += kThreads) {
    const uint32_t r = s_root[i];
    if (!r) continue;
    atomicAdd(&acc_reads[r], s_reads[i]);
    atomicAdd(&acc_disc[r], s_disc[i]);
    if (s_self[i]) atomicAdd(&acc_self[r], s_self[i]);
  }
}

struct CompFlag {
  __host__ __device__ uint32_t operator()(uint32_t records) const { return records ? 1u : 0u; }
};

__global__ __launch_bounds__(kThreads) void k_comp_table(const uint32_t* __restrict__ acc_reads,
                                                         const uint32_t* __restrict__ acc_disc,
                                                         const uint32_t* __restrict__ acc_self,
                                                         const uint32_t* __restrict__ pos, uint32_t n,
                                                         uint64_t n_comp, mg_comp* __restrict__ out) {
  const uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x + 1;
  if (r > n || !acc_disc[r]) return;
  const uint32_t at = pos[r];
  if (at < n_comp) out[at] = mg_comp{(uint32_t)r, acc_reads[r], acc_disc[r], acc_self[r]};
}

int label_components(mg_ctx* ctx) {
  const uint64_t N = ctx->n, entries = N + 2;
  DiscStage& ds = ctx->disc;  // its lists are the input; its count array and temporary storage are borrowed
  CompStage& cs = ctx->comp;
  cs.n = 0;
  MG_GROW(cs.parent, entries, "d_comp_parent");
  MG_GROW(cs.label, entries, "d_comp_label");
  MG_GROW(cs.acc, 2 * entries, "d_comp_acc");
  if (ds.cnt.cap < entries || !ds.cnt.p || ds.start.cap < entries || !ds.start.p ||
      (ds.n && (!ds.recs.p || ds.recs.cap < ds.n)))
    return set_err(ctx, "mg_build_components: the discovery-list buffers are missing");
  uint32_t* self_cnt = ds.cnt.p;  // (free after mg_build_discoveries) self records per read, then the scan's output
  uint32_t* acc_reads = cs.parent.p;  // (after the flatten)
  uint32_t* acc_disc = cs.acc.p;
  uint32_t* acc_self = cs.acc.p + entries;
  auto flags = rocprim::make_transform_iterator(acc_disc, CompFlag());
  size_t tb = 0;
  MG_TRY(rocprim::exclusive_scan(nullptr, tb, flags, self_cnt, 0u, (size_t)entries, rocprim::plus<uint32_t>(),
                                 ctx->stream));
  MG_GROW(ds.tmp, tb, "d_disc_tmp");
  tb = ds.tmp.cap;

  hipLaunchKernelGGL(k_comp_init, dim3(blocks_for(entries)), dim3(kThreads), 0, ctx->stream, cs.parent.p,
                     self_cnt, entries);
  MG_TRY(hipGetLastError());
  if (N && ds.n) {
    const uint64_t waves = (N + kWaveReads - 1) / kWaveReads;
    hipLaunchKernelGGL(k_comp_hook, dim3(blocks_for(waves * kWave)), dim3(kThreads), 0, ctx->stream, ds.recs.p,
                       ds.start.p, (uint32_t)N, cs.parent.p, self_cnt);
    MG_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_comp_flatten, dim3(blocks_for(N + 1)), dim3(kThreads), 0, ctx->stream, cs.parent.p,
                     (uint32_t)N, cs.label.p);
  MG_TRY(hipGetLastError());
  if (!N || !ds.n) return 0;
  MG_TRY(hipMemsetAsync(acc_reads, 0, entries * sizeof(uint32_t), ctx->stream));
  MG_TRY(hipMemsetAsync(cs.acc.p, 0, 2 * entries * sizeof(uint32_t), ctx->stream));
  const uint32_t sum_blocks = (uint32_t)((N + kSumReads - 1) / kSumReads);
  hipLaunchKernelGGL(k_comp_sums, dim3(sum_blocks), dim3(kThreads), 0, ctx->stream,
                     cs.label.p, ds.start.p, self_cnt, (uint32_t)N, acc_reads, acc_disc, acc_self);
  MG_TRY(hipGetLastError());
  MG_TRY(rocprim::exclusive_scan(ds.tmp.p, tb, flags, self_cnt, 0u, (size_t)entries,
                                 rocprim::plus<uint32_t>(), ctx->stream));
  uint32_t count = 0;  // (entry N + 1 is no root: the exclusive sum there is the total)
  MG_TRY(hipMemcpyAsync(&count, self_cnt + N + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  MG_TRY(hipStreamSynchronize(ctx->stream));
  MG_GROW(cs.table, count, "d_comp");
  hipLaunchKernelGGL(k_comp_table, dim3(blocks_for(N)), dim3(kThreads), 0, ctx->stream, acc_reads, acc_disc, acc_self,
                     self_cnt, (uint32_t)N, (uint64_t)count, cs.table.p);
  MG_TRY(hipGetLastError());
  cs.n = count;
  return 0;
}

}  // namespace

extern "C" {

int mg_build_components(mg_ctx* ctx, uint64_t* n_comp, float* device_ms) {
  if (!ctx) return -1;
  ctx->err.clear();
  MG_TRY(hipSetDevice(ctx->device));
  if (n_comp) *n_comp = 0;
  if (device_ms) *device_ms = 0.f;
  ctx->comp.ready = false;
  if (whole_multiset(ctx, "mg_build_components")) return -1;
  if (!ctx->index_ready || !ctx->rows_found || !ctx->disc.ready)
    return set_err(ctx, "mg_build_components: mg_build_discoveries must run for the current rows first");
  MG_TRY(ctx->comp.ev.start(ctx->stream));
  const int rc = label_components(ctx);
  if (rc) return rc;
  MG_TRY(ctx->comp.ev.end(ctx->stream));
  MG_TRY(ctx->comp.ev.wait());
  MG_TRY(ctx->comp.ev.elapsed(device_ms));
  ctx->comp.ready = true;
  if (n_comp) *n_comp = ctx->comp.n;
  return 0;
}

int mg_copy_components(mg_ctx* ctx, uint32_t* label, mg_comp* comps, uint64_t cap, uint64_t* n_copied) {
  if (!ctx) return -1;
  ctx->err.clear();
  MG_TRY(hipSetDevice(ctx->device));
  if (n_copied) *n_copied = 0;
  if (whole_multiset(ctx, "mg_copy_components")) return -1;
  if (!ctx->index_ready || !ctx->rows_found || !ctx->disc.ready || !ctx->comp.ready)
    return set_err(ctx, "mg_copy_components: mg_build_components must run for the current lists first");
  return copy_csr(ctx, ctx->comp.label.p, ctx->n + 1, label, ctx->comp.table.p, ctx->comp.n, comps, cap, n_copied);
}

}  // extern "C"
