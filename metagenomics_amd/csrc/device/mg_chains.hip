// mg_chains.hip — the safe chains of a freshly replayed graph on the device
// (mg_build_chains / mg_copy_chains, include/mg_overlap.h; the argument why
// contracting them first is exact: DESIGN.md §7d, host/mg_chains.cpp).
// Host counterpart of this file, and the definition of its output:
// mg::chains_build.
//
// Input: the caller's CSR (u order, lists in list order, twin indices).  It
// needs a context only.  Pipeline (one stream):
//   k_chain_check    : thread per node: dst in range, twin inside dst's list,
//                      twin[twin] = e, twin's dst = the node.  The first bad
//                      entry goes to a control word and the call returns -2
//                      before any kernel indexes through an entry;
//   k_chain_classify : thread per node: the interior flag (a 2-entry list, e0 no
//                      self-loop, matchEdgeType(twin(e0), e1));
//   k_chain_init     : thread per (node, port) state "leaving v through p": the
//                      next state (u, 1 - q), q = position of the twin in u's
//                      list, or, u not interior, the end: the twin's CSR index
//                      and u.  One hop, the edge's offset outward, the twin's
//                      inward;
//   k_chain_jump     : pointer jumping, one launch per round over two state
//                      buffers: a state with an unknown end takes over the state
//                      it links to (hops and both sums added).  A round reads
//                      one buffer and writes the other, so what it reads was
//                      written by an earlier launch: the kernel boundary makes
//                      it visible across the XCDs, and nothing needs an atomic
//                      or a coherent load.  After round j a state knows its end
//                      iff that is at most 2^j hops away, so ceil(log2(n_interior
//                      + 1)) + 1 rounds reach every end; a round that finds no
//                      new end stops the loop early (a chain of H > 2^(j-1) hops
//                      has a state at every distance 1..H, so round j finds one).
//                      States left unknown are pure cycles, or chains over a
//                      lowered cap (option "chain_rounds");
//   k_chain_safe     : thread per non-interior node a: the far end of each of its
//                      half-edges (dst, or the end of the chain it heads, 0 =
//                      unknown), then for each head the test: a < b, and b the
//                      far end of no other half-edge of a, none unknown.  Flags
//                      and 2 n per half-edge in CSR order;
//   two exclusive scans (hipCUB) over those: the chain index and `first` of every
//                      safe chain, in ascending start[a] + pa without a sort;
//   k_chain_emit     : thread per interior node whose two states end at a safe
//                      chain: its entry of the forward list at first + hops from
//                      a - 1 and of the reverse list at first + n + hops from b -
//                      1, offset and orientation from the twin of its half-edge
//                      towards a (towards b); the node next to a writes the record.
// Every index a kernel forms comes from an entry k_chain_check accepted: twins
// pair up and lie in their dst's list, so walks are reversible, hop counts from
// the two ends of a chain add up to n + 1 and every write lands inside its
// chain's range (the emit kernel still compares against the totals).
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "mg_overlap.h"
#include "mg_stage.hpp"

namespace {

typedef unsigned long long ull;

static_assert(sizeof(mg_chain_edge) == 12, "mg_chain_edge is 12 bytes");
static_assert(sizeof(mg_chain) == 48, "mg_chain is 48 bytes");
static_assert(sizeof(ChainState) == 32, "a state is 32 bytes");

constexpr uint32_t kKnown = 0x80000000u;  // ChainState::hops: the end is known
constexpr uint32_t kHops = 0x7FFFFFFFu;
constexpr int kMaxRounds = 40;
// control words
constexpr int kCtlBad = 0;       // first malformed half-edge (atomicMin, ~0 = none)
constexpr int kCtlInterior = 1;  // interior nodes
constexpr int kCtlUnsafe = 2;    // chains with known ends that are not safe
constexpr int kCtlUnknown = 3;   // states whose end stayed unknown
constexpr int kCtlRound = 4;     // + j: ends round j found
constexpr int kCtlWords = kCtlRound + kMaxRounds + 1;

// matchEdgeType (OverlapGraph.cpp:19-26) in bits
__device__ __forceinline__ bool chain_match(uint32_t t1, uint32_t t2) { return (t1 & 1u) == ((t2 >> 1) & 1u); }

// adds the wavefront's count of `flag` to *word with one atomic
__device__ __forceinline__ void wave_count(bool flag, ull* word) {
  const ull m = __ballot(flag);
  if (m && (threadIdx.x & (kWave - 1)) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(word, (ull)__popcll(m));
}

__global__ __launch_bounds__(kThreads) void k_chain_check(const uint64_t* __restrict__ start,
                                                          const mg_chain_edge* __restrict__ edges, uint64_t N,
                                                          ull* __restrict__ ctl) {
  const uint64_t v = (uint64_t)blockIdx.x * kThreads + threadIdx.x + 1;
  if (v > N) return;
  for (uint64_t e = start[v], end = start[v + 1]; e < end; ++e) {
    const uint32_t d = edges[e].dst, t = edges[e].twin;
    bool ok = d >= 1 && d <= N;
    if (ok) ok = t >= start[d] && t < start[d + 1];  // (inside the half-edges: start is monotone up to their number)
    if (ok) ok = edges[t].twin == e && edges[t].dst == v;
    if (!ok) {
      atomicMin(&ctl[kCtlBad], (ull)e);
      return;
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_chain_classify(const uint64_t* __restrict__ start,
                                                             const mg_chain_edge* __restrict__ edges, uint64_t N,
                                                             uint8_t* __restrict__ interior, ull* __restrict__ ctl) {
  const uint64_t v = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  bool in = false;
  if (v >= 1 && v <= N) {
    const uint64_t s = start[v];
    if (start[v + 1] - s == 2) {
      const mg_chain_edge e0 = edges[s], e1 = edges[s + 1];
      in = e0.dst != v && chain_match(edges[e0.twin].orient, e1.orient);
    }
  }
  if (v <= N + 1) interior[v] = in;
  wave_count(in, &ctl[kCtlInterior]);
}

__global__ __launch_bounds__(kThreads) void k_chain_init(const uint64_t* __restrict__ start,
                                                         const mg_chain_edge* __restrict__ edges, uint64_t N,
                                                         const uint8_t* __restrict__ interior,
                                                         ChainState* __restrict__ state) {
  const uint64_t x = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (x >= 2 * (N + 1)) return;
  const uint64_t v = x >> 1;
  ChainState s{0, 0, 0, 0, 0, 0};
  if (v >= 1 && interior[v]) {
    const mg_chain_edge e = edges[start[v] + (x & 1)];
    const uint32_t u = e.dst;
    s.out = e.offset;
    s.in = edges[e.twin].offset;
    if (interior[u]) {
      s.link = 2 * u + (1 - (uint32_t)(e.twin - start[u]));
      s.hops = 1;
    } else {
      s.link = e.twin;
      s.hops = 1 | kKnown;
      s.end = u;
    }
  }
  state[x] = s;
}

__global__ __launch_bounds__(kThreads) void k_chain_jump(const ChainState* __restrict__ in, ChainState* __restrict__ out,
                                                         uint64_t n_states, ull* __restrict__ found) {
  const uint64_t x = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  bool now = false;
  if (x < n_states) {
    ChainState s = in[x];
    if (s.hops && !(s.hops & kKnown)) {
      const ChainState t = in[s.link];  // (a state of an interior node: hops != 0)
      now = (t.hops & kKnown) != 0;
      s.link = t.link;
      s.end = t.end;
      const uint64_t hops = (uint64_t)s.hops + (t.hops & kHops);  // (saturates: only cycles get there)
      s.hops = (uint32_t)(hops < kHops ? hops : kHops) | (t.hops & kKnown);
      s.out += t.out;
      s.in += t.in;
    }
    out[x] = s;
  }
  wave_count(now, found);
}

__global__ __launch_bounds__(kThreads) void k_chain_safe(const uint64_t* __restrict__ start,
                                                         const mg_chain_edge* __restrict__ edges, uint64_t N,
                                                         const uint8_t* __restrict__ interior,
                                                         const ChainState* __restrict__ state,
                                                         uint32_t* __restrict__ far_end, uint32_t* __restrict__ head,
                                                         uint64_t* __restrict__ span, ull* __restrict__ ctl) {
  const uint64_t a = (uint64_t)blockIdx.x * kThreads + threadIdx.x + 1;
  if (a > N || interior[a]) return;
  const uint64_t lo = start[a], hi = start[a + 1];
  uint32_t unknown = 0;
  for (uint64_t h = lo; h < hi; ++h) {
    const mg_chain_edge e = edges[h];
    uint32_t f = e.dst;
    if (interior[f]) {
      const ChainState s = state[2 * (uint64_t)f + (1 - (e.twin - start[f]))];
      f = (s.hops & kKnown) ? s.end : 0;
      unknown += f == 0;
    }
    far_end[h] = f;
  }
  uint32_t unsafe = 0;
  for (uint64_t h = lo; h < hi; ++h) {
    const mg_chain_edge e = edges[h];
    if (!interior[e.dst]) continue;
    const ChainState s = state[2 * (uint64_t)e.dst + (1 - (e.twin - start[e.dst]))];
    if (!(s.hops & kKnown)) continue;
    const uint32_t b = s.end;
    if (!(a < b || (a == b && h < s.link))) continue;  // counted from its other end
    uint32_t same = 0;
    for (uint64_t k = lo; k < hi; ++k) same += far_end[k] == b;  // (this thread's own stores)
    if (a < b && same == 1 && unknown == 0) {
      head[h] = 1;
      span[h] = 2 * (uint64_t)(s.hops & kHops);
    } else {
      unsafe++;
    }
  }
  if (unsafe) atomicAdd(&ctl[kCtlUnsafe], (ull)unsafe);
}

__global__ __launch_bounds__(kThreads) void k_chain_emit(const uint64_t* __restrict__ start,
                                                         const mg_chain_edge* __restrict__ edges, uint64_t N,
                                                         const uint8_t* __restrict__ interior,
                                                         const ChainState* __restrict__ state,
                                                         const uint32_t* __restrict__ head,
                                                         const uint32_t* __restrict__ index,
                                                         const uint64_t* __restrict__ first_of, uint64_t n_chains,
                                                         uint64_t n_list, mg_chain* __restrict__ table,
                                                         uint32_t* __restrict__ reads, uint16_t* __restrict__ offs,
                                                         uint8_t* __restrict__ ors, ull* __restrict__ ctl) {
  const uint64_t v = (uint64_t)blockIdx.x * kThreads + threadIdx.x + 1;
  uint32_t unknown = 0;
  if (v <= N && interior[v]) {
    const ChainState s0 = state[2 * v], s1 = state[2 * v + 1];
    unknown = !(s0.hops & kKnown) + !(s1.hops & kKnown);
    if (!unknown) {
      const int x = head[s0.link] ? 0 : head[s1.link] ? 1 : -1;  // the port towards a
      if (x >= 0) {
        const ChainState sa = x ? s1 : s0, sb = x ? s0 : s1;
        const uint64_t ha = sa.hops & kHops, hb = sb.hops & kHops, n = ha + hb - 1;
        const uint64_t c = index[sa.link], first = first_of[sa.link];
        const uint64_t pf = first + ha - 1, pr = first + n + hb - 1;
        if (c < n_chains && ha >= 1 && hb >= 1 && pf < n_list && pr < n_list) {
          const mg_chain_edge to_a = edges[start[v] + x], to_b = edges[start[v] + 1 - x];
          const mg_chain_edge in_f = edges[to_a.twin], in_r = edges[to_b.twin];
          reads[pf] = (uint32_t)v;
          offs[pf] = in_f.offset;
          ors[pf] = in_f.orient & 1;
          reads[pr] = (uint32_t)v;
          offs[pr] = in_r.offset;
          ors[pr] = in_r.orient & 1;
          if (ha == 1) {
            const mg_chain_edge at_a = edges[sa.link], at_b = edges[sb.link];
            mg_chain r;
            r.a = sa.end;
            r.b = sb.end;
            r.pa = (uint32_t)(sa.link - start[sa.end]);
            r.pb = (uint32_t)(sb.link - start[sb.end]);
            r.n = (uint32_t)n;
            r.orient_fwd = (uint8_t)((at_a.orient & 2) | (edges[at_b.twin].orient & 1));
            r.orient_rev = (uint8_t)((at_b.orient & 2) | (edges[at_a.twin].orient & 1));
            r.pad[0] = r.pad[1] = 0;
            r.offset_fwd = sa.in + sb.out;
            r.offset_rev = sa.out + sb.in;
            r.first = first;
            table[c] = r;
          }
        }
      }
    }
  }
  if (unknown) atomicAdd(&ctl[kCtlUnknown], (ull)unknown);
}

uint32_t ceil_log2(uint64_t x) {
  uint32_t r = 0;
  while (r < 63 && (1ull << r) < x) ++r;
  return r;
}

// which rule half-edge e breaks (the host's copy of the caller's arrays)
std::string chain_fault(const uint64_t* start, const mg_chain_edge* edges, uint64_t N, uint64_t e) {
  const uint64_t v = (uint64_t)(std::upper_bound(start, start + N + 2, e) - start) - 1;
  const mg_chain_edge& x = edges[e];
  const std::string who =
      "half-edge " + std::to_string(e) + " (read " + std::to_string(v) + ", position " + std::to_string(e - start[v]) + ")";
  if (x.dst < 1 || x.dst > N) return who + ": dst " + std::to_string(x.dst) + " outside 1.." + std::to_string(N);
  if (x.twin < start[x.dst] || x.twin >= start[x.dst + 1])
    return who + ": twin " + std::to_string(x.twin) + " outside the list of its dst " + std::to_string(x.dst);
  if (edges[x.twin].twin != e) return who + ": twin[twin] is " + std::to_string(edges[x.twin].twin);
  return who + ": its twin's dst is " + std::to_string(edges[x.twin].dst);
}

int build_chains(mg_ctx* ctx, const uint64_t* start, const mg_chain_edge* edges, uint64_t N, uint64_t E,
                 uint64_t* info) {
  ChainStage& cs = ctx->chains;
  hipStream_t st = ctx->stream;
  const uint64_t entries = N + 2, n_states = 2 * (N + 1);
  MG_GROW(cs.start, entries, "d_chain_start");
  MG_GROW(cs.edges, E, "d_chain_edges");
  MG_GROW(cs.interior, entries, "d_chain_interior");
  MG_GROW(cs.state[0], n_states, "d_chain_state");
  MG_GROW(cs.state[1], n_states, "d_chain_state");
  MG_GROW(cs.far_end, E, "d_chain_far");
  MG_GROW(cs.head, E + 1, "d_chain_head");
  MG_GROW(cs.span, E + 1, "d_chain_span");
  MG_GROW(cs.ctl, kCtlWords, "d_chain_ctl");
  Scratch<uint32_t> index;  // exclusive scan of head: the chain index of a safe head
  Scratch<uint64_t> first;  // exclusive scan of span: where its lists start
  MG_SCRATCH(index, E + 1, "chain indices");
  MG_SCRATCH(first, E + 1, "chain list starts");
  size_t tb32 = 0, tb64 = 0;
  MG_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb32, cs.head.p, index.p, (int64_t)(E + 1), st));
  MG_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb64, cs.span.p, first.p, (int64_t)(E + 1), st));
  MG_GROW(cs.tmp, std::max(tb32, tb64), "d_chain_tmp");
  MG_TRY(hipMemcpyAsync(cs.start.p, start, entries * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  if (E) MG_TRY(hipMemcpyAsync(cs.edges.p, edges, E * sizeof(mg_chain_edge), hipMemcpyHostToDevice, st));
  MG_TRY(ctl_fill(st, cs.ctl.p, 1, ~0ull));
  MG_TRY(ctl_fill(st, cs.ctl.p + 1, kCtlWords - 1, 0));
  MG_TRY(hipMemsetAsync(cs.head.p, 0, (E + 1) * sizeof(uint32_t), st));
  MG_TRY(hipMemsetAsync(cs.span.p, 0, (E + 1) * sizeof(uint64_t), st));

  MG_TRY(cs.ev.start(st));
  hipLaunchKernelGGL(k_chain_check, dim3(blocks_for(N)), dim3(kThreads), 0, st, cs.start.p, cs.edges.p, N, cs.ctl.p);
  MG_TRY(hipGetLastError());
  ull w[kCtlWords];
  MG_TRY(ctl_read(st, cs.ctl.p, 1, w));
  if (w[kCtlBad] != ~0ull) {
    ctx->err = "mg_build_chains: " + chain_fault(start, edges, N, (uint64_t)w[kCtlBad]) + " (-2)";
    return -2;
  }
  hipLaunchKernelGGL(k_chain_classify, dim3(blocks_for(entries)), dim3(kThreads), 0, st, cs.start.p, cs.edges.p, N,
                     cs.interior.p, cs.ctl.p);
  MG_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_chain_init, dim3(blocks_for(n_states)), dim3(kThreads), 0, st, cs.start.p, cs.edges.p, N,
                     cs.interior.p, cs.state[0].p);
  MG_TRY(hipGetLastError());
  MG_TRY(ctl_read(st, cs.ctl.p, kCtlRound, w));
  const uint64_t n_interior = w[kCtlInterior];
  uint32_t cap = ceil_log2(n_interior + 1) + 1;
  if (cs.rounds) cap = std::min(cap, cs.rounds);
  cap = std::min<uint32_t>(cap, kMaxRounds);
  uint32_t rounds = 0;
  int cur = 0;
  for (uint32_t j = 1; n_interior && j <= cap; ++j) {
    hipLaunchKernelGGL(k_chain_jump, dim3(blocks_for(n_states)), dim3(kThreads), 0, st, cs.state[cur].p,
                       cs.state[cur ^ 1].p, n_states, cs.ctl.p + kCtlRound + j);
    MG_TRY(hipGetLastError());
    cur ^= 1;
    rounds = j;
    ull found = 0;
    MG_TRY(ctl_read(st, cs.ctl.p + kCtlRound + j, 1, &found));
    if (!found) break;
  }
  hipLaunchKernelGGL(k_chain_safe, dim3(blocks_for(N)), dim3(kThreads), 0, st, cs.start.p, cs.edges.p, N,
                     cs.interior.p, cs.state[cur].p, cs.far_end.p, cs.head.p, cs.span.p, cs.ctl.p);
  MG_TRY(hipGetLastError());
  size_t tb = cs.tmp.cap;
  MG_TRY(hipcub::DeviceScan::ExclusiveSum(cs.tmp.p, tb, cs.head.p, index.p, (int64_t)(E + 1), st));
  tb = cs.tmp.cap;
  MG_TRY(hipcub::DeviceScan::ExclusiveSum(cs.tmp.p, tb, cs.span.p, first.p, (int64_t)(E + 1), st));
  uint32_t n_chains = 0;  // (entry E of both inputs is 0: the exclusive sums there are the totals)
  uint64_t n_list = 0;
  MG_TRY(hipMemcpyAsync(&n_chains, index.p + E, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  MG_TRY(hipMemcpyAsync(&n_list, first.p + E, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  MG_TRY(hipStreamSynchronize(st));
  MG_GROW(cs.table, n_chains, "d_chains");
  MG_GROW(cs.reads, n_list, "d_chain_reads");
  MG_GROW(cs.offs, n_list, "d_chain_offs");
  MG_GROW(cs.ors, n_list, "d_chain_ors");
  hipLaunchKernelGGL(k_chain_emit, dim3(blocks_for(N)), dim3(kThreads), 0, st, cs.start.p, cs.edges.p, N, cs.interior.p,
                     cs.state[cur].p, cs.head.p, index.p, first.p, (uint64_t)n_chains, n_list, cs.table.p, cs.reads.p,
                     cs.offs.p, cs.ors.p, cs.ctl.p);
  MG_TRY(hipGetLastError());
  MG_TRY(cs.ev.end(st));
  MG_TRY(ctl_read(st, cs.ctl.p, kCtlRound, w));
  cs.n_chains = n_chains;
  cs.n_list = n_list;
  info[MG_CHAIN_INTERIOR] = n_interior;
  info[MG_CHAIN_SAFE] = n_chains;
  info[MG_CHAIN_CONTRACTED] = n_list / 2;
  info[MG_CHAIN_UNSAFE] = w[kCtlUnsafe];
  info[MG_CHAIN_UNRESOLVED] = w[kCtlUnknown];
  info[MG_CHAIN_ROUNDS] = rounds;
  return 0;
}

}  // namespace

extern "C" {

int mg_build_chains(mg_ctx* ctx, const uint64_t* start, const mg_chain_edge* edges, uint64_t n_reads,
                    uint64_t n_edges, uint64_t* n_chains, uint64_t* n_list, uint64_t* info, float* device_ms) {
  if (!ctx) return -1;
  ctx->err.clear();
  if (n_chains) *n_chains = 0;
  if (n_list) *n_list = 0;
  if (device_ms) *device_ms = 0.f;
  ctx->chains.ready = false;
  if (!start || (n_edges && !edges)) return set_err(ctx, "mg_build_chains: null argument");
  MG_TRY(hipSetDevice(ctx->device));
  if (whole_multiset(ctx, "mg_build_chains")) return -1;
  // the starts on the host: the kernels loop over [start[v], start[v + 1])
  auto malformed = [&](const std::string& s) {
    ctx->err = "mg_build_chains: " + s + " (-2)";
    return -2;
  };
  if (n_reads >= (1ull << 31) || n_edges >= (1ull << 32))
    return malformed("2^31 reads or 2^32 half-edges and more are not supported");
  if (start[0] != 0 || start[1] != 0) return malformed("start[0] and start[1] must be 0");
  for (uint64_t v = 1; v <= n_reads; ++v)
    if (start[v + 1] < start[v] || start[v + 1] > n_edges)
      return malformed("start[" + std::to_string(v + 1) + "] decreases or exceeds the " + std::to_string(n_edges) +
                       " half-edges");
  if (start[n_reads + 1] != n_edges) return malformed("start[n_reads + 1] is not the number of half-edges");
  uint64_t counters[MG_CHAIN_INFO] = {};
  const int rc = build_chains(ctx, start, edges, n_reads, n_edges, counters);
  if (rc) return rc;
  MG_TRY(ctx->chains.ev.elapsed(device_ms));
  ctx->chains.ready = true;
  if (n_chains) *n_chains = ctx->chains.n_chains;
  if (n_list) *n_list = ctx->chains.n_list;
  if (info) std::copy(counters, counters + MG_CHAIN_INFO, info);
  return 0;
}

int mg_copy_chains(mg_ctx* ctx, mg_chain* chains, uint64_t chain_cap, uint32_t* reads, uint16_t* offs, uint8_t* ors,
                   uint64_t list_cap) {
  if (!ctx) return -1;
  ctx->err.clear();
  MG_TRY(hipSetDevice(ctx->device));
  if (!ctx->chains.ready) return set_err(ctx, "mg_copy_chains: mg_build_chains must succeed on this context first");
  const ChainStage& cs = ctx->chains;
  hipStream_t st = ctx->stream;
  const uint64_t c = chains ? std::min(chain_cap, cs.n_chains) : 0, l = std::min(list_cap, cs.n_list);
  if (c) MG_TRY(hipMemcpyAsync(chains, cs.table.p, c * sizeof(mg_chain), hipMemcpyDeviceToHost, st));
  if (l && reads) MG_TRY(hipMemcpyAsync(reads, cs.reads.p, l * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (l && offs) MG_TRY(hipMemcpyAsync(offs, cs.offs.p, l * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
  if (l && ors) MG_TRY(hipMemcpyAsync(ors, cs.ors.p, l, hipMemcpyDeviceToHost, st));
  MG_TRY(hipStreamSynchronize(st));
  return 0;
}

}  // extern "C"
