// mg_disc.hip — the per-read discovery lists D(A) built on the device
// (mg_build_discoveries / mg_copy_discoveries, include/mg_overlap.h).
//
// Host path replaced: mg::Discoveries::build (host/mg_graph.cpp), i.e. the
// regrouping of the directed discovery multiset M into insertAllEdgesOfRead's
// loop order (the reference's OverlapGraph.cpp:529-565): D(A) =
// the rows with src = A ordered by (window j, partner ID, key o), each self row
// (present twice in M) once.
//
// Pipeline (one stream, all in HBM):
//   k_disc_count    : thread per row over the probe's per-wavefront row regions
//                     (walked as k_rows_digest walks them) -> rows per src;
//   exclusive scan  : start[A] (rocprim);
//   k_disc_scatter  : second walk: key = j << 34 | dst << 2 | o (50 bits) written
//                     through per-read cursors into the CSR array (any order
//                     inside a segment);
//   k_disc_classify : reads of degree > 64 listed for the workgroup path
//                     (<= block cap) or the oversize path;
//   k_disc_wave     : degree <= 64: one wavefront takes 32 consecutive reads and
//                     sorts runs of whole segments that fit its 64 lanes in
//                     registers (bitonic network over __shfl_xor; the segment's
//                     index rides above the key so segments stay apart);
//   k_disc_block    : 64 < degree <= cap: one workgroup per read, keys in LDS;
//   oversize        : gathered, rocprim::segmented_radix_sort_keys over those
//                     segments only, written back;
// every path ends by turning its sorted keys into mg_disc records in place and
// marking the second copy of a self row dead; only when one was marked (tandem
// repeats) a last pass compacts the lists.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>  // (brings rocprim in, as in mg_kernels.hip)

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>

#include "mg_overlap.h"
#include "mg_stage.hpp"

namespace {

constexpr int kWaveReads = 32;         // consecutive reads one wavefront of k_disc_wave takes
constexpr uint32_t kBlockCap = 2048;   // keys a workgroup sorts in LDS (16 KiB: 8 workgroups = 32 waves per CU in 128 of 160 KiB)
constexpr uint64_t kKeyMask = (1ULL << 50) - 1;
constexpr uint64_t kDead = 0xFFULL << 56;  // mg_disc::o = 0xFF: the dropped copy of a self row
// control words
enum { kErr = 0, kMid = 1, kBig = 2, kDup = 3, kDiscCtl = 4 };
// error bits (the codes of mg::Discoveries::build)
enum : unsigned long long { kErrId = 1, kErrJ = 2, kErrSelf = 4 };

static_assert(sizeof(mg_disc) == 8, "mg_disc is 8 bytes");

__device__ __forceinline__ uint32_t orient_to_key(uint32_t orient) {  // OverlapGraph.cpp:550-556 inverted
  return orient == 3 ? 0u : orient == 0 ? 1u : orient == 2 ? 2u : 3u;
}
__device__ __forceinline__ uint32_t key_to_orient(uint32_t o) { return o == 0 ? 3u : o == 1 ? 0u : o == 2 ? 2u : 1u; }

__device__ __forceinline__ uint32_t read_len(const uint16_t* __restrict__ len, const uint32_t* __restrict__ phys,
                                             uint32_t id) {
  return len[phys ? phys[id - 1] : id - 1];
}

// rows of region r: min(cnt[r], cap), as k_rows_digest
template <typename F>
__device__ __forceinline__ void for_each_row(const uint32_t* __restrict__ rows, uint64_t cap,
                                             const unsigned long long* __restrict__ cnt, uint64_t nreg, F f) {
  for (uint64_t reg = blockIdx.x; reg < nreg; reg += gridDim.x) {
    const uint64_t c = cnt[reg] < cap ? cnt[reg] : cap;
    for (uint64_t i = threadIdx.x; i < c; i += kThreads) f(rows + (reg * cap + i) * 3);
  }
}

__global__ __launch_bounds__(kThreads) void k_disc_count(const uint32_t* __restrict__ rows, uint64_t cap,
                                                         const unsigned long long* __restrict__ cnt, uint64_t nreg,
                                                         uint32_t n, uint32_t* __restrict__ deg,
                                                         unsigned long long* __restrict__ ctl) {
  for_each_row(rows, cap, cnt, nreg, [&](const uint32_t* r) {
    const uint32_t src = r[0], dst = r[1];
    if (src < 1 || src > n || dst < 1 || dst > n) {
      atomicOr(&ctl[kErr], kErrId);
      return;
    }
    atomicAdd(&deg[src], 1u);
  });
}

__global__ __launch_bounds__(kThreads) void k_disc_scatter(const uint32_t* __restrict__ rows, uint64_t cap,
                                                           const unsigned long long* __restrict__ cnt, uint64_t nreg,
                                                           uint32_t n, uint32_t h, const uint16_t* __restrict__ len,
                                                           const uint32_t* __restrict__ phys,
                                                           const uint64_t* __restrict__ start,
                                                           uint32_t* __restrict__ cursor, uint64_t* __restrict__ disc,
                                                           unsigned long long* __restrict__ ctl) {
  for_each_row(rows, cap, cnt, nreg, [&](const uint32_t* r) {
    const uint32_t src = r[0], dst = r[1];
    if (src < 1 || src > n || dst < 1 || dst > n) return;  // (counted out by k_disc_count)
    const uint32_t offset = r[2] & 0xFFFFu, o = orient_to_key((r[2] >> 16) & 0xFFu);
    const int n1 = (int)read_len(len, phys, src);
    // window j: offset = j for o = 0, 2; offset = n1 - h - j for o = 1, 3 (:550-557)
    const int j = (o & 1u) ? n1 - (int)h - (int)offset : (int)offset;
    if (j < 1 || j >= n1 - (int)h) atomicOr(&ctl[kErr], kErrJ);
    const uint64_t pos = start[src] + atomicAdd(&cursor[src], 1u);
    disc[pos] = ((uint64_t)((uint32_t)j & 0xFFFFu) << 34) | ((uint64_t)dst << 2) | o;
  });
}

// reads above the wavefront path's 64 records: the workgroup path's from the
// front of list, the oversized from its back with their offsets in the gather
// buffer (index and offset come from one atomic, so boff[i + 1] is segment i's end)
__global__ __launch_bounds__(kThreads) void k_disc_classify(const uint64_t* __restrict__ start, uint32_t n,
                                                            uint32_t block_cap, uint32_t* __restrict__ list,
                                                            uint64_t list_n, uint32_t* __restrict__ boff,
                                                            unsigned long long* __restrict__ ctl) {
  const uint64_t a = (uint64_t)blockIdx.x * kThreads + threadIdx.x + 1;
  if (a > n) return;
  const uint64_t d = start[a + 1] - start[a];
  if (d <= (uint64_t)kWave) return;
  if (d <= block_cap) {
    const unsigned long long i = atomicAdd(&ctl[kMid], 1ULL);
    if (i < list_n) list[i] = (uint32_t)a;
  } else {
    const unsigned long long old = atomicAdd(&ctl[kBig], (1ULL << 32) | d);
    const uint64_t i = old >> 32;
    const uint32_t off = (uint32_t)old;
    if (i < list_n) {
      list[list_n - 1 - i] = (uint32_t)a;
      boff[i] = off;
      boff[i + 1] = off + (uint32_t)d;
    }
  }
}

// A sorted key of read a -> its mg_disc record; the second copy of a self row
// is marked dead.  eq_*: the neighbour in the sorted segment exists and is
// identical.  A self row without its identical copy, or more than two copies,
// is the host's -3.
__device__ __forceinline__ uint64_t disc_record(uint64_t key, uint32_t a, uint32_t n1, uint32_t h, bool eq_prev,
                                                bool eq_prev2, bool eq_next, unsigned long long* __restrict__ ctl) {
  const uint32_t o = (uint32_t)key & 3u, dst = (uint32_t)(key >> 2), j = (uint32_t)(key >> 34) & 0xFFFFu;
  const uint32_t offset = ((o & 1u) ? n1 - h - j : j) & 0xFFFFu;
  uint64_t rec = (uint64_t)dst | ((uint64_t)offset << 32) | ((uint64_t)key_to_orient(o) << 48) | ((uint64_t)o << 56);
  if (dst == a) {
    if (eq_prev) {
      if (eq_prev2) atomicOr(&ctl[kErr], kErrSelf);
      rec |= kDead;
      atomicAdd(&ctl[kDup], 1ULL);
    } else if (!eq_next) {
      atomicOr(&ctl[kErr], kErrSelf);
    }
  }
  return rec;
}

// Degree <= 64.  A wavefront takes kWaveReads consecutive reads; their CSR
// segments are contiguous, so it repeatedly takes the longest run of whole
// segments that fits 64 lanes (larger segments are skipped: other paths),
// sorts (segment index, key) across the lanes and writes the records back.
__global__ __launch_bounds__(kThreads) void k_disc_wave(uint64_t* __restrict__ disc,
                                                        const uint64_t* __restrict__ start, uint32_t n, uint32_t h,
                                                        const uint16_t* __restrict__ len,
                                                        const uint32_t* __restrict__ phys,
                                                        unsigned long long* __restrict__ ctl) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint64_t wave = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) / kWave;
  const uint64_t a0 = 1 + wave * kWaveReads;
  if (a0 > n) return;  // (whole wavefront)
  const uint64_t s0 = start[a0];
  const uint64_t at = a0 + (uint64_t)lane;
  const uint32_t rel = (uint32_t)(start[at <= (uint64_t)n + 1 ? at : (uint64_t)n + 1] - s0);  // lanes 0..32 matter
  const uint32_t n1_lane = (lane < kWaveReads && at <= n) ? read_len(len, phys, (uint32_t)at) : 0u;
  int cur = 0;
  while (cur < kWaveReads) {
    const uint32_t sc = __shfl(rel, cur), sn = __shfl(rel, cur + 1);
    const uint32_t dg = sn - sc;
    if (dg == 0 || dg > (uint32_t)kWave) {
      ++cur;
      continue;
    }
    // rel is monotone: the lanes that fit are cur + 1 .. k
    const bool fits = lane > cur && lane <= kWaveReads && rel - sc <= (uint32_t)kWave;
    const int k = cur + __popcll(__ballot(fits));
    const uint32_t cnt = __shfl(rel, k) - sc;
    const uint64_t base = s0 + sc;
    const bool active = (uint32_t)lane < cnt;
    const uint64_t key = active ? disc[base + lane] : 0;
    // the record's segment: the last t in [cur, k) with rel[t] <= its position
    const uint32_t p = active ? sc + (uint32_t)lane : sc;
    int lo = cur, hi = k - 1;
#pragma unroll
    for (int it = 0; it < 6; ++it) {
      const int mid = (lo + hi + 1) >> 1;
      const uint32_t sm = __shfl(rel, mid);
      if (lo < hi) {
        if (sm <= p) lo = mid;
        else hi = mid - 1;
      }
    }
    uint64_t v = active ? (((uint64_t)lo << 50) | (key & kKeyMask)) : ~0ULL;
    // bitonic sorting network over the 64 lanes
#pragma unroll
    for (int k2 = 2; k2 <= kWave; k2 <<= 1) {
#pragma unroll
      for (int j = k2 >> 1; j >= 1; j >>= 1) {
        const uint64_t q = __shfl_xor(v, j);
        const bool lower = (lane & j) == 0, asc = (lane & k2) == 0;
        const uint64_t mn = v < q ? v : q, mx = v < q ? q : v;
        v = (lower == asc) ? mn : mx;
      }
    }
    const uint64_t prev = __shfl_up(v, 1), prev2 = __shfl_up(v, 2), next = __shfl_down(v, 1);
    const int seg = active ? (int)(v >> 50) : cur;
    const uint32_t n1 = __shfl(n1_lane, seg);
    if (active) {
      const uint32_t a = (uint32_t)(a0 + (uint64_t)seg);
      // (the segment index is part of v, so a neighbour of another segment never matches)
      disc[base + lane] = disc_record(v & kKeyMask, a, n1, h, lane >= 1 && prev == v, lane >= 2 && prev2 == v,
                                      lane + 1 < kWave && next == v, ctl);
    }
    cur = k;
  }
}

// bitonic sort of s[0 .. P) (P a power of two <= kBlockCap) by the workgroup
__device__ __forceinline__ void block_bitonic(uint64_t* s, uint32_t P) {
  for (uint32_t k2 = 2; k2 <= P; k2 <<= 1) {
    for (uint32_t j = k2 >> 1; j >= 1; j >>= 1) {
      for (uint32_t t = threadIdx.x; t < P / 2; t += kThreads) {
        const uint32_t lo = ((t / j) * 2 * j) + (t % j), hi = lo + j;
        const bool asc = (lo & k2) == 0;
        const uint64_t x = s[lo], y = s[hi];
        if ((x > y) == asc) {
          s[lo] = y;
          s[hi] = x;
        }
      }
      __syncthreads();
    }
  }
}

// 64 < degree <= block cap: one workgroup per read, the keys in LDS
__global__ __launch_bounds__(kThreads) void k_disc_block(uint64_t* __restrict__ disc,
                                                         const uint64_t* __restrict__ start,
                                                         const uint32_t* __restrict__ list, uint64_t list_n,
                                                         uint32_t h, const uint16_t* __restrict__ len,
                                                         const uint32_t* __restrict__ phys,
                                                         unsigned long long* __restrict__ ctl) {
  __shared__ uint64_t s[kBlockCap];
  const uint64_t n_mid = ctl[kMid] < list_n ? ctl[kMid] : list_n;
  for (uint64_t i = blockIdx.x; i < n_mid; i += gridDim.x) {
    const uint32_t a = list[i];
    const uint64_t base = start[a];
    const uint32_t d = (uint32_t)(start[a + 1] - base);
    if (d > kBlockCap) continue;  // (never: classified by the same bound)
    uint32_t P = 128;
    while (P < d) P <<= 1;
    for (uint32_t t = threadIdx.x; t < P; t += kThreads) s[t] = t < d ? disc[base + t] & kKeyMask : ~0ULL;
    __syncthreads();
    block_bitonic(s, P);
    const uint32_t n1 = read_len(len, phys, a);
    for (uint32_t t = threadIdx.x; t < d; t += kThreads)
      disc[base + t] = disc_record(s[t], a, n1, h, t >= 1 && s[t - 1] == s[t], t >= 2 && s[t - 2] == s[t],
                                   t + 1 < d && s[t + 1] == s[t], ctl);
    __syncthreads();
  }
}

// oversized segments: into / out of the segmented sort's dense buffer
__global__ __launch_bounds__(kThreads) void k_disc_gather(const uint64_t* __restrict__ disc,
                                                          const uint64_t* __restrict__ start,
                                                          const uint32_t* __restrict__ list, uint64_t list_n,
                                                          const uint32_t* __restrict__ boff, uint64_t n_big,
                                                          uint64_t* __restrict__ out) {
  for (uint64_t i = blockIdx.x; i < n_big; i += gridDim.x) {
    const uint32_t a = list[list_n - 1 - i];
    const uint64_t base = start[a], d = start[a + 1] - base, off = boff[i];
    for (uint64_t t = threadIdx.x; t < d; t += kThreads) out[off + t] = disc[base + t] & kKeyMask;
  }
}

__global__ __launch_bounds__(kThreads) void k_disc_big_records(uint64_t* __restrict__ disc,
                                                               const uint64_t* __restrict__ start,
                                                               const uint32_t* __restrict__ list, uint64_t list_n,
                                                               const uint32_t* __restrict__ boff, uint64_t n_big,
                                                               const uint64_t* __restrict__ sorted, uint32_t h,
                                                               const uint16_t* __restrict__ len,
                                                               const uint32_t* __restrict__ phys,
                                                               unsigned long long* __restrict__ ctl) {
  for (uint64_t i = blockIdx.x; i < n_big; i += gridDim.x) {
    const uint32_t a = list[list_n - 1 - i];
    const uint64_t base = start[a], d = start[a + 1] - base;
    const uint64_t* s = sorted + boff[i];
    const uint32_t n1 = read_len(len, phys, a);
    for (uint64_t t = threadIdx.x; t < d; t += kThreads)
      disc[base + t] = disc_record(s[t], a, n1, h, t >= 1 && s[t - 1] == s[t], t >= 2 && s[t - 2] == s[t],
                                   t + 1 < d && s[t + 1] == s[t], ctl);
  }
}

// compaction (only after a self row was dropped)
struct DiscLive {
  __host__ __device__ uint32_t operator()(uint64_t rec) const { return (rec >> 56) == 0xFFu ? 0u : 1u; }
};

__global__ __launch_bounds__(kThreads) void k_disc_compact(const uint64_t* __restrict__ disc,
                                                           const uint32_t* __restrict__ pre, uint64_t n_rows,
                                                           uint64_t* __restrict__ out) {
  const uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= n_rows) return;
  const uint64_t rec = disc[p];
  if ((rec >> 56) != 0xFFu) out[pre[p]] = rec;
}

__global__ __launch_bounds__(kThreads) void k_disc_restart(const uint64_t* __restrict__ start,
                                                           const uint32_t* __restrict__ pre, uint64_t n_rows,
                                                           uint64_t n_disc, uint64_t entries,
                                                           uint64_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= entries) return;
  const uint64_t s = start[i];
  out[i] = s < n_rows ? (uint64_t)pre[s] : n_disc;
}

int group_rows(mg_ctx* ctx) {
  const uint64_t N = ctx->n, R = ctx->n_rows, entries = N + 2;
  const uint32_t h = ctx->h;
  const uint32_t block_cap = std::max<uint32_t>(kWave, std::min<uint32_t>(ctx->disc.block_cap ? ctx->disc.block_cap : kBlockCap, kBlockCap));
  DiscStage& ds = ctx->disc;
  MG_GROW(ds.ctl, kDiscCtl, "d_disc_ctl");
  MG_GROW(ds.start, entries, "d_disc_start");
  MG_GROW(ds.cnt, entries, "d_disc_cnt");
  MG_GROW(ds.recs, R, "d_disc");
  ds.n = 0;
  if (!R || !N || !ctx->nreg) {
    MG_TRY(hipMemsetAsync(ds.start.p, 0, entries * sizeof(uint64_t), ctx->stream));
    return 0;
  }
  const uint64_t list_n = std::min<uint64_t>(N, R / (kWave + 1)) + 1;
  MG_GROW(ds.list, list_n, "d_disc_list");
  MG_GROW(ds.boff, list_n + 1, "d_disc_boff");
  size_t tb = 0;
  MG_TRY(rocprim::exclusive_scan(nullptr, tb, ds.cnt.p, ds.start.p, (uint64_t)0, (size_t)entries,
                                 rocprim::plus<uint64_t>(), ctx->stream));
  MG_GROW(ds.tmp, tb, "d_disc_tmp");
  tb = ds.tmp.cap;

  const uint64_t reg_cap = ctx->d_rows.cap / ctx->nreg;
  const uint32_t walk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(ctx->nreg, (uint64_t)ctx->n_cu * 32));
  MG_TRY(ctl_fill(ctx->stream, ds.ctl.p, kDiscCtl, 0));
  MG_TRY(hipMemsetAsync(ds.cnt.p, 0, entries * sizeof(uint32_t), ctx->stream));
  hipLaunchKernelGGL(k_disc_count, dim3(walk), dim3(kThreads), 0, ctx->stream, row_words(ctx), reg_cap, ctx->d_seg.p,
                     ctx->nreg, (uint32_t)N, ds.cnt.p, ds.ctl.p);
  MG_TRY(hipGetLastError());
  MG_TRY(rocprim::exclusive_scan(ds.tmp.p, tb, ds.cnt.p, ds.start.p, (uint64_t)0,
                                 (size_t)entries, rocprim::plus<uint64_t>(), ctx->stream));
  MG_TRY(hipMemsetAsync(ds.cnt.p, 0, entries * sizeof(uint32_t), ctx->stream));
  hipLaunchKernelGGL(k_disc_scatter, dim3(walk), dim3(kThreads), 0, ctx->stream, row_words(ctx), reg_cap, ctx->d_seg.p,
                     ctx->nreg, (uint32_t)N, h, ctx->d_len.p, ctx->d_phys, ds.start.p, ds.cnt.p,
                     ds.recs.p, ds.ctl.p);
  MG_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_disc_classify, dim3(blocks_for(N)), dim3(kThreads), 0, ctx->stream, ds.start.p,
                     (uint32_t)N, block_cap, ds.list.p, list_n, ds.boff.p, ds.ctl.p);
  MG_TRY(hipGetLastError());
  const uint64_t waves = (N + kWaveReads - 1) / kWaveReads;
  hipLaunchKernelGGL(k_disc_wave, dim3(blocks_for(waves * kWave)), dim3(kThreads), 0, ctx->stream, ds.recs.p,
                     ds.start.p, (uint32_t)N, h, ctx->d_len.p, ctx->d_phys, ds.ctl.p);
  MG_TRY(hipGetLastError());
  const uint32_t per_read_grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(list_n, (uint64_t)ctx->n_cu * 8));
  hipLaunchKernelGGL(k_disc_block, dim3(per_read_grid), dim3(kThreads), 0, ctx->stream, ds.recs.p,
                     ds.start.p, ds.list.p, list_n, h, ctx->d_len.p, ctx->d_phys, ds.ctl.p);
  MG_TRY(hipGetLastError());
  // the class counts (and, so far, the error bits) after everything above is queued
  unsigned long long ctl[kDiscCtl];
  MG_TRY(ctl_read(ctx->stream, ds.ctl.p, kDiscCtl, ctl));
  const uint64_t n_big = ctl[kBig] >> 32, big_total = ctl[kBig] & 0xFFFFFFFFULL;
  if (n_big && !(ctl[kErr] & kErrId)) {
    MG_GROW(ds.big[0], big_total, "d_disc_big[0]");
    MG_GROW(ds.big[1], big_total, "d_disc_big[1]");
    size_t sb = 0;
    MG_TRY(rocprim::segmented_radix_sort_keys(nullptr, sb, ds.big[0].p, ds.big[1].p,
                                              (unsigned int)big_total, (unsigned int)n_big, ds.boff.p,
                                              ds.boff.p + 1, 0u, 50u, ctx->stream));
    MG_GROW(ds.tmp, sb, "d_disc_tmp");
    sb = ds.tmp.cap;
    const uint32_t g = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_big, (uint64_t)ctx->n_cu * 8));
    hipLaunchKernelGGL(k_disc_gather, dim3(g), dim3(kThreads), 0, ctx->stream, ds.recs.p, ds.start.p,
                       ds.list.p, list_n, ds.boff.p, n_big, ds.big[0].p);
    MG_TRY(hipGetLastError());
    MG_TRY(rocprim::segmented_radix_sort_keys(ds.tmp.p, sb, ds.big[0].p, ds.big[1].p,
                                              (unsigned int)big_total, (unsigned int)n_big, ds.boff.p,
                                              ds.boff.p + 1, 0u, 50u, ctx->stream));
    hipLaunchKernelGGL(k_disc_big_records, dim3(g), dim3(kThreads), 0, ctx->stream, ds.recs.p, ds.start.p,
                       ds.list.p, list_n, ds.boff.p, n_big, ds.big[1].p, h, ctx->d_len.p,
                       ctx->d_phys, ds.ctl.p);
    MG_TRY(hipGetLastError());
    MG_TRY(ctl_read(ctx->stream, ds.ctl.p, kDiscCtl, ctl));
  }
  if (ctl[kErr] & kErrId) {
    ctx->err = "mg_build_discoveries: a row's src or dst is outside 1..n_reads (-1)";
    return -1;
  }
  if (ctl[kErr] & kErrJ) {
    ctx->err = "mg_build_discoveries: a row's window j is outside [1, len(src) - h) (-2: rows inconsistent with the read lengths)";
    return -2;
  }
  if (ctl[kErr] & kErrSelf) {
    ctx->err = "mg_build_discoveries: a self row without exactly one identical copy (-3: unpaired self rows)";
    return -3;
  }
  const uint64_t dups = ctl[kDup];
  ctx->disc.n = R - dups;
  if (dups) {  // tandem repeats only: drop the dead records, lists stay dense
    MG_GROW(ds.pre, R, "d_disc_pre");
    MG_GROW(ds.recs_alt, ds.n, "d_disc_alt");
    MG_GROW(ds.start_alt, entries, "d_disc_start_alt");
    auto live = rocprim::make_transform_iterator(ds.recs.p, DiscLive());
    size_t cb = 0;
    MG_TRY(rocprim::exclusive_scan(nullptr, cb, live, ds.pre.p, 0u, (size_t)R, rocprim::plus<uint32_t>(),
                                   ctx->stream));
    MG_GROW(ds.tmp, cb, "d_disc_tmp");
    cb = ds.tmp.cap;
    MG_TRY(rocprim::exclusive_scan(ds.tmp.p, cb, live, ds.pre.p, 0u, (size_t)R,
                                   rocprim::plus<uint32_t>(), ctx->stream));
    hipLaunchKernelGGL(k_disc_compact, dim3(blocks_for(R)), dim3(kThreads), 0, ctx->stream, ds.recs.p,
                       ds.pre.p, R, ds.recs_alt.p);
    MG_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_disc_restart, dim3(blocks_for(entries)), dim3(kThreads), 0, ctx->stream, ds.start.p,
                       ds.pre.p, R, ctx->disc.n, entries, ds.start_alt.p);
    MG_TRY(hipGetLastError());
    ds.recs.swap(ds.recs_alt);
    ds.start.swap(ds.start_alt);
  }
  return 0;
}

}  // namespace

extern "C" {

int mg_build_discoveries(mg_ctx* ctx, uint64_t* n_disc, float* device_ms) {
  if (!ctx) return -1;
  ctx->err.clear();
  MG_TRY(hipSetDevice(ctx->device));
  if (n_disc) *n_disc = 0;
  if (device_ms) *device_ms = 0.f;
  ctx->disc.ready = false;
  ctx->comp.ready = false;
  if (whole_multiset(ctx, "mg_build_discoveries")) return -1;
  if (!ctx->index_ready || !ctx->rows_found)
    return set_err(ctx, "mg_build_discoveries: mg_find_overlaps must complete for the current index first");
  if (ctx->n_rows >> 32 || ctx->n >= 0xFFFFFFFFULL)
    return set_err(ctx, "mg_build_discoveries: 2^32 or more rows are not supported");
  MG_TRY(ctx->disc.ev.start(ctx->stream));
  const int rc = group_rows(ctx);
  if (rc) return rc;
  MG_TRY(ctx->disc.ev.end(ctx->stream));
  MG_TRY(ctx->disc.ev.wait());
  MG_TRY(ctx->disc.ev.elapsed(device_ms));
  ctx->disc.ready = true;
  if (n_disc) *n_disc = ctx->disc.n;
  return 0;
}

int mg_copy_discoveries(mg_ctx* ctx, uint64_t* start, mg_disc* disc, uint64_t cap, uint64_t* n_copied) {
  if (!ctx) return -1;
  ctx->err.clear();
  MG_TRY(hipSetDevice(ctx->device));
  if (n_copied) *n_copied = 0;
  if (whole_multiset(ctx, "mg_copy_discoveries")) return -1;
  if (!ctx->index_ready || !ctx->rows_found || !ctx->disc.ready)
    return set_err(ctx, "mg_copy_discoveries: mg_build_discoveries must run for the current rows first");
  return copy_csr(ctx, ctx->disc.start.p, ctx->n + 2, start, ctx->disc.recs.p, ctx->disc.n, disc, cap, n_copied);
}

}  // extern "C"
