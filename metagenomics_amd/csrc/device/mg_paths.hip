// mg_paths.hip — mate-pair path support: for every mate entry the bounded
// depth-first search between the two reads' edges, and the list of supported
// edge pairs with their support.  The definitions are in include/mg_overlap.h
// ("mate-pair path support"); csrc/host/mg_paths.cpp is the mirror.
//
// Reference paths replaced (paths relative to the reference's MetaGenomics directory):
//   OverlapGraph::findSupportByMatepairsAndMerge   OverlapGraph.cpp:1892-1966 (up to the sort)
//   OverlapGraph::findPathBetweenMatepairs         OverlapGraph.cpp:1645-1730
//   OverlapGraph::exploreGraph                     OverlapGraph.cpp:1781-1870
//
// mg_mate_paths (one stream):
//   k_pt_edges / k_check_places / k_mate_owners (the last two in mg_stage.hpp,
//                 shared with mg_scaffold_pairs): validation, the first offender of
//                 each kind kept by atomicMin; per edge its adjacency range
//                 graph[dst] by two lower bounds over src; per mate entry its owner;
//   k_pt_explore: lane per mate entry, `path_batch` entries per launch.  The
//                 recursion is an explicit stack; stack, first path, kept path
//                 and their flags live in a global workspace laid out
//                 [level][lane] (101 levels, 26 B per level and lane), so the
//                 lanes of a wavefront at one level touch neighbouring
//                 addresses and no runtime-indexed private array exists;
//   ExclusiveSum + k_pt_gather: the kept paths of the batch end to end in
//                 "path space" behind the earlier batches';
//   aggregate   : k_pt_select (flagged positions whose pair is not two
//                 self-loops) -> ExclusiveSum -> k_pt_emit (canonical key,
//                 position) -> stable SortPairs by key -> k_run_heads ->
//                 ExclusiveSum -> k_pt_headrec (first position, run length by
//                 an upper bound) -> SortPairs by first position -> k_pt_pairs.
//                 Positions ascend in (entry, k), so a run's first position is
//                 where the reference first saw the pair and carries its
//                 orientation.  The three counters: ballot + popcount per
//                 wavefront, one integer atomic each.
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

constexpr int kLevels = 101;                   // levels 0..100 (:1800)
constexpr uint64_t kDefaultBatch = 1ull << 18;  // lanes per explore launch
constexpr uint64_t kDefaultBudget = 1ull << 16; // work units per mate entry

struct EdgeRec {
  uint64_t offset;
  uint32_t lo, hi;  // graph[dst] = edges [lo, hi)
  uint32_t orient;
  uint32_t self;    // src == dst
};

// the explore kernel's workspace, [level][lane]
struct Work {
  uint32_t* stk_e;    // listOfEdges
  uint64_t* stk_len;  // pathLengths
  uint32_t* stk_cur;  // the next child of a frame that has descended
  uint32_t* fp;       // firstPath
  uint8_t* ff;        // flags
  uint32_t* cp;       // copyOfPath
  uint8_t* cf;        // copyOfFlags
  uint64_t lanes;
};
#define W_(arr, level) w.arr[(uint64_t)(level) * w.lanes + ln]

__device__ __forceinline__ bool match_edge_type(uint32_t a, uint32_t b) {  // matchEdgeType :19-26
  return ((a == 1 || a == 3) && (b == 2 || b == 3)) || ((a == 0 || a == 2) && (b == 0 || b == 1));
}

__global__ __launch_bounds__(kThreads) void k_pt_edges(const mg_contig_edge* __restrict__ edges,
                                                       const uint32_t* __restrict__ twin, uint64_t n,
                                                       EdgeRec* __restrict__ er, ull* __restrict__ ctl) {
  const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k >= n) return;
  const mg_contig_edge e = edges[k];
  if (k && e.src < edges[k - 1].src) atomicMin(&ctl[0], (ull)k);
  if (twin[k] >= n) atomicMin(&ctl[1], (ull)k);
  uint64_t b[2];
  for (int s = 0; s < 2; ++s) {  // first edge with src >= dst + s (every index stays inside the edges)
    const uint64_t x = (uint64_t)e.dst + s;
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if ((uint64_t)edges[mid].src < x) lo = mid + 1;
      else hi = mid;
    }
    b[s] = lo;
  }
  er[k] = EdgeRec{e.offset, (uint32_t)b[0], (uint32_t)b[1], e.orient, e.src == e.dst ? 1u : 0u};
}

// exploreGraph (:1781-1870) from level 0 for lane ln; the number of paths
// found, the first of them in w.fp / w.ff (fplen edges).  The current frame
// (edge, length, cursor, end) is kept in registers; a frame that descends
// leaves its cursor in the workspace, its edge and length are there already.
__device__ uint32_t explore(const EdgeRec* __restrict__ er, const Work& w, uint64_t ln, uint32_t first, uint32_t last,
                            uint64_t d1, uint64_t d2, uint64_t bhi, uint64_t blo, uint32_t budget, uint32_t& visits,
                            bool& over, uint32_t& fplen) {
  uint32_t found = 0;
  fplen = 0;
  int level = 0;
  EdgeRec r = er[first];
  uint64_t len = d1;
  uint32_t cur = r.lo, end = r.hi, eor = r.orient;
  W_(stk_e, 0) = first;
  W_(stk_len, 0) = d1;
  for (;;) {
    if (cur >= end) {  // :1863 ends
      if (!level) break;
      --level;
      r = er[W_(stk_e, level)];
      len = W_(stk_len, level);
      cur = W_(stk_cur, level);
      end = r.hi;
      eor = r.orient;
      continue;
    }
    const uint32_t c = cur++;
    if (++visits > budget) {
      over = true;
      return 0;
    }
    if (!(len < bhi)) continue;  // :1866, second half
    const EdgeRec rc = er[c];
    if (!match_edge_type(eor, rc.orient)) continue;
    const int nl = level + 1;
    if (nl > kLevels - 1) continue;  // :1800
    if (c == last) {                 // :1810
      const uint64_t total = d2 + len;
      if (total >= blo && total <= bhi) {  // :1812
        ++found;
        if (found == 1) {  // :1817-1825
          for (int j = 0; j < nl; ++j) {
            W_(fp, j) = W_(stk_e, j);
            W_(ff, j) = 1;
          }
          W_(fp, nl) = c;
          fplen = (uint32_t)nl + 1;
        } else {  // :1828-1838: this path is stk_e[0 .. level], c
          for (uint32_t k = 0; k + 1 < fplen; ++k) {
            if (++visits > budget) {
              over = true;
              return 0;
            }
            const uint32_t a = W_(fp, k), b = W_(fp, k + 1);
            bool adjacent = false;
            uint32_t x = W_(stk_e, 0);
            for (int j = 0; j < nl && !adjacent; ++j) {
              const uint32_t y = j + 1 < nl ? W_(stk_e, j + 1) : c;
              adjacent = a == x && b == y;
              x = y;
            }
            if (!adjacent) W_(ff, k) = 0;
          }
        }
        continue;  // :1848
      }
    }
    W_(stk_cur, level) = cur;  // :1852-1859
    level = nl;
    r = rc;
    len = rc.offset + len;
    cur = rc.lo;
    end = rc.hi;
    eor = rc.orient;
    W_(stk_e, level) = c;
    W_(stk_len, level) = len;
  }
  return found;
}

// Lane per mate entry t0 + ln: findPathBetweenMatepairs (:1645-1730).
__global__ __launch_bounds__(kThreads) void k_pt_explore(const EdgeRec* __restrict__ er, const uint32_t* __restrict__ twin,
                                                         const uint64_t* __restrict__ pstart,
                                                         const mg_place* __restrict__ places,
                                                         const mg_mate* __restrict__ mates,
                                                         const uint32_t* __restrict__ owner,
                                                         const uint64_t* __restrict__ mean,
                                                         const uint64_t* __restrict__ sd, uint64_t t0, uint64_t nb,
                                                         uint32_t budget, Work w, uint8_t* __restrict__ status,
                                                         uint32_t* __restrict__ visits_out, uint64_t* __restrict__ plen,
                                                         ull* __restrict__ counters) {
  const uint64_t ln = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  uint32_t st = 255;
  if (ln < nb) {
    const uint64_t t = t0 + ln;
    const mg_mate mt = mates[t];
    const uint64_t a = owner[t];
    uint32_t visits = 0, cplen = 0;
    bool over = false;
    const uint64_t mu = mean[mt.dataset], sg = sd[mt.dataset];
    if (a > mt.id || mu == 0) {  // :1911-1914
      st = MG_PATH_SKIPPED;
    } else {
      const uint32_t want1 = (mt.orient == 2 || mt.orient == 3) ? 1u : 0u;  // :1657
      const uint32_t want2 = (mt.orient == 0 || mt.orient == 2) ? 1u : 0u;  // :1664
      const uint64_t p0 = pstart[a], p1 = pstart[a + 1], q0 = pstart[mt.id], q1 = pstart[mt.id + 1];
      uint32_t n1 = 0, n2 = 0;
      for (uint64_t p = p0; p < p1; ++p) n1 += (places[p].flags & 1u) == want1;
      for (uint64_t q = q0; q < q1; ++q) n2 += (places[q].flags & 1u) == want2;
      if (!n1 || !n2) {  // :1667
        st = MG_PATH_SAME_EDGE;
      } else {
        st = MG_PATH_NONE;
        for (uint64_t p = p0; p < p1 && st == MG_PATH_NONE; ++p) {  // :1673-1684
          const mg_place pa = places[p];
          if ((pa.flags & 1u) != want1) continue;
          for (uint64_t q = q0; q < q1; ++q) {
            const mg_place pb = places[q];
            if ((pb.flags & 1u) != want2) continue;
            if (++visits > budget) {
              st = MG_PATH_DEFERRED;
              break;
            }
            if (pa.edge == pb.edge || pa.edge == twin[pb.edge]) {
              st = MG_PATH_SAME_EDGE;
              break;
            }
          }
        }
      }
      if (st == MG_PATH_NONE) {
        const uint64_t bhi = mu + 3 * sg, blo = mu - 3 * sg;         // (mod 2^64)
        for (uint64_t p = p0; p < p1 && !over; ++p) {                // :1687-1728
          const mg_place pa = places[p];
          if ((pa.flags & 1u) != want1) continue;
          const uint64_t d1 = er[pa.edge].offset - pa.distance;      // :1695
          for (uint64_t q = q0; q < q1 && !over; ++q) {
            const mg_place pb = places[q];
            if ((pb.flags & 1u) != want2) continue;
            const uint64_t d2 = pb.distance;
            if (!(d1 + d2 < bhi)) continue;  // :1697
            uint32_t fplen = 0;
            const uint32_t found = explore(er, w, ln, pa.edge, pb.edge, d1, d2, bhi, blo, budget, visits, over, fplen);
            if (over || !found) continue;
            if (!cplen) {  // :1703-1709
              for (uint32_t k = 0; k < fplen; ++k) {
                W_(cp, k) = W_(fp, k);
                W_(cf, k) = k + 1 < fplen ? W_(ff, k) : (uint8_t)0;
              }
              cplen = fplen;
            } else {  // :1713-1722
              for (uint32_t k = 0; k + 1 < cplen && !over; ++k) {
                if (++visits > budget) {
                  over = true;
                  break;
                }
                const uint32_t x = W_(cp, k), y = W_(cp, k + 1);
                bool kept = false;
                for (uint32_t l = 0; l + 1 < fplen && !kept; ++l)
                  kept = x == W_(fp, l) && y == W_(fp, l + 1) && W_(ff, l) == 1;
                if (!kept) W_(cf, k) = 0;
              }
            }
          }
        }
        if (over) st = MG_PATH_DEFERRED;
        else if (cplen) st = MG_PATH_FOUND;
      }
    }
    status[t] = (uint8_t)st;
    visits_out[t] = visits;
    plen[t] = st == MG_PATH_FOUND ? cplen : 0;
  }
  // noPathsFound, pathsFound, mpOnSameEdge, and the deferred entries
  const uint32_t kinds[4] = {MG_PATH_NONE, MG_PATH_FOUND, MG_PATH_SAME_EDGE, MG_PATH_DEFERRED};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const ull n = (ull)__popcll(__ballot(st == kinds[i]));
    if ((threadIdx.x & (kWave - 1)) == 0 && n) atomicAdd(&counters[i], n);
  }
}

// grid (lanes, levels): the kept paths of a batch into path space
__global__ __launch_bounds__(kThreads) void k_pt_gather(Work w, uint64_t t0, uint64_t nb,
                                                        const uint64_t* __restrict__ plen,
                                                        const uint64_t* __restrict__ boff, uint64_t base,
                                                        uint64_t* __restrict__ pstart, uint32_t* __restrict__ path,
                                                        uint8_t* __restrict__ flags) {
  const uint64_t ln = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  const uint32_t level = blockIdx.y;
  if (ln >= nb) return;
  const uint64_t at = base + boff[ln];
  if (level == 0) pstart[t0 + ln] = at;
  if (level >= plen[t0 + ln]) return;
  path[at + level] = W_(cp, level);
  flags[at + level] = W_(cf, level);
}

__global__ __launch_bounds__(kThreads) void k_pt_select(const uint32_t* __restrict__ path,
                                                        const uint8_t* __restrict__ flags, uint64_t P,
                                                        const EdgeRec* __restrict__ er, uint32_t* __restrict__ sel) {
  const uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p > P) return;
  uint32_t s = 0;
  if (p < P && flags[p] == 1)  // (a flagged position is never a path's last)
    s = !(er[path[p]].self && er[path[p + 1]].self);  // :1951
  sel[p] = s;
}

__global__ __launch_bounds__(kThreads) void k_pt_emit(const uint32_t* __restrict__ path, uint64_t P,
                                                      const uint32_t* __restrict__ sel,
                                                      const uint32_t* __restrict__ idx,
                                                      const uint32_t* __restrict__ twin, uint64_t n_edges,
                                                      uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= P || !sel[p]) return;
  const uint64_t a = path[p], b = path[p + 1];
  const uint64_t k1 = a * n_edges + b, k2 = (uint64_t)twin[b] * n_edges + twin[a];
  keys[idx[p]] = k1 < k2 ? k1 : k2;
  vals[idx[p]] = (uint32_t)p;
}

__global__ __launch_bounds__(kThreads) void k_pt_headrec(const uint64_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ vals, uint64_t F,
                                                         const uint32_t* __restrict__ head,
                                                         const uint32_t* __restrict__ hidx, uint32_t* __restrict__ hseq,
                                                         uint64_t* __restrict__ hsup) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= F || !head[i]) return;
  const uint64_t key = keys[i];
  uint64_t lo = i + 1, hi = F;  // first index past the run
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (keys[mid] <= key) lo = mid + 1;
    else hi = mid;
  }
  hseq[hidx[i]] = vals[i];  // the sort is stable and positions were emitted ascending: the run's first
  hsup[hidx[i]] = lo - i;
}

__global__ __launch_bounds__(kThreads) void k_pt_pairs(const uint32_t* __restrict__ hseq,
                                                       const uint64_t* __restrict__ hsup, uint64_t H,
                                                       const uint32_t* __restrict__ path,
                                                       mg_pair_support* __restrict__ out) {
  const uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= H) return;
  const uint32_t p = hseq[r];
  out[r] = mg_pair_support{path[p], path[p + 1], hsup[r]};
}

// a.p to at least `need` elements, its first `used` kept
template <typename T>
int grow_keep(mg_ctx* ctx, DevArray<T>& a, size_t used, size_t need, size_t target, const char* what) {
  if (a.p && a.cap >= need) return 0;
  const size_t cap = std::max<size_t>(std::max(need, target), 1024);
  T* np = nullptr;
  if (ctx_malloc(ctx, reinterpret_cast<void**>(&np), cap * sizeof(T), what) != hipSuccess) return -1;
  hipError_t e = hipSuccess;
  if (used && a.p) e = hipMemcpyAsync(np, a.p, used * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    (void)hipFree(np);
    return set_err(ctx, std::string("copying ") + what + " failed: " + hipGetErrorString(e));
  }
  if (a.p) (void)hipFree(a.p);
  a.p = np;
  a.cap = cap;
  return 0;
}

}  // namespace

extern "C" {

int mg_mate_paths(mg_ctx* ctx, const mg_contig_edge* edges, const uint32_t* twin, uint64_t n_edges, uint64_t n_reads,
                  const uint64_t* place_start, const mg_place* places, const uint64_t* mate_start,
                  const mg_mate* mates, const uint64_t* mean, const uint64_t* sd, uint32_t n_datasets,
                  uint64_t* counters, uint64_t* n_pairs, uint64_t* n_deferred, float* device_ms) {
  if (!ctx) return -1;
  ctx->err.clear();
  if (n_pairs) *n_pairs = 0;
  if (n_deferred) *n_deferred = 0;
  if (device_ms) *device_ms = 0.f;
  if (counters) counters[0] = counters[1] = counters[2] = 0;
  PathStage& ps = ctx->paths;
  ps.ready = false;
  if ((n_edges && (!edges || !twin)) || (n_datasets && (!mean || !sd)))
    return set_err(ctx, "mg_mate_paths: null argument");
  if (n_datasets > 256) return set_err(ctx, "mg_mate_paths: more than 256 datasets (datasetNumber is UINT8)");
  if (n_edges >> 31) return set_err(ctx, "mg_mate_paths: 2^31 or more edges are not supported");
  MG_TRY(hipSetDevice(ctx->device));
  if (whole_multiset(ctx, "mg_mate_paths")) return -1;
  const uint64_t N = n_reads;
  hipStream_t st = ctx->stream;

  // the two CSRs: the caller's in scratch, or the resident ones
  PairCsrs csr;
  if (const int rc = csr.take(ctx, "mg_mate_paths", N, n_edges, place_start, places, mate_start, mates)) return rc;
  const uint64_t* pstart = csr.pstart;
  const mg_place* prec = csr.prec;
  const uint64_t P0 = csr.P;
  const uint64_t* mstart = csr.mstart;
  const mg_mate* mrec = csr.mrec;
  const uint64_t M = csr.M;

  Scratch<mg_contig_edge> d_edges;
  Scratch<uint32_t> d_twin, d_owner;
  Scratch<EdgeRec> d_er;
  Scratch<uint64_t> d_mean, d_sd;
  Scratch<ull> ctl;  // [0..3] first offenders, [4..7] the counters and the deferred entries
  MG_SCRATCH(d_edges, n_edges, "path edges");
  MG_SCRATCH(d_twin, n_edges, "path edge twins");
  MG_SCRATCH(d_er, n_edges, "path edge records");
  MG_SCRATCH(d_owner, M, "mate entry owners");
  MG_SCRATCH(d_mean, n_datasets, "insert-size means");
  MG_SCRATCH(d_sd, n_datasets, "insert-size deviations");
  MG_SCRATCH(ctl, 8, "path control words");
  if (n_edges) {
    MG_TRY(hipMemcpyAsync(d_edges.p, edges, n_edges * sizeof(mg_contig_edge), hipMemcpyHostToDevice, st));
    MG_TRY(hipMemcpyAsync(d_twin.p, twin, n_edges * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  }
  if (n_datasets) {
    MG_TRY(hipMemcpyAsync(d_mean.p, mean, n_datasets * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    MG_TRY(hipMemcpyAsync(d_sd.p, sd, n_datasets * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  }
  MG_TRY(ctl_fill(st, ctl.p, 4, ~0ull));
  MG_TRY(ctl_fill(st, ctl.p + 4, 4, 0));

  // --- validation: nothing below indexes with an unchecked value
  if (n_edges) {
    hipLaunchKernelGGL(k_pt_edges, dim3(blocks_for(n_edges)), dim3(kThreads), 0, st, d_edges.p, d_twin.p, n_edges,
                       d_er.p, ctl.p);
    MG_TRY(hipGetLastError());
  }
  if (P0) {
    hipLaunchKernelGGL(k_check_places<ull>, dim3(blocks_for(P0)), dim3(kThreads), 0, st, prec, P0, n_edges, ctl.p + 2);
    MG_TRY(hipGetLastError());
  }
  if (M) {
    hipLaunchKernelGGL(k_mate_owners<ull>, dim3(blocks_for(M)), dim3(kThreads), 0, st, mstart, mrec, M, N, n_datasets,
                       d_owner.p, ctl.p + 3);
    MG_TRY(hipGetLastError());
  }
  ull bad[4] = {~0ull, ~0ull, ~0ull, ~0ull};
  MG_TRY(ctl_read(st, ctl.p, 4, bad));
  if (bad[0] != ~0ull) {
    ctx->err = "mg_mate_paths: " + edge_name(edges, bad[0]) + ": its source ID is below the previous edge's (-2)";
    return -2;
  }
  if (bad[1] != ~0ull) {
    ctx->err = "mg_mate_paths: " + edge_name(edges, bad[1]) + ": its twin " + std::to_string(twin[bad[1]]) +
               " is not below " + std::to_string(n_edges) + " (-2)";
    return -2;
  }
  if (bad[2] != ~0ull) return bad_place(ctx, "mg_mate_paths", prec, bad[2], n_edges);
  if (bad[3] != ~0ull) return bad_mate(ctx, "mg_mate_paths", bad[3], n_datasets, N);

  // --- explore, a batch of lanes at a time
  const uint64_t batch = std::max<uint64_t>(1, std::min<uint64_t>(ps.batch ? ps.batch : kDefaultBatch, std::max<uint64_t>(M, 1)));
  const uint32_t budget = (uint32_t)std::min<uint64_t>(ps.budget ? ps.budget : kDefaultBudget, 0x7FFFFFFFull);
  MG_GROW(ps.status, M, "d_path_status");
  MG_GROW(ps.visits, M, "d_path_visits");
  MG_GROW(ps.plen, M + 1, "d_path_len");
  MG_GROW(ps.pstart, M + 1, "d_path_start");
  MG_TRY(hipMemsetAsync(ps.plen.p, 0, (M + 1) * sizeof(uint64_t), st));
  Scratch<uint32_t> w_e, w_cur, w_fp, w_cp;
  Scratch<uint64_t> w_len, boff;
  Scratch<uint8_t> w_ff, w_cf, scan_tmp;
  const uint64_t cells = batch * kLevels;
  MG_SCRATCH(w_e, cells, "path stack edges");
  MG_SCRATCH(w_len, cells, "path stack lengths");
  MG_SCRATCH(w_cur, cells, "path stack cursors");
  MG_SCRATCH(w_fp, cells, "first paths");
  MG_SCRATCH(w_ff, cells, "first path flags");
  MG_SCRATCH(w_cp, cells, "kept paths");
  MG_SCRATCH(w_cf, cells, "kept path flags");
  MG_SCRATCH(boff, batch + 1, "batch path offsets");
  size_t scan_bytes = 0;
  MG_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, ps.plen.p, boff.p, (int64_t)(batch + 1), st));
  MG_SCRATCH(scan_tmp, scan_bytes, "batch scan storage");
  const Work w{w_e.p, w_len.p, w_cur.p, w_fp.p, w_ff.p, w_cp.p, w_cf.p, batch};
  uint64_t P = 0;
  ps.explore_ms = ps.aggregate_ms = 0.f;
  for (uint64_t t0 = 0; t0 < M; t0 += batch) {
    const uint64_t nb = std::min(batch, M - t0);
    MG_TRY(ps.ev.start(st));
    hipLaunchKernelGGL(k_pt_explore, dim3(blocks_for(nb)), dim3(kThreads), 0, st, d_er.p, d_twin.p, pstart, prec, mrec,
                       d_owner.p, d_mean.p, d_sd.p, t0, nb, budget, w, ps.status.p, ps.visits.p, ps.plen.p, ctl.p + 4);
    MG_TRY(hipGetLastError());
    MG_TRY(ps.ev.end(st));
    size_t tb = scan_bytes;  // plen[t0 + nb] is 0 (a later batch's slot, or the spare one): boff[nb] = the batch's total
    MG_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp.p, tb, ps.plen.p + t0, boff.p, (int64_t)(nb + 1), st));
    uint64_t total = 0;
    MG_TRY(hipMemcpyAsync(&total, boff.p + nb, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    MG_TRY(hipStreamSynchronize(st));
    float ms = 0.f;
    MG_TRY(ps.ev.elapsed(&ms));
    ps.explore_ms += ms;
    if ((P + total) >> 31) return set_err(ctx, "mg_mate_paths: 2^31 or more path positions are not supported");
    if (total) {
      // sized for all batches from the ones seen so far, so a steady stream grows once
      const uint64_t target = (uint64_t)((double)(P + total) * ((double)M / (double)(t0 + nb)) * 1.05) + 1024;
      if (grow_keep(ctx, ps.path, P, P + total + 1, target, "d_path_edges")) return -1;
      if (grow_keep(ctx, ps.flags, P, P + total + 1, target, "d_path_flags")) return -1;
    }
    hipLaunchKernelGGL(k_pt_gather, dim3(blocks_for(nb), kLevels), dim3(kThreads), 0, st, w, t0, nb, ps.plen.p, boff.p, P,
                       ps.pstart.p, ps.path.p, ps.flags.p);
    MG_TRY(hipGetLastError());
    P += total;
  }
  MG_TRY(hipMemcpyAsync(ps.pstart.p + M, &P, sizeof(uint64_t), hipMemcpyHostToDevice, st));
  MG_TRY(hipStreamSynchronize(st));  // (P is a local)
  if (!ps.path.p) {
    MG_GROW(ps.path, 1, "d_path_edges");
    MG_GROW(ps.flags, 1, "d_path_flags");
  }

  // --- aggregate
  uint64_t H = 0;
  MG_TRY(ps.ev.start(st));
  if (P) {
    Scratch<uint32_t> sel, idx;
    Scratch<uint8_t> tmp;
    MG_SCRATCH(sel, P + 1, "path pair selection");
    MG_SCRATCH(idx, P + 1, "path pair indices");
    size_t tb = 0;
    MG_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, sel.p, idx.p, (int64_t)(P + 1), st));
    MG_SCRATCH(tmp, tb, "path pair scan storage");
    hipLaunchKernelGGL(k_pt_select, dim3(blocks_for(P + 1)), dim3(kThreads), 0, st, ps.path.p, ps.flags.p, P, d_er.p,
                       sel.p);
    MG_TRY(hipGetLastError());
    MG_TRY(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, sel.p, idx.p, (int64_t)(P + 1), st));
    uint32_t F32 = 0;
    MG_TRY(hipMemcpyAsync(&F32, idx.p + P, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    MG_TRY(hipStreamSynchronize(st));
    const uint64_t F = F32;
    if (F) {
      Scratch<uint64_t> keys_a, keys_b, hsup_a, hsup_b;
      Scratch<uint32_t> vals_a, vals_b, head, hidx, hseq_a, hseq_b;
      Scratch<uint8_t> tmp2;
      MG_SCRATCH(keys_a, F, "path pair keys");
      MG_SCRATCH(keys_b, F, "path pair keys");
      MG_SCRATCH(vals_a, F, "path pair positions");
      MG_SCRATCH(vals_b, F, "path pair positions");
      MG_SCRATCH(head, F + 1, "path pair run heads");
      MG_SCRATCH(hidx, F + 1, "path pair run indices");
      const int key_bits = bits_of(n_edges * n_edges - 1), pos_bits = bits_of(P);
      size_t b1 = 0, b2 = 0, b3 = 0;
      MG_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, b1, keys_a.p, keys_b.p, vals_a.p, vals_b.p, (int)F, 0,
                                                key_bits, st));
      MG_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b2, head.p, hidx.p, (int64_t)(F + 1), st));
      MG_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, b3, hseq_a.p, hseq_b.p, hsup_a.p, hsup_b.p, (int)F, 0,
                                                pos_bits, st));
      const size_t tb2 = std::max(b1, std::max(b2, b3));
      MG_SCRATCH(tmp2, tb2, "path pair sort storage");
      hipLaunchKernelGGL(k_pt_emit, dim3(blocks_for(P)), dim3(kThreads), 0, st, ps.path.p, P, sel.p, idx.p, d_twin.p,
                         n_edges, keys_a.p, vals_a.p);
      MG_TRY(hipGetLastError());
      size_t t2 = tb2;
      MG_TRY(hipcub::DeviceRadixSort::SortPairs(tmp2.p, t2, keys_a.p, keys_b.p, vals_a.p, vals_b.p, (int)F, 0, key_bits,
                                                st));
      hipLaunchKernelGGL(k_run_heads<uint64_t>, dim3(blocks_for(F + 1)), dim3(kThreads), 0, st, keys_b.p, F, head.p);
      MG_TRY(hipGetLastError());
      t2 = tb2;
      MG_TRY(hipcub::DeviceScan::ExclusiveSum(tmp2.p, t2, head.p, hidx.p, (int64_t)(F + 1), st));
      uint32_t H32 = 0;
      MG_TRY(hipMemcpyAsync(&H32, hidx.p + F, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      MG_TRY(hipStreamSynchronize(st));
      H = H32;
      MG_SCRATCH(hseq_a, H, "path pair first positions");
      MG_SCRATCH(hseq_b, H, "path pair first positions");
      MG_SCRATCH(hsup_a, H, "path pair supports");
      MG_SCRATCH(hsup_b, H, "path pair supports");
      MG_GROW(ps.pairs, H, "d_path_pairs");
      hipLaunchKernelGGL(k_pt_headrec, dim3(blocks_for(F)), dim3(kThreads), 0, st, keys_b.p, vals_b.p, F, head.p, hidx.p,
                         hseq_a.p, hsup_a.p);
      MG_TRY(hipGetLastError());
      t2 = tb2;
      MG_TRY(hipcub::DeviceRadixSort::SortPairs(tmp2.p, t2, hseq_a.p, hseq_b.p, hsup_a.p, hsup_b.p, (int)H, 0, pos_bits,
                                                st));
      hipLaunchKernelGGL(k_pt_pairs, dim3(blocks_for(H)), dim3(kThreads), 0, st, hseq_b.p, hsup_b.p, H, ps.path.p,
                         ps.pairs.p);
      MG_TRY(hipGetLastError());
      MG_TRY(hipStreamSynchronize(st));  // the scratch above is released here
    }
  }
  MG_TRY(ps.ev.end(st));
  ull cnt[4] = {0, 0, 0, 0};
  MG_TRY(ctl_read(st, ctl.p + 4, 4, cnt));
  MG_TRY(ps.ev.elapsed(&ps.aggregate_ms));
  const uint64_t deferred = cnt[3];
  ps.n_entries = M;
  ps.n_path = P;
  ps.n_pairs = H;
  ps.n_deferred = deferred;
  ps.ready = true;
  if (counters) std::copy(cnt, cnt + 3, counters);
  if (n_pairs) *n_pairs = H;
  if (n_deferred) *n_deferred = deferred;
  if (device_ms) *device_ms = ps.explore_ms + ps.aggregate_ms;
  return 0;
}

int mg_mate_paths_info(mg_ctx* ctx, uint64_t* out, float* ms) {
  if (!ctx) return -1;
  ctx->err.clear();
  if (!ctx->paths.ready) return set_err(ctx, "mg_mate_paths_info: mg_mate_paths must succeed first");
  const PathStage& ps = ctx->paths;
  if (out) {
    out[0] = ps.n_entries;
    out[1] = ps.n_path;
    out[2] = ps.n_pairs;
    out[3] = ps.n_deferred;
  }
  if (ms) {
    ms[0] = ps.explore_ms;
    ms[1] = ps.aggregate_ms;
  }
  return 0;
}

int mg_copy_mate_paths(mg_ctx* ctx, uint8_t* status, uint32_t* visits, uint64_t* path_start, uint32_t* path,
                       uint8_t* flags, uint64_t path_cap) {
  if (!ctx) return -1;
  ctx->err.clear();
  MG_TRY(hipSetDevice(ctx->device));
  if (!ctx->paths.ready) return set_err(ctx, "mg_copy_mate_paths: mg_mate_paths must succeed first");
  const PathStage& ps = ctx->paths;
  hipStream_t st = ctx->stream;
  const uint64_t M = ps.n_entries, P = ps.n_path;
  if (status && M) MG_TRY(hipMemcpyAsync(status, ps.status.p, M, hipMemcpyDeviceToHost, st));
  if (visits && M) MG_TRY(hipMemcpyAsync(visits, ps.visits.p, M * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (path_start) MG_TRY(hipMemcpyAsync(path_start, ps.pstart.p, (M + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  if (P && path_cap >= P) {
    if (path) MG_TRY(hipMemcpyAsync(path, ps.path.p, P * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (flags) MG_TRY(hipMemcpyAsync(flags, ps.flags.p, P, hipMemcpyDeviceToHost, st));
  }
  MG_TRY(hipStreamSynchronize(st));
  return 0;
}

int mg_copy_path_pairs(mg_ctx* ctx, mg_pair_support* out, uint64_t cap, uint64_t* n_copied) {
  if (!ctx) return -1;
  ctx->err.clear();
  if (n_copied) *n_copied = 0;
  MG_TRY(hipSetDevice(ctx->device));
  if (!ctx->paths.ready) return set_err(ctx, "mg_copy_path_pairs: mg_mate_paths must succeed first");
  const uint64_t c = out ? std::min(cap, ctx->paths.n_pairs) : 0;
  if (c) MG_TRY(hipMemcpyAsync(out, ctx->paths.pairs.p, c * sizeof(mg_pair_support), hipMemcpyDeviceToHost, ctx->stream));
  MG_TRY(hipStreamSynchronize(ctx->stream));
  if (n_copied) *n_copied = c;
  return 0;
}

}  // extern "C"
