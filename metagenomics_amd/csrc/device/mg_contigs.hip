// mg_contigs.hip — the strings of overlap-graph edges (contigs) on the device.
//
// Reference path replaced (paths relative to the reference's MetaGenomics directory):
//   OverlapGraph::getStringInEdge                     OverlapGraph.cpp:2009-2041
//
// An edge's string is n + 2 pieces laid end to end (include/mg_overlap.h): the
// whole source read, one suffix per read of the edge's list and a suffix of the
// destination read.  A piece's length depends on two read lengths and one
// offset only, so all output positions are one prefix sum and every output base
// is one 2-bit extract from one resident read.
//
// Pipeline (one stream):
//   k_ctg_len   : thread per piece: its read's slot, the position its suffix
//                 starts at, strand and 'N' flags, the bases it writes; the
//                 smallest invalid piece index is kept by atomicMin;
//   ExclusiveSum: 64-bit positions of all pieces of all edges;
//   k_ctg_start : the edges' string starts (the positions of their first pieces);
//   k_ctg_copy  : one wavefront per 64 consecutive pieces, whose output is
//                 contiguous.  Sub-runs of pieces that fit the LDS span are
//                 staged there, a lane per piece, and stored coalesced; a piece
//                 longer than the span is written by the whole wavefront.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "mg_overlap.h"
#include "mg_stage.hpp"

namespace {

// LDS staging span of one wavefront (one 64-thread workgroup), bytes.  A
// sub-run of pieces is staged when its bases fit; a single piece above it takes
// the wavefront-per-piece path.  4 KiB + one word per workgroup keeps 32
// workgroups per CU inside the 160 KiB of LDS.
constexpr uint32_t kSpan = 4096;

constexpr uint8_t kFwd = 1, kN = 2;

__device__ __forceinline__ uint64_t desc_of(uint64_t slot, uint32_t pos, uint32_t len) {
  return slot | (uint64_t)pos << 32 | (uint64_t)len << 48;
}

// Thread per piece.  pbase[k] = first piece of edge k (n_k + 2 pieces each).
__global__ __launch_bounds__(kThreads) void k_ctg_len(ReadView v, const mg_contig_edge* __restrict__ edges,
                                                      uint64_t n_edges, const uint64_t* __restrict__ pbase,
                                                      const uint32_t* __restrict__ reads,
                                                      const uint16_t* __restrict__ offs, const uint8_t* __restrict__ ors,
                                                      uint64_t n_pieces, uint64_t* __restrict__ desc,
                                                      uint8_t* __restrict__ flag, uint64_t* __restrict__ plen,
                                                      unsigned long long* __restrict__ ctl) {
  const uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= n_pieces) return;
  uint64_t lo = 0, hi = n_edges;  // last edge whose first piece is <= p
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (pbase[mid] <= p) lo = mid;
    else hi = mid;
  }
  const mg_contig_edge e = edges[lo];
  const uint64_t i = p - pbase[lo];  // 0 = source read, 1..n = list, n + 1 = tail
  const uint32_t o = e.orient;
  // the read of this piece and the one before it
  uint32_t id, prev_id = 0;
  bool fwd;
  if (i == 0) {
    id = e.src;
    fwd = o == 2 || o == 3;
  } else if (i <= e.n) {
    id = reads[e.first + i - 1];
    fwd = ors[e.first + i - 1] == 1;
    prev_id = i == 1 ? e.src : reads[e.first + i - 2];
  } else {
    id = e.dst;
    fwd = o == 1 || o == 3;
    prev_id = e.src;  // (read only when n == 0)
  }
  const bool need_prev = i >= 1 && (i <= e.n || e.n == 0);
  bool ok = id >= 1 && id <= v.n && (!need_prev || (prev_id >= 1 && prev_id <= v.n));
  uint64_t slot = 0;
  uint32_t len = 0, pos = 0;
  bool nflag = false;
  if (ok) {
    slot = v.phys ? v.phys[id - 1] : id - 1;
    len = v.len[slot];
    if (i == 0) {
      pos = 0;
    } else if (i <= e.n) {
      const uint32_t prev = v.len[v.phys ? v.phys[prev_id - 1] : prev_id - 1];
      const uint32_t off = offs[e.first + i - 1];
      ok = off <= prev && prev - off <= len;
      pos = prev - off;
      nflag = off == prev;
    } else if (e.n == 0) {
      const uint32_t len1 = v.len[v.phys ? v.phys[prev_id - 1] : prev_id - 1];
      ok = e.offset <= len1 && len1 - (uint32_t)e.offset <= len;
      pos = len1 - (uint32_t)e.offset;
    } else {
      ok = e.tail <= len;
      pos = len - e.tail;
    }
  }
  if (!ok) {
    atomicMin(&ctl[0], (unsigned long long)p);
    pos = len;  // an empty piece: nothing downstream reads out of range
    nflag = false;
  }
  desc[p] = desc_of(slot, pos, len);
  flag[p] = (uint8_t)((fwd ? kFwd : 0) | (nflag ? kN : 0));
  plen[p] = (uint64_t)(len - pos) + (nflag ? 1u : 0u);
}

__global__ __launch_bounds__(kThreads) void k_ctg_start(const uint64_t* __restrict__ pbase,
                                                        const uint64_t* __restrict__ pos, uint64_t entries,
                                                        uint64_t* __restrict__ start) {
  const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k < entries) start[k] = pos[pbase[k]];
}

// Reverse complement of 32 packed bases (complement = ~b, then reverse the 2-bit groups).
__device__ __forceinline__ uint64_t rc_word(uint64_t x) {
  x = __builtin_bitreverse64(~x);
  return ((x >> 1) & 0x5555555555555555ULL) | ((x & 0x5555555555555555ULL) << 1);
}

// The word that holds bases [32 k, 32 k + 32) of the chosen strand of a read of
// `len` bases at w (its words past the read are zero padding, at least one).
// Reverse strand: base q is the complement of forward base len - 1 - q, so the
// word is rc_word of the forward bases [len - 32 k - 32, len - 32 k), which span
// two forward words; bases before position 0 never reach the output.
__device__ __forceinline__ uint64_t strand_word(const uint64_t* __restrict__ w, uint32_t len, uint32_t k, bool fwd) {
  if (fwd) return w[k];
  const int s = (int)len - 32 * (int)k - 32;  // first forward base of the window (may be negative)
  uint64_t x;
  if (s < 0) {
    x = w[0] >> (2 * -s);
  } else {
    const int a = s >> 5, sh = (s & 31) << 1;
    x = sh ? (w[a] << sh) | (w[a + 1] >> (64 - sh)) : w[a];
  }
  return rc_word(x);
}

__device__ __forceinline__ char base_char(uint64_t word, uint32_t q) {
  return "ACGT"[(word >> (62u - 2u * (q & 31u))) & 3u];
}

// One 64-thread workgroup = one wavefront = pieces [64 b, 64 b + 64).
__global__ __launch_bounds__(kWave) void k_ctg_copy(ReadView v, const uint64_t* __restrict__ desc,
                                                    const uint8_t* __restrict__ flag, const uint64_t* __restrict__ pos,
                                                    uint64_t n_pieces, char* __restrict__ out) {
  __shared__ uint32_t lds32[kSpan / 4 + 1];
  char* lds = reinterpret_cast<char*>(lds32);
  const uint32_t lane = threadIdx.x;
  const uint64_t p0 = (uint64_t)blockIdx.x * kWave;
  const uint64_t p = p0 + lane;
  const bool have = p < n_pieces;
  // my piece: output range [o, e), its read and where its suffix starts
  const uint64_t o = have ? pos[p] : 0, e = have ? pos[p + 1] : 0;
  const uint64_t d = have ? desc[p] : 0;
  const uint8_t fl = have ? flag[p] : 0;
  const uint64_t* w = v.words + (d & 0xFFFFFFFFull) * v.stride;
  const uint32_t rpos = (uint32_t)(d >> 32) & 0xFFFFu, rlen = (uint32_t)(d >> 48);
  const bool fwd = fl & kFwd;
  const uint32_t cnt = (uint32_t)(e - o);           // bytes I write ('N' included); <= 65,536
  const uint32_t np = (uint32_t)min((uint64_t)kWave, n_pieces - p0);  // pieces of this wavefront

  uint32_t b = 0;  // first piece not yet written (wavefront-uniform)
  while (b < np) {
    const uint64_t ob = __shfl(o, b);
    // the sub-run [b, c): pieces that end inside the span counted from ob
    const uint64_t fits = __ballot(have && lane >= b && e - ob <= kSpan);
    const uint32_t c = b + (uint32_t)__popcll(fits);  // (e is monotone over the lanes: the set is a prefix of [b, np))
    if (c == b) {
      // piece b alone exceeds the span: the whole wavefront writes it, a byte per lane and round
      const uint64_t db = __shfl(d, b);
      const uint32_t cb = __shfl(cnt, b);
      const uint8_t fb = (uint8_t)__shfl((int)fl, b);
      const uint64_t* wb = v.words + (db & 0xFFFFFFFFull) * v.stride;
      const uint32_t posb = (uint32_t)(db >> 32) & 0xFFFFu, lenb = (uint32_t)(db >> 48);
      const uint32_t nn = (fb & kN) ? 1u : 0u;
      for (uint32_t j = lane; j < cb; j += kWave) {
        char ch = 'N';
        if (j >= nn) {
          const uint32_t q = posb + (j - nn);
          ch = base_char(strand_word(wb, lenb, q >> 5, fb & kFwd), q);
        }
        out[ob + j] = ch;
      }
      b += 1;
      continue;
    }
    // stage my piece at the offset it has from ob, shifted so that LDS words and
    // output words share their alignment
    const uint32_t a = (uint32_t)(ob & 3u);
    if (have && lane >= b && lane < c && cnt) {
      char* dst = lds + a + (uint32_t)(o - ob);
      uint32_t j = 0;
      if (fl & kN) dst[j++] = 'N';
      uint32_t q = rpos;
      uint32_t kw = q >> 5;
      uint64_t word = strand_word(w, rlen, kw, fwd);
      for (; j < cnt; ++j, ++q) {
        if ((q >> 5) != kw) {
          kw = q >> 5;
          word = strand_word(w, rlen, kw, fwd);
        }
        dst[j] = base_char(word, q);
      }
    }
    __syncthreads();
    const uint32_t total = a + (uint32_t)(__shfl(e, c - 1) - ob);  // staged bytes end here (a pad bytes first)
    const uint64_t gbase = ob - a;                                 // 4-byte aligned (out is)
    for (uint32_t x = lane; 4 * x < total; x += kWave) {
      const uint32_t lo = 4 * x, hi = lo + 4;
      if (lo >= a && hi <= total) {
        *reinterpret_cast<uint32_t*>(out + gbase + lo) = lds32[x];
      } else {
        for (uint32_t y = max(lo, a); y < min(hi, total); ++y) out[gbase + y] = lds[y];
      }
    }
    __syncthreads();
    b = c;
  }
}

}  // namespace

extern "C" {

int mg_build_contigs(mg_ctx* ctx, const mg_contig_edge* edges, uint64_t n_edges, const uint32_t* reads,
                     const uint16_t* offs, const uint8_t* ors, uint64_t n_list, uint64_t* total_bases,
                     float* device_ms) {
  if (!ctx) return -1;
  ctx->err.clear();
  if (total_bases) *total_bases = 0;
  if (device_ms) *device_ms = 0.f;
  ctx->contigs.ready = false;
  if ((n_edges && !edges) || (n_list && (!reads || !offs || !ors))) return set_err(ctx, "mg_build_contigs: null argument");
  MG_TRY(hipSetDevice(ctx->device));
  if (!ctx->n || !ctx->d_words.p || !ctx->d_len.p) return set_err(ctx, "mg_build_contigs: no reads on the device");
  // first piece of every edge; list ranges must lie inside the lists
  std::vector<uint64_t> pbase;
  if (edge_bases(ctx, "mg_build_contigs", edges, n_edges, n_list, 2, pbase)) return -1;
  const uint64_t P = pbase[n_edges];
  hipStream_t st = ctx->stream;
  ContigStage& cg = ctx->contigs;
  MG_GROW(cg.desc, P, "d_ctg_desc");
  MG_GROW(cg.flag, P, "d_ctg_flag");
  MG_GROW(cg.len, P + 1, "d_ctg_len");
  MG_GROW(cg.pos, P + 1, "d_ctg_pos");
  MG_GROW(cg.pbase, n_edges + 1, "d_ctg_pbase");
  MG_GROW(cg.start, n_edges + 1, "d_ctg_start");
  MG_GROW(cg.ctl, 1, "d_ctg_ctl");
  size_t tmp_bytes = 0;
  MG_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, cg.len.p, cg.pos.p, (int64_t)(P + 1), st));
  MG_GROW(cg.tmp, tmp_bytes, "d_ctg_tmp");
  // the caller's lists, for the length kernel only
  Scratch<mg_contig_edge> d_edges;
  EdgeLists lists;
  MG_SCRATCH(d_edges, n_edges, "contig edges");
  if (n_edges) MG_TRY(hipMemcpyAsync(d_edges.p, edges, n_edges * sizeof(mg_contig_edge), hipMemcpyHostToDevice, st));
  if (lists.upload(ctx, "contig", reads, offs, ors, n_list)) return -1;
  MG_TRY(hipMemcpyAsync(cg.pbase.p, pbase.data(), (n_edges + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  MG_TRY(ctl_fill(st, cg.ctl.p, 1, ~0ull));
  MG_TRY(hipMemsetAsync(cg.len.p + P, 0, sizeof(uint64_t), st));
  const ReadView v = view_of(ctx);

  MG_TRY(cg.ev.start(st));
  if (P) {
    hipLaunchKernelGGL(k_ctg_len, dim3(blocks_for(P)), dim3(kThreads), 0, st, v, d_edges.p, n_edges, cg.pbase.p,
                       lists.reads.p, lists.offs.p, lists.ors.p, P, cg.desc.p, cg.flag.p, cg.len.p, cg.ctl.p);
    MG_TRY(hipGetLastError());
  }
  MG_TRY(hipcub::DeviceScan::ExclusiveSum(cg.tmp.p, tmp_bytes, cg.len.p, cg.pos.p, (int64_t)(P + 1), st));
  hipLaunchKernelGGL(k_ctg_start, dim3(blocks_for(n_edges + 1)), dim3(kThreads), 0, st, cg.pbase.p, cg.pos.p,
                     n_edges + 1, cg.start.p);
  MG_TRY(hipGetLastError());
  // one host read: the error word and the total decide whether and where the copy kernel writes
  unsigned long long bad = ~0ull;
  uint64_t total = 0;
  MG_TRY(hipMemcpyAsync(&total, cg.pos.p + P, sizeof(total), hipMemcpyDeviceToHost, st));
  MG_TRY(ctl_read(st, cg.ctl.p, 1, &bad));
  if (bad != ~0ull) {
    const uint64_t k = (uint64_t)(std::upper_bound(pbase.begin(), pbase.end(), (uint64_t)bad) - pbase.begin()) - 1;
    const uint64_t i = bad - pbase[k];
    const std::string which = i == 0 ? "the source read"
                              : i <= edges[k].n ? "list entry " + std::to_string(i - 1)
                                                : "the destination read";
    ctx->err = "mg_build_contigs: " + edge_name(edges, k) + ", piece " + std::to_string(i) + " (" + which +
               "): a read ID outside 1.." + std::to_string(ctx->n) +
               " or a substring position outside its read (std::string::substr would throw) (-2)";
    return -2;
  }
  MG_GROW(cg.out, (total + 3) & ~3ull, "d_ctg_out");
  if (P) {
    hipLaunchKernelGGL(k_ctg_copy, dim3((uint32_t)((P + kWave - 1) / kWave)), dim3(kWave), 0, st, v, cg.desc.p,
                       cg.flag.p, cg.pos.p, P, cg.out.p);
    MG_TRY(hipGetLastError());
  }
  MG_TRY(cg.ev.end(st));
  MG_TRY(hipStreamSynchronize(st));
  MG_TRY(cg.ev.elapsed(device_ms));
  cg.n_edges = n_edges;
  cg.n_bases = total;
  ctx->contigs.ready = true;
  if (total_bases) *total_bases = total;
  return 0;
}

int mg_copy_contigs(mg_ctx* ctx, uint64_t* start, char* out, uint64_t cap, uint64_t* n_copied) {
  if (!ctx) return -1;
  ctx->err.clear();
  MG_TRY(hipSetDevice(ctx->device));
  if (n_copied) *n_copied = 0;
  if (!ctx->contigs.ready)
    return set_err(ctx, "mg_copy_contigs: mg_build_contigs must succeed for the current reads first");
  const ContigStage& cg = ctx->contigs;
  return copy_csr(ctx, cg.start.p, cg.n_edges + 1, start, cg.out.p, cg.n_bases, out, cap, n_copied);
}

}  // extern "C"
