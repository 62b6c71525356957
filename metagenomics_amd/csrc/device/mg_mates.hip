// mg_mates.hip — batched read lookup and the per-read mate lists on the device.
//
// Reference path replaced (paths relative to the reference's MetaGenomics directory):
//   Dataset::getReadFromString (binary search)        Dataset.cpp:421-455
//   storeMatePairInformation, per-pair body           Dataset.cpp:269-301
//   Read::addMatePair (append unless already present) Read.cpp:132-166
//
// Pipeline (one stream):
//   k_ingest / k_ingest_long : the ingest's own per-record stage over the raw
//                     mates (mg_dataset.hip): testRead, canonical strand packed,
//                     and "the record is its own canonical string";
//   k_find_reads    : thread per record, binary search over the reads in ID
//                     order (through d_phys when the slots are clustered):
//                     packed words first, then length = std::string order;
//   k_mate_emit     : thread per pair: good / bad, superReadID redirect, the
//                     substring test of a redirected mate, two records with
//                     sequence numbers 2p and 2p + 1;
//   stable radix passes by (dataset, orient), then (owner, mate) -> equal
//                     records adjacent, sequence ascending inside a run;
//   k_mate_first    : the first of each run keeps its owner, the rest drop;
//   stable radix by owner over the sequence order -> every list in ascending
//                     sequence number = addMatePair's order;
//   k_mate_write / k_csr_starts : mg_mate records and the CSR starts (mg_stage.hpp).
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "mg_overlap.h"
#include "mg_stage.hpp"

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;  // owner of a record that is not kept

// base p (0..3) of a packed string, most-significant base first
__device__ __forceinline__ uint32_t base_at(const uint64_t* w, uint32_t p) {
  return (uint32_t)(w[p >> 5] >> (62u - 2u * (p & 31u))) & 3u;
}

// Thread per record: Dataset::getReadFromString.  The comparison is the
// ingest's sort order: words first (zero padding reads as 'A'), then length.
__global__ __launch_bounds__(kThreads) void k_find_reads(ReadView v, const uint64_t* __restrict__ canon,
                                                         const uint16_t* __restrict__ qlen,
                                                         const uint8_t* __restrict__ valid,
                                                         const uint8_t* __restrict__ fwd, uint64_t nq, uint32_t cw,
                                                         uint32_t* __restrict__ id_out, uint8_t* __restrict__ flags_out) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= nq) return;
  uint32_t id = 0;
  uint8_t flags = 0;
  if (valid[i]) {
    flags = 1;
    const uint64_t* q = canon + i * cw;
    const uint32_t L = qlen[i];
    // words of the record past the slot width: a non-zero one makes it larger than every read
    bool tail = false;
    for (uint32_t k = v.maxw; k < cw; ++k) tail = tail || q[k] != 0;
    uint64_t lo = 0, hi = v.n;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      const uint64_t slot = slot_of(v, mid);
      const uint64_t* r = v.words + slot * v.stride;
      int c = 0;  // read mid <=> record
      for (uint32_t k = 0; k < v.maxw && c == 0; ++k) {
        const uint64_t rw = r[k], qw = k < cw ? q[k] : 0ull;
        if (rw != qw) c = rw < qw ? -1 : 1;
      }
      if (c == 0 && tail) c = -1;
      if (c == 0) {
        const uint32_t rl = v.len[slot];
        c = rl < L ? -1 : rl > L ? 1 : 0;
      }
      if (c == 0) {
        id = (uint32_t)mid + 1;
        break;
      }
      if (c < 0) lo = mid + 1;
      else hi = mid;
    }
    if (id && fwd[i]) flags |= 2;
  }
  id_out[i] = id;
  flags_out[i] = flags;
}

// string::find of raw mate i in the forward string of the read in `slot`
// (Dataset.cpp:291-292).  The raw mate is its canonical string (fwd) or that
// string's reverse complement.  At each offset the mate's first min(L, 32)
// bases are compared as one packed word; the rest base by base.
__device__ bool mate_occurs(const ReadView& v, uint64_t slot, const uint64_t* q, uint32_t L, bool fwd) {
  const uint32_t n2 = v.len[slot];
  if (L > n2) return false;
  const uint64_t* t = v.words + slot * v.stride;
  auto qbase = [&](uint32_t j) { return fwd ? base_at(q, j) : 3u - base_at(q, L - 1 - j); };
  const uint32_t m = L < 32u ? L : 32u;
  uint64_t q0 = 0;
  for (uint32_t j = 0; j < m; ++j) q0 |= (uint64_t)qbase(j) << (62u - 2u * j);
  const uint64_t mask = m == 32u ? ~0ull : ~(~0ull >> (2u * m));
  for (uint32_t s = 0; s + L <= n2; ++s) {
    const uint32_t k = s >> 5, sh = 2u * (s & 31u);
    uint64_t win = t[k] << sh;
    if (sh && k + 1 < v.maxw) win |= t[k + 1] >> (64u - sh);  // (the bases compared lie below n2 <= 32 maxw)
    if ((win & mask) != q0) continue;
    bool eq = true;
    for (uint32_t j = 32; j < L && eq; ++j) eq = base_at(t, s + j) == qbase(j);
    if (eq) return true;
  }
  return false;
}

// ctl[0] = smallest raw index of a good mate without a resident read, ctl[1] = good pairs
__global__ __launch_bounds__(kThreads) void k_mate_emit(ReadView v, const uint64_t* __restrict__ canon,
                                                        const uint16_t* __restrict__ qlen,
                                                        const uint8_t* __restrict__ valid,
                                                        const uint8_t* __restrict__ fwd, const uint32_t* __restrict__ ids,
                                                        uint64_t n_pairs, uint32_t cw,
                                                        const uint64_t* __restrict__ ds_end, uint32_t n_datasets,
                                                        const uint32_t* __restrict__ super,
                                                        uint32_t* __restrict__ owner, uint32_t* __restrict__ mate,
                                                        uint16_t* __restrict__ od, unsigned long long* __restrict__ ctl) {
  const uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  bool good = false;
  if (p < n_pairs) {
    const uint64_t i1 = 2 * p, i2 = 2 * p + 1;
    good = valid[i1] && valid[i2];  // Dataset.cpp:275
    uint32_t r1 = 0, r2 = 0;
    if (good) {
      r1 = ids[i1];
      r2 = ids[i2];
      if (!r1) atomicMin(&ctl[0], (unsigned long long)i1);
      if (!r2) atomicMin(&ctl[0], (unsigned long long)i2);
    }
    uint32_t o1 = 0, o2 = 0;
    uint16_t d = 0;
    if (good && r1 && r2) {
      o1 = fwd[i1];
      o2 = fwd[i2];
      if (super) {  // once, not transitively (:280-284)
        const uint32_t s1 = super[slot_of(v, r1 - 1)], s2 = super[slot_of(v, r2 - 1)];
        if (s1) {
          r1 = s1;
          o1 = mate_occurs(v, slot_of(v, r1 - 1), canon + i1 * cw, qlen[i1], fwd[i1] != 0) ? 1u : 0u;
        }
        if (s2) {
          r2 = s2;
          o2 = mate_occurs(v, slot_of(v, r2 - 1), canon + i2 * cw, qlen[i2], fwd[i2] != 0) ? 1u : 0u;
        }
      }
      uint32_t lo = 0, hi = n_datasets;  // first dataset whose end lies beyond p
      while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (ds_end[mid] <= p) lo = mid + 1;
        else hi = mid;
      }
      d = (uint16_t)lo;
    }
    const bool emit = good && r1 && r2;
    owner[i1] = emit ? r1 : kNone;
    mate[i1] = r2;
    od[i1] = (uint16_t)(d << 2 | (o1 * 2 + o2));
    owner[i2] = emit ? r2 : kNone;
    mate[i2] = r1;
    od[i2] = (uint16_t)(d << 2 | (o1 + o2 * 2));
  }
  const uint64_t bal = __ballot(good);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&ctl[1], (unsigned long long)__popcll(bal));
}

__global__ __launch_bounds__(kThreads) void k_mate_iota(uint32_t* __restrict__ v, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) v[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kThreads) void k_mate_gather64(const uint32_t* __restrict__ owner,
                                                            const uint32_t* __restrict__ mate,
                                                            const uint32_t* __restrict__ idx, uint64_t n,
                                                            uint64_t* __restrict__ key) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) key[i] = (uint64_t)owner[idx[i]] << 32 | mate[idx[i]];
}

// sorted by (owner, mate, dataset, orient), sequence ascending inside a run:
// the first record of a run is the one addMatePair appends
__global__ __launch_bounds__(kThreads) void k_mate_first(const uint32_t* __restrict__ owner,
                                                         const uint32_t* __restrict__ mate,
                                                         const uint16_t* __restrict__ od,
                                                         const uint32_t* __restrict__ idx, uint64_t n,
                                                         uint32_t* __restrict__ okey) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t a = idx[i];
  bool first = owner[a] != kNone;
  if (first && i) {
    const uint32_t b = idx[i - 1];
    first = owner[a] != owner[b] || mate[a] != mate[b] || od[a] != od[b];
  }
  okey[a] = first ? owner[a] : kNone;
}

__global__ __launch_bounds__(kThreads) void k_mate_write(const uint32_t* __restrict__ sorted_owner,
                                                         const uint32_t* __restrict__ seq,
                                                         const uint32_t* __restrict__ mate,
                                                         const uint16_t* __restrict__ od, uint64_t n,
                                                         mg_mate* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n || sorted_owner[i] == kNone) return;
  const uint32_t a = seq[i];
  mg_mate m;
  m.id = mate[a];
  m.orient = (uint8_t)(od[a] & 3u);
  m.dataset = (uint8_t)(od[a] >> 2);
  m.pad = 0;
  out[i] = m;
}

// the raw records on the device, filtered, packed and looked up
struct Lookup {
  Scratch<char> ascii;
  Scratch<uint64_t> off, canon;
  Scratch<uint16_t> len;
  Scratch<uint8_t> valid, fwd, flags;
  Scratch<uint32_t> ids;
  uint32_t cw = 1;
};

// uploads the records, starts the stage's clock after the transfers, runs the filter and the search
int lookup(mg_ctx* ctx, const char* concat, const uint64_t* offsets, uint64_t n_raw, uint32_t min_overlap, Lookup& q) {
  hipStream_t st = ctx->stream;
  uint64_t longest = 0;
  for (uint64_t i = 0; i < n_raw; ++i) {
    if (offsets[i + 1] < offsets[i]) return set_err(ctx, "record offsets must not decrease");
    const uint64_t L = offsets[i + 1] - offsets[i];
    if (L > min_overlap && L <= 65535) longest = std::max(longest, L);
  }
  const uint64_t total = n_raw ? offsets[n_raw] : 0;
  q.cw = ingest_record_words(longest);
  MG_SCRATCH(q.ascii, total, "mate records");
  MG_SCRATCH(q.off, n_raw + 1, "mate record offsets");
  MG_SCRATCH(q.canon, n_raw * q.cw, "mate canonical words");
  MG_SCRATCH(q.len, n_raw, "mate record lengths");
  MG_SCRATCH(q.valid, n_raw, "mate filter flags");
  MG_SCRATCH(q.fwd, n_raw, "mate strand flags");
  MG_SCRATCH(q.flags, n_raw, "mate lookup flags");
  MG_SCRATCH(q.ids, n_raw, "mate read IDs");
  if (total) MG_TRY(hipMemcpyAsync(q.ascii.p, concat, total, hipMemcpyHostToDevice, st));
  if (n_raw) MG_TRY(hipMemcpyAsync(q.off.p, offsets, (n_raw + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  MG_TRY(hipMemsetAsync(q.fwd.p, 0, std::max<uint64_t>(n_raw, 1), st));
  MG_TRY(ctx->mates.ev.start(st));
  if (!n_raw) return 0;
  if (ingest_records(ctx, q.ascii.p, q.off.p, n_raw, min_overlap, q.cw, q.canon.p, q.len.p, q.valid.p, q.fwd.p))
    return -1;
  hipLaunchKernelGGL(k_find_reads, dim3(blocks_for(n_raw)), dim3(kThreads), 0, st, view_of(ctx), q.canon.p, q.len.p,
                     q.valid.p, q.fwd.p, n_raw, q.cw, q.ids.p, q.flags.p);
  MG_TRY(hipGetLastError());
  return 0;
}

int have_reads(mg_ctx* ctx, const char* who) {
  if (ctx->n && (!ctx->d_words.p || !ctx->d_len.p)) return set_err(ctx, std::string(who) + ": no reads on the device");
  return 0;
}

}  // namespace

extern "C" {

int mg_find_reads(mg_ctx* ctx, const char* concat, const uint64_t* offsets, uint64_t n_raw, uint32_t min_overlap,
                  uint32_t* id_out, uint8_t* flags_out, float* device_ms) {
  if (!ctx) return -1;
  ctx->err.clear();
  if (device_ms) *device_ms = 0.f;
  if (n_raw && (!concat || !offsets || !id_out || !flags_out)) return set_err(ctx, "mg_find_reads: null argument");
  MG_TRY(hipSetDevice(ctx->device));
  if (n_raw >> 31) return set_err(ctx, "mg_find_reads: 2^31 or more records are not supported");
  if (have_reads(ctx, "mg_find_reads")) return -1;
  Lookup q;
  if (lookup(ctx, concat, offsets, n_raw, min_overlap, q)) return -1;
  MG_TRY(ctx->mates.ev.end(ctx->stream));
  if (n_raw) {
    MG_TRY(hipMemcpyAsync(id_out, q.ids.p, n_raw * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    MG_TRY(hipMemcpyAsync(flags_out, q.flags.p, n_raw, hipMemcpyDeviceToHost, ctx->stream));
  }
  MG_TRY(hipStreamSynchronize(ctx->stream));
  MG_TRY(ctx->mates.ev.elapsed(device_ms));
  return 0;
}

int mg_build_mate_pairs(mg_ctx* ctx, const char* concat, const uint64_t* offsets, uint64_t n_raw,
                        const uint64_t* pairs_per_dataset, uint32_t n_datasets, uint32_t min_overlap, int use_super,
                        uint64_t* n_records, uint64_t* good_bad_pairs, float* device_ms) {
  if (!ctx) return -1;
  ctx->err.clear();
  if (n_records) *n_records = 0;
  if (good_bad_pairs) good_bad_pairs[0] = good_bad_pairs[1] = 0;
  if (device_ms) *device_ms = 0.f;
  ctx->mates.ready = false;
  if (n_raw & 1) return set_err(ctx, "mg_build_mate_pairs: n_raw must be even (two mates per pair)");
  if (n_raw && (!concat || !offsets)) return set_err(ctx, "mg_build_mate_pairs: null argument");
  if (n_datasets > 256) return set_err(ctx, "mg_build_mate_pairs: more than 256 datasets (datasetNumber is UINT8)");
  if (n_datasets && !pairs_per_dataset) return set_err(ctx, "mg_build_mate_pairs: null argument");
  const uint64_t n_pairs = n_raw / 2;
  std::vector<uint64_t> ds_end(std::max<uint32_t>(n_datasets, 1), 0);
  uint64_t sum = 0;
  for (uint32_t d = 0; d < n_datasets; ++d) {
    if (pairs_per_dataset[d] > n_pairs - sum)
      return set_err(ctx, "mg_build_mate_pairs: pairs_per_dataset does not add up to n_raw / 2");
    sum += pairs_per_dataset[d];
    ds_end[d] = sum;
  }
  if (sum != n_pairs) return set_err(ctx, "mg_build_mate_pairs: pairs_per_dataset does not add up to n_raw / 2");
  MG_TRY(hipSetDevice(ctx->device));
  if (n_raw >> 31) return set_err(ctx, "mg_build_mate_pairs: 2^31 or more records are not supported");
  if (have_reads(ctx, "mg_build_mate_pairs")) return -1;
  if (use_super) {
    if (whole_multiset(ctx, "mg_build_mate_pairs (use_super)")) return -1;
    if (!ctx->index_ready || !ctx->contained_done || !ctx->d_super.p)
      return set_err(ctx, "mg_build_mate_pairs: use_super needs a completed mg_mark_contained for the current reads");
  }
  hipStream_t st = ctx->stream;
  const uint64_t N = ctx->n, entries = N + 2;
  MG_GROW(ctx->mates.start, entries, "d_mate_start");
  MG_GROW(ctx->mates.recs, n_raw, "d_mates");
  ctx->mates.n = 0;

  Lookup q;
  Scratch<uint32_t> owner, mate, idx_a, idx_b, okey_a, okey_b;
  Scratch<uint16_t> od, od_sorted;
  Scratch<uint64_t> k64_a, k64_b, d_ds;
  Scratch<unsigned long long> ctl;
  Scratch<uint8_t> tmp;
  MG_SCRATCH(owner, n_raw, "mate record owners");
  MG_SCRATCH(mate, n_raw, "mate record mates");
  MG_SCRATCH(od, n_raw, "mate dataset and orientation keys");
  MG_SCRATCH(idx_a, n_raw, "mate sort values");
  MG_SCRATCH(idx_b, n_raw, "mate sort values");
  MG_SCRATCH(okey_a, n_raw, "mate owner keys");
  MG_SCRATCH(okey_b, n_raw, "mate owner keys");
  MG_SCRATCH(od_sorted, n_raw, "mate dataset and orientation keys");
  MG_SCRATCH(k64_a, n_raw, "mate pair keys");
  MG_SCRATCH(k64_b, n_raw, "mate pair keys");
  MG_SCRATCH(d_ds, ds_end.size(), "mate dataset ends");
  MG_SCRATCH(ctl, 2, "mate control words");
  size_t tmp_bytes = 0;
  {
    size_t t = 0;
    MG_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, t, od.p, od_sorted.p, idx_a.p, idx_b.p, (int)n_raw, 0, 10, st));
    tmp_bytes = std::max(tmp_bytes, t);
    MG_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, t, k64_a.p, k64_b.p, idx_b.p, idx_a.p, (int)n_raw, 0, 64, st));
    tmp_bytes = std::max(tmp_bytes, t);
    MG_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, t, okey_a.p, okey_b.p, idx_b.p, idx_a.p, (int)n_raw, 0, 32, st));
    tmp_bytes = std::max(tmp_bytes, t);
  }
  MG_SCRATCH(tmp, tmp_bytes, "mate sort storage");
  MG_TRY(ctl_fill(st, ctl.p, 1, ~0ull));  // the smallest raw index of a good mate without a read
  MG_TRY(ctl_fill(st, ctl.p + 1, 1, 0));  // good pairs
  MG_TRY(hipMemcpyAsync(d_ds.p, ds_end.data(), ds_end.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));

  if (lookup(ctx, concat, offsets, n_raw, min_overlap, q)) return -1;
  unsigned long long ctlh[2] = {~0ull, 0ull};
  if (n_raw) {
    hipLaunchKernelGGL(k_mate_emit, dim3(blocks_for(n_pairs)), dim3(kThreads), 0, st, view_of(ctx), q.canon.p, q.len.p,
                       q.valid.p, q.fwd.p, q.ids.p, n_pairs, q.cw, d_ds.p, n_datasets,
                       use_super ? (const uint32_t*)ctx->d_super.p : (const uint32_t*)nullptr, owner.p, mate.p, od.p,
                       ctl.p);
    MG_TRY(hipGetLastError());
    // (dataset, orient), then (owner, mate): stable, so a run of equal records is in sequence order
    hipLaunchKernelGGL(k_mate_iota, dim3(blocks_for(n_raw)), dim3(kThreads), 0, st, idx_a.p, n_raw);
    size_t tb = tmp_bytes;
    MG_TRY(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, od.p, od_sorted.p, idx_a.p, idx_b.p, (int)n_raw, 0, 10, st));
    hipLaunchKernelGGL(k_mate_gather64, dim3(blocks_for(n_raw)), dim3(kThreads), 0, st, owner.p, mate.p, idx_b.p, n_raw,
                       k64_a.p);
    tb = tmp_bytes;
    MG_TRY(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, k64_a.p, k64_b.p, idx_b.p, idx_a.p, (int)n_raw, 0, 64, st));
    hipLaunchKernelGGL(k_mate_first, dim3(blocks_for(n_raw)), dim3(kThreads), 0, st, owner.p, mate.p, od.p, idx_a.p, n_raw,
                       okey_a.p);
    // kept records by owner over the sequence order
    hipLaunchKernelGGL(k_mate_iota, dim3(blocks_for(n_raw)), dim3(kThreads), 0, st, idx_b.p, n_raw);
    tb = tmp_bytes;
    MG_TRY(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, okey_a.p, okey_b.p, idx_b.p, idx_a.p, (int)n_raw, 0, 32, st));
    hipLaunchKernelGGL(k_mate_write, dim3(blocks_for(n_raw)), dim3(kThreads), 0, st, okey_b.p, idx_a.p, mate.p, od.p, n_raw,
                       ctx->mates.recs.p);
    MG_TRY(hipGetLastError());
  }
  MG_TRY(csr_starts(st, okey_b.p, n_raw, entries, ctx->mates.start.p));
  MG_TRY(ctx->mates.ev.end(st));
  uint64_t total = 0;
  MG_TRY(hipMemcpyAsync(&total, ctx->mates.start.p + (entries - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  MG_TRY(ctl_read(st, ctl.p, 2, ctlh));
  MG_TRY(ctx->mates.ev.elapsed(device_ms));
  if (good_bad_pairs) {
    good_bad_pairs[0] = ctlh[1];
    good_bad_pairs[1] = n_pairs - ctlh[1];
  }
  if (ctlh[0] != ~0ull) {
    ctx->err = "mg_build_mate_pairs: String not found in Dataset: raw record " + std::to_string(ctlh[0]) +
               " passes the filter but no resident read equals it (-2)";
    return -2;
  }
  ctx->mates.n = total;
  ctx->mates.ready = true;
  if (n_records) *n_records = total;
  return 0;
}

int mg_copy_mate_pairs(mg_ctx* ctx, uint64_t* start, mg_mate* out, uint64_t cap, uint64_t* n_copied) {
  if (!ctx) return -1;
  ctx->err.clear();
  MG_TRY(hipSetDevice(ctx->device));
  if (n_copied) *n_copied = 0;
  if (!ctx->mates.ready)
    return set_err(ctx, "mg_copy_mate_pairs: mg_build_mate_pairs must run for the current reads first");
  return copy_csr(ctx, ctx->mates.start.p, ctx->n + 2, start, ctx->mates.recs.p, ctx->mates.n, out, cap, n_copied);
}

}  // extern "C"
