// mg_ctx.hpp — INTERNAL: the device context behind include/mg_overlap.h,
// shared by the kernel translation units (mg_kernels.hip: index + discovery +
// exchange; mg_dataset.hip: Dataset ingest on the device; mg_disc.hip: the
// per-read discovery lists D(A); mg_comp.hip: their components; mg_mates.hip:
// read lookup and the per-read mate lists; mg_contigs.hip: the strings of edges;
// mg_places.hip: read placements, insert sizes and edge coverage; mg_paths.hip:
// mate-pair paths; mg_scaffold.hip: scaffolder support; mg_chains.hip: safe
// chains of a replayed graph).  The core
// fields of mg_ctx belong to mg_kernels.hip; each
// derived stage keeps its state in one struct (DiscStage .. ChainStage: ready
// flag, counts, test options, buffers, EventPair) that mg_ctx embeds by value.
// The whole context follows one ownership model: every resident device buffer
// is a DevArray (grown with MG_GROW / MG_ENSURE, freed by its destructor when
// mg_destroy deletes the context), every call-lifetime buffer a Scratch, and
// both allocate through ctx_malloc; the plain pointers left in mg_ctx are
// aliases into those arrays or into the caller's memory and own nothing.
// What the stage files share beyond this (the read view, CSR helpers) is in
// mg_stage.hpp.
#ifndef MG_CTX_HPP_
#define MG_CTX_HPP_
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "mg_overlap.h"

// Device slot of a read: a power-of-two number of words (W = 5 -> 8 words, one
// aligned 64-B sector), so a partner fetch never straddles two sectors.
__host__ __device__ constexpr int slot_words(int w) {
  return w <= 1 ? 1 : w <= 2 ? 2 : w <= 4 ? 4 : w <= 8 ? 8 : w <= 16 ? 16 : 32;
}

// The slot's word that carries the read's reference ID - 1 in clustered slots
// (low 32 bits, high 32 bits 0), or -1 when the width has no
// spare word: the last word of the slot where it lies beyond word W, the zero
// pad that load_slot, the scan's rw[MAXW] and ext_slot read.  Written by
// k_layout_gather, read by k_probe's verification, both at the template width
// dispatch_w selects (never mg_ctx::maxw: maxw 7 runs template 8, 9-11 run 12).
__host__ __device__ constexpr int slot_id_word(int w) { return slot_words(w) >= w + 2 ? slot_words(w) - 1 : -1; }
static_assert(slot_id_word(5) == 7 && slot_id_word(6) == 7 && slot_id_word(12) == 15, "widths with a spare word");
static_assert(slot_id_word(1) == -1 && slot_id_word(2) == -1 && slot_id_word(3) == -1 && slot_id_word(4) == -1 &&
                  slot_id_word(8) == -1 && slot_id_word(16) == -1 && slot_id_word(32) == -1,
              "widths whose slot ends at the pad word (or before it)");

// A device array that lives as long as the context and is freed with it
// (mg_destroy deletes the context with its device set and its stream idle):
// pointer and capacity travel together (a layout commit and mg_disc.hip swap
// two of them whole).  Grown with MG_GROW / MG_ENSURE (below).
template <typename T>
struct DevArray {
  T* p = nullptr;
  size_t cap = 0;  // elements
  DevArray() = default;
  DevArray(const DevArray&) = delete;
  DevArray& operator=(const DevArray&) = delete;
  ~DevArray() { release(); }
  // at least `count` elements (contents not kept); `what` names the buffer in the error message
  hipError_t ensure(mg_ctx* ctx, size_t count, const char* what);
  void swap(DevArray& o) {
    std::swap(p, o.p);
    std::swap(cap, o.cap);
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// Device memory for the length of one call, allocated through ctx_malloc under
// a readable name (option "alloc_cap" and the allocation message apply) and
// freed on return.  p stays null until alloc(): hipcub's size queries take it so.
template <typename T>
struct Scratch {
  T* p = nullptr;
  Scratch() = default;
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  ~Scratch() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(mg_ctx* ctx, size_t count, const char* what);
};

// The two events a stage times itself with, created on first use, destroyed
// with the context.
struct EventPair {
  hipEvent_t ev[2] = {};
  EventPair() = default;
  EventPair(const EventPair&) = delete;
  EventPair& operator=(const EventPair&) = delete;
  ~EventPair() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  hipError_t start(hipStream_t st) {
    for (auto& e : ev)
      if (!e) {
        const hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) return rc;
      }
    return hipEventRecord(ev[0], st);
  }
  hipError_t end(hipStream_t st) { return hipEventRecord(ev[1], st); }
  hipError_t wait() { return hipEventSynchronize(ev[1]); }
  // (both events completed) device_ms may be null
  hipError_t elapsed(float* device_ms) { return device_ms ? hipEventElapsedTime(device_ms, ev[0], ev[1]) : hipSuccess; }
};

// per-read discovery lists D(A) (mg_disc.hip, mg_build_discoveries): the rows
// of the last mg_find_overlaps grouped by src into a CSR array and each
// segment sorted by (window j, dst, key o).  ready: the lists belong to those rows
struct DiscStage {
  bool ready = false;
  uint64_t n = 0;          // records
  uint32_t block_cap = 0;  // option "disc_block_cap" (tests): records the workgroup sort takes (0 = 2,048)
  DevArray<uint32_t> cnt;    // rows per src, then the scatter's cursors (n + 2)
  DevArray<uint64_t> start;  // start[A] (n + 2)
  DevArray<uint64_t> recs;   // one 8-B record per row: the sort key, then the mg_disc record
  DevArray<uint32_t> list;   // reads of degree > 64: workgroup path from the front, oversized from the back
  DevArray<uint32_t> boff;   // oversized segments: their offsets in big[]
  DevArray<uint64_t> big[2];  // oversized segments gathered for the segmented radix sort
  DevArray<uint8_t> tmp;      // rocprim temporary storage (scans, segmented sort)
  DevArray<unsigned long long> ctl;  // kDiscCtl control words (errors, class counts, self duplicates)
  // self rows only (tandem repeats): the duplicate-free copy and its starts, swapped with recs / start
  DevArray<uint64_t> recs_alt, start_alt;
  DevArray<uint32_t> pre;  // kept records before each record
  EventPair ev;
};

// connected components of the discovery lists (mg_comp.hip, mg_build_components):
// ready: labels and table belong to the current lists (cleared with disc.ready
// and by every mg_build_discoveries)
struct CompStage {
  bool ready = false;
  uint64_t n = 0;             // components in the table
  DevArray<uint32_t> parent;  // union-find parent[0 .. n + 1]; after the flatten: reads per root
  DevArray<uint32_t> label;   // label[0 .. n + 1], label[0] = 0
  DevArray<uint32_t> acc;     // per root: records [0, n + 2), self records [n + 2, 2 (n + 2))
  DevArray<mg_comp> table;    // ascending root
  EventPair ev;
};

// per-read mate lists (mg_mates.hip, mg_build_mate_pairs): one CSR of mg_mate
// records over the reads; ready until new reads arrive (reset_derived)
struct MateStage {
  bool ready = false;
  uint64_t n = 0;            // records
  DevArray<uint64_t> start;  // start[A] (n + 2)
  DevArray<mg_mate> recs;
  EventPair ev;
};

// contig strings (mg_contigs.hip, mg_build_contigs): one descriptor and one
// output position per piece, the edges' string starts and the ASCII bases;
// ready until new reads arrive (reset_derived)
struct ContigStage {
  bool ready = false;
  uint64_t n_edges = 0, n_bases = 0;
  DevArray<uint64_t> desc;   // per piece: slot | position << 32 | read length << 48
  DevArray<uint8_t> flag;    // per piece: bit 0 forward strand, bit 1 'N' first
  DevArray<uint64_t> len;    // per piece: bases it writes (scan input)
  DevArray<uint64_t> pos;    // per piece (+ 1): where it writes
  DevArray<uint64_t> pbase;  // per edge (+ 1): its first piece
  DevArray<uint64_t> start;  // per edge (+ 1): where its string starts
  DevArray<char> out;
  DevArray<uint8_t> tmp;     // the scan's temporary storage
  DevArray<unsigned long long> ctl;  // [0] = first invalid piece
  EventPair ev;
};

// read placements (mg_places.hip, mg_build_placements): one CSR of mg_place
// records over the reads, each read's forward-placement count, and what
// mg_edge_coverage reads again: the edges and, per list entry of every edge
// ("entry space", edge k at ebase[k]), its read, edge and distance.
// ready until new reads arrive (reset_derived)
struct PlaceStage {
  bool ready = false;
  uint64_t n = 0;                     // records
  std::vector<mg_contig_edge> edges;  // the edges of the last build (messages, chunking)
  std::vector<uint64_t> ebase;        // per edge (+ 1): its first entry
  DevArray<uint64_t> start;           // start[A] (n + 2)
  DevArray<mg_place> recs;
  DevArray<uint32_t> fwd;  // forward placements of read A (n + 2)
  DevArray<mg_contig_edge> d_edges;
  DevArray<uint64_t> d_ebase;
  DevArray<uint32_t> eread, eedge;
  DevArray<uint64_t> edist;
  // option "cov_budget" (tests): per-base counters one chunk of mg_edge_coverage holds (0 = 2^25)
  uint64_t cov_budget = 0;
  EventPair ev;
};

// mate-pair paths (mg_paths.hip, mg_mate_paths): per mate entry its status,
// work units and path, the paths of all entries end to end ("path space",
// entry t at pstart[t]) with one flag per position, and the supported pairs.
// ready until the next mg_mate_paths
struct PathStage {
  bool ready = false;
  uint64_t n_entries = 0, n_path = 0, n_pairs = 0, n_deferred = 0;
  DevArray<uint8_t> status;   // per entry: MG_PATH_*
  DevArray<uint32_t> visits;  // per entry: work units spent
  DevArray<uint64_t> plen;    // per entry (+ 1): edges in its path (scan input)
  DevArray<uint64_t> pstart;  // per entry (+ 1): where its path starts
  DevArray<uint32_t> path;    // path space: edge indices
  DevArray<uint8_t> flags;    // path space: 1 = (path[p], path[p + 1]) is supported
  DevArray<mg_pair_support> pairs;
  // options "path_batch" (mate entries per explore launch, 0 = 2^18) and
  // "path_budget" (work units per mate entry, 0 = 2^16)
  uint64_t batch = 0, budget = 0;
  float explore_ms = 0.f, aggregate_ms = 0.f;
  EventPair ev;
};

// scaffolder support (mg_scaffold.hip, mg_scaffold_pairs): per mate entry its
// status, and the supported edge pairs with support and summed distance.
// ready until the next mg_scaffold_pairs
struct ScaffoldStage {
  bool ready = false;
  uint64_t n_entries = 0, n_counted = 0, n_pairs = 0;
  DevArray<uint8_t> status;  // per entry: MG_SCAF_*
  DevArray<mg_scaffold_pair> pairs;
  float score_ms = 0.f, aggregate_ms = 0.f;
  EventPair ev;
};

// one (node, port) state of the chain ranking (mg_chains.hip): "leaving node v
// through port p".  Unknown end: link = the next state.  Known end: link = the
// CSR index of the end half-edge, end = its node.  out / in = sums of the
// offsets of the edges walked and of their twins.
struct ChainState {
  uint32_t link;
  uint32_t hops;  // edges walked; bit 31 = the end is known; 0 = no state (the node is not interior)
  uint32_t end;
  uint32_t pad;
  uint64_t out, in;
};

// safe chains of a replayed graph (mg_chains.hip, mg_build_chains): the table
// and the SoA read lists of the last build; ready until the next build
struct ChainStage {
  bool ready = false;
  uint64_t n_chains = 0, n_list = 0;
  uint32_t rounds = 0;  // option "chain_rounds" (tests): cap on the jump rounds (0 = auto)
  DevArray<uint64_t> start;        // the caller's CSR starts (n + 2)
  DevArray<mg_chain_edge> edges;   // and half-edges
  DevArray<uint8_t> interior;      // per node (n + 2)
  DevArray<ChainState> state[2];   // 2 (n + 1) states, double-buffered over the rounds
  DevArray<uint32_t> far_end;      // per half-edge of a non-interior node: its far end, 0 = unknown
  DevArray<uint32_t> head;         // per half-edge: 1 = heads a safe chain; then its chain index (scan)
  DevArray<uint64_t> span;         // per half-edge: 2 n of the safe chain it heads; then its `first` (scan)
  DevArray<uint8_t> tmp;           // the scans' temporary storage
  DevArray<unsigned long long> ctl;  // control words (see mg_chains.hip)
  DevArray<mg_chain> table;
  DevArray<uint32_t> reads;
  DevArray<uint16_t> offs;
  DevArray<uint8_t> ors;
  EventPair ev;
};

struct mg_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  // reads
  uint64_t n = 0;
  uint32_t maxw = 0;
  uint32_t stride = 0;  // words per device slot (slot_words(maxw))
  uint32_t minlen = 0, maxlen = 0;
  DevArray<uint64_t> d_words;
  DevArray<uint16_t> d_len;
  // device layout (option "layout"): slots clustered by each
  // read's canonical global minimizer, so overlapping reads sit near each
  // other; d_id[slot] = reference ID - 1, d_phys[ID - 1] = slot (both nullptr:
  // slots in ID order).  Everything on the device works in slots; rows,
  // superReadIDs, lookups and downloads leave in reference IDs.  With a
  // source-read range set (mg_set_shard), the reads of the range take the
  // slots [read_lo, read_hi) (clustered among themselves), so a shard's slot
  // range holds exactly its reference IDs.
  bool layout = true;
  int layout_hash = 0;  // option "layout_hash": the layout's 16-mer hash (0 fmix32, 1 24-bit multiply-adds)
  uint32_t* d_id = nullptr;    // alias: one of id_store[], or nullptr
  uint32_t* d_phys = nullptr;  // alias: one of phys_store[], or nullptr
  DevArray<uint32_t> id_store[2];  // a re-layout builds the maps in the unused pair
  DevArray<uint32_t> phys_store[2];
  uint64_t layout_lo = 0, layout_hi = 0;  // the source-read range the current layout groups (0, 0: none)
  // layout scratch, kept between uploads so a re-upload allocates nothing:
  // sort keys / values (double buffers), the sort's temporary storage, and the
  // second slot array the gather writes (the two slot arrays swap)
  DevArray<uint64_t> d_lay_k[2];
  DevArray<uint32_t> d_lay_v[2];
  DevArray<uint8_t> d_lay_tmp;
  DevArray<uint64_t> d_words_alt;
  DevArray<uint16_t> d_len_alt;
  DevArray<uint32_t> d_tmp32;  // ID-order staging of per-read outputs
  // index
  uint32_t l = 0, h = 0, m = 0, w = 0;
  uint32_t nb_log2 = 0, nb_log2_opt = 0;
  bool index_ready = false;
  DevArray<uint64_t> d_cells;  // cells of kCell entries (this rank's bucket range)
  // option "cells_double" (default off): a second table, cleared on the side
  // stream for the next build (cells_alt_clean entries, done at ev[13]).
  // Measured: the clear beside the scan slowed the scan more than the clear
  // costs (C3 scan 2.22 -> 2.72 ms, step 6.91 -> 7.26; profiles/r06s_ab_cells_double.txt)
  DevArray<uint64_t> d_cells_alt;
  size_t cells_alt_clean = 0;
  bool cells_double = false;
  // the index holds the o = 1 keys (suffix keys of the forward strand) only
  // when a probe reads them: discovery never does (an o = 1 hit is the twin of
  // the partner's o = 0 hit) and containment only without the
  // prefix-containment kernel; getListOfReads then takes a lookup table of all
  // four keys, built on the first lookup after a build (d_lkcells)
  bool index_o1 = true;
  // the o = 3 keys likewise (fused mixed lengths with k_prefix_contain and the
  // live discovery index: containment drops o = 1/3 hits, discovery walks the
  // live table, which has them)
  bool index_o3 = true;
  DevArray<uint64_t> d_lkcells;
  bool lookup_ready = false;
  uint64_t cell_lo = 0, cell_n = 0;  // local bucket range [cell_lo, cell_lo + cell_n)
  // containment
  DevArray<unsigned long long> d_superkey;
  unsigned long long* superkey = nullptr;  // alias: the containment key array in use (d_superkey or caller-owned)
  DevArray<uint32_t> d_super;
  // contained slots as a bitmap (bit a of word a / 32 = d_super[a] != 0,
  // k_super_finalize): the discovery probe drops contained partners before
  // they take a verification (:548), from a 1/32-size array that stays in cache
  DevArray<uint32_t> d_cbits;
  // contained reads counted by k_super_finalize (64 counters, one per 64-B line)
  DevArray<unsigned int> d_ccnt;
  uint64_t n_contained = 0;
  // discovery index (option "live_index", unsharded fused path, mixed lengths):
  // after markContainedReads the discovery probe only needs the keys of
  // uncontained reads (:548 drops contained partners), so it probes a table of
  // those alone, sized for them (C5: a quarter of the entries and chains)
  bool live_index = true;
  bool live_runs = true;          // option live_runs: k_live_runs compacts the runs of contained sources before discovery
  // option live_overlap: k_live_runs (HBM streaming) on a side stream beside the
  // live index build (memory-side atomics), both before the discovery probe
  bool live_overlap = true;
  hipStream_t side = nullptr;
  bool live_ready = false;
  DevArray<uint64_t> d_lcells;
  uint32_t lnb_log2 = 0;
  uint64_t live_cells = 0;  // cells of the discovery index (mg_counters::live_cells)
  DevArray<unsigned int> d_any;  // k_super_finalize's "some read is contained" word
  DevArray<unsigned long long> d_digest;  // mg_rows_digest / mg_super_digest accumulators (4 u64)
  bool contained_done = false, super_any = false;
  // rows: d_rows counts rows (its capacity divides into one region per probe
  // wavefront); the kernels address them as three 32-bit words each (row_words)
  DevArray<mg_edge> d_rows;
  uint64_t rows_cap_opt = 0;
  DevArray<unsigned long long> d_seg;  // rows per region
  uint64_t n_rows = 0;
  std::vector<unsigned long long> seg_host;
  bool stats = false;
  DevArray<unsigned long long> d_stats;  // kSegs * 4 + 1 work counters (zero_stats)
  mg_counters counters{};
  // host-side counters of the current step (mg_counters, kept without option "stats"):
  // discovery reruns after a row overflow (settle_rows), rescans after a run-region
  // overflow (settle_runs), the virtual split of the last discovery probe launch
  uint64_t row_reruns = 0, run_reruns = 0, probe_vsplit = 1;
  // shard
  uint32_t rank = 0, nranks = 1;
  uint64_t read_lo = 0, read_hi = 0;  // source-read range: reference IDs - 1 = slots [read_lo, read_hi)
  uint32_t max_blocks = 8192;  // cap on the persistent discovery grid (blocks of 4 wavefronts)
  int phase_limit = 99;        // diagnostics (option "phase_limit")
  int contain_phase_limit = 99;  // diagnostics (option "contain_phase_limit")
  bool halving_low = false;    // option "halving": o=2/3 pair side rule
  int n_cu = 256;              // compute units of the device
  uint64_t nreg = 0;           // row regions of the last discovery launch (one per probe wavefront)
  uint64_t nrun_reg = 0;       // run regions (one per scan wavefront)
  DevArray<ulonglong2> d_runs;  // run records, one region per wavefront
  uint64_t run_cap = 0, run_cap_need = 0, run_cap_opt = 0;  // run_cap_opt: option "run_cap" (tests)
  DevArray<unsigned long long> d_run_cnt;
  std::vector<unsigned long long> run_cnt_host;
  DevArray<uint32_t> d_compact;  // mg_copy_rows: the row regions gathered into one array
  // exchange mode (one process per GPU): mg_xchg_begin's scan
  // leaves key records (d_kb / d_ke) and the run regions of this rank's
  // sources; packable = bit mask of what mg_xchg_pack can route now
  bool xchg = false;                     // the context's current build is an exchange-mode build
  // one rank (P = 1, no source range): mg_xchg_begin runs the fused build and
  // the exchange calls delegate to the fused probes (option "xchg_fused1")
  bool xchg_fused = false;
  bool xchg_fused1 = true;
  bool index_keys = true;  // option "index_keys": LaunchIndex takes k_index_keys (0: k_index_build)
  // mg_xchg_prefix_marks ran this step's offset-0 containments; xmarks = the
  // caller's marks (all-reduced before mg_xchg_probe(1) folds them in)
  uint64_t scan_runs = 0;  // run records of the last window scan (settle_runs)
  bool xmarks_done = false;
  uint8_t* xmarks = nullptr;  // alias: the caller's marks array (mg_xchg_prefix_marks)
  uint64_t xchg_lo = 0, xchg_hi = 0;     // its source reads
  DevArray<unsigned long long> d_blk;    // routing: per-(block, rank) counts / offsets
  // exchange mode, equal lengths: the register scan counts its runs per
  // destination rank (one row of nranks per run region), so routing the runs
  // skips k_part's count pass (runs_counted: valid for the last scan)
  DevArray<unsigned long long> d_rcnt;
  // k_xchg_keys' per-(flat region, rank) counts of the key records (keys first):
  // mg_xchg_pack(MG_KEYS) skips k_part's count pass while keys_counted
  // the keys-first receiver scan's run regions hold 8-B metas, d_rdst their owner ranks
  DevArray<uint8_t> d_rdst;
  bool runs_meta8 = false;
  uint64_t super_zero_n = 0;  // leading d_super entries known to be 0 (skips the equal-length clear)
  DevArray<unsigned long long> d_kblk;
  bool keys_counted = false;
  bool runs_counted = false;
  // mg_build_index leaves its timings (index_ms, shared_scan_ms) to be read once
  // its events have completed (settle_index_times): no host round trip between
  // the build and the probe
  bool index_times_pending = false;
  // exchange-mode discovery probe: rows per (probe wavefront, destination
  // rank), so routing the rows skips k_part's count pass (rows_counted)
  DevArray<unsigned long long> d_dcnt;
  bool rows_counted = false;
  // option "xchg_route_rows" (default 1): the exchange-mode discovery probe
  // counts its rows per src owner for mg_xchg_pack(MG_ROWS); a host that keeps
  // the rows where they were verified sets 0 and the probe counts nothing
  bool xchg_route_rows = true;
  // option "xchg_scan_lds": the exchange scan of equal lengths takes k_scan<KEYREC>
  // (LDS sliding minimum, all four keys in one pass) instead of k_scan_reg + k_rc_keys
  bool xchg_scan_lds = true;
  uint32_t xchg_region = 512;  // option "xchg_region": records per probe region of the received runs (0: 1,024)
  uint32_t xchg_split_max = 4;  // option "xchg_split_max": mg_xchg_probe_own splits the probe at up to this many ranks
  int packable = 0;                      // 1 << MG_KEYS | 1 << MG_RUNS | 1 << MG_ROWS
  DevArray<unsigned long long> d_flat_cnt;  // per-region counts of the received runs (probe input)
  DevArray<unsigned long long> d_slot_cnt;  // per-region counts of a slot-layout buffer (digest)
  DevArray<uint32_t> d_kb;  // key records: bucket / index entry, key o of read a at o * n + a
  DevArray<uint64_t> d_ke;
  // timing
  hipEvent_t ev[16] = {};  // [14], [15]: apply_layout
  // unsharded contexts build the index inside the window scan (k_scan<INDEX>);
  // its runs then serve the containment and the discovery probes
  int scan_state = 0;        // 0 none, 1 launched (not settled), 2 settled
  bool runs_live = false;    // the run regions hold only runs of uncontained sources (k_live_runs)
  bool run_masks = true;       // option "run_masks": k_scan records runs as per-lane bit sets (0: staged in LDS)
  bool probe_share = true;     // option "probe_share": a discovery-probe block's 4 wavefronts share its regions
  bool probe_compact = true;   // option "probe_compact": sparse run batches compacted in the probe (C5 probe 30.4 -> 26.8 ms)
  // prefix containments (k_prefix_contain): each read's o = 0 key (bucket,
  // fingerprint, q) written by k_scan<INDEX> for mixed-length sets; when ready
  // the containment probe skips suffix-key hits (containment)
  DevArray<uint64_t> d_key0;
  // offset-0 containments through the containment probe (option prefix_probe,
  // default): the fused scan writes each read's window-0 run (its o = 0 key's
  // minimizer, window range [0, 0]) here, one 16-B record per slot, and the
  // probe takes them first in fixed regions of d_p0cnt records
  bool prefix_probe = true;
  DevArray<ulonglong2> d_p0runs;
  DevArray<unsigned long long> d_p0cnt;
  // exchange mode: the received runs ordered by local bucket (sort_xruns), the
  // input of both probes; xruns_ready until the next mg_xchg_begin
  DevArray<uint32_t> d_xk[2];
  DevArray<ulonglong2> d_xv[2];
  DevArray<uint8_t> d_xsort_tmp;  // the sort / scan / select scratch of the exchange build
  int xv_sel = 0;
  uint64_t xruns_n = 0;
  bool own_probed = false;
  // exchange mode, keys first (option xchg_keys_first, equal lengths, P > 1):
  // mg_xchg_begin computes the key records only (k_xchg_keys); the window scan
  // runs in mg_xchg_insert_keys and CAS-inserts the received key records
  // (rk_*: slot layout) as it goes (k_scan<RECV>, rk_on during that launch)
  bool xchg_keys_first = true;
  bool keys_first = false;  // the current exchange build is a keys-first one
  bool rk_on = false;
  const uint64_t* rk_keys = nullptr;  // aliases: the caller's receive buffer and its counts, during that launch
  const unsigned long long* rk_cnt = nullptr;
  uint64_t rk_slot = 0, rk_total = 0;
  int xruns_part = 0;       // the probe regions prepared: 0 all, 1 own stream, 2 the peers' (split probe)
  uint64_t xruns_K = 0;     // probe regions per peer slot and round  // mg_xchg_probe_own probed this rank's own stream; mg_xchg_probe(0) appends the peers
  // the received runs expanded to 16-B probe records (k_xruns_expand), slot layout
  DevArray<ulonglong2> d_xexp;
  bool xruns_ready = false;
  ulonglong2* xruns_base = nullptr;  // alias: the probes' run regions: d_xv (sorted), d_xexp, or (one rank) d_runs
  unsigned long long* xruns_cnt = nullptr;  // alias: their per-region counts (d_flat_cnt, or d_run_cnt)
  uint64_t xruns_reg = 0, xruns_nreg = 0;
  // exchange mode: the key records this rank received, dense and sorted by
  // home cell (mg_xchg_insert_keys: key = local home cell, ent = index
  // entry); they build the cells, the o = 0 ones drive the prefix containments
  // (k_prefix_contain_keys, xchg_prefix) and the live ones the discovery index
  DevArray<uint32_t> d_xkk[2];
  DevArray<uint64_t> d_xke[2];
  uint64_t xkeys_n = 0;
  uint32_t xkey_cls = 0;       // 1: key = home cell << 1 | (o == 3) (the full table leaves out o = 3)
  uint32_t xkey_fs = 0;        // low fingerprint bits below the cell / class bits (chain_par)
  bool xkey_par = false;       // the received records' cells are built by the parallel placement
  // aliases: the sorted records (one of d_xkk[] / d_kb, d_xke[] / d_ke) and the other buffer pair
  uint32_t* xkey_k = nullptr;
  uint64_t* xkey_e = nullptr;
  uint32_t* xkey_k_alt = nullptr;
  uint64_t* xkey_e_alt = nullptr;
  // the live records' in-order compaction (build_live_index_xchg)
  DevArray<uint8_t> d_xflag;
  DevArray<unsigned long long> d_nlive;  // their count (one word)
  // the exchange mode's discovery index coarsens the rank's cells (cell =
  // local home cell >> live_shift) instead of rebuilding entries
  bool live_coarse = false;
  uint32_t live_shift = 0;
  bool xchg_sort_runs = false;  // option "xchg_sort_runs": received runs ordered by bucket before the probes
  bool xchg_windows = true;    // option "xchg_windows": the exchange scan of mixed lengths in length-ranked windows
  bool layout_scratch = true;  // option "layout_scratch" = 0: free the layout's double buffers after each layout
  // option "chain_par": build_cells places a cell's overflow records in
  // parallel by their index in their fingerprint's run (k_cells_place; else one
  // thread per overflowing cell, k_cells_chain); d_rhead / d_rstart: run heads
  // and their max-scan
  bool chain_par = true;
  bool check_cells = false;  // diagnostics (option "check_cells"): verify each sorted cell build
  int xchg_fs = -1;  // diagnostics (option "xchg_fs"): fingerprint bits in the exchange sort key (-1: fp_sort_bits)
  DevArray<uint32_t> d_rhead;
  DevArray<uint32_t> d_rstart;
  bool xchg_prefix = false;
  bool key0_ready = false;
  bool prefix_contain = true;  // option "prefix_contain"
  bool contain_jcut = true;    // option "contain_jcut": containment probe drops runs with jlo > n1 - minlen (C5: 60 -> 47 ms)
  bool contain_skip = true;    // option "contain_skip": skip runs of sources already known contained (C5: 42.8 -> 29.7 ms)
  uint32_t probe_split_max = 8;  // option "probe_split_max": virtual run regions per region for the probe's balance (1 = off)
  bool contain_prune = true;   // option "contain_prune": skip candidates that cannot raise the superkey (C5: 388M -> 110M compares)
  float shared_scan_ms = 0.f;  // k_scan<INDEX> kernel time of the last mg_build_index
  mg_timings t{};
  // Dataset ingest on the device (mg_ingest_*): frequency of each unique read
  DevArray<uint32_t> d_freq;
  uint64_t n_good = 0;  // reads that passed testRead (Dataset::getNumberOfReads)
  // option "alloc_cap" (tests): a device allocation above this many bytes fails
  // as out of memory (0 = no cap), so the error path is exercised on purpose
  uint64_t alloc_cap = 0;
  // mg_find_overlaps completed for the current index (the discovery lists need its rows)
  bool rows_found = false;
  // d_freq belongs to the resident reads (set by the device ingest, cleared by an upload)
  bool freq_ready = false;
  // the derived stages, one struct each (above)
  DiscStage disc;
  CompStage comp;
  MateStage mates;
  ContigStage contigs;
  PlaceStage places;
  PathStage paths;
  ScaffoldStage scaffold;
  ChainStage chains;
};

#define MG_TRY(expr)                                                                  \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess) {                                                           \
      ctx->err = std::string(#expr) + " failed: " + hipGetErrorString(e_);            \
      return -1;                                                                      \
    }                                                                                 \
  } while (0)

inline int set_err(mg_ctx* ctx, const std::string& s) {
  ctx->err = s;
  return -1;
}

// Every device buffer of a context is allocated here.  A failure -- or, with
// option "alloc_cap" (tests), a request above that many bytes, reported as
// out of memory -- leaves the buffer's name, the bytes asked for and the HIP
// error in ctx->err, so no later message has to guess the cause.
inline hipError_t ctx_malloc(mg_ctx* ctx, void** p, size_t bytes, const char* what) {
  *p = nullptr;
  const hipError_t e =
      (ctx->alloc_cap && bytes > ctx->alloc_cap) ? hipErrorOutOfMemory : hipMalloc(p, std::max<size_t>(bytes, 1));
  if (e != hipSuccess) {
    *p = nullptr;
    ctx->err = std::string("device allocation of ") + what + " (" + std::to_string(bytes) + " B) failed: " +
               hipGetErrorString(e) + (ctx->alloc_cap && bytes > ctx->alloc_cap ? " (option alloc_cap)" : "");
  }
  return e;
}

// (a failure leaves its cause in ctx->err: ctx_malloc's message, or the failed free of the old buffer)
template <typename T>
inline hipError_t DevArray<T>::ensure(mg_ctx* ctx, size_t count, const char* what) {
  if (cap >= count && p) return hipSuccess;
  if (p) {
    const hipError_t e = hipFree(p);
    if (e != hipSuccess) {
      ctx->err = std::string("freeing ") + what + " to grow it failed: " + hipGetErrorString(e);
      return e;
    }
    p = nullptr;
    cap = 0;
  }
  const size_t c = std::max<size_t>(count, 1);
  const hipError_t e = ctx_malloc(ctx, reinterpret_cast<void**>(&p), c * sizeof(T), what);
  if (e == hipSuccess) cap = c;
  return e;
}
template <typename T>
inline hipError_t Scratch<T>::alloc(mg_ctx* ctx, size_t count, const char* what) {
  return ctx_malloc(ctx, reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T), what);
}
// DevArray::ensure() under the name the buffer's messages carry (the d_* names
// callers know); returns -1 from the caller with ctx->err set
#define MG_GROW(arr, count, what)                                         \
  do {                                                                    \
    if ((arr).ensure(ctx, (count), (what)) != hipSuccess) return -1;      \
  } while (0)
// MG_GROW of a core field of the context under the field's own name
#define MG_ENSURE(field, count) MG_GROW(ctx->field, (count), #field)
// Scratch::alloc(); returns -1 from the caller with ctx->err set
#define MG_SCRATCH(buf, count, what)                                      \
  do {                                                                    \
    if ((buf).alloc(ctx, (count), (what)) != hipSuccess) return -1;       \
  } while (0)
// the context's rows as the kernels address them: three 32-bit words per row
static_assert(sizeof(mg_edge) == 3 * sizeof(uint32_t), "a row is three 32-bit words");
inline uint32_t* row_words(const mg_ctx* ctx) { return reinterpret_cast<uint32_t*>(ctx->d_rows.p); }
// a launch wrapper that failed: keep the cause a callee left in ctx->err
inline int launch_fail(mg_ctx* ctx, const std::string& what) {
  ctx->err = ctx->err.empty() ? what : what + ": " + ctx->err;
  return -1;
}

// word counts the kernels are instantiated for (reads up to 1024 bp)
inline uint32_t supported_maxw(uint32_t need) {
  static const uint32_t kW[] = {1, 2, 3, 4, 5, 6, 8, 12, 16, 32};
  for (uint32_t w : kW)
    if (w >= need) return w;
  return 0;
}

// Reads longer than 1024 bp (up to 65,535, Read.h:62) take the long-read
// kernels (mg_kernels.hip: k_index_long, k_probe_long): maxw is then the exact
// word count and a slot holds it plus at least one zero pad word.
inline bool long_mode(const mg_ctx* ctx) { return ctx->maxw > 32; }
inline uint32_t long_stride(uint32_t maxw) { return (maxw + 1 + 7) & ~7u; }
// slot width for reads of `need` words: the instantiated widths up to 32,
// else the long-read width (maxw = need); 0 = longer than 65,535 bp
inline uint32_t slot_maxw(uint32_t need) {
  if (need <= 32) return supported_maxw(need < 1 ? 1 : need);
  return need <= 2048 ? need : 0;
}
inline uint32_t slot_stride(uint32_t maxw) { return maxw > 32 ? long_stride(maxw) : (uint32_t)slot_words((int)maxw); }

// the device layout of freshly uploaded reads (mg_kernels.hip): clusters the
// slots by canonical global minimizer and fills d_id / d_phys (option "layout"
// = 0: ID order); records t.layout_ms
int apply_layout(mg_ctx* ctx);

// new reads invalidate everything derived from them
inline void reset_derived(mg_ctx* ctx) {
  ctx->scan_state = 0;
  ctx->index_ready = false;
  ctx->lookup_ready = false;
  ctx->contained_done = false;
  ctx->super_any = false;
  ctx->live_ready = false;
  ctx->live_coarse = false;
  ctx->n_contained = 0;
  ctx->n_rows = 0;
  ctx->rows_found = false;
  ctx->disc.ready = false;
  ctx->comp.ready = false;
  ctx->mates.ready = false;
  ctx->contigs.ready = false;
  ctx->places.ready = false;
}

// mg_dataset.hip: the ingest's per-record stage alone (k_ingest / k_ingest_long
// over device-resident ASCII records): testRead, the canonical strand packed
// into cw words per record, and fwd[i] = 1 when record i is its own canonical
// string (forward strand chosen, or both strands equal).  cw =
// ingest_record_words(longest record that can pass the length bounds).
uint32_t ingest_record_words(uint64_t longest);
int ingest_records(mg_ctx* ctx, const char* d_ascii, const uint64_t* d_off, uint64_t n, uint32_t min_overlap,
                   uint32_t cw, uint64_t* canon, uint16_t* len, uint8_t* valid, uint8_t* fwd);
// D(A) and what is derived from it need the whole multiset in one context
inline int whole_multiset(mg_ctx* ctx, const char* who) {
  if (ctx->nranks > 1 || ctx->read_lo || ctx->read_hi)
    return set_err(ctx, std::string(who) + ": the context is sharded (mg_set_shard): its rows are not the whole "
                                           "multiset; multi-rank D(A) is not supported");
  if (ctx->xchg || ctx->xchg_fused)
    return set_err(ctx, std::string(who) + ": exchange-mode build: its rows are not the whole multiset; multi-rank "
                                           "D(A) is not supported");
  return 0;
}

#endif  // MG_CTX_HPP_
