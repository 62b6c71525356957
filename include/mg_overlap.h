/* mg_overlap.h — the drop-in C-ABI for the read-overlap hot path on MI355X.
 *
 * The reference has no FFI: its boundary is the C++ class API that main.cpp
 * calls (main.cpp:45-47).  Each entry point below names the reference
 * interface it replaces (paths relative to /root/reference/MetaGenomics).
 * The host-side C++ mirror of those classes (metagenomics_amd/csrc/host/)
 * is implemented on top of these functions; INTEGRATION.md shows how a
 * maintainer wires them in.
 *
 * Conventions: plain pointers and sizes, int status (0 = ok,
 * <0 = error; never exit() across the ABI — the reference's MYEXIT calls
 * exit(0), Common.h:47), mg_last_error() for the message, all device buffers
 * owned by the context, one host thread per context, device chosen at create.
 *
 * Read model: reads are the Dataset's unique canonical forward strings in ID
 * order (ID = index + 1, Dataset.cpp:335-339), 2-bit packed A0 C1 G2 T3,
 * most-significant base first, `words_per_read` u64 words per read (bases
 * past the read's length are zero).
 */
#ifndef MG_OVERLAP_H_
#define MG_OVERLAP_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mg_ctx mg_ctx;

/* One directed row of the overlap graph, i.e. one Edge object
 * (Edge.h:18-29): source read ID, destination read ID, overlapOrientation
 * 0..3 (0 = u<-----<v, 1 = u<----->v, 2 = u>-----<v, 3 = u>----->v) and
 * overlapOffset (start of v relative to u).  12 bytes. */
typedef struct mg_edge {
  uint32_t src;
  uint32_t dst;
  uint16_t offset;
  uint8_t orient;
  uint8_t flags; /* 0 */
} mg_edge;

/* Device-side phase timings of the last call (HIP events on the context's
 * stream), milliseconds. */
typedef struct mg_timings {
  float pack_ms;        /* 2-bit encoding of ASCII reads            */
  float index_ms;       /* HashTable::insertDataset equivalent (with the window scan when fused) */
  float contained_ms;   /* markContainedReads equivalent (0 if skipped) */
  float overlap_ms;     /* discovery = scan + probe (insertAllEdgesOfRead) */
  float total_ms;       /* device wall of index + contained + overlap */
  float scan_ms;        /* minimizer-run scan kernel (unsharded: the index-building scan, part of index_ms) */
  float probe_ms;       /* probe kernel (fused path: probe + verify) */
  float verify_ms;      /* 0 (the probe verifies inline)                */
  float upload_ms;      /* H2D copy of raw reads (mg_ingest_*)        */
  float ingest_ms;      /* device Dataset ingest (mg_ingest_*)        */
  float sort_ms;        /* always 0 (no run sort since the clustered layout; field kept for ABI) */
  float layout_ms;      /* device layout of the last upload / ingest (clustered slots, option "layout") */
} mg_timings;

/* Work counters of the last discovery launch (only with option "stats" = 1):
 * the units the roofline's algorithmic byte count is built from. */
typedef struct mg_counters {
  uint64_t sources;   /* source reads handled                         */
  uint64_t runs;      /* minimizer runs whose bucket was probed       */
  uint64_t entries;   /* bucket entries scanned                       */
  uint64_t verified;  /* partner reads fetched and compared           */
  uint64_t rows;      /* directed rows emitted                        */
  uint64_t live_cells; /* cells of the discovery index of uncontained reads the probe
                          walked (option live_index); 0 = the full table */
  /* the last containment pass (markContainedReads), same units */
  uint64_t c_runs, c_entries, c_verified, c_contained;
  /* run records the last window scan wrote (every source read's windows; kept
   * without option "stats") */
  uint64_t scan_runs;
  /* host-side values of the last step (mg_build_index / mg_xchg_begin .. the
   * discovery probe), kept without option "stats".  A step starts at the build:
   * a second mg_find_overlaps over the same index starts row_reruns again but
   * keeps the build's run_reruns (containment may have rescanned before it);
   * probe_vsplit is that of its own probe launch */
  uint64_t row_reruns;   /* reruns of the discovery probe after a row-capacity overflow */
  uint64_t run_reruns;   /* rescans after a run-region overflow */
  uint64_t probe_vsplit; /* virtual region split of the last discovery probe launch (1 = none) */
} mg_counters;

/* --- context ------------------------------------------------------------ */
/* Creates a context on HIP device `device`.  Replaces nothing in the
 * reference (it is single-process); owns every device buffer below. */
int mg_create(mg_ctx** ctx, int device);
void mg_destroy(mg_ctx* ctx);
const char* mg_last_error(const mg_ctx* ctx);
/* Number of HIP devices visible (0 when no GPU). */
int mg_device_count(void);

/* --- reads (Dataset / Read) ---------------------------------------------- */
/* Upload the Dataset's unique reads, already 2-bit packed (the host mirror of
 * Dataset packs while it canonicalises/sorts, Dataset.cpp:158-202,316-345).
 * lens[i] = Read::getReadLength() of read ID i+1 (Read.h:62).  Any length up to
 * 65,535 (UINT16): reads up to 1,024 bp take the register-resident kernels,
 * longer ones the long-read kernels (the exchange mode refuses
 * them).  The same holds for every upload and ingest below. */
int mg_upload_reads_packed(mg_ctx* ctx, const uint64_t* words, const uint16_t* lens, uint64_t n_reads,
                           uint32_t words_per_read);
/* Upload reads as ASCII (upper-case ACGT only, already filtered by
 * Dataset::testRead, Dataset.cpp:398-413): concat holds read i at
 * [offsets[i], offsets[i+1]).  The 2-bit encoding runs on the GPU
 * (replaces Read::setRead's string storage, Read.cpp:75-82). */
int mg_upload_reads_ascii(mg_ctx* ctx, const char* concat, const uint64_t* offsets, uint64_t n_reads);
uint64_t mg_num_reads(const mg_ctx* ctx);
/* Dataset ingest ON THE DEVICE: raw reads in, the unique
 * canonical reads in ID order out, resident in the context exactly as
 * mg_upload_reads_packed would leave them.  Restates Dataset::Dataset's
 * per-read path (Dataset.cpp:39-65): upper-case (:158-159), testRead (length >
 * min_overlap, only ACGT, no base >= floor(0.8 len); :160, :398-413),
 * canonical strand min(s, revcomp(s)) (:163-167), sortReads in std::string
 * order (:197-202) and removeDupicateReads (frequency, IDs 1..N; :316-345).
 * ASCII: read i = concat[offsets[i], offsets[i+1]) (FASTA/FASTQ record text as
 * readDataset extracts it, Dataset.cpp:123-182); codes: codes[i*stride + k]
 * in {0:A,1:C,2:G,3:T, >3: not ACGT}, k < lens[i].  *n_unique = unique reads. */
int mg_ingest_ascii(mg_ctx* ctx, const char* concat, const uint64_t* offsets, uint64_t n_raw, uint32_t min_overlap,
                    uint64_t* n_unique);
int mg_ingest_codes(mg_ctx* ctx, const uint8_t* codes, uint64_t n_raw, uint64_t stride, const uint16_t* lens,
                    uint32_t min_overlap, uint64_t* n_unique);
/* Dataset::getNumberOfReads (reads that passed testRead) and
 * getNumberOfUniqueReads of the last device ingest. */
int mg_dataset_counts(const mg_ctx* ctx, uint64_t* n_good, uint64_t* n_unique);
/* Read::getFrequency of every unique read (n_reads entries, ID order). */
int mg_download_frequency(mg_ctx* ctx, uint32_t* freq);
/* Copy back the packed reads (words_per_read words each) for inspection. */
int mg_download_reads_packed(mg_ctx* ctx, uint64_t* words, uint16_t* lens, uint32_t* words_per_read);
/* Device slot of every read: slot_of_id[ID - 1] (the device stores the reads
 * clustered for locality, option "layout"; identity when it is off).  Only
 * diagnostics need it: every result leaves the device in reference IDs. */
int mg_read_slots(mg_ctx* ctx, uint32_t* slot_of_id);

/* --- index (HashTable) ---------------------------------------------------- */
/* HashTable::insertDataset(Dataset*, minOverlapLength) (HashTable.h:30,
 * HashTable.cpp:50-80): keys are the h = l-1 prefixes/suffixes of both
 * strands of every read (hashRead, HashTable.cpp:88-104).  The device index
 * files each key under its (seed_k)-mer minimizer (seed_k <= min(32, h);
 * 0 = min(31, h)); exact-key equality is re-established by verification, so
 * results equal the reference's exact-key buckets. */
int mg_build_index(mg_ctx* ctx, uint32_t min_overlap, uint32_t seed_k);
/* HashTable::getListOfReads(string) (HashTable.cpp:202-221): the exact-key
 * bucket of `key` (length h, ACGT), entries id | o << 62 in the reference's
 * list order (ID ascending, then o).  *n_out = list length (may exceed cap). */
int mg_lookup_key(mg_ctx* ctx, const char* key, uint32_t key_len, uint64_t* out, uint64_t cap,
                  uint64_t* n_out);

/* --- overlap discovery (OverlapGraph) ------------------------------------- */
/* markContainedReads (OverlapGraph.cpp:225-290).  Runs only when read lengths
 * differ (:228-233), as the reference does.  super_out (optional, n_reads+1
 * entries): superReadID per ID, 0 = not contained. */
int mg_mark_contained(mg_ctx* ctx, uint32_t* super_out);
/* The edge-discovery part of buildOverlapGraphFromHashTable
 * (OverlapGraph.cpp:144-204 via insertAllEdgesOfRead :529-565, checkOverlap
 * :354-383, insertEdge :407-419): produces the full directed multiset
 * (every Edge and its twin) on the device.  Calls mg_mark_contained first if
 * it has not run for the current index.  *n_rows = directed rows
 * (= 2 x insertEdge(Read*,...) calls). */
int mg_find_overlaps(mg_ctx* ctx, uint64_t* n_rows);
/* Copy the rows to the host (any order; the multiset is what the reference
 * defines).  cap in rows; returns rows copied via *n_copied. */
int mg_copy_rows(mg_ctx* ctx, mg_edge* out, uint64_t cap, uint64_t* n_copied);
/* Rows held by the context after the last mg_find_overlaps / mg_xchg_probe(0)
 * (the count mg_copy_rows copies and mg_rows_digest(rows = NULL) digests). */
uint64_t mg_num_rows(const mg_ctx* ctx);

/* --- per-read discovery lists D(A) ------------------------------------------
 * One discovery of read A as insertAllEdgesOfRead meets it (OverlapGraph.cpp:
 * 529-565): partner dst, the Edge's overlapOffset and overlapOrientation, and
 * the HashTable key o (orient 3 -> 0, 0 -> 1, 2 -> 2, 1 -> 3; :550-556).  The
 * window is j = offset for o = 0, 2 and j = len(A) - (l - 1) - offset for
 * o = 1, 3.  8 bytes. */
typedef struct mg_disc {
  uint32_t dst;
  uint16_t offset;
  uint8_t orient;
  uint8_t o;
} mg_disc;
/* After mg_find_overlaps: group the context's rows into D(A) on the device:
 * the rows with src = A in insertAllEdgesOfRead's loop order (window j, then
 * partner ID, then key o, ascending; a total order), a self row (dst = A,
 * twice in the multiset) once.  *n_disc = total list length; *device_ms
 * (optional) = HIP-event time of the grouping on the context's stream.
 * Errors (< 0, message in mg_last_error): no completed mg_find_overlaps for
 * the current index; a context whose rows are not the whole multiset (nranks
 * > 1 or a source range set by mg_set_shard, or an exchange-mode build:
 * multi-rank D(A) is out of scope); and the codes of the host grouping:
 * -1 a src / dst outside 1..n_reads, -2 a window j outside [1, len - h), -3 a
 * self row without exactly one identical copy. */
int mg_build_discoveries(mg_ctx* ctx, uint64_t* n_disc, float* device_ms);
/* start: n_reads + 2 entries, D(A) = disc[start[A] .. start[A+1]), start[0] =
 * start[1] = 0; disc: cap records.  Either may be NULL.  Fails unless
 * mg_build_discoveries ran for the current rows: a later mg_build_index,
 * upload, ingest, mg_set_shard or mg_find_overlaps invalidates the lists. */
int mg_copy_discoveries(mg_ctx* ctx, uint64_t* start, mg_disc* disc, uint64_t cap, uint64_t* n_copied);

/* --- connected components of the discovery lists ----------------------------
 * Two reads are connected when a discovery record joins them.  The reference's
 * outer loop (OverlapGraph.cpp:144-204) explores one component at a time from
 * its smallest read ID, so components can be replayed independently
 * (mgh_graph_replay_comp, include/mg_host.h).  One component that holds at
 * least one record: */
typedef struct mg_comp { /* 16 bytes */
  uint32_t root;         /* smallest read ID of the component */
  uint32_t n_reads;      /* reads in it */
  uint32_t n_disc;       /* records of their lists D(A), self records once */
  uint32_t n_self;       /* of those, records with dst == A */
} mg_comp;
/* After mg_build_discoveries: label every read with the smallest read ID
 * connected to it (itself for a read with an empty list) and list the
 * components that hold records in strictly ascending root, all on the device
 * (union-find over the resident lists).  Labels and table are functions of the
 * lists alone: two calls give identical arrays.  *n_comp = table length;
 * *device_ms (optional) = HIP-event time on the context's stream.  Errors (< 0)
 * as mg_build_discoveries refuses (sharded / source range / exchange mode), and
 * unless mg_build_discoveries ran for the current rows. */
int mg_build_components(mg_ctx* ctx, uint64_t* n_comp, float* device_ms);
/* label: n_reads + 1 entries, label[0] = 0; comps: cap entries.  Either may be
 * NULL.  Fails unless mg_build_components ran for the current lists: whatever
 * invalidates the lists, and every mg_build_discoveries, invalidates it. */
int mg_copy_components(mg_ctx* ctx, uint32_t* label, mg_comp* comps, uint64_t cap, uint64_t* n_copied);

/* --- safe chains of the replayed graph ("Safe chains") ----------
 * The first contractCompositePaths pass (OverlapGraph.cpp:669-696) of a freshly
 * replayed graph (every edge simple, no flow) is order-free on most of the
 * graph.  Input: the graph as a CSR in u order, each list in list order
 * (mgh_graph_simple_csr, include/mg_host.h): list of read u =
 * edges[start[u] .. start[u + 1]), start has n_reads + 2 entries with
 * start[0] = start[1] = 0 and start[n_reads + 1] = n_edges < 2^32. */
typedef struct mg_chain_edge { /* 12 bytes: one half-edge */
  uint32_t dst;                /* read ID of its far node */
  uint32_t twin;               /* CSR index of its reverse edge (in dst's list) */
  uint16_t offset;             /* overlapOffset */
  uint8_t orient;              /* overlapOrientation */
  uint8_t pad;
} mg_chain_edge;
/* A node is INTERIOR when its list is [e0, e1], matchEdgeType(twin(e0), e1)
 * holds and e0 is no self-loop: the nodes contractCompositePaths may merge at.
 * A CHAIN is a maximal path a -> n1 -> .. -> nk -> b of interior nodes between
 * two half-edges (a, pa), (b, pb) of non-interior nodes (pa = position in a's
 * list).  The FAR END of a half-edge of a non-interior node is its dst when that
 * is non-interior, else the other end of the chain it heads.  A chain is SAFE
 * when a < b and no other half-edge of a's list has far end b (nor an unknown
 * one, see "chain_rounds"): isEdgePresent (:679) is then false at each of its
 * nodes in any order, and contracting it first leaves the loop's result
 * unchanged.  One safe chain, its n interior nodes contracted into the edge
 * a -> b and its reverse (mergeEdges / mergeList, :702-785): */
typedef struct mg_chain { /* 48 bytes */
  uint32_t a, b;          /* end nodes, a < b */
  uint32_t pa, pb;        /* positions of the end half-edges in a's and b's list */
  uint32_t n;             /* interior nodes */
  uint8_t orient_fwd;     /* orientation of a -> b */
  uint8_t orient_rev;     /* orientation of b -> a */
  uint8_t pad[2];
  uint64_t offset_fwd;    /* overlapOffset of a -> b: the sum over its n + 1 edges */
  uint64_t offset_rev;    /* the same for b -> a */
  uint64_t first;         /* its lists: forward [first, first + n), reverse [first + n, first + 2 n) */
} mg_chain;
/* counters of a build (mg_build_chains, mgh_chains_build) */
enum { MG_CHAIN_INTERIOR = 0,   /* interior nodes */
       MG_CHAIN_SAFE = 1,       /* safe chains (the table's length) */
       MG_CHAIN_CONTRACTED = 2, /* interior nodes on them */
       MG_CHAIN_UNSAFE = 3,     /* chains with both ends known that are not safe */
       MG_CHAIN_UNRESOLVED = 4, /* (node, port) states without a known end: pure cycles, chains over the cap */
       MG_CHAIN_ROUNDS = 5,     /* pointer-jumping rounds run */
       MG_CHAIN_INFO = 6 };
/* The safe chains on the device, in ascending start[a] + pa: list ranking by
 * pointer jumping over the 2 n_interior (node, port) states, two scans and a
 * scatter of the read lists (reads / listOfOverlapOffsets / listOfOrientations
 * of both new edges).  Needs a context only: no reads, no index.  A function of
 * the CSR alone: two calls give identical arrays, equal to mgh_chains_build's.
 * At most ceil(log2(n_interior + 1)) + 1 rounds run (every chain's ends are
 * known by then), fewer when a round finds no new end; option "chain_rounds"
 * lowers that cap: a chain is then known only when it has at most 2^rounds
 * interior nodes, and a half-edge that heads an unknown chain makes every chain
 * of its node unsafe.  *n_chains, *n_list = lengths of the table and of the
 * lists; info (optional) = MG_CHAIN_INFO counters; *device_ms (optional) =
 * HIP-event time from the first kernel to the last.  -1 = bad arguments, a
 * sharded / exchange-mode context, a device error; -2 = start not monotone
 * from 0 to n_edges, a dst outside 1..n_reads, a twin outside its dst's list,
 * twin[twin[e]] != e or a twin whose dst is not e's node: mg_last_error names
 * the first such entry, found before anything is indexed through it. */
int mg_build_chains(mg_ctx* ctx, const uint64_t* start, const mg_chain_edge* edges, uint64_t n_reads,
                    uint64_t n_edges, uint64_t* n_chains, uint64_t* n_list, uint64_t* info, float* device_ms);
/* chains: chain_cap records; reads / offs / ors: list_cap entries each.  Any may
 * be NULL; what exceeds a cap is not written.  Fails unless mg_build_chains
 * succeeded on this context. */
int mg_copy_chains(mg_ctx* ctx, mg_chain* chains, uint64_t chain_cap, uint32_t* reads, uint16_t* offs, uint8_t* ors,
                   uint64_t list_cap);

/* --- read lookup and mate pairs (Dataset::getReadFromString, storeMatePairInformation)
 * Batched Dataset::getReadFromString (Dataset.cpp:421-455) over the resident
 * reads.  Raw record i = concat[offsets[i], offsets[i+1]), any case, as
 * mg_ingest_ascii takes it.  id_out[i] = the reference ID of the resident read
 * equal to min(s, revcomp s), or 0 when the record fails the ingest's filter
 * (length > min_overlap, ACGT only, the 80 % rule, length <= 65,535) or no
 * resident read equals it (the reference exits there; here it is a value).
 * flags_out[i]: bit 0 = the record passed the filter; bit 1 = a read was found
 * and the upper-cased record itself is its stored forward string (so a read
 * that is its own reverse complement sets it).  The search is a binary search
 * over the reads in ID order = std::string order (packed words, then length).
 * Works in every context that holds the reads (after any upload or ingest,
 * layout on or off, sharded and exchange-mode contexts included).
 * *device_ms (optional) = HIP-event time of the kernels (no transfers). */
int mg_find_reads(mg_ctx* ctx, const char* concat, const uint64_t* offsets, uint64_t n_raw, uint32_t min_overlap,
                  uint32_t* id_out, uint8_t* flags_out, float* device_ms);
/* One entry of Read::getMatePairList() (MPlist, Read.h): the mate's read ID,
 * matePairOrientation 0..3 and datasetNumber.  8 bytes. */
typedef struct mg_mate {
  uint32_t id;
  uint8_t orient;
  uint8_t dataset;
  uint16_t pad; /* 0 */
} mg_mate;
/* storeMatePairInformation's per-pair body (Dataset.cpp:275-301) and
 * Read::addMatePair (Read.cpp:132-166) for every pair of every paired-end
 * file: records 2p and 2p + 1 are line1 and line2 of pair p, pairs in file
 * order, file by file; pairs_per_dataset[d] pairs belong to file d (their sum
 * is n_raw / 2; d < 256, UINT8 as in MPlist).  A pair is good iff both mates
 * pass the filter; r1, r2 = the lookup above; with use_super a read with
 * superReadID != 0 is replaced by that read (once, :280-284; the IDs of the
 * context's completed mg_mark_contained); orient_k = 1 iff the upper-cased raw
 * mate occurs in the forward string of the (redirected) read (:291-292); r1
 * gets (r2, orient1 * 2 + orient2, d), then r2 gets (r1, orient1 + orient2 * 2,
 * d), each unless its list already holds an equal entry.  The lists stay on
 * the device as one CSR until new reads arrive.  *n_records = total list
 * length; good_bad_pairs[0 / 1] = good / bad pairs.  Errors: n_raw odd or the
 * dataset counts do not add up; use_super on a sharded, source-range or
 * exchange-mode context or before mg_mark_contained completed; a good mate
 * with no resident read (-2; the message names the first such raw index; the
 * reference exits with "String not found in Dataset"). */
int mg_build_mate_pairs(mg_ctx* ctx, const char* concat, const uint64_t* offsets, uint64_t n_raw,
                        const uint64_t* pairs_per_dataset, uint32_t n_datasets, uint32_t min_overlap, int use_super,
                        uint64_t* n_records, uint64_t* good_bad_pairs, float* device_ms);
/* start: n_reads + 2 entries (as mg_copy_discoveries), the list of read A =
 * out[start[A] .. start[A+1]) in addMatePair's order; out: cap records.  Either
 * may be NULL.  Fails unless mg_build_mate_pairs ran for the current reads. */
int mg_copy_mate_pairs(mg_ctx* ctx, uint64_t* start, mg_mate* out, uint64_t cap, uint64_t* n_copied);

/* --- contig sequences (OverlapGraph::getStringInEdge, OverlapGraph.cpp:2009-2041)
 * One edge whose string is to be spelled.  Its reads / offsets / orientations
 * (listOfReads, listOfOverlapOffsets, listOfOrientations) are entries
 * [first, first + n) of the shared lists; tail = the reverse edge's
 * listOfOverlapOffsets[0] (read only when n > 0).  40 bytes. */
typedef struct mg_contig_edge {
  uint32_t src, dst; /* read IDs */
  uint64_t offset;   /* getOverlapOffset */
  uint64_t first;
  uint32_t n;
  uint32_t tail;
  uint8_t orient, pad[7];
} mg_contig_edge;
/* The string of edge k is n + 2 pieces laid end to end:
 *   piece 0      the whole source read, forward strand iff orient is 2 or 3;
 *   piece i + 1  reads[first + i], forward strand iff ors[first + i] == 1: with
 *                prev = the length of the previous piece's read, the bases of
 *                that strand from position prev - offs[first + i] on, preceded
 *                by 'N' iff offs[first + i] == prev;
 *   tail         the destination read, forward strand iff orient is 1 or 3, from
 *                position len(src) - offset (n == 0) or len(dst) - tail on.
 * A piece is valid iff its position lies in [0, length of its read] (std::string::
 * substr throws otherwise); an empty piece is valid.  All pieces of all edges are
 * sized by one kernel, placed by one 64-bit exclusive scan and written by one
 * copy kernel that reads each piece's read from the resident packed reads (the
 * reverse strand is derived in registers).  Needs only a context that holds the
 * reads (any upload or ingest, either slot layout, any width, long reads
 * included); no index.  *total_bases = the length of all strings together;
 * *device_ms (optional) = HIP-event time of the kernels (no transfers).
 * Errors: -1 (bad arguments, a context without reads, a list range outside
 * n_list, a HIP error); -2 an invalid piece or a read ID outside 1..n_reads: no
 * copy kernel runs and mg_last_error names the first such edge and piece.  The
 * strings stay on the device until the next upload or ingest. */
int mg_build_contigs(mg_ctx* ctx, const mg_contig_edge* edges, uint64_t n_edges, const uint32_t* reads,
                     const uint16_t* offs, const uint8_t* ors, uint64_t n_list, uint64_t* total_bases,
                     float* device_ms);
/* start: n_edges + 1 entries, the string of edge k = out[start[k] .. start[k+1])
 * (ASCII, no terminator); out: cap bytes.  Either may be NULL.  Fails unless
 * mg_build_contigs succeeded for the current reads. */
int mg_copy_contigs(mg_ctx* ctx, uint64_t* start, char* out, uint64_t cap, uint64_t* n_copied);

/* --- read placements, insert sizes, edge coverage ---------------------------
 * (OverlapGraph::updateReadLocations :1048-1071, calculateMeanAndSdOfInsertSize
 * :1124-1211, getBaseByBaseCoverage :2722-2792)
 * One placement of a read: list entry i of edge k places reads[first + i] on
 * edge k at distance D(k, i) = offs[first] + ... + offs[first + i], forward iff
 * ors[first + i] == 1.  A read's forward placements are its
 * getListOfEdgesForward / getLocationOnEdgeForward, the others the ...Reverse
 * pair.  16 bytes. */
typedef struct mg_place {
  uint32_t edge;     /* index into the edges given to mg_build_placements */
  uint32_t flags;    /* bit 0 = forward */
  uint64_t distance; /* D(k, i) */
} mg_place;
/* updateReadLocations (:1048-1071) of every edge at once.  `edges` and the
 * shared lists are what mg_build_contigs takes, every directed edge once
 * (mgh_graph_contig_edges(all = 1)); src, dst, offset, tail and orient are not
 * read here (mg_edge_coverage reads src, dst and offset).  Builds one CSR of
 * mg_place over the reads, each read's records in ascending (edge index, list
 * position) -- the reference's order inside a read's lists depends on the
 * contraction history, so only the set is promised to equal its lists -- and
 * each read's forward-placement count.  One 64-bit device-wide inclusive scan
 * of the offsets with each edge's base subtracted gives the distances; one
 * stable radix sort of the entries by read ID gives the CSR in the promised
 * order.  Needs only a context that holds the reads (any upload or ingest,
 * either slot layout, any width, long reads included); a sharded or
 * exchange-mode context refuses.  *n_places = total records (the edges' n
 * together, < 2^31); *device_ms (optional) = HIP-event time of the kernels (no
 * transfers).  Errors: -1 (bad arguments, a list range outside n_list, a HIP
 * error); -2 a read ID outside 1..n_reads: mg_last_error names the first such
 * edge and entry.  The CSR stays on the device until the next upload or ingest. */
int mg_build_placements(mg_ctx* ctx, const mg_contig_edge* edges, uint64_t n_edges, const uint32_t* reads,
                        const uint16_t* offs, const uint8_t* ors, uint64_t n_list, uint64_t* n_places,
                        float* device_ms);
/* start: n_reads + 2 entries (as mg_copy_mate_pairs), the placements of read A =
 * out[start[A] .. start[A+1]); out: cap records.  Either may be NULL.  Fails
 * unless mg_build_placements succeeded for the current reads. */
int mg_copy_placements(mg_ctx* ctx, uint64_t* start, mg_place* out, uint64_t cap, uint64_t* n_copied);
/* The sums behind calculateMeanAndSdOfInsertSize (:1140-1179).  For every read
 * A, every entry (B, orient, dataset = d) of A's mate list, every placement p
 * of A and q of B (either strand each) with p.edge == q.edge, p.distance >
 * q.distance and x = p.distance - q.distance < max_distance (the reference's
 * 1000): sums[3 d] += 1, sums[3 d + 1] += x, sums[3 d + 2] += x * x (64-bit,
 * wrapping); every matching (p, q) combination counts.  The host finishes:
 * mean = sum / count, variance = sumsq - 2 mean sum + count mean^2 (mod 2^64),
 * sd = (uint64)sqrt((double)(variance / count)); count == 0 gives 0, 0.
 * mate_start == NULL: the resident lists of mg_build_mate_pairs; otherwise a
 * CSR in mg_copy_mate_pairs' layout (mate_start: n_reads + 2 non-decreasing
 * entries, mate_start[0] = 0; mates: mate_start[n_reads + 1] records).  One
 * thread per mate entry; the integer sums are reduced across the wavefront
 * and leave it as one 64-bit atomic per counter, so the result does not depend
 * on the order.  sums: 3 * n_datasets entries.  Errors: -1 (bad arguments, no
 * placements, no resident mate lists); -2 a mate entry whose dataset >=
 * n_datasets or whose owner or mate ID lies outside 1..n_reads:
 * mg_last_error names the first such entry. */
int mg_insert_sizes(mg_ctx* ctx, const uint64_t* mate_start, const mg_mate* mates, uint32_t n_datasets,
                    uint64_t max_distance, uint64_t* sums, float* device_ms);
/* getBaseByBaseCoverage (:2722-2792) of every edge of the last
 * mg_build_placements.  Edge k: L = offset + len(dst), counters c[0 .. L];
 * every list entry adds freq[read - 1] to c[D, D + len(read)); every entry
 * whose read has more than one forward placement over all edges zeroes its
 * interval (the reference tests the forward list only); then c[0, len(src)) and
 * the last len(dst) counters are zeroed; out[3 k .. 3 k + 2] = count, sum and
 * sum of squares (64-bit, wrapping) over the non-zero counters.  The host
 * finishes mean and sd as for the insert sizes.  freq: n_reads entries, or NULL
 * = the frequencies the device ingest left (an error when the reads were
 * uploaded).  Per base one 64-bit delta word (zeroing entries in the high half,
 * frequencies in the low half) takes integer atomics at interval starts and
 * ends, one scan turns the deltas into counters and one pass reduces them per
 * edge, so interval ends need not be monotone.  Edges are taken in chunks of at
 * most "cov_budget" counters (mg_set_option; an edge above it is a chunk of its
 * own).  Errors: -1 (bad arguments, no placements, no frequencies, an edge
 * whose offset is >= 2^40, an edge whose list frequencies sum to >= 2^32: the
 * frequency half of a delta word is 32 bits wide); -2 an invalid edge, where
 * the reference's at() would throw: src or dst outside 1..n_reads, D + len(read)
 * > L + 1, or len(src) > L + 1: mg_last_error names the first such edge (and
 * entry) and no result is written. */
int mg_edge_coverage(mg_ctx* ctx, const uint32_t* freq, uint64_t* out, float* device_ms);

/* --- mate-pair path support: the scoring half of findSupportByMatepairsAndMerge
 * (OverlapGraph.cpp:1892-1966) with findPathBetweenMatepairs (:1645-1730) and
 * exploreGraph (:1781-1870), one lane per mate entry.
 *
 * INPUTS.  edges: every directed edge once, in mgh_graph_contig_edges(all = 1)
 * order (u order, each graph[u] in list order), so src never decreases, the
 * edges of one source are contiguous and their order is the order exploreGraph
 * walks (:1863); only src, dst, offset and orient are read.  twin[k]: the index
 * of edge k's reverse edge (mgh_graph_edge_twins).  Placements: a CSR over read
 * IDs (n_reads + 2 starts) of mg_place records; a read's forward list is its
 * records with flags bit 0 set, in CSR order, its reverse list the others, in
 * CSR order.  mgh_graph_location_lists gives the reference's list order (the
 * order loc_fwd / loc_rev keep); place_start = NULL takes the resident
 * placements of mg_build_placements, which hold the same SET in (edge,
 * position) order: the order of the combos decides which path is "first", so
 * the supported set of an entry is the same, but which of two equal adjacent
 * pairs of a path carries the flag, and so a pair's multiplicity, can differ
 * when a path repeats an adjacent pair.  Mates: a CSR in mg_copy_mate_pairs'
 * layout, or NULL: the resident lists.  mean[d], sd[d] per dataset.
 *
 * PER MATE ENTRY t = (A, j) holding (B, orient, d), t ascending in (A, j):
 *   skipped (MG_PATH_SKIPPED): A > B (A = B is processed) or mean[d] == 0.
 *   A's list is its forward list iff orient is 2 or 3, B's iff orient is 0 or 2.
 *   same edge (MG_PATH_SAME_EDGE): either list is empty (:1667 returns false
 *     too), or some (i, j) has first == last or first == twin[last].
 *   otherwise the combos (i, j), i-major: d1 = offset(first) - loc1[i], d2 =
 *     loc2[j]; explored iff d1 + d2 < mean + 3 sd.  All arithmetic is unsigned
 *     64-bit and wraps; with 3 sd > mean the bound mean - 3 sd wraps and no
 *     destination is ever in range.
 *   exploreGraph: level 0 holds (first, d1).  A child of the edge at `level` is
 *     an edge c of graph[dst] in list order with matchEdgeType(edge, c) and
 *     len[level] < mean + 3 sd.  At level + 1 > 100 the child returns at once (a
 *     path has at most 101 edges).  c == last with d2 + len[level] in [mean -
 *     3 sd, mean + 3 sd] (both inclusive) ends a path there without descending;
 *     any other child (an out-of-range arrival at `last` too) is pushed with
 *     len = offset(c) + len[level] and walked through.  The first path of a
 *     combo is kept with all flags 1; every later path of that combo clears the
 *     flag of each adjacent pair of the first path that is not adjacent in it.
 *   across combos: the first combo that finds a path gives the entry's path
 *     and flags; every later successful combo clears flag k unless (path[k],
 *     path[k + 1]) is adjacent in its own first path at a position whose flag
 *     is 1.
 *   status MG_PATH_NONE (no combo found a path) or MG_PATH_FOUND (path, flags).
 * WORK UNITS of an entry: one per (i, j) of the same-edge test, one per child
 * looked at, one per first-path position compared when a later path arrives and
 * one per kept-path position compared when a later combo succeeds.  An entry
 * whose units exceed option "path_budget" (default 2^16) is MG_PATH_DEFERRED
 * and leaves no partial result: the reference's search has no limit, a kernel
 * has.  mgh_mate_paths finishes deferred entries exactly (its `prior`).
 *
 * AGGREGATE: listOfPairedEdges before :1968.  Over the entries in t order and
 * k ascending, every flagged pair (a, b) = (path[k], path[k + 1]) is dropped if
 * a and b are both self-loops, else joins the record that holds (a, b) or
 * (twin[b], twin[a]), else opens a record with the orientation first seen.
 * Records (edge1, edge2, support) come in first-seen order.  counters[3] =
 * noPathsFound, pathsFound, mpOnSameEdge (:1901).
 *
 * mg_mate_paths: a validation pass first, so nothing indexes with an unchecked
 * value: -2 with mg_last_error naming the first offender, in this order: an
 * edge whose src is below its predecessor's, a twin outside the edges, a
 * placement whose edge is outside the edges, a mate entry whose owner or mate
 * ID lies outside 1..n_reads or whose dataset is not below n_datasets.  Then
 * the entries are explored in batches of option "path_batch" lanes (default
 * 2^18) over a level-major workspace, and aggregated: flagged positions
 * compacted by a scan, a stable radix sort by canonical key min((a, b),
 * (twin[b], twin[a])), run heads (first position, run length = support), and a
 * sort of the heads by first position.  With deferred entries (*n_deferred >
 * 0) counters and pairs cover the other entries only; the caller finishes with
 * mgh_mate_paths over the copied entries.  n_reads must equal the resident
 * read count when a resident CSR is taken; with two caller CSRs the context
 * needs no reads.  -1: bad arguments, a malformed CSR, a sharded or
 * exchange-mode context, 2^31 or more edges, entries or path positions. */
enum { MG_PATH_SKIPPED = 0, MG_PATH_SAME_EDGE = 1, MG_PATH_NONE = 2, MG_PATH_FOUND = 3, MG_PATH_DEFERRED = 4 };
typedef struct mg_pair_support {
  uint32_t edge1, edge2; /* indices into edges, in the orientation first seen */
  uint64_t support;
} mg_pair_support;
int mg_mate_paths(mg_ctx* ctx, const mg_contig_edge* edges, const uint32_t* twin, uint64_t n_edges, uint64_t n_reads,
                  const uint64_t* place_start, const mg_place* places, const uint64_t* mate_start,
                  const mg_mate* mates, const uint64_t* mean, const uint64_t* sd, uint32_t n_datasets,
                  uint64_t* counters, uint64_t* n_pairs, uint64_t* n_deferred, float* device_ms);
/* Sizes and times of the last mg_mate_paths: out[4] = mate entries, path
 * positions, pairs, deferred entries; ms[2] = the explore kernels, the
 * aggregate (device time by events).  Either may be NULL. */
int mg_mate_paths_info(mg_ctx* ctx, uint64_t* out, float* ms);
/* Per-entry results: status and visits (work units; of a deferred entry, those
 * spent before it gave up) have one entry per mate entry, path_start one more;
 * path / flags (path_cap positions, written only when path_cap >= the total):
 * entry t's path = path[path_start[t] .. path_start[t + 1]), flags[p] = 1 when
 * (path[p], path[p + 1]) is supported (0 at a path's last position).  Any
 * pointer may be NULL. */
int mg_copy_mate_paths(mg_ctx* ctx, uint8_t* status, uint32_t* visits, uint64_t* path_start, uint32_t* path,
                       uint8_t* flags, uint64_t path_cap);
int mg_copy_path_pairs(mg_ctx* ctx, mg_pair_support* out, uint64_t cap, uint64_t* n_copied);

/* --- scaffolder: the scoring half of OverlapGraph::scaffolder
 * (OverlapGraph.cpp:2120-2195), one lane per mate entry.
 *
 * INPUTS as for mg_mate_paths, without the edges: twin[k] (the index of edge
 * k's reverse edge), the placement CSR, the mate CSR, mean[d] and sd[d] per
 * dataset.  place_start = NULL takes the resident placements of
 * mg_build_placements, mate_start = NULL the resident mate lists.  Only lists
 * that hold exactly one placement are ever read, so the resident (edge,
 * position) order and the reference's list order give identical results.
 *
 * PER MATE ENTRY t = (A, j) holding (B, orient, d), t ascending in (A, j):
 *   skipped (MG_SCAF_SKIPPED): A > B (:2137; A = B is processed, and there is
 *     no mean[d] == 0 test here, unlike :1911).
 *   A's list is its forward list iff orient is 0 or 1 (:2149; the opposite
 *     choice to findPathBetweenMatepairs), B's iff orient is 0 or 2 (:2153).
 *   not unique (MG_SCAF_NOT_UNIQUE): unless both lists hold exactly one
 *     placement (:2157), (L1, loc1) and (L2, loc2).
 *   far (MG_SCAF_FAR): dist = loc1 + loc2; unless dist < mean[d] + 3 sd[d]
 *     (:2157).  All arithmetic is unsigned 64-bit and wraps; a dataset with
 *     mean 0 and sd 0 therefore counts nothing.
 *   same edge (MG_SCAF_SAME_EDGE): L1 == L2 or L1 == twin[L2] (:2161).
 *   counted (MG_SCAF_COUNTED) otherwise: the entry joins the record that holds
 *     (twin[L1], L2) or (twin[L2], L1) (:2168, :2174), adding 1 to its support
 *     and dist to its distance (wrapping 64-bit sums); if there is none it
 *     opens the record (edge1 = twin[L1], edge2 = L2) (:2184-2190).
 * Records come in first-seen order (listOfPairedEdges before :2197).
 *
 * The record of an entry is found by its canonical key min(twin[L1] E + L2,
 * twin[L2] E + L1), E = n_edges.  The two forms of one entry can never name
 * the same record twice: they are equal only if twin[L1] == twin[L2] and L2 ==
 * L1, which the same-edge test has excluded.  With twin an involution (every
 * graph's is) the second form of an entry is the first form of the entry seen
 * from the other strand, (a, b) -> (twin[b], twin[a]), so two entries share a
 * key iff the reference's linear search finds the one's record for the other.
 *
 * mg_scaffold_pairs: validation first, in mg_mate_paths' order and wording, so
 * nothing indexes with an unchecked value: -2 with mg_last_error naming the
 * first twin outside the edges, else the first placement whose edge is
 * outside the edges, else the first mate entry whose owner or mate ID lies
 * outside 1..n_reads or whose dataset is not below n_datasets.  Then
 * k_sc_score (status, key, dist per entry; the status counters leave a
 * wavefront as one integer atomic each), a scan that compacts the counted
 * entries in entry order, a stable radix sort of (key, index) over the bits
 * E^2 needs, run heads, a 64-bit inclusive scan of dist in sorted order whose
 * differences at the heads are the distances (exact modulo 2^64), and a sort of
 * the heads by first index.  No floating point.  counters[5] = entries of each
 * status, indexed by MG_SCAF_*; *n_pairs = records.  With no counted entry no
 * sort is launched.  -1: bad arguments, a malformed CSR, a sharded or
 * exchange-mode context, 2^31 or more edges, placements or entries. */
enum { MG_SCAF_SKIPPED = 0, MG_SCAF_NOT_UNIQUE = 1, MG_SCAF_FAR = 2, MG_SCAF_SAME_EDGE = 3, MG_SCAF_COUNTED = 4 };
typedef struct mg_scaffold_pair {
  uint32_t edge1, edge2; /* indices into the edges, in the orientation first seen */
  uint64_t support;
  uint64_t distance; /* the sum of dist over the record's entries (mod 2^64) */
} mg_scaffold_pair;
int mg_scaffold_pairs(mg_ctx* ctx, const uint32_t* twin, uint64_t n_edges, uint64_t n_reads,
                      const uint64_t* place_start, const mg_place* places, const uint64_t* mate_start,
                      const mg_mate* mates, const uint64_t* mean, const uint64_t* sd, uint32_t n_datasets,
                      uint64_t counters[5], uint64_t* n_pairs, float* device_ms);
/* status: one MG_SCAF_* per mate entry of the last mg_scaffold_pairs. */
int mg_copy_scaffold_entries(mg_ctx* ctx, uint8_t* status);
int mg_copy_scaffold_pairs(mg_ctx* ctx, mg_scaffold_pair* out, uint64_t cap, uint64_t* n_copied);
/* Sizes and times of the last mg_scaffold_pairs: out[3] = mate entries,
 * counted entries, records; ms[2] = the score kernel, the aggregate (device
 * time by events).  Either may be NULL. */
int mg_scaffold_info(mg_ctx* ctx, uint64_t* out, float* ms);

/* --- sharding (multi-GPU, one process per GPU) ---------------------------- */
/* Restrict this context to index buckets owned by `rank` of `nranks`
 * (bucket-range sharding) and/or to the source reads with
 * reference IDs in [read_lo + 1, read_hi] (0-based range; read_hi = 0 means
 * all): every row this context produces then has its `src` in that range or
 * is the twin of such a row, so each rank holds the discoveries of its reads
 * (insertAllEdgesOfRead of its sources, OverlapGraph.cpp:529-565).  The union
 * over ranks is the whole multiset.  With the clustered slot layout the
 * range's reads are re-clustered into slots [read_lo, read_hi) at the next
 * mg_build_index.  A bucket range over every source (rank, nranks, 0, 0) with
 * one read length is the bucket mode (bench --multi bucket): mg_build_index's
 * one window scan reads every read, files the keys and keeps the runs of the
 * rank's buckets only, and mg_find_overlaps finds all of their discoveries. */
int mg_set_shard(mg_ctx* ctx, uint32_t rank, uint32_t nranks, uint64_t read_lo, uint64_t read_hi);

/* --- exchange mode: one process per GPU, SURVEY §8(e) ------------------------
 * Rank r of P (mg_set_shard(ctx, r, P, 0, 0)) owns the index buckets b with
 * floor(b P / 2^nb) == r and the source reads (IDs - 1) in
 * [floor(r N / P), floor((r+1) N / P)); every rank holds all packed reads.
 *
 * SLOT LAYOUT.  Records travel between ranks in caller-owned device buffers of
 * rounds * P * slot records (slot a multiple of 64).  The records a rank sends
 * to peer d -- or receives from peer s -- form one stream whose i-th record
 * sits at
 *     ((i / slot) * P + d) * slot + i % slot,      i < rounds * slot,
 * so round t of every peer is the contiguous block [t P slot, (t+1) P slot):
 * one equal-split all-to-all per round moves it (no split sizes on the host),
 * and one more moves the P per-peer counts (uint64 device arrays).  A stream
 * longer than rounds * slot is cut there but its count keeps the full length:
 * the caller reads the counts once at the end of the step (MAX over ranks),
 * and on an overflow grows the capacity and reruns the step.  Capacities must
 * be the same on every rank; mg_xchg_caps gives first estimates from global
 * quantities only.  Every call below only enqueues work on the context's
 * stream except mg_xchg_begin (one sync: the run count) and mg_xchg_probe(0)
 * (one sync: the row count); a caller that runs its collectives on the same
 * stream (metagenomics_amd/sharded.py) never waits on the host in between.
 *
 * One step (HashTable::insertDataset + OverlapGraph markContainedReads +
 * insertAllEdgesOfRead, distributed):
 *   mg_xchg_begin                 one window scan of this rank's sources: their
 *                                 index keys + minimizer runs (in scan order);
 *                                 keys first (mg_xchg_keys_first): the keys only
 *   mg_xchg_pack(MG_KEYS) -> a2a -> mg_xchg_insert_keys        (insertDataset;
 *                                 keys first: the window scan runs here)
 *   mg_xchg_pack(MG_RUNS) -> a2a   (the received runs serve both probes;
 *                                 one length: mg_xchg_probe_own meanwhile)
 *   mg_begin_contained(superkey)
 *   [lengths differ: (mg_xchg_prefix_marks -> all-reduce MAX of the marks)
 *                    mg_xchg_probe(1) -> all-reduce MAX of superkey]
 *   mg_finalize_contained                                       (markContainedReads)
 *   mg_xchg_probe(0) -> mg_xchg_pack(MG_ROWS) -> a2a             (insertAllEdgesOfRead)
 * and every rank ends with the rows whose src it owns (or, when the host skips
 * the last pack, with the rows it verified: the union over the ranks is the
 * same multiset).  Record sizes, mg_record_bytes(): keys 8 B (the index entry:
 * read slot | o | q | fingerprint | length), runs 8 B (the run meta: read slot
 * | minimizer position p | window range); the receiver recomputes the bucket
 * and fingerprint by hashing the minimizer m-mer of its own copy of the read
 * (every rank holds all reads), so they never travel; rows 12 B (mg_edge). */
enum { MG_KEYS = 0, MG_RUNS = 1, MG_ROWS = 2 };
uint32_t mg_record_bytes(int what);
/* First per-peer stream capacities (records) for keys, runs and rows:
 * caps[3], identical on every rank (global read count and lengths only). */
int mg_xchg_caps(mg_ctx* ctx, uint32_t min_overlap, uint32_t seed_k, uint64_t* caps);
/* Set up this rank's part of the index, then one scan of its source reads:
 * the index keys (hashRead, HashTable.cpp:88-104; the o = 1 key only when the
 * containment probe reads it) and the windows' minimizer runs
 * (OverlapGraph.cpp:534-537), in the scan's order. */
int mg_xchg_begin(mg_ctx* ctx, uint32_t min_overlap, uint32_t seed_k);
/* 1 when the current exchange build is KEYS FIRST (option xchg_keys_first,
 * default: several ranks and reads of one length): mg_xchg_begin then made the
 * key records only, and the window scan runs inside mg_xchg_insert_keys, which
 * CAS-inserts the received key records as it goes (k_scan<RECV>: no sort, no
 * separate cell build); MG_RUNS can be packed only after mg_xchg_insert_keys.
 * 0: one scan in mg_xchg_begin made keys and runs (MG_RUNS packable at once). */
int mg_xchg_keys_first(const mg_ctx* ctx);
/* Route what = MG_KEYS / MG_RUNS (after mg_xchg_begin) or MG_ROWS (after
 * mg_xchg_probe(0)) into dst in the slot layout; counts = P device uint64.
 * With one rank (P = 1) every stream is the rank's own: nothing is copied and
 * counts[0] = 0; mg_xchg_insert_keys and mg_xchg_probe then read the
 * context's own key records and run regions (recv / counts ignored), and the
 * rows stay in the context (mg_num_rows, mg_rows_digest, mg_copy_rows).
 * self_dst (optional): the stream bound for this rank itself is written there
 * instead -- the caller's receive buffer, whose slots for this rank sit at the
 * same offsets -- so it never travels (the all-to-all then moves only the
 * other peers' slots; dst may be NULL when P == 1). */
int mg_xchg_pack(mg_ctx* ctx, int what, void* dst, uint64_t slot, uint32_t rounds, uint64_t* counts,
                 void* self_dst);
/* File the received key records into the local cells (insertIntoTable,
 * HashTable.cpp:163-195); recv / counts as the all-to-all delivered them.  The
 * records are sorted by home cell and stored without atomics (a cell's 9th+
 * entries chain on); one host read of the counts.  Keys first
 * (mg_xchg_keys_first): the rank's window scan runs here instead and
 * CAS-inserts the received records between its windows, leaving the runs
 * (OverlapGraph.cpp:534-537) for mg_xchg_pack(MG_RUNS). */
int mg_xchg_insert_keys(mg_ctx* ctx, const void* recv, uint64_t slot, uint32_t rounds, const uint64_t* counts);
/* Probe the received runs against the local cells: contain = 1 atomicMax-es
 * containment keys into the buffer of mg_begin_contained; contain = 0 verifies
 * overlaps (sources with superReadID != 0 give none) and keeps the rows
 * (+ twins) for mg_xchg_pack(MG_ROWS).  The probes read the runs in place in
 * recv (pass the same recv / counts to both calls of a step); contain = 0
 * first compacts away, in place, the runs of contained sources, so recv is
 * the library's scratch until the step ends.  (Option xchg_sort_runs = 1: the
 * first call orders them by bucket into the context's own array instead.) */
int mg_xchg_probe(mg_ctx* ctx, int contain, const void* recv, uint64_t slot, uint32_t rounds, const uint64_t* counts);
/* Optional, after mg_finalize_contained and before mg_xchg_probe(0): the
 * discovery probe (insertAllEdgesOfRead's window loop + checkOverlap,
 * OverlapGraph.cpp:529-565, 354-383) of this rank's OWN run stream, which mg_xchg_pack(MG_RUNS)
 * wrote straight into recv (send_counts = that pack's counts; only this
 * rank's entry is read), so it runs while the peers' streams are still on the
 * links; mg_xchg_probe(0) then probes the peers' streams and appends its rows.
 * Same rows as one mg_xchg_probe(0).  A no-op (everything is left to
 * mg_xchg_probe(0)) with one rank, mixed lengths (the containment probe needs
 * every stream first) or option xchg_sort_runs. */
int mg_xchg_probe_own(mg_ctx* ctx, const void* recv, uint64_t slot, uint32_t rounds, const uint64_t* send_counts);
/* Containment: *needed = 1 when read lengths differ (OverlapGraph.cpp:228-233).
 * superkey = caller-owned device array of n_reads u64 (NULL: context-owned),
 * cleared here; the contain probe atomicMax-es (len << 32 | ~index) into it,
 * the host all-reduces it with MAX over the ranks, and mg_finalize_contained
 * turns it into superReadID (super_out optional, n_reads + 1 entries). */
int mg_begin_contained(mg_ctx* ctx, void* superkey, int* needed);
/* Optional, between mg_begin_contained and mg_xchg_probe(1) (lengths differ):
 * run this rank's offset-0 containments (checkOverlapForContainedRead at s = 0,
 * OverlapGraph.cpp:302-340, over the o = 0 key records it received) now and
 * write marks[i] = 1 for every read they found contained (n_reads bytes,
 * device; NULL: no marks).  The caller all-reduces marks with MAX over the
 * ranks on the context's stream; mg_xchg_probe(1) then folds them into the
 * key array, so that its contained-source skip (contain_skip) sees every
 * rank's offset-0 containments, not only this rank's.  marks stays the
 * caller's and must stay valid until mg_xchg_probe(1) is enqueued. */
int mg_xchg_prefix_marks(mg_ctx* ctx, void* marks);
int mg_finalize_contained(mg_ctx* ctx, uint32_t* super_out);

/* --- parity digests (no reference counterpart: test/bench support) ----------
 * Order-independent digests of the directed edge multiset and of the
 * superReadID vector, computed on the device, so that a 10^8-row result is
 * compared with the reference's (oracle/_ref/ref_harness digest) without a
 * multi-GB download.  out[4] = {count, sum h, xor h, sum mix64(h ^ SALT)}
 * mod 2^64, with mix64 the bijective finaliser (x ^= x>>31; x *= 0x7fb5d329728ea185;
 * x ^= x>>27; x *= 0x81dadef4bc2dd44d; x ^= x>>33), SALT = 0xD6E8FEB86659FD93 and
 *   row (u, v, orient, offset): h = mix64(((u << 32) | v) ^ mix64(((orient << 16) | offset)
 *                                   + 0x9E3779B97F4A7C15))
 *   contained read id:          h = mix64((id << 32) | superReadID)
 * Digests of disjoint parts combine by adding count/sum/sum2 and xor-ing xor.
 * mg_rows_digest: rows = NULL digests the context's rows of the last
 * mg_find_overlaps / mg_xchg_probe; else `rows` is a device array of n_rows
 * mg_edge records.  mg_slots_digest: rows received in the slot layout of the
 * exchange mode (counts = the P device uint64 per-peer counts). */
int mg_rows_digest(mg_ctx* ctx, const void* rows, uint64_t n_rows, uint64_t* out);
int mg_slots_digest(mg_ctx* ctx, const void* rows, uint64_t slot, uint32_t rounds, const uint64_t* counts,
                    uint64_t* out);
int mg_super_digest(mg_ctx* ctx, uint64_t* out);

/* --- diagnostics ----------------------------------------------------------- */
int mg_get_timings(const mg_ctx* ctx, mg_timings* t);
int mg_get_counters(const mg_ctx* ctx, mg_counters* c);
/* Options (results never depend on any of them):
 *  "nb_log2"        log2 directory buckets (0 = auto);
 *  "rows_cap"       initial row capacity (0 = auto; overflowing regions are resized
 *                   and the probe reruns);
 *  "stats"          1 = count work units (mg_get_counters) in the next launches;
 *  "layout"         1 = slots clustered by canonical global minimizer (default),
 *                   0 = ID order; takes effect at the next upload;
 *  "halving"        side of a self-symmetric o = 2/3 pair: 0 = parity-alternating
 *                   (default, even load over source IDs), 1 = lower ID;
 *  "prefix_contain" 1 = mixed-length sets find offset-0 containments with
 *                   k_prefix_contain and the containment probe skips suffix-key
 *                   hits (default); 0 = the probe verifies them itself;
 *  "contain_jcut", "contain_prune", "contain_skip"
 *                   containment pruning, all exact, default 1;
 *  "run_masks"      the window scan records a read's minimizer positions in a
 *                   per-lane bit set and emits its runs after the read (reads up
 *                   to 256 bp, l - k <= 32; default 1); 0 = every closed run is
 *                   staged in LDS.  Same run records, in another order;
 *  "probe_share"    a discovery block's 4 wavefronts share its run regions (default 1);
 *  "probe_compact"  sparse run batches are compacted in the probe (default 1);
 *  "live_index"     mixed lengths: after mg_mark_contained the discovery probe
 *                   walks an index of the uncontained reads' keys only
 *                   (OverlapGraph.cpp:548; exact, default 1; the exchange mode
 *                   coarsens the rank's cells for it); with it, the full index
 *                   of a mixed-length set holds the o = 0 / 2 keys only;
 *  "xchg_sort_runs" exchange mode: order the received runs by bucket before
 *                   the probes (default 0: probed in place, arrival order);
 *  "xchg_keys_first" exchange mode, one read length, P > 1: key records first,
 *                   filed by CAS inside the receiver's window scan (default 1;
 *                   0: one scan makes keys and runs, the receiver sorts the keys);
 *  "xchg_scan_lds"  exchange mode, one read length: k_scan's LDS sliding minimum
 *                   (default 1) instead of the register scan;
 *  "xchg_split_max" mg_xchg_probe_own splits the discovery probe up to this many
 *                   ranks (default 4);
 *  "xchg_region"    records per probe region of the received runs (power of two,
 *                   default 512);
 *  "xchg_route_rows" exchange mode: the discovery probe counts its rows per src
 *                   owner for mg_xchg_pack(MG_ROWS) (default 1); 0 when the
 *                   host keeps the rows where they were verified;
 *  "xchg_windows"   exchange mode, mixed lengths: the scan takes length-ranked
 *                   windows of 256 reads (default 1);
 *  "layout_scratch" 0 = free the layout's double buffers after each layout
 *                   (many contexts on one device); default 1 keeps them;
 *  "cells_double"   1 = two cell tables: each build takes the one the previous
 *                   build cleared on the side stream and clears the table it
 *                   retires there (2x the cells' memory; measured slower: the
 *                   clear beside the scan slows the scan); 0 (default) = one
 *                   table, cleared at the start of each build;
 *  "chain_par"      sorted cell builds (exchange mode): records past their home
 *                   cell placed in parallel by their index in their fingerprint's
 *                   run (default 1); 0 = one thread walks each overflowing cell;
 *  "check_cells"    diagnostics: after each sorted cell build, walk every record
 *                   from its home and fail the call if one is not found;
 *  "xchg_fs"        diagnostics: fingerprint bits in the exchange sort key
 *                   (-1 = auto: what fills the sort's last 8-bit digit);
 *  "alloc_cap"      tests: a device allocation above this many bytes fails as
 *                   out of memory (0 = no cap); every failed allocation leaves
 *                   the buffer's name, its size and the HIP error in mg_last_error;
 *  "run_cap"        tests: initial run records per scan region (0 = sized from
 *                   the reads; overflowing regions are resized and rescanned);
 *  "disc_block_cap" tests: records per read the workgroup sort of mg_build_discoveries
 *                   takes (0 = default 2,048; at least 64, where the wavefront path
 *                   ends); longer lists take the segmented radix sort;
 *  "cov_budget"     tests: per-base counters one chunk of mg_edge_coverage holds
 *                   (0 = default 2^25); an edge above it is a chunk of its own;
 *  "path_batch"     mate entries one explore launch of mg_mate_paths takes (0 = default
 *                   2^18; its workspace is 2,626 B per entry of a batch);
 *  "path_budget"    work units one mate entry of mg_mate_paths may spend before it is
 *                   deferred to the host mirror (0 = default 2^16): the one option a
 *                   call's own output depends on; the finished result does not;
 *  "chain_rounds"   tests: cap on the pointer-jumping rounds of mg_build_chains (0 = auto);
 *                   chains of more than 2^rounds interior nodes are then left out;
 *  "phase_limit", "max_blocks"
 *                   diagnostics: stop the probe after a phase / cap its grid. */
int mg_set_option(mg_ctx* ctx, const char* name, int64_t value);
/* HIP stream the context launches on (hipStream_t as void*), for callers that
 * time or capture it themselves. */
void* mg_stream(mg_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* MG_OVERLAP_H_ */
