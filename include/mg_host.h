/* mg_host.h — C-ABI over the host-side Dataset mirror (metagenomics_amd/csrc/host).
 *
 * The host Dataset mirror (the device version is mg_ingest_* in mg_overlap.h)
 * is the reference's Dataset semantics restated in C++ with packed reads:
 *   readDataset  Dataset.cpp:110-193  (FASTA/FASTQ parse, upper-case)
 *   testRead     Dataset.cpp:398-413  (only ACGT, no base >= floor(0.8 len))
 *   canonical    Dataset.cpp:163-167  (store min(s, revcomp(s)))
 *   sortReads    Dataset.cpp:197-202  (std::string order)
 *   removeDupicateReads Dataset.cpp:316-345 (frequency, IDs 1..N)
 * The result is handed to the device through mg_upload_reads_packed().
 */
#ifndef MG_HOST_H_
#define MG_HOST_H_
#include <stdint.h>

#include "mg_overlap.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mgh_dataset mgh_dataset;

/* Dataset(pe, se, minOverlap) (Dataset.cpp:39-65).  Returns 0 on success,
 * -1 on an unreadable file, -2 on an unknown format (first byte not '>'/'@'). */
int mgh_dataset_from_files(const char* const* files, int nfiles, uint64_t min_overlap, mgh_dataset** out);
/* Same pipeline from in-memory reads: codes[i*stride + k] in {0:A,1:C,2:G,3:T,
 * anything else = not ACGT} for k < lens[i].  nthreads <= 0: hardware threads. */
int mgh_dataset_from_codes(const uint8_t* codes, uint64_t n, uint64_t stride, const uint16_t* lens,
                           uint64_t min_overlap, int nthreads, mgh_dataset** out);
void mgh_dataset_free(mgh_dataset* ds);

uint64_t mgh_num_reads(const mgh_dataset* ds);   /* Dataset::getNumberOfReads (good reads) */
uint64_t mgh_num_unique(const mgh_dataset* ds);  /* Dataset::getNumberOfUniqueReads */
uint64_t mgh_shortest(const mgh_dataset* ds);    /* Dataset::shortestReadLength */
uint64_t mgh_longest(const mgh_dataset* ds);     /* Dataset::longestReadLength */
/* Zero-copy views of the packed unique reads in ID order (ID = index + 1). */
int mgh_packed(const mgh_dataset* ds, const uint64_t** words, const uint16_t** lens, uint32_t* words_per_read);
/* Read::getStringForward() of read `id` into buf (NUL-terminated); returns its
 * length, or -1 if id is out of range (Dataset.cpp:484-490). */
int64_t mgh_read_string(const mgh_dataset* ds, uint64_t id, char* buf, uint64_t cap);
uint32_t mgh_frequency(const mgh_dataset* ds, uint64_t id); /* Read::getFrequency */
/* Dataset::getReadFromString (Dataset.cpp:421-455): ID of a read given either
 * strand, 0 if absent. */
uint64_t mgh_find_read(const mgh_dataset* ds, const char* s, uint64_t len);

/* --- HashTable API values (no device counterpart) --------------------------------
 * HashTable::getHashTableSize() after insertDataset: the first entry of the
 * reference's prime table greater than 8 N + 1 (getPrimeLargerThanNumber,
 * HashTable.cpp:20-29,56); N = unique reads.  HashTable::hashFunction(key)
 * (HashTable.cpp:135-155) for a table of `table_size` entries.  The device
 * index does not use either: its exact-key buckets do not depend on the hash
 * (SURVEY §8(a) a8). */
uint64_t mgh_hash_table_size(uint64_t n_unique);
uint64_t mgh_hash_function(const char* key, uint64_t len, uint64_t table_size);

/* --- record splitting -------------------------------------
 * Dataset::readDataset's record splitting (Dataset.cpp:110-193) on a
 * memory-mapped file with nthreads host threads (<= 0: all): FASTA = header
 * line, then everything up to the next '>' with '\n' removed; FASTQ = the 2nd
 * of every 4 lines.  Record i's raw sequence (bytes as in the file, before
 * upper-casing / testRead) is text[off[i] .. off[i+1]); n_records + 1 offsets.
 * The outputs are malloc'ed: release with mgh_parse_free.  They are the input
 * mg_ingest_ascii (include/mg_overlap.h) takes.  0 = ok, -1 = cannot open,
 * -2 = unknown format (first byte not '>' / '@'), -3 = out of memory. */
int mgh_parse_file(const char* path, int nthreads, char** text, uint64_t** offsets, uint64_t* n_records,
                   double* seconds);
/* several files, concatenated in order (Dataset.cpp:52-60 reads paired-end files first) */
int mgh_parse_files(const char* const* paths, int nfiles, int nthreads, char** text, uint64_t** offsets,
                    uint64_t* n_records, double* seconds);
int mgh_parse_buffer(const char* buf, uint64_t n, int nthreads, char** text, uint64_t** offsets,
                     uint64_t* n_records, double* seconds);
void mgh_parse_free(void* p);
/* smallest chunk one thread splits (default 1 MiB; 0 restores it) */
void mgh_parse_set_min_chunk(uint64_t bytes);

/* --- mate pairs (storeMatePairInformation, Dataset.cpp:208-310) --------------------
 * The mates of every pair of the paired-end files, file by file, as
 * storeMatePairInformation's own loop extracts them (not readDataset's):
 * FASTQ = eight getlines per pair, mates on lines 1 and 5; FASTA = getline,
 * getline(.., '>'), getline, getline(.., '>') with only '\n' erased; a string
 * is cleared only while the stream is good.  So a FASTQ file that ends in a
 * newline gives one more pair of two empty mates, a FASTA file with an odd
 * record count pairs its last sequence with itself, and CRLF leaves '\r' in.
 * Records 2p and 2p + 1 are the mates of pair p (bytes as in the file);
 * pairs_per_file (optional) gets nfiles counts.  Serial.  The outputs are
 * malloc'ed (mgh_parse_free) and are what mg_find_reads / mg_build_mate_pairs
 * take.  0 = ok, -1 = cannot open, -2 = unknown format, -3 = bad arguments /
 * out of memory. */
int mgh_read_pairs(const char* const* paths, int nfiles, char** text, uint64_t** offsets, uint64_t* n_records,
                   uint64_t* pairs_per_file, double* seconds);
int mgh_read_pairs_buffer(const char* buf, uint64_t n, char** text, uint64_t** offsets, uint64_t* n_records);
/* The host mirror of mg_build_mate_pairs + mg_copy_mate_pairs (mg::MatePairs::
 * build): the reference's statements (getReadFromString's binary search, the
 * superReadID redirect, string::find, Read::addMatePair) over the packed unique
 * reads in ID order; super = superReadID per ID (n_reads + 1 entries) or NULL
 * (all 0).  start: n_reads + 2 entries; out: cap records (cap >= n_raw is
 * always enough); either may be NULL.  0 = ok, -1 = bad arguments, -2 = a good
 * mate has no read (*not_found = its raw index; the reference exits with
 * "String not found in Dataset"). */
int mgh_mate_pairs_build(const uint64_t* words, const uint16_t* lens, uint64_t n_reads, uint32_t words_per_read,
                         const uint32_t* super, const char* concat, const uint64_t* offsets, uint64_t n_raw,
                         const uint64_t* pairs_per_dataset, uint32_t n_datasets, uint32_t min_overlap,
                         uint64_t* start, mg_mate* out, uint64_t cap, uint64_t* n_records, uint64_t* good_bad_pairs,
                         int64_t* not_found);

/* --- multi-process rendezvous (exchange mode over RCCL) ---------
 * Rank 0 serves the n-byte blob (the RCCL unique id) to the world - 1 other
 * ranks over TCP at addr:port; the others receive it into blob.  addr is a
 * dotted address or a host name (torchrun's MASTER_ADDR, e.g. "localhost").
 * Every wait is bounded by timeout_ms (<= 0: 10 minutes).  0 = ok, -1 bad
 * arguments, -2 addr does not resolve, -3 cannot listen (rank 0), -4 deadline
 * passed (a peer never connected / rank 0 never reachable), -5 I/O error.
 * Replaces torch.distributed's store for the C++ host (mg_overlap -xchg). */
int mgh_rendezvous(int rank, int world, const char* addr, int port, void* blob, uint64_t n, int timeout_ms);

/* --- graph construction order ----------------------------
 * Replays OverlapGraph::buildOverlapGraphFromHashTable's exploration and
 * transitive reduction (OverlapGraph.cpp:144-204, 574-661) on the device's
 * discovery multiset (mg_find_overlaps + mg_copy_rows, or the rows of every
 * rank in exchange mode): the resulting graph[u] lists, in list order, and the
 * numberOfNodes / numberOfEdges counters are the reference's just before its
 * contraction loop (:211-215).  lens[id - 1] = read lengths, h = l - 1. */
typedef struct mgh_graph mgh_graph;
/* 0 = ok; -1 bad arguments; -2 rows inconsistent with lens / h; -3 unpaired self rows */
int mgh_graph_replay(const mg_edge* rows, uint64_t n_rows, const uint16_t* lens, uint64_t n_reads, uint32_t h,
                     mgh_graph** out);
/* The same replay on the device-grouped lists (mg_build_discoveries +
 * mg_copy_discoveries, include/mg_overlap.h): start has n_reads + 2 entries.
 * The handle is mgh_graph_replay's.  0 = ok; -1 bad arguments, start not
 * monotone, start[n_reads + 1] != n_disc or a dst out of range; -2 a record
 * inconsistent with lens / h; -3 a list not strictly increasing in (j, dst, o). */
int mgh_graph_replay_disc(const uint64_t* start, const mg_disc* disc, uint64_t n_disc, const uint16_t* lens,
                          uint64_t n_reads, uint32_t h, mgh_graph** out);
/* The host grouping on its own (mg::Discoveries::build, what mgh_graph_replay
 * starts with): rows -> the lists in the layout mg_copy_discoveries gives
 * (start: n_reads + 2 entries; disc: cap records, cap >= n_rows is always
 * enough; either may be NULL).  Same return codes as mgh_graph_replay. */
int mgh_discoveries_build(const mg_edge* rows, uint64_t n_rows, const uint16_t* lens, uint64_t n_reads, uint32_t h,
                          uint64_t* start, mg_disc* disc, uint64_t cap, uint64_t* n_disc);
/* The validation and j pass of mgh_graph_replay_disc on its own
 * (mg::Discoveries::from_lists), same return codes; builds no graph. */
int mgh_discoveries_check(const uint64_t* start, const mg_disc* disc, uint64_t n_disc, const uint16_t* lens,
                          uint64_t n_reads, uint32_t h);
/* The connected components of the lists on the host (mg::Components::build, a
 * plain union-find): what mg_build_components + mg_copy_components give
 * (include/mg_overlap.h).  label: n_reads + 1 entries; comps: cap entries
 * (n_reads / 2 is always enough); either may be NULL.  0 = ok, -1 = bad
 * arguments, start malformed or a dst out of range. */
int mgh_components_build(const uint64_t* start, const mg_disc* disc, uint64_t n_disc, uint64_t n_reads,
                         uint32_t* label, mg_comp* comps, uint64_t cap, uint64_t* n_comp);
/* mgh_graph_replay_disc with the components replayed in parallel by `threads`
 * host threads (0 = min(16, hardware threads) or MG_REPLAY_THREADS; 1 = the
 * serial replay): the same handle, the same graph.  label (n_reads + 1
 * entries) and comps are validated against the lists.  Codes of
 * mgh_graph_replay_disc, -1 also for a label or root outside 1..n_reads, and
 * -4 = label / comps are not the components of these lists (no graph is
 * built). */
int mgh_graph_replay_comp(const uint64_t* start, const mg_disc* disc, uint64_t n_disc, const uint16_t* lens,
                          uint64_t n_reads, uint32_t h, const uint32_t* label, const mg_comp* comps, uint64_t n_comp,
                          uint32_t threads, mgh_graph** out);
/* OverlapGraph::readGraphFromFile (OverlapGraph.cpp:1270-1367): a .unitig
 * checkpoint back into a graph (both edges of every record, twins rebuilt,
 * read locations updated); lens[id - 1] of the Dataset it was written for.
 * The handle then behaves as a contracted one (sort_edges, save_unitig,
 * save_lists, unitig_edges).  0 ok; -1 cannot open; -2 malformed or a read ID
 * out of range; -3 bad arguments. */
int mgh_graph_read_unitig(const char* path, const uint16_t* lens, uint64_t n_reads, mgh_graph** out);
void mgh_graph_free(mgh_graph* g);
uint64_t mgh_graph_nodes(const mgh_graph* g); /* OverlapGraph::getNumberOfNodes */
uint64_t mgh_graph_edges(const mgh_graph* g); /* OverlapGraph::getNumberOfEdges (directed) */
/* All lists concatenated in u order, each in list order (n_out = edges).
 * Returns the number of rows written (<= cap); cap = 0 returns the count. */
uint64_t mgh_graph_rows(const mgh_graph* g, mg_edge* out, uint64_t cap);

/* --- unitig contraction + .unitig checkpoint -------------
 * Runs the loop that ends new OverlapGraph(ht) (OverlapGraph.cpp:211-215):
 *   do { contractCompositePaths() :669-696; removeDeadEndNodes() :931-988 }
 *   while (anything merged or removed)
 * on the replayed graph, with the reference's mergeEdges / mergeList /
 * removeEdge list surgery and (track_locations != 0) the per-read location
 * lists of updateReadLocations / removeReadLocations (:1048-1115).  After it,
 * mgh_graph_nodes / mgh_graph_edges are the reference's counters after the
 * loop and mgh_graph_rows returns 0 (offsets of composite edges exceed 16 bits:
 * use mgh_graph_unitig_edges).  0 = ok; -1 bad handle / already contracted;
 * -4 an orientation pair mergedEdgeOrientation rejects (:830-833 MYEXIT). */
int mgh_graph_contract(mgh_graph* g, int track_locations, uint64_t* iterations, uint64_t* merged,
                       uint64_t* dead_end_nodes);
/* --- safe chains: the order-free bulk of the first contraction pass ------------
 * Definitions: include/mg_overlap.h ("safe chains"); argument: DESIGN.md §7d.
 * The replayed (not yet contracted) graph as the CSR mg_build_chains and
 * mgh_chains_build take: u order, each list in list order (the order of
 * mgh_graph_rows), twin = CSR index of the reverse edge.  start: n_reads + 2
 * entries; edges: cap records; either may be NULL.  Returns the number of
 * half-edges (0 for a contracted handle); beyond cap nothing is written. */
uint64_t mgh_graph_simple_csr(const mgh_graph* g, uint64_t* start, mg_chain_edge* edges, uint64_t cap);
/* The inverse: an uncontracted handle whose lists are those of the CSR (edges
 * created in CSR order), for graphs that no discovery multiset produced (tests,
 * the stand-alone check).  0 = ok; -1 = bad arguments; -2 = a malformed CSR, as
 * mg_build_chains refuses it. */
int mgh_graph_from_csr(const uint64_t* start, const mg_chain_edge* edges, uint64_t n_reads, uint64_t n_edges,
                       mgh_graph** out);
/* The host mirror of mg_build_chains + mg_copy_chains (mg::chains_build): a
 * serial walk over the same CSR, the definition of the device's arrays, in the
 * same order.  rounds: as option "chain_rounds" (0 = auto).  chains: chain_cap
 * records; reads / offs / ors: list_cap entries; written only when the cap
 * holds all of them.  info: MG_CHAIN_INFO counters.  Any output may be NULL.
 * 0 = ok; -1 = bad arguments; -2 = as mg_build_chains (err names the entry). */
int mgh_chains_build(const uint64_t* start, const mg_chain_edge* edges, uint64_t n_reads, uint64_t n_edges,
                     uint32_t rounds, mg_chain* chains, uint64_t chain_cap, uint32_t* reads, uint16_t* offs,
                     uint8_t* ors, uint64_t list_cap, uint64_t* n_chains, uint64_t* n_list, uint64_t* info, char* err,
                     uint64_t err_cap);
/* mgh_graph_contract with a table of safe chains of this handle's CSR
 * contracted first (mg::UnitigGraph::apply_chains): the edges a -> b and b -> a
 * of every chain installed at lists[a][pa] and lists[b][pb], the interior lists
 * emptied, read locations added, then the loop unchanged, with the contracted
 * nodes counted as merges of its first pass.  The handle ends in the state
 * mgh_graph_contract leaves: lists in list order, read lists, location lists in
 * list order, counters, *iterations, *merged, *dead_end_nodes.  Any subset of
 * the safe chains may be given.  The table is validated for soundness (every
 * entry locally, threaded; ends; no read in two chains; each chain's safeness
 * from a's list): -4 = it is not a set of safe chains of this graph, and the
 * handle is unchanged (still uncontracted).  Other codes as mgh_graph_contract. */
int mgh_graph_contract_chains(mgh_graph* g, const mg_chain* chains, uint64_t n_chains, const uint32_t* reads,
                              const uint16_t* offs, const uint8_t* ors, uint64_t n_list, int track_locations,
                              uint64_t* iterations, uint64_t* merged, uint64_t* dead_end_nodes);
/* sortEdges (:2799-2808): every list sorted by destination ID (std::sort). */
int mgh_graph_sort_edges(mgh_graph* g);
/* saveGraphToFile (:1219-1261): the .unitig checkpoint of the current graph
 * (main.cpp:49-50 calls it after sortEdges).  0 = ok, -1 = open/write error. */
int mgh_graph_save_unitig(const mgh_graph* g, const char* path);
/* every list in list order as "u v orient offset nreads r:o:d ..." rows, then
 * the read location lists as "F|R read src dst orient offset location" rows
 * (the parity dump of oracle/ref_harness unitig). */
int mgh_graph_save_lists(const mgh_graph* g, const char* path);
typedef struct mgh_unitig_edge {
  uint32_t src, dst;  /* getSourceRead / getDestinationRead IDs */
  uint64_t offset;    /* getOverlapOffset (UINT64) */
  uint32_t n_reads;   /* getListOfReads()->size() */
  uint8_t orient;     /* getOrientation */
  uint8_t pad[3];
} mgh_unitig_edge;
/* contracted lists concatenated in u order, each in list order; the reads of
 * edge k are reads[read_start[k] .. read_start[k] + n_reads) (with their
 * listOfOverlapOffsets / listOfOrientations entries in offs / ors).  Any
 * output may be NULL.  Returns the number of edges; *n_reads_total the
 * length of reads/offs/ors.  Edges beyond edge_cap or reads beyond read_cap
 * are not written. */
uint64_t mgh_graph_unitig_edges(const mgh_graph* g, mgh_unitig_edge* edges, uint64_t edge_cap,
                                uint64_t* read_start, uint32_t* reads, uint16_t* offs, uint8_t* ors,
                                uint64_t read_cap, uint64_t* n_reads_total);

/* --- contig sequences: getStringInEdge + printGraph (OverlapGraph.cpp:2009-2041, 428-520)
 * The edges of a contracted or re-read handle as mg_build_contigs /
 * mgh_contigs_build take them (mg_contig_edge, include/mg_overlap.h), in u
 * order, each list in list order, `tail` filled from the reverse edge, with
 * their read lists gathered into reads / offs / ors (`first` indexes those).
 * all = 0: printGraph's contigs only, in its selection order (:460): src < dst,
 * and of a self-loop pair the edge created first (the rule mgh_graph_save_unitig
 * uses for the reference's pointer compare); all != 0: every edge.  Any output
 * may be NULL.  Returns the number of edges; *n_list the length of the lists.
 * Edges beyond edge_cap or list entries beyond list_cap are not written. */
uint64_t mgh_graph_contig_edges(const mgh_graph* g, int all, mg_contig_edge* edges, uint64_t edge_cap,
                                uint32_t* reads, uint16_t* offs, uint8_t* ors, uint64_t list_cap, uint64_t* n_list);
/* The host mirror of mg_build_contigs + mg_copy_contigs on packed words (ID
 * order, words_per_read words each): the definition of the pieces, in
 * O(output).  start: n_edges + 1 entries; out: cap bytes, written only when cap
 * >= the total; either may be NULL.  *total = length of all strings.  0 = ok;
 * -1 = bad arguments; -2 = an invalid piece or a read ID outside 1..n_reads:
 * err (err_cap bytes, NUL-terminated, optional) names the first such edge and
 * piece, and nothing is read out of range. */
int mgh_contigs_build(const uint64_t* words, const uint16_t* lens, uint64_t n_reads, uint32_t words_per_read,
                      const mg_contig_edge* edges, uint64_t n_edges, const uint32_t* reads, const uint16_t* offs,
                      const uint8_t* ors, uint64_t n_list, uint64_t* start, char* out, uint64_t cap, uint64_t* total,
                      char* err, uint64_t err_cap);
/* printGraph (:428-520) of a contracted or re-read handle: the .gdl file byte
 * for byte (header block, node lines, one edge line per contig, "}" without a
 * newline) and the contigs as FASTA, sorted by std::sort with compareEdges
 * (offset) and reversed, headers as :484 writes them (Flow and Coverage are 0
 * until flow exists), 100 bases per line.  start / strings: the strings of the
 * contigs in mgh_graph_contig_edges(all = 0) order as a device built them
 * (mg_copy_contigs), or NULL: the mirror spells them from words / lens.  The
 * cout statistics (:495-514) are not reproduced.  0 = ok; -1 = bad arguments or
 * a file cannot be written; -2 = an invalid piece (err as above). */
int mgh_graph_print(const mgh_graph* g, const uint64_t* words, const uint16_t* lens, uint64_t n_reads,
                    uint32_t words_per_read, const uint64_t* start, const char* strings, const char* gdl_path,
                    const char* fasta_path, char* err, uint64_t err_cap);

/* --- read placements, insert sizes, edge coverage (OverlapGraph.cpp:1048-1071,
 * 1124-1211, 2722-2792): the host mirrors of mg_build_placements +
 * mg_copy_placements, mg_insert_sizes and mg_edge_coverage (mg::placements_build,
 * mg::insert_sizes, mg::edge_coverage): linear restatements of the reference's
 * loops over the same arrays, with the same -2 errors.  err (err_cap bytes,
 * NUL-terminated, optional) gets the message. */
/* start: n_reads + 2 entries; out: cap records, written only when cap >= the
 * total; fwd_count: n_reads + 2 entries (forward placements per read ID).  Any
 * of them may be NULL.  0 = ok; -1 = bad arguments; -2 = a read ID outside
 * 1..n_reads. */
int mgh_placements_build(uint64_t n_reads, const mg_contig_edge* edges, uint64_t n_edges, const uint32_t* reads,
                         const uint16_t* offs, const uint8_t* ors, uint64_t n_list, uint64_t* start, mg_place* out,
                         uint64_t cap, uint32_t* fwd_count, uint64_t* n_places, char* err, uint64_t err_cap);
/* place_start / places: a placement CSR (n_reads + 2 starts); mate_start /
 * mates: a mate CSR in mg_copy_mate_pairs' layout; sums: 3 * n_datasets. */
int mgh_insert_sizes(uint64_t n_reads, const uint64_t* place_start, const mg_place* places,
                     const uint64_t* mate_start, const mg_mate* mates, uint32_t n_datasets, uint64_t max_distance,
                     uint64_t* sums, char* err, uint64_t err_cap);
/* lens[id - 1], freq[id - 1]; out: 3 * n_edges (count, sum, sum of squares over
 * the non-zero counters of each edge).  The forward-placement counts are those
 * of the same edges.  64-bit counters: no limit on an edge's frequency sum. */
int mgh_edge_coverage(const uint16_t* lens, uint64_t n_reads, const mg_contig_edge* edges, uint64_t n_edges,
                      const uint32_t* reads, const uint16_t* offs, const uint8_t* ors, uint64_t n_list,
                      const uint32_t* freq, uint64_t* out, char* err, uint64_t err_cap);
/* mean and sd from count, sum and sum of squares as the reference computes
 * them (:1196-1201, :2776-2786): mean = sum / count, variance = sumsq - 2 mean
 * sum + count mean^2 (mod 2^64), sd = (uint64)sqrt((double)(variance / count));
 * count == 0 gives 0, 0. */
void mgh_mean_sd(uint64_t count, uint64_t sum, uint64_t sumsq, uint64_t* mean, uint64_t* sd);
/* The read locations a contracted or re-read handle tracked (updateReadLocations
 * / removeReadLocations through the contraction) as placements: edge = the
 * edge's index in mgh_graph_contig_edges(all = 1); each read's records sorted by
 * (edge, distance, flags).  *n_reads (optional) = the reads the handle tracks (0
 * for a handle that tracked no locations); start: *n_reads + 2 entries; out:
 * cap records; either may be NULL.  Returns the number of records. */
uint64_t mgh_graph_read_locations(const mgh_graph* g, uint64_t* n_reads, uint64_t* start, mg_place* out,
                                  uint64_t cap);

/* --- mate-pair path support: findSupportByMatepairsAndMerge (OverlapGraph.cpp:1892-2002)
 * with findPathBetweenMatepairs (:1645-1730) and exploreGraph (:1781-1870).  The
 * definitions are in include/mg_overlap.h ("mate-pair path support"). */
/* twin[k] = the index of edge k's reverse edge, both in
 * mgh_graph_contig_edges(all = 1) order.  Returns the number of edges; entries
 * beyond cap are not written. */
uint64_t mgh_graph_edge_twins(const mgh_graph* g, uint32_t* twin, uint64_t cap);
/* mgh_graph_read_locations in the reference's list order: per read its forward
 * list (listOfEdgesForward / locationOnEdgeForward) in list order, then its
 * reverse list in list order -- the order findPathBetweenMatepairs walks. */
uint64_t mgh_graph_location_lists(const mgh_graph* g, uint64_t* n_reads, uint64_t* start, mg_place* out,
                                  uint64_t cap);
/* The host mirror of mg_mate_paths + mg_copy_mate_paths + mg_copy_path_pairs
 * over the same arrays (mg::mate_paths, mg::path_pairs), with the same -2
 * errors.  budget = work units per entry (0 = no limit; an entry above it is
 * MG_PATH_DEFERRED).  prior_* (all or none): the entries a device run over the
 * same input copied out; only its MG_PATH_DEFERRED entries are searched, the
 * others are taken as they are, so the result is the undeferred one.  status /
 * visits: one per mate entry; path_start: one more; path / flags: written only
 * when path_cap >= *n_path; pairs: written only when pair_cap >= *n_pairs;
 * counters[3] = noPathsFound, pathsFound, mpOnSameEdge.  Any output may be
 * NULL.  0 = ok; -1 = bad arguments; -2 = see mg_mate_paths. */
int mgh_mate_paths(uint64_t n_reads, const mg_contig_edge* edges, const uint32_t* twin, uint64_t n_edges,
                   const uint64_t* place_start, const mg_place* places, const uint64_t* mate_start,
                   const mg_mate* mates, const uint64_t* mean, const uint64_t* sd, uint32_t n_datasets,
                   uint64_t budget, const uint8_t* prior_status, const uint32_t* prior_visits,
                   const uint64_t* prior_start, const uint32_t* prior_path, const uint8_t* prior_flags,
                   uint8_t* status, uint32_t* visits, uint64_t* path_start, uint32_t* path, uint8_t* flags,
                   uint64_t path_cap, uint64_t* n_path, mg_pair_support* pairs, uint64_t pair_cap, uint64_t* n_pairs,
                   uint64_t* counters, char* err, uint64_t err_cap);
/* The second half (:1968-1992) on a contracted or re-read handle: std::sort of
 * the records by support (descending, pairedEdges::operator<), in the order
 * given, then mergeEdges of every pair that no earlier merge freed and whose
 * support is >= min_support (the reference: minimumSupport = 3).  The pairs'
 * edges index mgh_graph_contig_edges(all = 1) of the handle as it is now.
 * *merged = pairsOfEdgesMerged.  0 = ok; -1 = bad arguments; -4 = an
 * orientation pair mergeEdges rejects; -5 = a pair that would be merged is one
 * edge twice or an edge and its twin (the reference touches a removed edge
 * there): err names it and the graph is unchanged. */
int mgh_graph_merge_supported(mgh_graph* g, const mg_pair_support* pairs, uint64_t n, uint64_t min_support,
                              uint64_t* merged, char* err, uint64_t err_cap);

/* --- scaffolder: OverlapGraph::scaffolder (OverlapGraph.cpp:2120-2223) with
 * mergeEdgesDisconnected (:2386-2468).  The definitions of the scoring half
 * are in include/mg_overlap.h ("scaffolder"). */
/* The host mirror of mg_scaffold_pairs + mg_copy_scaffold_entries +
 * mg_copy_scaffold_pairs over the same arrays (mg::scaffold_pairs), with the
 * same -2 errors.  status: one MG_SCAF_* per mate entry; pairs: the first
 * min(pair_cap, *n_pairs) records in first-seen order, as
 * mg_copy_scaffold_pairs copies them (*n_pairs = all records, never more than
 * the mate entries); counters[5] = the entries of each status.  Any output may be NULL.  0 = ok; -1 = bad arguments; -2 = see
 * mg_scaffold_pairs. */
int mgh_scaffold_pairs(uint64_t n_reads, const uint32_t* twin, uint64_t n_edges, const uint64_t* place_start,
                       const mg_place* places, const uint64_t* mate_start, const mg_mate* mates,
                       const uint64_t* mean, const uint64_t* sd, uint32_t n_datasets, uint8_t* status,
                       mg_scaffold_pair* pairs, uint64_t pair_cap, uint64_t* n_pairs, uint64_t* counters, char* err,
                       uint64_t err_cap);
/* The merging half (:2197-2219) on a contracted or re-read handle: std::sort of
 * the records by support (descending, pairedEdges::operator<), in the order
 * given; then, for every record that no earlier merge freed and whose support
 * is >= min_support (the reference: 3): distance /= support, the reference's
 * "are supported" line, character for character (Flow is 0 on such a graph),
 * and mergeEdgesDisconnected (:2386-2468): mergeEdges when dst(edge1) ==
 * src(edge2) and matchEdgeType; otherwise findOverlap (:2368-2379) between the
 * two nodes' strings, strands as at :2396-2397, over the packed reads in ID
 * order (words: n_reads rows of words_per_read; lens), the merged lists of
 * mergeListDisconnected with its UINT16 truncations, both new edges inserted
 * and both old ones removed.  The pairs' edges index
 * mgh_graph_contig_edges(all = 1) of the handle as it is now.  lines: at most
 * lines_cap bytes are written, *lines_len = the bytes of all lines (at most 192
 * per merged pair).  *merged = pairsOfEdgesMerged.  0 = ok; -1 = bad
 * arguments; -4 = an orientation with no merged orientation; -5 = a pair that
 * would be merged is one edge twice or an edge and its twin: a dry run finds
 * it first, err names it and the graph is unchanged. */
int mgh_graph_merge_scaffold(mgh_graph* g, const mg_scaffold_pair* pairs, uint64_t n, uint64_t min_support,
                             const uint64_t* words, const uint16_t* lens, uint64_t n_reads, uint32_t words_per_read,
                             char* lines, uint64_t lines_cap, uint64_t* lines_len, uint64_t* merged, char* err,
                             uint64_t err_cap);

#ifdef __cplusplus
}
#endif
#endif /* MG_HOST_H_ */
