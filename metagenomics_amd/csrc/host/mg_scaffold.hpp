// mg_scaffold.hpp — INTERNAL: the host mirror of mg_scaffold_pairs
// (include/mg_overlap.h, "scaffolder"): the scoring half of
// OverlapGraph::scaffolder (OverlapGraph.cpp:2120-2195), per mate entry its
// status and listOfPairedEdges before the sort (:2197).  The mirror defines what
// the device computes, is its checker, and is the path taken when no device is
// present.  And the merging half (:2197-2219 with mergeEdgesDisconnected,
// :2386-2468) on a UnitigGraph.  See mg_scaffold.cpp.
#ifndef MG_SCAFFOLD_HPP_
#define MG_SCAFFOLD_HPP_
#include <cstdint>
#include <string>
#include <vector>

#include "mg_overlap.h"
#include "mg_unitig.hpp"

namespace mg {

// the inputs of one call, as mg_scaffold_pairs takes them (both CSRs given)
struct ScaffoldInput {
  uint64_t n_reads = 0;
  const uint32_t* twin = nullptr;
  uint64_t n_edges = 0;
  const uint64_t* place_start = nullptr;
  const mg_place* places = nullptr;
  const uint64_t* mate_start = nullptr;
  const mg_mate* mates = nullptr;
  const uint64_t* mean = nullptr;
  const uint64_t* sd = nullptr;
  uint32_t n_datasets = 0;
};

// -1 = bad arguments or a malformed CSR; -2 = the first offender in
// mg_scaffold_pairs' order (err names it); 0 = ok
int scaffold_validate(const ScaffoldInput& in, std::string* err);
// Every mate entry in (A, j) order: status[t] = MG_SCAF_*, counters[5] = the
// entries of each status, pairs = the records in first-seen order (a hash map
// over the canonical key in place of the reference's linear search: the order
// of the records is the same).  Validates first.
int scaffold_pairs(const ScaffoldInput& in, std::vector<uint8_t>* status, std::vector<mg_scaffold_pair>* pairs,
                   uint64_t* counters, std::string* err);

// The merging half (:2197-2219) on u: std::sort by support (descending,
// operator< of pairedEdges) over the records in the order given, then for every
// record not freed with support >= min_support: distance /= support, the
// reference's line appended to *lines (Flow as the edges hold it, 0 on the
// .unitig graph), mergeEdgesDisconnected (mergeEdges when dst(edge1) ==
// src(edge2) and matchEdgeType; else findOverlap between the two nodes over the
// packed reads words / lens), and the isFreed marking over both edges and both
// twins.  pairs' edges index pool_of.  0 = ok; -1 = an edge index outside
// pool_of or a node outside the reads; -4 = an orientation with no merged
// orientation; -5 = a pair that would be merged is one edge twice or an edge
// and its twin: found by a dry run first, err names it, the graph is unchanged.
int merge_scaffold(UnitigGraph* u, const std::vector<uint32_t>& pool_of, const mg_scaffold_pair* pairs, uint64_t n,
                   uint64_t min_support, const uint64_t* words, const uint16_t* lens, uint64_t n_reads,
                   uint32_t words_per_read, std::string* lines, uint64_t* merged, std::string* err);

}  // namespace mg
#endif  // MG_SCAFFOLD_HPP_
