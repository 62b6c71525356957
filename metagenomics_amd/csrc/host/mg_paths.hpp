// mg_paths.hpp — INTERNAL: the host mirror of mg_mate_paths (include/mg_overlap.h,
// "mate-pair path support"): findPathBetweenMatepairs and exploreGraph
// (OverlapGraph.cpp:1645-1730, :1781-1870) per mate entry, the pair list of
// findSupportByMatepairsAndMerge before its sort (:1903-1966), and the sort and
// merge loop after it (:1968-1992) on a UnitigGraph.  The mirror defines what
// the device computes, is its checker, finishes the entries the device
// deferred, and is the path taken when no device is present.  See mg_paths.cpp.
#ifndef MG_PATHS_HPP_
#define MG_PATHS_HPP_
#include <cstdint>
#include <string>
#include <vector>

#include "mg_overlap.h"
#include "mg_unitig.hpp"

namespace mg {

struct PathEntries {
  std::vector<uint8_t> status;   // per mate entry: MG_PATH_*
  std::vector<uint32_t> visits;  // per mate entry: work units
  std::vector<uint64_t> start;   // per mate entry (+ 1): where its path starts
  std::vector<uint32_t> path;    // edge indices
  std::vector<uint8_t> flags;    // per path position: (path[p], path[p + 1]) is supported
};

// the inputs of one call, as mg_mate_paths takes them
struct PathInput {
  uint64_t n_reads = 0;
  const mg_contig_edge* edges = nullptr;
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
// mg_mate_paths' order (err names it); 0 = ok
int paths_validate(const PathInput& in, std::string* err);
// Every mate entry (validated input).  budget = work units per entry (0 = no
// limit): an entry above it is MG_PATH_DEFERRED.  prior (optional): the
// entries of an earlier run over the same input; only its MG_PATH_DEFERRED
// entries are searched again, the others are taken as they are.
int mate_paths(const PathInput& in, uint64_t budget, const PathEntries* prior, PathEntries* out, std::string* err);
// listOfPairedEdges before the sort (:1929-1964) and the three counters
// (noPathsFound, pathsFound, mpOnSameEdge) over the entries in order
void path_pairs(const PathInput& in, const PathEntries& e, std::vector<mg_pair_support>* pairs, uint64_t* counters);

// :1968-1992 on u: std::sort by support (descending, operator< of pairedEdges),
// then mergeEdges of every pair not freed with support >= min_support.
// pairs' edges index pool_of (the pool entries of the edges the pairs were
// found on).  0 = ok; -1 = an edge index outside pool_of; -4 = mergeEdges met
// an orientation pair it rejects; -5 = a pair that would be merged is one edge
// twice or an edge and its twin (the reference touches a removed edge there):
// err names it and the graph is left as it was.
int merge_supported(UnitigGraph* u, const std::vector<uint32_t>& pool_of, const mg_pair_support* pairs, uint64_t n,
                    uint64_t min_support, uint64_t* merged, std::string* err);

}  // namespace mg
#endif  // MG_PATHS_HPP_
