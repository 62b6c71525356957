// mg_places.hpp — INTERNAL: the host mirrors of the placement calls
// (include/mg_overlap.h): OverlapGraph::updateReadLocations
// (OverlapGraph.cpp:1048-1071) over every edge, the quadruple loop of
// calculateMeanAndSdOfInsertSize (:1140-1179) and getBaseByBaseCoverage's
// per-base vector (:2724-2788), as linear restatements of the reference's
// statements.  They take the arrays the device calls take, define what those
// compute, are their checkers and run where no device is present.
// See mg_places.cpp.
#ifndef MG_PLACES_HPP_
#define MG_PLACES_HPP_
#include <cstdint>
#include <string>
#include <vector>

#include "mg_overlap.h"

namespace mg {

// updateReadLocations of edges 0 .. n_edges - 1 in order: start gets n_reads + 2
// entries, out the records of read A at [start[A], start[A + 1]) in ascending
// (edge index, list position), fwd_count[A] (n_reads + 2 entries) the forward
// ones.  0 = ok; -1 = bad arguments or a list range outside n_list; -2 = a read
// ID outside 1..n_reads (err names the first such edge and entry).
int placements_build(uint64_t n_reads, const mg_contig_edge* edges, uint64_t n_edges, const uint32_t* reads,
                     const uint16_t* offs, const uint8_t* ors, uint64_t n_list, std::vector<uint64_t>* start,
                     std::vector<mg_place>* out, std::vector<uint32_t>* fwd_count, std::string* err);

// :1140-1179 for all datasets in one pass over the reads: sums[3 d .. 3 d + 2] =
// count, sum and sum of squares of the insert sizes of dataset d.  mate_start:
// n_reads + 2 entries.  0 = ok; -1 = bad arguments; -2 = a mate entry whose
// dataset >= n_datasets or whose owner or mate ID lies outside 1..n_reads.
int insert_sizes(uint64_t n_reads, const uint64_t* place_start, const mg_place* places, const uint64_t* mate_start,
                 const mg_mate* mates, uint32_t n_datasets, uint64_t max_distance, uint64_t* sums, std::string* err);

// getBaseByBaseCoverage of every edge: out[3 k .. 3 k + 2] = count, sum and sum
// of squares over the non-zero counters.  fwd_count as placements_build leaves
// it.  0 = ok; -1 = bad arguments (an offset of 2^40 or more included); -2 = an
// invalid edge (err names it): nothing is written.
int edge_coverage(const uint16_t* lens, uint64_t n_reads, const mg_contig_edge* edges, uint64_t n_edges,
                  const uint32_t* reads, const uint16_t* offs, const uint8_t* ors, uint64_t n_list,
                  const uint32_t* fwd_count, const uint32_t* freq, uint64_t* out, std::string* err);

// mean = sum / count; variance = sum over the values of (mean - x)^2 in wrapping
// 64-bit arithmetic = sumsq - 2 mean sum + count mean^2; sd = sqrt(variance /
// count) through a double, as :1196-1201 and :2776-2786 compute them; count == 0
// gives 0, 0.
void mean_sd(uint64_t count, uint64_t sum, uint64_t sumsq, uint64_t* mean, uint64_t* sd);

}  // namespace mg
#endif  // MG_PLACES_HPP_
