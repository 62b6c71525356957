// mg_contigs.hpp — INTERNAL: the host mirror of OverlapGraph::getStringInEdge
// (OverlapGraph.cpp:2009-2041) as pieces over the packed reads, and printGraph
// (:428-520): contig selection, the sort, the .gdl file and the FASTA file.
// The mirror defines what mg_build_contigs (include/mg_overlap.h) computes, is
// its checker, and is the path taken when no device is present.  See mg_contigs.cpp.
#ifndef MG_CONTIGS_HPP_
#define MG_CONTIGS_HPP_
#include <cstdint>
#include <string>
#include <vector>

#include "mg_overlap.h"
#include "mg_unitig.hpp"

namespace mg {

// The strings of `edges` in O(output): start gets n_edges + 1 entries, out the
// bases of all edges end to end.  0 = ok; -1 = bad arguments (a list range
// outside n_list); -2 = an invalid piece or a read ID outside 1..n_reads: err
// names the first such edge and piece, and nothing is read out of range.
// fill = false sizes only (start is complete, out stays empty).
int contigs_build(const uint64_t* words, const uint16_t* lens, uint64_t n_reads, uint32_t words_per_read,
                  const mg_contig_edge* edges, uint64_t n_edges, const uint32_t* reads, const uint16_t* offs,
                  const uint8_t* ors, uint64_t n_list, std::vector<uint64_t>* start, std::string* out,
                  std::string* err, bool fill = true);

struct ContigLists {
  std::vector<mg_contig_edge> edges;
  std::vector<uint32_t> pool;  // the edges' indices in UnitigGraph::pool
  std::vector<uint32_t> reads;
  std::vector<uint16_t> offs;
  std::vector<uint8_t> ors;
};
// The edges of the lists in u order, each in list order, with `tail` filled and
// their read lists gathered.  all = false: printGraph's contigs only (:460):
// src < dst, and of a self-loop pair the edge created first (the rule
// save_unitig uses for the reference's pointer compare).
void contig_edges(const UnitigGraph& u, bool all, ContigLists* out);

// printGraph's two files from the contigs `c` (selection order) and their
// strings: std::sort by offset (compareEdges), reverse, then the FASTA records;
// the .gdl header block, node lines, one edge line per contig in selection
// order and the closing brace.  0 = ok, -1 = cannot open / write.
int print_graph(const UnitigGraph& u, const ContigLists& c, const uint64_t* start, const char* bases,
                const char* gdl_path, const char* fasta_path);

}  // namespace mg
#endif  // MG_CONTIGS_HPP_
