// mg_chains.hpp — INTERNAL: the safe chains of a freshly replayed graph on the
// host (the mirror of device/mg_chains.hip) and their validation.  Definitions:
// include/mg_overlap.h ("safe chains"); the apply step is
// UnitigGraph::apply_chains (mg_unitig.hpp).  See mg_chains.cpp.
#ifndef MG_CHAINS_HPP_
#define MG_CHAINS_HPP_
#include <cstdint>
#include <string>
#include <vector>

#include "mg_graph.hpp"
#include "mg_overlap.h"

namespace mg {

// matchEdgeType (OverlapGraph.cpp:19-26) in bits: t1 in {1, 3} pairs with t2 in
// {2, 3}, t1 in {0, 2} with t2 in {0, 1}
inline bool chain_match(uint8_t t1, uint8_t t2) { return (t1 & 1u) == ((t2 >> 1) & 1u); }

// the rounds mg_build_chains runs at most: ceil(log2(n_interior + 1)) + 1,
// lowered by `rounds` when that is not 0
uint32_t chain_round_cap(uint64_t n_interior, uint32_t rounds);

// The replayed graph as the CSR mg_build_chains takes: u order, each list in
// list order (mgh_graph_rows' order), twin = CSR index of the reverse edge.
// start: lists.size() + 1 entries.
void simple_csr(const std::vector<GraphEdge>& pool, const std::vector<std::vector<uint32_t>>& lists,
                std::vector<uint64_t>* start, std::vector<mg_chain_edge>* edges);

// what mg_build_chains refuses with -2; *err names the first offending entry
int chains_check_csr(const uint64_t* start, const mg_chain_edge* edges, uint64_t n_reads, uint64_t n_edges,
                     std::string* err);

struct ChainTable {
  std::vector<mg_chain> chains;
  std::vector<uint32_t> reads;
  std::vector<uint16_t> offs;
  std::vector<uint8_t> ors;
  uint64_t info[MG_CHAIN_INFO] = {};
};

// The definition of mg_build_chains' output: a serial walk from every half-edge
// of a non-interior node.  rounds as option "chain_rounds".  0 = ok, -2 = the
// CSR is malformed (chains_check_csr).
int chains_build(const uint64_t* start, const mg_chain_edge* edges, uint64_t n_reads, uint64_t n_edges,
                 uint32_t rounds, ChainTable* out, std::string* err);

}  // namespace mg
#endif  // MG_CHAINS_HPP_
