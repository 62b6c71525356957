// mg_graph.hpp — INTERNAL: host replay of the reference's graph construction
// order (exploration + transitive reduction) on the device's discovery rows.
// See mg_graph.cpp.
#ifndef MG_GRAPH_HPP_
#define MG_GRAPH_HPP_
#include <cstdint>
#include <vector>

#include "mg_overlap.h"

namespace mg {

struct GraphEdge {  // Edge (Edge.h:18-44) without the contraction fields
  uint32_t src, dst;
  uint16_t offset;
  uint8_t orient;
  uint8_t trans;  // transitiveRemovalFlag
  uint32_t rev;   // reverseEdge (index into the pool)
};

// One discovery of read A: window j, partner r2, key o (HashTable's 2-bit
// orientation) and the edge insertEdge(A, r2, orient, offset) would create
// (OverlapGraph.cpp:550-557).
struct Disc {
  uint32_t j;
  uint32_t r2;
  uint8_t o;
  uint8_t orient;
  uint16_t offset;
};

// D(A) for every read A, in insertAllEdgesOfRead's loop order (window j
// ascending, then getListOfReads order: partner ID, then key o;
// OverlapGraph.cpp:534-547, HashTable.cpp:58-60), from the device's directed
// discovery multiset.  D(A) = disc[start[A] .. start[A + 1]).
struct Discoveries {
  std::vector<uint64_t> start;
  std::vector<Disc> disc;
  // rows: the full directed multiset (any order); lens[id - 1]; h = l - 1.
  // 0 = ok, < 0 = rows inconsistent with the lengths / h.
  int build(const mg_edge* rows, uint64_t n_rows, const uint16_t* lens, uint64_t n_reads, uint32_t h);
  // The same lists from the device's grouping (mg_build_discoveries +
  // mg_copy_discoveries): start_in has n_reads + 2 entries.  One linear pass
  // fills Disc (j recomputed) and validates what it is given: 0 = ok, -1 start
  // not monotone from 0 / start[n_reads + 1] != n_disc / a dst outside
  // 1..n_reads, -2 a window j outside [1, len - h) or a key o that does not
  // belong to the orientation, -3 a list not strictly increasing in (j, dst, o).
  int from_lists(const uint64_t* start_in, const mg_disc* d, uint64_t n_disc, const uint16_t* lens, uint64_t n_reads,
                 uint32_t h);
};

// The connected components of the lists (two reads are connected when a record
// joins them): label[A] = the smallest read ID connected to A (A itself for an
// empty list; label[0] = 0), and the components that hold records in strictly
// ascending root.  The reference explores one component at a time from its
// root (OverlapGraph.cpp:144-204), so they can be replayed independently.
struct Components {
  std::vector<uint32_t> label;
  std::vector<mg_comp> comps;
  // host union-find over the lists; 0 = ok, -1 = a dst outside 1..n_reads
  int build(const Discoveries& D);
  // The device's arrays (mg_build_components + mg_copy_components): label_in
  // has n_reads + 1 entries.  Validated in linear, threaded passes: roots
  // strictly ascending with label[root] == root; label[A] <= A and a root, A
  // itself where D(A) is empty; label[dst] == label[A] for every record; each
  // entry's n_reads / n_disc / n_self equal to a recount under the labels; the
  // n_disc sum equal to the list total.  0 = ok, -1 = an ID outside
  // 1..n_reads, -4 = not the lists' components.  (Two components under one
  // label pass: the replay finds that, see build_from.)
  int from_device(const uint32_t* label_in, const mg_comp* comps_in, uint64_t n_comp, const Discoveries& D);
};

// host threads a parallel replay takes by default: min(16, hardware threads),
// or the environment variable MG_REPLAY_THREADS
unsigned replay_threads();

class GraphReplay {
 public:
  GraphReplay();
  ~GraphReplay();
  GraphReplay(const GraphReplay&) = delete;
  GraphReplay& operator=(const GraphReplay&) = delete;
  // rows: the full directed discovery multiset (any order); lens[id - 1]; h = l - 1.
  // 0 = ok, < 0 = rows inconsistent with the lengths / h.
  int build(const mg_edge* rows, uint64_t n_rows, const uint16_t* lens, uint64_t n_reads, uint32_t h);
  // The same replay on lists already grouped (Discoveries::build / from_lists).
  // comps == nullptr or threads <= 1: the serial replay, always 0.  Otherwise
  // the components are replayed by `threads` workers, each into its own slice
  // of the pool (sized n_disc + n_self per component, in root order): the same
  // pool, lists and counters.  -4 = a walk did not create exactly its slice or
  // explore exactly its n_reads reads: the table is not the lists' (nothing is
  // built then).
  int build_from(Discoveries&& D, const uint16_t* lens, uint64_t n_reads, uint32_t h,
                 const Components* comps = nullptr, unsigned threads = 1);
  std::vector<GraphEdge> pool;               // every Edge ever created (removed ones stay, unlisted)
  std::vector<std::vector<uint32_t>> lists;  // graph[u]: pool indices in list order
  uint64_t nodes = 0, edges = 0;             // numberOfNodes, numberOfEdges

 private:
  struct Impl;
  Impl* impl;
};

}  // namespace mg
#endif  // MG_GRAPH_HPP_
