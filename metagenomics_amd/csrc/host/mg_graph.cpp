// mg_graph.cpp — host replay of OverlapGraph::buildOverlapGraphFromHashTable's
// exploration and transitive reduction on the discovery
// multiset the device produced.  Paths relative to /root/reference/MetaGenomics.
//
// The device computes every discovery of every read at once:
// the directed multiset M.  The reference builds its graph in a specific order
// instead: a queue per component (OverlapGraph.cpp:144-204), each read's
// discoveries inserted when it is explored (insertAllEdgesOfRead :529-565,
// skipping partners already explored), each list sorted by overlap offset with
// std::sort (:563, unstable), and Myers' transitive reduction interleaved
// (markTransitiveEdges :574-615, removeTransitiveEdges :623-661).  The list
// ORDER, and with it which edges the reduction removes, depends on that order.
// This file replays it exactly:
//   * D(A), A's discoveries in the reference's loop order (window j ascending,
//     then getListOfReads order = partner ID, then key o; HashTable.cpp:58-60),
//     are the rows of M with src = A: j and o follow from (orient, offset)
//     (:550-557); a self-overlap's rows come twice in M (discovery + twin of
//     the symmetric discovery), so each self row counts once;
//   * the exploration, insertEdge (:390-419), std::sort (same libstdc++
//     algorithm and comparator -> the same permutation) and the reduction run
//     as in the reference on compact edge records instead of Edge objects.
// tests/test_graph_replay.py pins the result (list order, numberOfNodes,
// numberOfEdges) to the reference's own graph (oracle/_ref/ref_harness bfs).
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <utility>
#include <vector>

#include "mg_graph.hpp"

namespace mg {

namespace {

enum : uint8_t { UNEXPLORED = 0, EXPLORED = 1, EXPLORED_AND_MARKED = 2 };  // nodeType (OverlapGraph.h:20-25)
enum : uint8_t { VACANT = 0, INPLAY = 1, ELIMINATED = 2 };                // markType (OverlapGraph.h:26-30)

inline uint8_t orient_to_key(uint8_t orient) {  // inverse of the switch at OverlapGraph.cpp:550-556
  return orient == 3 ? 0 : orient == 0 ? 1 : orient == 2 ? 2 : 3;
}

inline uint8_t twin_orient(uint8_t o) { return o == 0 ? 3 : (o == 3 ? 0 : o); }  // :841-855

}  // namespace

struct GraphReplay::Impl {
  const uint16_t* len = nullptr;
  uint64_t n = 0;
  uint32_t h = 0;
  std::vector<uint64_t> dstart;  // D(A) = disc[dstart[A] .. dstart[A+1])
  std::vector<Disc> disc;
  std::vector<uint8_t> state, marks;

  GraphReplay* g = nullptr;

  void run();
  int run_components(const Components& C, unsigned threads);
};

namespace {

// Where a walk puts the Edges it creates.  Serial replay: the end of the one
// pool, which grows.  Parallel replay: the component's own slice of the pool
// sized beforehand, so every index is final when it is written.
struct GrowingPool {
  std::vector<GraphEdge>& v;
  GraphEdge* data() const { return v.data(); }
  uint32_t size() const { return (uint32_t)v.size(); }
  bool push2(const GraphEdge& a, const GraphEdge& b) {
    v.push_back(a);
    v.push_back(b);
    return true;
  }
};

struct SlicePool {
  GraphEdge* base;    // the whole pool
  uint32_t cur, end;  // the slice left
  GraphEdge* data() const { return base; }
  uint32_t size() const { return cur; }
  bool push2(const GraphEdge& a, const GraphEdge& b) {
    if (end - cur < 2) return false;
    base[cur++] = a;
    base[cur++] = b;
    return true;
  }
};

// The reference's exploration of one component (OverlapGraph.cpp:144-204 for
// one seed) with its own counters.  Everything it reads or writes belongs to
// reads of the seed's component: state and marks bytes, graph[u] lists, pool
// entries it created.
template <class Pool>
struct Walk {
  const uint16_t* len;
  const uint64_t* dstart;
  const Disc* disc;
  uint8_t* state;
  uint8_t* marks;
  std::vector<std::vector<uint32_t>>& lists;
  Pool pool;
  uint64_t nodes = 0, edges = 0;  // this walk's share of numberOfNodes / numberOfEdges (may wrap; sums are exact)
  uint64_t explored = 0;          // reads explored that have discoveries
  bool bad = false;               // the slice or the queue was too small: the table was wrong

  uint16_t L(uint64_t id) const { return len[id - 1]; }

  void insert(uint32_t e) {  // insertEdge(Edge*) :390-400
    const uint32_t src = pool.data()[e].src;
    if (lists[src].empty()) nodes++;
    lists[src].push_back(e);
    edges++;
  }

  void insert_pair(uint32_t r1, uint32_t r2, uint8_t orient, uint16_t off) {  // insertEdge(Read*, ...) :407-419
    const uint32_t e1 = pool.size();
    const uint16_t rev = (uint16_t)(L(r2) + off - L(r1));  // UINT16 arithmetic (:410)
    if (!pool.push2({r1, r2, off, orient, 0, e1 + 1}, {r2, r1, rev, twin_orient(orient), 0, e1})) {
      bad = true;
      return;
    }
    insert(e1);
    insert(e1 + 1);
  }

  void explore(uint32_t r) {  // insertAllEdgesOfRead :529-565
    if (dstart[r + 1] > dstart[r]) explored++;
    for (uint64_t k = dstart[r]; k < dstart[r + 1]; ++k) {
      const Disc& d = disc[k];
      if (state[d.r2] != UNEXPLORED) continue;  // :546
      insert_pair(r, d.r2, d.orient, d.offset);
    }
    auto& lst = lists[r];
    if (!lst.empty()) {
      const GraphEdge* P = pool.data();
      std::sort(lst.begin(), lst.end(), [P](uint32_t a, uint32_t b) { return P[a].offset < P[b].offset; });
    }
  }

  void mark_transitive(uint32_t u) {  // markTransitiveEdges :574-615
    GraphEdge* P = pool.data();
    auto& lu = lists[u];
    for (uint32_t e : lu) marks[P[e].dst] = INPLAY;
    for (size_t i = 0; i < lu.size(); ++i) {
      const uint32_t v = P[lu[i]].dst;
      if (marks[v] != INPLAY) continue;
      const uint8_t t1 = P[lu[i]].orient;
      for (uint32_t e2 : lists[v]) {
        const uint32_t w = P[e2].dst;
        if (marks[w] != INPLAY) continue;
        const uint8_t t2 = P[e2].orient;
        if ((t1 == 0 || t1 == 2) && (t2 == 0 || t2 == 1))
          marks[w] = ELIMINATED;
        else if ((t1 == 1 || t1 == 3) && (t2 == 2 || t2 == 3))
          marks[w] = ELIMINATED;
      }
    }
    for (uint32_t e : lu) {
      if (marks[P[e].dst] == ELIMINATED) {
        P[e].trans = 1;
        P[P[e].rev].trans = 1;
      }
    }
    for (uint32_t e : lu) marks[P[e].dst] = VACANT;
    marks[u] = VACANT;
  }

  void remove_transitive(uint32_t u) {  // removeTransitiveEdges :623-661
    const GraphEdge* P = pool.data();
    auto& lu = lists[u];
    for (size_t i = 0; i < lu.size(); ++i) {
      if (!P[lu[i]].trans) continue;
      const uint32_t twin = P[lu[i]].rev;
      auto& lt = lists[P[twin].src];
      for (size_t k = 0; k < lt.size(); ++k) {
        if (lt[k] == twin) {  // move the last edge into its place
          lt[k] = lt.back();
          lt.pop_back();
          if (lt.empty()) nodes--;
          edges--;
          break;
        }
      }
    }
    size_t j = 0;
    for (size_t i = 0; i < lu.size(); ++i) {
      if (!P[lu[i]].trans)
        lu[j++] = lu[i];
      else
        edges--;
    }
    lu.resize(j);
    if (lu.empty()) nodes--;
  }

  // the seed's whole component through the queue (:146-203); queue holds qcap
  // entries: every read enters it at most once
  void component(uint32_t seed, uint32_t* queue, uint64_t qcap) {
    uint64_t head = 0, tail = 0;
    if (!qcap) {
      bad = true;
      return;
    }
    queue[tail++] = seed;
    while (head < tail && !bad) {
      const uint32_t r1 = queue[head++];
      if (state[r1] == UNEXPLORED) {
        explore(r1);
        state[r1] = EXPLORED;
      }
      if (lists[r1].empty()) continue;
      if (state[r1] == EXPLORED) {
        for (size_t a = 0; a < lists[r1].size(); ++a) {  // the list may grow inside explore()
          const uint32_t r2 = pool.data()[lists[r1][a]].dst;
          if (state[r2] == UNEXPLORED) {
            if (tail >= qcap) {
              bad = true;
              return;
            }
            queue[tail++] = r2;
            explore(r2);
            state[r2] = EXPLORED;
          }
        }
        mark_transitive(r1);
        state[r1] = EXPLORED_AND_MARKED;
      }
      if (state[r1] == EXPLORED_AND_MARKED) {
        for (size_t a = 0; a < lists[r1].size(); ++a) {
          const uint32_t r2 = pool.data()[lists[r1][a]].dst;
          if (state[r2] != EXPLORED) continue;
          for (size_t b = 0; b < lists[r2].size(); ++b) {
            const uint32_t r3 = pool.data()[lists[r2][b]].dst;
            if (state[r3] == UNEXPLORED) {
              if (tail >= qcap) {
                bad = true;
                return;
              }
              queue[tail++] = r3;
              explore(r3);
              state[r3] = EXPLORED;
            }
          }
          mark_transitive(r2);
          state[r2] = EXPLORED_AND_MARKED;
        }
        remove_transitive(r1);
      }
    }
  }
};

}  // namespace

void GraphReplay::Impl::run() {  // OverlapGraph.cpp:144-204
  state.assign(n + 1, UNEXPLORED);
  marks.assign(n + 1, VACANT);
  std::vector<uint32_t> queue(n + 1, 0);
  Walk<GrowingPool> w{len, dstart.data(), disc.data(), state.data(), marks.data(), g->lists, GrowingPool{g->pool}};
  for (uint64_t seed = 1; seed <= n; ++seed) {
    if (state[seed] != UNEXPLORED) continue;
    w.component((uint32_t)seed, queue.data(), queue.size());
  }
  g->nodes = w.nodes;
  g->edges = w.edges;
}

// The same graph, component by component on several threads.  The outer loop
// above meets the components in ascending root and finishes one before it
// looks for the next, so the pool is the components' pools concatenated in
// that order; a component creates n_disc + n_self pool entries (a non-self
// discovery sits in two lists and is inserted from whichever end is explored
// first, a self discovery in one and makes two entries).  Reads outside the
// table have no discoveries: exploring them changes nothing but their state.
// Each walk must use up its slice and explore its n_reads reads exactly, or
// the table was not the lists' (-4): a label class made of two components
// passes every static check.
int GraphReplay::Impl::run_components(const Components& C, unsigned threads) {
  const size_t nc = C.comps.size();
  std::vector<uint64_t> at(nc + 1, 0);
  for (size_t i = 0; i < nc; ++i) {
    const mg_comp& c = C.comps[i];
    if (c.root < 1 || c.root > n || (i && c.root <= C.comps[i - 1].root)) return -4;
    at[i + 1] = at[i] + c.n_disc + c.n_self;
  }
  if (at[nc] >> 32) return -4;  // (pool indices are 32-bit)
  state.assign(n + 1, UNEXPLORED);
  marks.assign(n + 1, VACANT);
  g->pool.resize(at[nc]);
  std::vector<uint32_t> order(nc);
  for (size_t i = 0; i < nc; ++i) order[i] = (uint32_t)i;
  std::stable_sort(order.begin(), order.end(),
                   [&](uint32_t a, uint32_t b) { return C.comps[a].n_disc > C.comps[b].n_disc; });
  const unsigned T = (unsigned)std::max<size_t>(1, std::min<size_t>(threads, nc));
  std::atomic<size_t> next{0};
  std::atomic<bool> bad{false};
  std::vector<uint64_t> nodes(T, 0), edges(T, 0);
  auto work = [&](unsigned t) {
    std::vector<uint32_t> queue;
    uint64_t tn = 0, te = 0;
    for (;;) {
      const size_t k = next.fetch_add(1, std::memory_order_relaxed);
      if (k >= nc || bad.load(std::memory_order_relaxed)) break;
      const size_t i = order[k];
      const mg_comp& c = C.comps[i];
      if (queue.size() < c.n_reads) queue.resize(c.n_reads);
      Walk<SlicePool> w{len,          dstart.data(), disc.data(), state.data(),
                        marks.data(), g->lists,      SlicePool{g->pool.data(), (uint32_t)at[i], (uint32_t)at[i + 1]}};
      if (state[c.root] == UNEXPLORED) w.component(c.root, queue.data(), c.n_reads);
      if (w.bad || w.pool.cur != w.pool.end || w.explored != c.n_reads) {
        bad.store(true, std::memory_order_relaxed);
        break;
      }
      tn += w.nodes;
      te += w.edges;
    }
    nodes[t] = tn;
    edges[t] = te;
  };
  if (T == 1) {
    work(0);
  } else {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < T; ++t) th.emplace_back(work, t);
    for (auto& x : th) x.join();
  }
  if (bad.load()) return -4;
  for (unsigned t = 0; t < T; ++t) {
    g->nodes += nodes[t];
    g->edges += edges[t];
  }
  return 0;
}

GraphReplay::GraphReplay() : impl(new Impl) { impl->g = this; }
GraphReplay::~GraphReplay() { delete impl; }

int Discoveries::build(const mg_edge* rows, uint64_t n_rows, const uint16_t* lens, uint64_t n_reads, uint32_t h) {
  // D(A) from the rows with src = A (counting sort by src)
  start.assign(n_reads + 2, 0);
  for (uint64_t i = 0; i < n_rows; ++i) {
    if (rows[i].src < 1 || rows[i].src > n_reads || rows[i].dst < 1 || rows[i].dst > n_reads) return -1;
    start[rows[i].src + 1]++;
  }
  for (uint64_t a = 1; a <= n_reads + 1; ++a) start[a] += start[a - 1];
  disc.assign(n_rows, Disc{});
  {
    std::vector<uint64_t> at(start.begin(), start.end() - 1);
    for (uint64_t i = 0; i < n_rows; ++i) {
      const mg_edge& r = rows[i];
      const uint8_t o = orient_to_key(r.orient);
      const int64_t n1 = lens[r.src - 1];
      // window j: offset = j for o = 0, 2; offset = n1 - h - j for o = 1, 3 (:550-557)
      const int64_t j = (o == 0 || o == 2) ? r.offset : n1 - (int64_t)h - r.offset;
      if (j < 1 || j >= n1 - (int64_t)h) return -2;
      disc[at[r.src]++] = Disc{(uint32_t)j, r.dst, o, r.orient, r.offset};
    }
  }
  // loop order; each self row is present twice in M and counts once
  for (uint64_t a = 1; a <= n_reads; ++a) {
    const uint64_t lo = start[a], hi = start[a + 1];
    std::sort(disc.begin() + lo, disc.begin() + hi, [](const Disc& x, const Disc& y) {
      if (x.j != y.j) return x.j < y.j;
      if (x.r2 != y.r2) return x.r2 < y.r2;
      return x.o < y.o;
    });
  }
  uint64_t w = 0;
  std::vector<uint64_t> ns(n_reads + 2, 0);
  for (uint64_t a = 1; a <= n_reads; ++a) {
    ns[a] = w;
    const uint64_t lo = start[a], hi = start[a + 1];
    for (uint64_t k = lo; k < hi; ++k) {
      const Disc& d = disc[k];
      if (d.r2 == a) {
        if (k + 1 >= hi || std::memcmp(&disc[k + 1], &d, sizeof(Disc)) != 0) return -3;  // must come in pairs
        disc[w++] = d;
        ++k;
      } else {
        disc[w++] = d;
      }
    }
  }
  ns[n_reads + 1] = w;
  ns[0] = 0;
  start.swap(ns);
  disc.resize(w);
  return 0;
}

int Discoveries::from_lists(const uint64_t* start_in, const mg_disc* d, uint64_t n_disc, const uint16_t* lens,
                            uint64_t n_reads, uint32_t h) {
  if (start_in[0] != 0 || start_in[1] != 0) return -1;
  for (uint64_t a = 1; a <= n_reads; ++a)
    if (start_in[a + 1] < start_in[a]) return -1;
  if (start_in[n_reads + 1] != n_disc) return -1;
  start.assign(start_in, start_in + n_reads + 2);
  disc.assign(n_disc, Disc{});
  // one pass over the records of reads [lo, hi): Disc with j recomputed, each
  // list strictly increasing in (j, dst, o); the first bad read and its code
  auto pass = [&](uint64_t lo, uint64_t hi, uint64_t* bad_read, int* bad_rc) {
    for (uint64_t a = lo; a < hi; ++a) {
      const int64_t n1 = lens[a - 1];
      int rc = 0;
      for (uint64_t k = start[a]; k < start[a + 1] && !rc; ++k) {
        const mg_disc& r = d[k];
        if (r.dst < 1 || r.dst > n_reads) {
          rc = -1;
          break;
        }
        if (r.orient > 3 || r.o != orient_to_key(r.orient)) {
          rc = -2;
          break;
        }
        const int64_t j = (r.o == 0 || r.o == 2) ? r.offset : n1 - (int64_t)h - r.offset;
        if (j < 1 || j >= n1 - (int64_t)h) {
          rc = -2;
          break;
        }
        disc[k] = Disc{(uint32_t)j, r.dst, r.o, r.orient, r.offset};
        if (k > start[a]) {  // the loop order is total
          const Disc& p = disc[k - 1];
          const Disc& c = disc[k];
          const bool less = p.j != c.j ? p.j < c.j : p.r2 != c.r2 ? p.r2 < c.r2 : p.o < c.o;
          if (!less) rc = -3;
        }
      }
      if (rc) {
        *bad_read = a;
        *bad_rc = rc;
        return;
      }
    }
  };
  // the reads are independent: threads take ranges of about equal record counts
  const unsigned hw = std::thread::hardware_concurrency();
  const uint64_t T = n_disc < (1u << 20) ? 1 : std::max<uint64_t>(1, std::min<uint64_t>(16, hw ? hw : 1));
  std::vector<uint64_t> cut(T + 1, 1), bad_read(T, 0);
  std::vector<int> bad_rc(T, 0);
  cut[T] = n_reads + 1;
  for (uint64_t t = 1; t < T; ++t)  // first read whose list starts at or after record t * n_disc / T
    cut[t] = std::max<uint64_t>(
        cut[t - 1], (uint64_t)(std::lower_bound(start.begin() + 1, start.begin() + n_reads + 1, t * (n_disc / T)) -
                               start.begin()));
  if (T == 1) {
    pass(1, n_reads + 1, &bad_read[0], &bad_rc[0]);
  } else {
    std::vector<std::thread> th;
    for (uint64_t t = 0; t < T; ++t) th.emplace_back(pass, cut[t], cut[t + 1], &bad_read[t], &bad_rc[t]);
    for (auto& x : th) x.join();
  }
  for (uint64_t t = 0; t < T; ++t)  // (ranges ascend: the first bad read overall)
    if (bad_rc[t]) return bad_rc[t];
  return 0;
}

int GraphReplay::build(const mg_edge* rows, uint64_t n_rows, const uint16_t* lens, uint64_t n_reads, uint32_t h) {
  Discoveries D;
  const int rc = D.build(rows, n_rows, lens, n_reads, h);
  if (rc) return rc;
  return build_from(std::move(D), lens, n_reads, h);
}

int GraphReplay::build_from(Discoveries&& D, const uint16_t* lens, uint64_t n_reads, uint32_t h,
                            const Components* comps, unsigned threads) {
  Impl& I = *impl;
  I.len = lens;
  I.n = n_reads;
  I.h = h;
  pool.clear();
  lists.assign(n_reads + 1, {});
  nodes = edges = 0;
  I.dstart.swap(D.start);
  I.disc.swap(D.disc);
  if (comps && threads > 1) {
    const int rc = I.run_components(*comps, threads);
    if (rc) {  // no half-built graph
      pool.clear();
      lists.assign(n_reads + 1, {});
      nodes = edges = 0;
    }
    return rc;
  }
  pool.reserve(I.disc.size());
  I.run();
  return 0;
}

unsigned replay_threads() {
  if (const char* v = std::getenv("MG_REPLAY_THREADS"))
    if (*v) return (unsigned)std::max(1, std::atoi(v));
  const unsigned hw = std::thread::hardware_concurrency();
  return std::max(1u, std::min(16u, hw ? hw : 1u));
}

namespace {

// fn(t, lo, hi) over the reads [1, n_reads] cut into ranges of about equal record counts
template <class F>
void over_reads(const std::vector<uint64_t>& start, uint64_t n_reads, F fn) {
  const uint64_t n_disc = start[n_reads + 1];
  const unsigned hw = std::thread::hardware_concurrency();
  const uint64_t T = n_disc < (1u << 20) ? 1 : std::max<uint64_t>(1, std::min<uint64_t>(16, hw ? hw : 1));
  std::vector<uint64_t> cut(T + 1, 1);
  cut[T] = n_reads + 1;
  for (uint64_t t = 1; t < T; ++t)
    cut[t] = std::max<uint64_t>(
        cut[t - 1], (uint64_t)(std::lower_bound(start.begin() + 1, start.begin() + n_reads + 1, t * (n_disc / T)) -
                               start.begin()));
  if (T == 1) {
    fn(0, cut[0], cut[1]);
    return;
  }
  std::vector<std::thread> th;
  for (uint64_t t = 0; t < T; ++t) th.emplace_back(fn, t, cut[t], cut[t + 1]);
  for (auto& x : th) x.join();
}

inline void add_relaxed(uint32_t* p, uint32_t x) { __atomic_fetch_add(p, x, __ATOMIC_RELAXED); }

}  // namespace

int Components::build(const Discoveries& D) {
  const uint64_t n = D.start.size() - 2;
  label.assign(n + 1, 0);
  comps.clear();
  std::vector<uint32_t>& parent = label;
  for (uint64_t a = 0; a <= n; ++a) parent[a] = (uint32_t)a;
  auto find = [&](uint32_t v) {
    while (parent[v] != v) {
      parent[v] = parent[parent[v]];
      v = parent[v];
    }
    return v;
  };
  for (uint64_t a = 1; a <= n; ++a)
    for (uint64_t k = D.start[a]; k < D.start[a + 1]; ++k) {
      const uint32_t b = D.disc[k].r2;
      if (b < 1 || b > n) return -1;
      if (b >= a) continue;  // (self; or the other list's record)
      const uint32_t ra = find((uint32_t)a), rb = find(b);
      if (ra != rb) parent[std::max(ra, rb)] = std::min(ra, rb);  // roots are minima
    }
  for (uint64_t a = 1; a <= n; ++a) label[a] = label[label[a]];  // (ascending: label[label[a]] is final)
  std::vector<uint32_t> slot(n + 1, 0);
  for (uint64_t a = 1; a <= n; ++a)
    if (label[a] == a && D.start[a + 1] > D.start[a]) {
      slot[a] = (uint32_t)comps.size();
      comps.push_back(mg_comp{(uint32_t)a, 0, 0, 0});
    }
  for (uint64_t a = 1; a <= n; ++a) {
    const uint64_t d = D.start[a + 1] - D.start[a];
    if (!d) continue;
    mg_comp& c = comps[slot[label[a]]];
    c.n_reads++;
    c.n_disc += (uint32_t)d;
    for (uint64_t k = D.start[a]; k < D.start[a + 1]; ++k) c.n_self += D.disc[k].r2 == a;
  }
  return 0;
}

int Components::from_device(const uint32_t* label_in, const mg_comp* comps_in, uint64_t n_comp, const Discoveries& D) {
  const uint64_t n = D.start.size() - 2, n_disc = D.start[n + 1];
  label.clear();
  comps.clear();
  if (!label_in || (n_comp && !comps_in) || n_comp > n) return n_comp > n ? -4 : -1;
  if (label_in[0] != 0) return -4;
  uint64_t total = 0;
  for (uint64_t i = 0; i < n_comp; ++i) {
    const mg_comp& c = comps_in[i];
    if (c.root < 1 || c.root > n) return -1;
    if (i && c.root <= comps_in[i - 1].root) return -4;
    if (label_in[c.root] != c.root) return -4;
    total += c.n_disc;
  }
  if (total != n_disc) return -4;
  // one pass per thread over its reads: the labels are roots, no greater than
  // the read, the read itself where the list is empty, and equal at both ends
  // of every record; reads / records / self records recounted per label (a run
  // of equal labels is added at once)
  std::vector<uint32_t> acc(3 * (n + 1), 0);
  uint32_t *acc_reads = acc.data(), *acc_disc = acc.data() + (n + 1), *acc_self = acc.data() + 2 * (n + 1);
  std::vector<int> rcs(16, 0);
  over_reads(D.start, n, [&](uint64_t t, uint64_t lo, uint64_t hi) {
    uint32_t run = 0, r_reads = 0, r_disc = 0, r_self = 0;
    auto flush = [&] {
      if (run && r_reads) {
        add_relaxed(&acc_reads[run], r_reads);
        add_relaxed(&acc_disc[run], r_disc);
        if (r_self) add_relaxed(&acc_self[run], r_self);
      }
      r_reads = r_disc = r_self = 0;
    };
    int rc = 0;
    for (uint64_t a = lo; a < hi && !rc; ++a) {
      const uint32_t la = label_in[a];
      if (la < 1 || la > n) {
        rc = -1;
        break;
      }
      const uint64_t d = D.start[a + 1] - D.start[a];
      if (la > a || label_in[la] != la || (!d && la != a)) {
        rc = -4;
        break;
      }
      if (!d) continue;
      if (la != run) {
        flush();
        run = la;
      }
      r_reads++;
      r_disc += (uint32_t)d;
      for (uint64_t k = D.start[a]; k < D.start[a + 1]; ++k) {
        const uint32_t b = D.disc[k].r2;
        if (b < 1 || b > n) {
          rc = -1;
          break;
        }
        if (label_in[b] != la) {
          rc = -4;
          break;
        }
        r_self += b == a;
      }
    }
    flush();
    rcs[t] = rc;
  });
  for (int rc : rcs)
    if (rc) return rc;
  for (uint64_t i = 0; i < n_comp; ++i) {
    const mg_comp& c = comps_in[i];
    if (!c.n_disc || acc_reads[c.root] != c.n_reads || acc_disc[c.root] != c.n_disc || acc_self[c.root] != c.n_self)
      return -4;
  }
  // (the table's records sum to the list total and each entry equals its
  // label's recount: no label with records is missing from the table)
  label.assign(label_in, label_in + n + 1);
  comps.assign(comps_in, comps_in + n_comp);
  return 0;
}

}  // namespace mg
