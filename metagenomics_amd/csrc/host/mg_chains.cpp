// mg_chains.cpp — safe chains of a freshly replayed graph: the host mirror of
// device/mg_chains.hip (chains_build, the definition of its output) and the
// apply step (UnitigGraph::apply_chains) that contracts a validated table of
// them before the reference's loop runs.
//
// Why it is exact ("Safe chains"): during a
// contractCompositePaths pass (OverlapGraph.cpp:669-696) the new edge of
// mergeEdges (:702-753) is appended to its end's list and removeEdge (:863-896)
// then swaps it into the slot of the edge it replaces, so the end lists keep
// their order and length and no degree changes; mergeList (:760-785) is
// associative, so the edge a fully contracted chain a -> n1 -> .. -> nk -> b
// leaves is a function of the chain alone.  The one order-dependent test is
// isEdgePresent(a, b) (:679), and for a safe chain it is false at every node in
// any order.  So contracting any subset of the safe chains first and running the
// loop unchanged, with the contracted nodes credited to the first pass's counter,
// gives the reference's lists, read lists, location lists, counters and
// iteration count.  The apply step therefore validates soundness only (every
// claimed chain is a chain and is safe), never completeness.
#include "mg_chains.hpp"

#include <algorithm>
#include <atomic>
#include <thread>

#include "mg_unitig.hpp"

namespace mg {

namespace {

inline uint8_t twin_orient(uint8_t o) { return o == 0 ? 3 : (o == 3 ? 0 : o); }  // :841-855

inline uint32_t ceil_log2(uint64_t x) {  // x >= 1
  uint32_t r = 0;
  while (r < 63 && (1ull << r) < x) ++r;
  return r;
}

}  // namespace

uint32_t chain_round_cap(uint64_t n_interior, uint32_t rounds) {
  const uint32_t full = ceil_log2(n_interior + 1) + 1;
  return rounds ? std::min(rounds, full) : full;
}

void simple_csr(const std::vector<GraphEdge>& pool, const std::vector<std::vector<uint32_t>>& lists,
                std::vector<uint64_t>* start, std::vector<mg_chain_edge>* edges) {
  const size_t n = lists.empty() ? 0 : lists.size() - 1;
  start->assign(n + 2, 0);
  for (size_t u = 1; u <= n; ++u) (*start)[u + 1] = (*start)[u] + lists[u].size();
  std::vector<uint32_t> at(pool.size(), UINT32_MAX);  // pool entry -> CSR index
  for (size_t u = 1; u <= n; ++u)
    for (size_t p = 0; p < lists[u].size(); ++p) at[lists[u][p]] = (uint32_t)((*start)[u] + p);
  edges->resize((*start)[n + 1]);
  for (size_t u = 1; u <= n; ++u)
    for (size_t p = 0; p < lists[u].size(); ++p) {
      const GraphEdge& x = pool[lists[u][p]];
      (*edges)[(*start)[u] + p] = mg_chain_edge{x.dst, at[x.rev], x.offset, x.orient, 0};
    }
}

int chains_check_csr(const uint64_t* start, const mg_chain_edge* edges, uint64_t N, uint64_t E, std::string* err) {
  auto fail = [&](const std::string& s) {
    if (err) *err = s + " (-2)";
    return -2;
  };
  if (N >= (1ull << 31) || E >= (1ull << 32)) return fail("2^31 reads or 2^32 half-edges and more are not supported");
  if (start[0] != 0 || start[1] != 0) return fail("start[0] and start[1] must be 0");
  for (uint64_t v = 1; v <= N; ++v)
    if (start[v + 1] < start[v] || start[v + 1] > E)
      return fail("start[" + std::to_string(v + 1) + "] decreases or exceeds the " + std::to_string(E) + " half-edges");
  if (start[N + 1] != E) return fail("start[n_reads + 1] is not the number of half-edges");
  for (uint64_t v = 1; v <= N; ++v)
    for (uint64_t e = start[v]; e < start[v + 1]; ++e) {
      const mg_chain_edge& x = edges[e];
      const std::string who =
          "half-edge " + std::to_string(e) + " (read " + std::to_string(v) + ", position " + std::to_string(e - start[v]) + ")";
      if (x.dst < 1 || x.dst > N) return fail(who + ": dst " + std::to_string(x.dst) + " outside 1.." + std::to_string(N));
      if (x.twin < start[x.dst] || x.twin >= start[x.dst + 1])
        return fail(who + ": twin " + std::to_string(x.twin) + " outside the list of its dst " + std::to_string(x.dst));
      if (edges[x.twin].twin != e) return fail(who + ": twin[twin] is " + std::to_string(edges[x.twin].twin));
      if (edges[x.twin].dst != v) return fail(who + ": its twin's dst is " + std::to_string(edges[x.twin].dst));
    }
  return 0;
}

int chains_build(const uint64_t* start, const mg_chain_edge* edges, uint64_t N, uint64_t E, uint32_t rounds,
                 ChainTable* out, std::string* err) {
  *out = ChainTable{};
  const int rc = chains_check_csr(start, edges, N, E, err);
  if (rc) return rc;
  std::vector<uint8_t> interior(N + 2, 0);
  uint64_t n_interior = 0;
  for (uint64_t v = 1; v <= N; ++v) {
    if (start[v + 1] - start[v] != 2) continue;
    const mg_chain_edge &e0 = edges[start[v]], &e1 = edges[start[v] + 1];
    interior[v] = e0.dst != v && chain_match(edges[e0.twin].orient, e1.orient);
    n_interior += interior[v];
  }
  const uint32_t cap = chain_round_cap(n_interior, rounds);
  const uint64_t reach = cap >= 63 ? UINT64_MAX : 1ull << cap;  // interior nodes of the longest chain whose ends become known
  // the walk from a head half-edge: its chain's length, end node and end half-edge
  struct End {
    uint32_t n = 0, node = 0, at = 0;
  };
  auto walk = [&](uint64_t h) {
    End r;
    uint64_t e = h;
    for (;;) {
      const uint32_t v = edges[e].dst;
      if (!interior[v]) {
        r.node = v;
        r.at = edges[e].twin;
        return r;
      }
      e = start[v] + (1 - (edges[e].twin - start[v]));
      r.n++;
    }
  };
  // far ends of the half-edges of non-interior nodes (0 = unknown), every chain walked once
  std::vector<uint32_t> far_end(E, 0);
  std::vector<End> ends(E);
  uint64_t on_chains = 0, unresolved = 0, longest = 0;
  for (uint64_t a = 1; a <= N; ++a) {
    if (interior[a]) continue;
    for (uint64_t h = start[a]; h < start[a + 1]; ++h) {
      if (!interior[edges[h].dst]) {
        far_end[h] = edges[h].dst;
        continue;
      }
      if (ends[h].n) continue;  // walked from its other end
      const End r = walk(h);
      ends[h] = r;
      ends[r.at] = End{r.n, (uint32_t)a, (uint32_t)h};
      on_chains += r.n;
      longest = std::max<uint64_t>(longest, r.n);
      if (r.n <= reach) {
        far_end[h] = r.node;
        far_end[r.at] = (uint32_t)a;
      } else {
        unresolved += 2 * (r.n - reach);
      }
    }
  }
  unresolved += 2 * (n_interior - on_chains);  // pure cycles
  uint64_t unsafe = 0;
  for (uint64_t a = 1; a <= N; ++a) {
    if (interior[a]) continue;
    for (uint64_t h = start[a]; h < start[a + 1]; ++h) {
      const End r = ends[h];
      if (!r.n || r.n > reach) continue;
      const uint32_t b = r.node;
      if (!(a < b || (a == b && h < r.at))) continue;  // counted from its other end
      uint64_t same = 0, unknown = 0;
      for (uint64_t k = start[a]; k < start[a + 1]; ++k) {
        same += far_end[k] == b;
        unknown += far_end[k] == 0;
      }
      if (!(a < b && same == 1 && unknown == 0)) {
        unsafe++;
        continue;
      }
      const uint64_t n = r.n, first = out->reads.size();
      out->reads.resize(first + 2 * n);
      out->offs.resize(first + 2 * n);
      out->ors.resize(first + 2 * n);
      uint64_t e = h, off_f = 0, off_r = 0;
      for (uint64_t i = 0; i < n; ++i) {
        const uint32_t v = edges[e].dst;
        out->reads[first + i] = v;
        out->offs[first + i] = edges[e].offset;
        out->ors[first + i] = edges[e].orient & 1;
        off_f += edges[e].offset;
        off_r += edges[edges[e].twin].offset;
        e = start[v] + (1 - (edges[e].twin - start[v]));
        const mg_chain_edge& back = edges[edges[e].twin];  // next -> v
        const uint64_t j = first + n + (n - 1 - i);
        out->reads[j] = v;
        out->offs[j] = back.offset;
        out->ors[j] = back.orient & 1;
      }
      off_f += edges[e].offset;
      off_r += edges[edges[e].twin].offset;
      mg_chain c{};
      c.a = (uint32_t)a;
      c.b = b;
      c.pa = (uint32_t)(h - start[a]);
      c.pb = (uint32_t)(r.at - start[b]);
      c.n = (uint32_t)n;
      c.orient_fwd = (uint8_t)((edges[h].orient & 2) | (edges[e].orient & 1));
      c.orient_rev = (uint8_t)((edges[r.at].orient & 2) | (edges[edges[h].twin].orient & 1));
      c.offset_fwd = off_f;
      c.offset_rev = off_r;
      c.first = first;
      out->chains.push_back(c);
    }
  }
  out->info[MG_CHAIN_INTERIOR] = n_interior;
  out->info[MG_CHAIN_SAFE] = out->chains.size();
  out->info[MG_CHAIN_CONTRACTED] = out->reads.size() / 2;
  out->info[MG_CHAIN_UNSAFE] = unsafe;
  out->info[MG_CHAIN_UNRESOLVED] = unresolved;
  // a round finds new ends while the longest chain exceeds what the rounds before it reached
  out->info[MG_CHAIN_ROUNDS] = n_interior ? std::min<uint64_t>(cap, ceil_log2(std::max<uint64_t>(longest, 1)) + 1) : 0;
  return 0;
}

int UnitigGraph::apply_chains(const mg_chain* ch, uint64_t nc, const uint32_t* rd, const uint16_t* of,
                              const uint8_t* orr, uint64_t n_list, unsigned threads, uint64_t* contracted) {
  if (contracted) *contracted = 0;
  if (!nc) return 0;
  if (!ch || (n_list && (!rd || !of || !orr))) return -4;
  const uint64_t N = lists.empty() ? 0 : lists.size() - 1;
  std::vector<uint8_t> interior(N + 1, 0);
  for (uint64_t v = 1; v <= N; ++v) {
    if (lists[v].size() != 2) continue;
    const UnitigEdge &e0 = pool[lists[v][0]], &e1 = pool[lists[v][1]];
    interior[v] = e0.dst != v && chain_match(pool[e0.rev].orient, e1.orient);
  }
  // the records: ranges, ends, and no read in two chains
  std::vector<uint64_t> base(nc + 1, 0);  // forward entries before chain c
  std::vector<uint8_t> taken(N + 1, 0);
  for (uint64_t c = 0; c < nc; ++c) {
    const mg_chain& x = ch[c];
    if (!x.n || x.first > n_list || 2 * (uint64_t)x.n > n_list - x.first) return -4;
    if (x.a < 1 || x.b > N || x.a >= x.b || interior[x.a] || interior[x.b]) return -4;
    if (x.pa >= lists[x.a].size() || x.pb >= lists[x.b].size()) return -4;
    base[c + 1] = base[c] + x.n;
    if (base[c + 1] > N) return -4;
    for (uint64_t i = 0; i < x.n; ++i) {
      const uint32_t v = rd[x.first + i];
      if (v < 1 || v > N || taken[v]) return -4;
      taken[v] = 1;
    }
  }
  // every list entry on its own: an interior node that links to its neighbours
  // through twin pairs, with that twin's offset and orientation in both lists
  std::atomic<bool> bad{false};
  auto check = [&](uint64_t lo, uint64_t hi) {
    uint64_t c = (uint64_t)(std::upper_bound(base.begin(), base.end(), lo) - base.begin()) - 1;
    for (uint64_t t = lo; t < hi && !bad.load(std::memory_order_relaxed); ++t) {
      while (t >= base[c + 1]) ++c;
      const mg_chain& x = ch[c];
      const uint64_t i = t - base[c], n = x.n, f = x.first + i, r = x.first + n + (n - 1 - i);
      const uint32_t v = rd[f];
      const uint32_t prev = i ? rd[f - 1] : x.a, next = i + 1 < n ? rd[f + 1] : x.b;
      bool ok = interior[v] && rd[r] == v;
      if (ok) {
        const int p = pool[lists[v][0]].dst == prev ? 0 : 1;
        const UnitigEdge &to_prev = pool[lists[v][p]], &to_next = pool[lists[v][1 - p]];
        const UnitigEdge &in_f = pool[to_prev.rev], &in_r = pool[to_next.rev];
        ok = to_prev.dst == prev && to_next.dst == next && of[f] == (uint16_t)in_f.offset && in_f.offset <= 0xFFFF &&
             orr[f] == (in_f.orient & 1) && of[r] == (uint16_t)in_r.offset && in_r.offset <= 0xFFFF &&
             orr[r] == (in_r.orient & 1);
        if (ok && i == 0) ok = lists[x.a][x.pa] == to_prev.rev;
        if (ok && i + 1 == n) ok = lists[x.b][x.pb] == to_next.rev;
      }
      if (!ok) bad.store(true, std::memory_order_relaxed);
    }
  };
  const uint64_t total = base[nc];
  const unsigned T = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(threads ? threads : 1, total / 65536));
  if (T <= 1) {
    check(0, total);
  } else {
    std::vector<std::thread> pool_t;
    for (unsigned k = 0; k < T; ++k) pool_t.emplace_back(check, total * k / T, total * (k + 1) / T);
    for (auto& th : pool_t) th.join();
  }
  if (bad.load()) return -4;
  // the records' own fields, from the lists just checked
  for (uint64_t c = 0; c < nc; ++c) {
    const mg_chain& x = ch[c];
    const UnitigEdge &ha = pool[lists[x.a][x.pa]], &hb = pool[lists[x.b][x.pb]];
    uint64_t off_f = pool[hb.rev].offset, off_r = pool[ha.rev].offset;
    for (uint64_t i = 0; i < x.n; ++i) off_f += of[x.first + i], off_r += of[x.first + x.n + i];
    const uint8_t o_f = (uint8_t)((ha.orient & 2) | (pool[hb.rev].orient & 1));
    const uint8_t o_r = (uint8_t)((hb.orient & 2) | (pool[ha.rev].orient & 1));
    if (x.offset_fwd != off_f || x.offset_rev != off_r || x.orient_fwd != o_f || x.orient_rev != o_r ||
        o_r != twin_orient(o_f))
      return -4;
  }
  // safeness again, from a's list: far ends of the claimed chains from the table,
  // of the others by a walk, each chain walked once
  std::vector<uint32_t> far_end(pool.size(), 0);
  for (uint64_t c = 0; c < nc; ++c) {
    far_end[lists[ch[c].a][ch[c].pa]] = ch[c].b;
    far_end[lists[ch[c].b][ch[c].pb]] = ch[c].a;
  }
  for (uint64_t c = 0; c < nc; ++c) {
    const mg_chain& x = ch[c];
    uint64_t same = 0;
    for (uint32_t h : lists[x.a]) {
      uint32_t d = pool[h].dst;
      if (interior[d]) {
        if (!far_end[h]) {
          uint32_t e = h;
          while (interior[pool[e].dst]) {
            const uint32_t v = pool[e].dst;
            e = lists[v][lists[v][0] == pool[e].rev ? 1 : 0];
          }
          far_end[h] = pool[e].dst;
          far_end[pool[e].rev] = x.a;
        }
        d = far_end[h];
      }
      same += d == x.b;
    }
    if (same != 1) return -4;
  }
  // install: forward edge first, as mergeEdges creates them
  pool.reserve(pool.size() + 2 * nc);
  reads.reserve(reads.size() + 2 * nc);
  for (uint64_t c = 0; c < nc; ++c) {
    const mg_chain& x = ch[c];
    const uint64_t n = x.n;
    auto lf = std::make_unique<EdgeReads>(), lr = std::make_unique<EdgeReads>();
    lf->reads.assign(rd + x.first, rd + x.first + n);
    lf->offs.assign(of + x.first, of + x.first + n);
    lf->ors.assign(orr + x.first, orr + x.first + n);
    lr->reads.assign(rd + x.first + n, rd + x.first + 2 * n);
    lr->offs.assign(of + x.first + n, of + x.first + 2 * n);
    lr->ors.assign(orr + x.first + n, orr + x.first + 2 * n);
    for (uint64_t i = 0; i < n; ++i) {
      const uint32_t v = rd[x.first + i];
      for (uint32_t e : lists[v]) pool[e].alive = pool[pool[e].rev].alive = 0;
      std::vector<uint32_t>().swap(lists[v]);
    }
    const uint32_t ef = new_edge(x.a, x.b, x.orient_fwd, x.offset_fwd, std::move(lf));
    const uint32_t er = new_edge(x.b, x.a, x.orient_rev, x.offset_rev, std::move(lr));
    pool[ef].rev = er;
    pool[er].rev = ef;
    lists[x.a][x.pa] = ef;
    lists[x.b][x.pb] = er;
    update_locations(ef);
    update_locations(er);
    nodes -= n;
    edges -= 2 * n;
  }
  if (contracted) *contracted = total;
  return 0;
}

}  // namespace mg
