// mg_chains_check — a stand-alone host check of the safe-chain code
// (mg::simple_csr's layout, mg::chains_build, mg::UnitigGraph::apply_chains and
// contract(credit); host/mg_chains.cpp), meant to be built with
// -fsanitize=address,undefined (make chains_check_asan) and run on the CPU.  It
// takes no arguments.  From a fixed seed it draws random bidirected multigraphs
// (junctions joined by chains of 0..6 nodes, parallel chains, chains beside a
// direct edge, chains from a node to itself, pure cycles, leaves, type
// mismatches, shuffled lists), runs the mirror and the apply step with every
// array at its exact size, and compares the contracted graph with the plain
// loop's: every list in list order with its read lists, the location lists in
// list order, the counters and the iteration count; the same with every second
// chain only and with a lowered round cap.  Then the tables that must be refused
// with -4 and leave the graph untouched: an entry swapped, a wrong offset or
// orientation, a = b, a chain beside a direct edge, a read in two chains, pa off
// by one, a truncated list; and the malformed CSRs that give -2.
// Exit status 0 = all checks passed.
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "mg_chains.hpp"
#include "mg_unitig.hpp"

namespace {

int fail(const std::string& what) {
  std::fprintf(stderr, "mg_chains_check: FAILED: %s\n", what.c_str());
  return 1;
}

struct Half {
  uint32_t owner, dst, twin;
  uint16_t offset;
  uint8_t orient;
};

// nodes use a strand (0 / 1) at each end of an edge: u -> v has orientation
// su << 1 | sv, its twin the reference's twin of that
struct Builder {
  std::mt19937_64 rng;
  std::vector<std::vector<uint32_t>> adj{1};
  std::vector<Half> half;
  explicit Builder(uint64_t seed) : rng(seed) {}
  uint32_t node() {
    adj.emplace_back();
    return (uint32_t)adj.size() - 1;
  }
  uint32_t strand() { return (uint32_t)(rng() & 1); }
  uint16_t offset() { return (uint16_t)(rng() % 4 == 0 ? 65535 : 1 + rng() % 65535); }
  void edge(uint32_t u, uint32_t su, uint32_t v, uint32_t sv) {
    const uint8_t o = (uint8_t)(su << 1 | sv), t = o == 0 ? 3 : (o == 3 ? 0 : o);
    const uint32_t h = (uint32_t)half.size();
    half.push_back(Half{u, v, h + 1, offset(), o});
    half.push_back(Half{v, u, h, offset(), t});
    adj[u].push_back(h);
    adj[v].push_back(h + 1);
  }
  void chain(uint32_t a, uint32_t b, uint32_t k, int mismatch_at = -1) {
    uint32_t prev = a, s_out = strand();
    for (uint32_t i = 0; i <= k; ++i) {
      const uint32_t next = i == k ? b : node(), s_in = strand();
      edge(prev, s_out, next, s_in);
      s_out = (int)i == mismatch_at ? s_in ^ 1 : s_in;
      prev = next;
    }
  }
  void cycle(uint32_t k) {
    std::vector<uint32_t> ns, s;
    for (uint32_t i = 0; i < k; ++i) ns.push_back(node()), s.push_back(strand());
    for (uint32_t i = 0; i < k; ++i) edge(ns[i], s[i], ns[(i + 1) % k], s[(i + 1) % k]);
  }
  void csr(bool shuffle, std::vector<uint64_t>* start, std::vector<mg_chain_edge>* edges) {
    const size_t n = adj.size() - 1;
    start->assign(n + 2, 0);
    std::vector<uint32_t> at(half.size());
    std::vector<uint32_t> order;
    for (size_t u = 1; u <= n; ++u) {
      std::vector<uint32_t> l = adj[u];
      if (shuffle)
        for (size_t i = l.size(); i > 1; --i) std::swap(l[i - 1], l[rng() % i]);
      (*start)[u + 1] = (*start)[u] + l.size();
      for (uint32_t h : l) at[h] = (uint32_t)order.size(), order.push_back(h);
    }
    edges->clear();
    for (uint32_t h : order) edges->push_back(mg_chain_edge{half[h].dst, at[half[h].twin], half[h].offset, half[h].orient, 0});
  }
};

void random_graph(uint64_t seed, std::vector<uint64_t>* start, std::vector<mg_chain_edge>* edges) {
  Builder g(seed);
  std::vector<uint32_t> j;
  for (uint32_t i = 0, n = 2 + g.rng() % 5; i < n; ++i) j.push_back(g.node());
  for (uint32_t i = 0, n = 3 + g.rng() % 9; i < n; ++i) {
    const uint32_t a = j[g.rng() % j.size()], b = j[g.rng() % j.size()], k = (uint32_t)(g.rng() % 7);
    switch (g.rng() % 8) {
      case 0:
        g.chain(a, b, 1 + k % 4), g.chain(a, b, 1 + (k + 1) % 4);
        break;
      case 1:
        g.chain(a, b, k + 1), g.chain(a, b, 0);
        break;
      case 2:
        g.chain(a, a, k);
        break;
      case 3:
        g.chain(a, g.node(), k);
        break;
      case 4:
        g.chain(a, b, k + 2, (int)(g.rng() % (k + 2)));
        break;
      default:
        g.chain(a, b, k);
    }
  }
  if (g.rng() % 3 == 0) g.cycle(2 + (uint32_t)(g.rng() % 4));
  g.csr(true, start, edges);
}

void graph_of(const std::vector<uint64_t>& start, const std::vector<mg_chain_edge>& edges, mg::UnitigGraph* u) {
  const size_t n = start.size() - 2;
  std::vector<mg::GraphEdge> pool(edges.size());
  std::vector<std::vector<uint32_t>> lists(n + 1);
  uint64_t nodes = 0;
  for (size_t v = 1; v <= n; ++v) {
    for (uint64_t e = start[v]; e < start[v + 1]; ++e) {
      pool[e] = mg::GraphEdge{(uint32_t)v, edges[e].dst, edges[e].offset, edges[e].orient, 0, edges[e].twin};
      lists[v].push_back((uint32_t)e);
    }
    nodes += start[v + 1] > start[v];
  }
  u->init(pool, lists, nodes, edges.size(), n, true);
}

// everything that is compared, free of pool indices
std::string dump(const mg::UnitigGraph& u, int64_t iterations) {
  std::string s;
  auto edge = [&](uint32_t e) {
    const mg::UnitigEdge& x = u.pool[e];
    s += std::to_string(x.src) + ">" + std::to_string(x.dst) + " o" + std::to_string(x.orient) + " +" +
         std::to_string(x.offset) + (x.src == x.dst ? (e < x.rev ? " first" : " second") : "");
    if (u.reads[e])
      for (size_t k = 0; k < u.reads[e]->reads.size(); ++k)
        s += " " + std::to_string(u.reads[e]->reads[k]) + ":" + std::to_string(u.reads[e]->offs[k]) + ":" +
             std::to_string(u.reads[e]->ors[k]);
  };
  for (size_t v = 1; v < u.lists.size(); ++v)
    for (uint32_t e : u.lists[v]) s += "L" + std::to_string(v) + " ", edge(e), s += "\n";
  for (size_t r = 1; r < u.loc_fwd.size(); ++r)
    for (int side = 0; side < 2; ++side)
      for (const mg::ReadLoc& l : side ? u.loc_rev[r] : u.loc_fwd[r])
        s += (side ? "R" : "F") + std::to_string(r) + " @" + std::to_string(l.loc) + " ", edge(l.edge), s += "\n";
  s += "counters " + std::to_string(u.nodes) + " " + std::to_string(u.edges) + " " + std::to_string(u.merged_total) + " " +
       std::to_string(u.dead_end_total) + " " + std::to_string(iterations) + "\n";
  return s;
}

std::string plain_loop(const std::vector<uint64_t>& start, const std::vector<mg_chain_edge>& edges) {
  mg::UnitigGraph u;
  graph_of(start, edges, &u);
  return dump(u, u.contract());
}

// apply + loop; "refused" when apply_chains returns -4 (and then the untouched graph's loop must still be the plain one)
std::string with_chains(const std::vector<uint64_t>& start, const std::vector<mg_chain_edge>& edges,
                        const mg::ChainTable& t, unsigned threads, const std::string& plain) {
  mg::UnitigGraph u;
  graph_of(start, edges, &u);
  uint64_t credit = 0;
  // exact-size copies: a read one past an end is caught
  const std::vector<mg_chain> ch(t.chains.begin(), t.chains.end());
  const std::vector<uint32_t> rd(t.reads.begin(), t.reads.end());
  const std::vector<uint16_t> of(t.offs.begin(), t.offs.end());
  const std::vector<uint8_t> orr(t.ors.begin(), t.ors.end());
  const int rc = u.apply_chains(ch.data(), ch.size(), rd.data(), of.data(), orr.data(), rd.size(), threads, &credit);
  if (rc) return dump(u, u.contract()) == plain ? "refused" : "refused, but the graph changed";
  return dump(u, u.contract(credit));
}

}  // namespace

int main() {
  uint64_t contracted = 0, chains = 0, capped = 0;
  for (uint64_t seed = 1; seed <= 400; ++seed) {
    std::vector<uint64_t> start;
    std::vector<mg_chain_edge> edges;
    random_graph(seed, &start, &edges);
    const std::string tag = "graph " + std::to_string(seed);
    const std::string plain = plain_loop(start, edges);
    mg::ChainTable t;
    std::string err;
    if (mg::chains_build(start.data(), edges.data(), start.size() - 2, edges.size(), 0, &t, &err))
      return fail(tag + ": chains_build: " + err);
    if (with_chains(start, edges, t, 1 + seed % 3, plain) != plain) return fail(tag + ": apply + loop differs from the loop");
    contracted += t.info[MG_CHAIN_CONTRACTED];
    chains += t.chains.size();
    mg::ChainTable half = t;  // any subset is exact
    half.chains.clear();
    for (size_t c = seed & 1; c < t.chains.size(); c += 2) half.chains.push_back(t.chains[c]);
    if (with_chains(start, edges, half, 1, plain) != plain) return fail(tag + ": a subset of the chains differs from the loop");
    mg::ChainTable low;
    if (mg::chains_build(start.data(), edges.data(), start.size() - 2, edges.size(), 1, &low, &err))
      return fail(tag + ": chains_build with a round cap: " + err);
    for (const mg_chain& c : low.chains)
      if (c.n > 2) return fail(tag + ": a chain over the round cap's reach");
    capped += low.chains.size() < t.chains.size();
    if (with_chains(start, edges, low, 1, plain) != plain) return fail(tag + ": the capped chains differ from the loop");
    if (t.chains.empty()) continue;
    // tables that must be refused
    size_t big = 0;
    for (size_t c = 0; c < t.chains.size(); ++c)
      if (t.chains[c].n > t.chains[big].n) big = c;
    const mg_chain& b = t.chains[big];
    auto refused = [&](const mg::ChainTable& m, const char* what) {
      const std::string r = with_chains(start, edges, m, 2, plain);
      return r == "refused" ? 0 : fail(tag + ": " + what + ": " + (r == plain ? "accepted" : r));
    };
    mg::ChainTable m = t;
    if (b.n >= 2) {
      std::swap(m.reads[b.first], m.reads[b.first + 1]);
      if (refused(m, "an entry swapped")) return 1;
    }
    m = t, m.offs[b.first + b.n - 1] ^= 1;
    if (refused(m, "a wrong offset")) return 1;
    m = t, m.offs[b.first + 2 * b.n - 1] ^= 0x100;
    if (refused(m, "a wrong reverse offset")) return 1;
    m = t, m.ors[b.first] ^= 1;
    if (refused(m, "a wrong orientation")) return 1;
    m = t, m.chains[big].b = m.chains[big].a;
    if (refused(m, "a = b")) return 1;
    m = t, m.chains[big].pa += 1;
    if (refused(m, "pa off by one")) return 1;
    m = t, m.chains[big].pb += 1;
    if (refused(m, "pb off by one")) return 1;
    m = t, m.chains.push_back(t.chains[0]);
    if (refused(m, "a read in two chains")) return 1;
    m = t, m.reads.pop_back(), m.offs.pop_back(), m.ors.pop_back();
    if (refused(m, "a truncated list")) return 1;
    m = t, m.chains[big].n -= 1;
    if (refused(m, "a chain cut short")) return 1;
    m = t, m.chains[big].offset_rev += 1;
    if (refused(m, "a wrong offset sum")) return 1;
  }
  if (!contracted || !chains || !capped) return fail("the random graphs have no safe chains");
  {  // a chain that is safe until a direct edge joins its ends: the same table, then unsafe
    for (int direct = 0; direct < 2; ++direct) {
      Builder g(77);
      const uint32_t a = g.node(), b = g.node();
      for (int i = 0; i < 2; ++i) g.edge(a, g.strand(), g.node(), g.strand()), g.edge(b, g.strand(), g.node(), g.strand());
      g.chain(a, b, 5);
      static mg::ChainTable safe;
      if (direct) g.edge(a, g.strand(), b, g.strand());  // (appended: pa and pb stay)
      std::vector<uint64_t> start;
      std::vector<mg_chain_edge> edges;
      g.csr(false, &start, &edges);
      mg::ChainTable t;
      std::string err;
      if (mg::chains_build(start.data(), edges.data(), start.size() - 2, edges.size(), 0, &t, &err)) return fail(err);
      const std::string plain = plain_loop(start, edges);
      if (!direct) {
        if (t.chains.size() != 1 || t.chains[0].n != 5) return fail("the lone chain is not found");
        safe = t;
        if (with_chains(start, edges, safe, 1, plain) != plain) return fail("the lone chain differs from the loop");
      } else {
        if (!t.chains.empty() || t.info[MG_CHAIN_UNSAFE] != 1) return fail("a chain beside a direct edge counts as safe");
        if (with_chains(start, edges, safe, 1, plain) != "refused") return fail("a chain beside a direct edge is accepted");
      }
    }
  }
  {  // malformed CSRs
    std::vector<uint64_t> start;
    std::vector<mg_chain_edge> edges;
    random_graph(5, &start, &edges);
    mg::ChainTable t;
    std::string err;
    const uint64_t n = start.size() - 2, m = edges.size();
    auto code = [&](const std::vector<uint64_t>& s, const std::vector<mg_chain_edge>& e) {
      return mg::chains_build(s.data(), e.data(), n, e.size(), 0, &t, &err);
    };
    std::vector<mg_chain_edge> e = edges;
    e[m / 2].dst = (uint32_t)n + 1;
    if (code(start, e) != -2) return fail("a dst out of range is accepted");
    e = edges, e[m / 2].dst = 0;
    if (code(start, e) != -2) return fail("a dst of 0 is accepted");
    e = edges, e[1].twin = (uint32_t)m;
    if (code(start, e) != -2) return fail("a twin out of range is accepted");
    e = edges, e[1].twin = 0xFFFFFFFFu;
    if (code(start, e) != -2) return fail("a twin of 2^32 - 1 is accepted");
    e = edges, e[0].twin = e[0].twin == 1 ? 2 : 1;
    if (code(start, e) != -2) return fail("twin[twin] != e is accepted");
    std::vector<uint64_t> s = start;
    std::swap(s[2], s[3]), s[2] += 1;
    if (code(s, edges) != -2) return fail("a start that decreases is accepted");
    s = start, s[n + 1] += 1;
    if (code(s, edges) != -2) return fail("a start beyond the half-edges is accepted");
    if (code(start, edges) != 0) return fail("the unchanged CSR is refused: " + err);
  }
  std::printf("mg_chains_check: ok (%llu chains, %llu nodes contracted, %llu graphs lose chains to the round cap)\n",
              (unsigned long long)chains, (unsigned long long)contracted, (unsigned long long)capped);
  return 0;
}
