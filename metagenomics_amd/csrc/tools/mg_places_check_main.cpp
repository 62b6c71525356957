// mg_places_check — a stand-alone host check of the placement code
// (mg::placements_build, mg::insert_sizes, mg::edge_coverage, mg::mean_sd;
// host/mg_places.cpp), meant to be built with -fsanitize=address,undefined
// (make places_check_asan) and run on the CPU.  It takes no arguments: it draws
// random edges, lists, mate lists and frequencies from a fixed seed, runs the
// three mirrors with every array allocated at its exact size (so a read or a
// write one past an end is caught), compares them with direct restatements of
// the definitions (a per-read scan of all entries; all pairs of entries of one
// edge; one counter array per edge), and feeds the malformed inputs that must be
// refused with their codes: a list range outside the lists, a read ID of 0 and
// of n + 1, a mate entry with a dataset or an ID out of range, an entry that
// ends beyond the edge's counters, a source read longer than them.
// Exit status 0 = all checks passed.
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "mg_places.hpp"

namespace {

int fail(const std::string& what) {
  std::fprintf(stderr, "mg_places_check: FAILED: %s\n", what.c_str());
  return 1;
}

struct Graph {
  std::vector<mg_contig_edge> edges;
  std::vector<uint32_t> reads;
  std::vector<uint16_t> offs;
  std::vector<uint8_t> ors;
};

Graph random_graph(std::mt19937_64& rng, const std::vector<uint16_t>& lens, const std::vector<uint32_t>& sizes) {
  Graph g;
  const uint32_t n = (uint32_t)lens.size();
  for (uint32_t m : sizes) {
    mg_contig_edge e{};
    e.src = 1 + rng() % n;
    e.dst = 1 + rng() % n;
    e.first = g.reads.size();
    e.n = m;
    e.orient = 3;
    uint64_t d = 0, need = lens[e.src - 1] ? lens[e.src - 1] - 1 : 0;
    for (uint32_t i = 0; i < m; ++i) {
      const uint32_t r = 1 + rng() % n;
      const uint16_t off = (uint16_t)(rng() % 30);
      d += off;
      if (d + lens[r - 1] > need + 1) need = d + lens[r - 1] - 1;
      g.reads.push_back(r);
      g.offs.push_back(off);
      g.ors.push_back((uint8_t)(rng() & 1));
    }
    const uint64_t L = need + rng() % 20;
    e.offset = L > lens[e.dst - 1] ? L - lens[e.dst - 1] : 0;
    g.edges.push_back(e);
  }
  return g;
}

}  // namespace

int main() {
  std::mt19937_64 rng(20241020);
  for (int round = 0; round < 20; ++round) {
    const uint32_t n = 5 + (uint32_t)(rng() % 60);
    std::vector<uint16_t> lens(n);
    std::vector<uint32_t> freq(n);
    for (uint32_t i = 0; i < n; ++i) {
      lens[i] = (uint16_t)(1 + rng() % 80);
      freq[i] = (uint32_t)(rng() % 4);
    }
    std::vector<uint32_t> sizes;
    for (int k = 0, ne = 1 + (int)(rng() % 8); k < ne; ++k) sizes.push_back((uint32_t)(rng() % 70));
    const Graph g = random_graph(rng, lens, sizes);
    const uint64_t ne = g.edges.size(), nl = g.reads.size();
    std::vector<uint64_t> start;
    std::vector<mg_place> pl;
    std::vector<uint32_t> fc;
    std::string err;
    if (mg::placements_build(n, g.edges.data(), ne, g.reads.data(), g.offs.data(), g.ors.data(), nl, &start, &pl, &fc,
                             &err))
      return fail("placements_build refused a valid graph: " + err);
    if (start.size() != n + 2 || start[n + 1] != pl.size() || pl.size() != nl) return fail("placement CSR sizes");
    // restated: read A's records are the entries that name A, in (edge, position) order
    for (uint32_t a = 1; a <= n; ++a) {
      uint64_t at = start[a];
      uint32_t fwd = 0;
      for (uint64_t k = 0; k < ne; ++k) {
        uint64_t d = 0;
        for (uint64_t i = 0; i < g.edges[k].n; ++i) {
          const uint64_t q = g.edges[k].first + i;
          d += g.offs[q];
          if (g.reads[q] != a) continue;
          if (at >= start[a + 1] || pl[at].edge != k || pl[at].distance != d || pl[at].flags != (g.ors[q] == 1 ? 1u : 0u))
            return fail("placement record of read " + std::to_string(a));
          fwd += g.ors[q] == 1;
          ++at;
        }
      }
      if (at != start[a + 1] || fc[a] != fwd) return fail("placement count of read " + std::to_string(a));
    }
    // mate lists: 0..3 entries per read, three datasets
    std::vector<uint64_t> ms(n + 2, 0);
    std::vector<mg_mate> mates;
    for (uint32_t a = 1; a <= n; ++a) {
      ms[a] = mates.size();
      for (int k = 0, c = (int)(rng() % 4); k < c; ++k)
        mates.push_back(mg_mate{(uint32_t)(1 + rng() % n), (uint8_t)(rng() % 4), (uint8_t)(rng() % 3), 0});
    }
    ms[n + 1] = mates.size();
    std::vector<uint64_t> sums(9, 7), want(9, 0);
    if (mg::insert_sizes(n, start.data(), pl.data(), ms.data(), mates.data(), 3, 50, sums.data(), &err))
      return fail("insert_sizes refused valid lists: " + err);
    for (uint32_t a = 1; a <= n; ++a)
      for (uint64_t m = ms[a]; m < ms[a + 1]; ++m)
        for (const mg_place& p : pl)
          for (const mg_place& q : pl) {
            const uint64_t ip = (uint64_t)(&p - pl.data()), iq = (uint64_t)(&q - pl.data());
            if (ip < start[a] || ip >= start[a + 1] || iq < start[mates[m].id] || iq >= start[mates[m].id + 1]) continue;
            if (p.edge != q.edge || p.distance <= q.distance || p.distance - q.distance >= 50) continue;
            const uint64_t x = p.distance - q.distance;
            want[3 * mates[m].dataset] += 1;
            want[3 * mates[m].dataset + 1] += x;
            want[3 * mates[m].dataset + 2] += x * x;
          }
    if (sums != want) return fail("insert-size sums");
    std::vector<uint64_t> cov(3 * ne, 7);
    if (mg::edge_coverage(lens.data(), n, g.edges.data(), ne, g.reads.data(), g.offs.data(), g.ors.data(), nl, fc.data(),
                          freq.data(), cov.data(), &err))
      return fail("edge_coverage refused a valid graph: " + err);
    for (uint64_t k = 0; k < ne; ++k) {
      const mg_contig_edge& e = g.edges[k];
      const uint64_t L = e.offset + lens[e.dst - 1];
      std::vector<uint64_t> c(L + 1, 0);
      std::vector<uint8_t> dead(L + 1, 0);
      uint64_t d = 0;
      for (uint64_t i = 0; i < e.n; ++i) {
        const uint32_t r = g.reads[e.first + i];
        d += g.offs[e.first + i];
        for (uint64_t j = d; j < d + lens[r - 1]; ++j) {
          c.at(j) += freq[r - 1];
          if (fc[r] > 1) dead.at(j) = 1;
        }
      }
      uint64_t s[3] = {0, 0, 0};
      for (uint64_t j = 0; j <= L; ++j) {
        if (dead[j] || j < lens[e.src - 1] || j + lens[e.dst - 1] > L || !c[j] || !e.n) continue;
        s[0] += 1;
        s[1] += c[j];
        s[2] += c[j] * c[j];
      }
      if (cov[3 * k] != s[0] || cov[3 * k + 1] != s[1] || cov[3 * k + 2] != s[2])
        return fail("coverage sums of edge " + std::to_string(k));
      uint64_t mean = 1, sd = 1;
      mg::mean_sd(s[0], s[1], s[2], &mean, &sd);
      if (!s[0] && (mean || sd)) return fail("mean_sd of an empty edge");
      if (s[0] && mean != s[1] / s[0]) return fail("mean_sd");
    }
    // refusals
    if (ne && nl) {
      Graph b = g;
      b.edges[0].first = nl;
      b.edges[0].n = 1;
      if (mg::placements_build(n, b.edges.data(), ne, b.reads.data(), b.offs.data(), b.ors.data(), nl, &start, &pl, &fc,
                               &err) != -1)
        return fail("a list range outside the lists was not refused with -1");
      for (uint32_t bad_id : {0u, n + 1}) {
        b = g;
        b.reads[nl - 1] = bad_id;
        if (mg::placements_build(n, b.edges.data(), ne, b.reads.data(), b.offs.data(), b.ors.data(), nl, &start, &pl,
                                 &fc, &err) != -2 ||
            err.find("list entry") == std::string::npos)
          return fail("a read ID out of range was not refused with -2");
      }
      if (mg::placements_build(n, g.edges.data(), ne, g.reads.data(), g.offs.data(), g.ors.data(), nl, &start, &pl, &fc,
                               &err))
        return fail("rebuild");
    }
    if (!mates.empty()) {
      std::vector<mg_mate> bm = mates;
      bm.back().dataset = 3;
      if (mg::insert_sizes(n, start.data(), pl.data(), ms.data(), bm.data(), 3, 50, sums.data(), &err) != -2)
        return fail("a dataset out of range was not refused with -2");
      bm = mates;
      bm.front().id = n + 1;
      if (mg::insert_sizes(n, start.data(), pl.data(), ms.data(), bm.data(), 3, 50, sums.data(), &err) != -2)
        return fail("a mate ID out of range was not refused with -2");
    }
    for (uint64_t k = 0; k < ne; ++k) {
      if (!g.edges[k].n) continue;
      Graph b = g;
      b.edges[k].offset = 0;  // L = len(dst): an entry or the source read may no longer fit
      const uint64_t L = lens[b.edges[k].dst - 1];
      bool fits = lens[b.edges[k].src - 1] <= L + 1;
      uint64_t d = 0;
      for (uint64_t i = 0; i < b.edges[k].n; ++i) {
        d += b.offs[b.edges[k].first + i];
        fits = fits && d + lens[b.reads[b.edges[k].first + i] - 1] <= L + 1;
      }
      std::vector<uint64_t> out(3 * ne, 7);
      const int rc = mg::edge_coverage(lens.data(), n, b.edges.data(), ne, b.reads.data(), b.offs.data(), b.ors.data(),
                                       nl, fc.data(), freq.data(), out.data(), &err);
      if (rc != (fits ? 0 : -2)) return fail("an edge that does not fit its counters: code " + std::to_string(rc));
      if (!fits && (out[0] != 7 || err.find("edge " + std::to_string(k)) == std::string::npos))
        return fail("an invalid edge wrote a result or was not named");
      break;
    }
  }
  std::printf("mg_places_check: ok\n");
  return 0;
}
