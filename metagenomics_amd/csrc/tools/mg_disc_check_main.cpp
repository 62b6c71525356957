// mg_disc_check — a stand-alone host check of the discovery-list entry points
// (mg::Discoveries::from_lists, GraphReplay::build_from), meant to be built with
// -fsanitize=address,undefined (make disc_check_asan) and run on the CPU:
//
//   mg_disc_check rows.txt lens.txt l
//
// rows.txt: "src dst orient offset" per line (a fixture's golden rows,
// decompressed); lens.txt: one read length per line in ID order.  Builds the
// lists in C++ (group by src, sort by (j, dst, o), self rows once), checks that
// build_from on them gives the graph GraphReplay::build gives from the rows,
// contracts it, and feeds from_lists each malformed variant, which it must
// reject.  Exit status 0 = all checks passed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <utility>
#include <vector>

#include "mg_graph.hpp"
#include "mg_unitig.hpp"

namespace {

struct Key {
  uint32_t src, j;
  mg_disc d;
};

int fail(const char* what) {
  std::fprintf(stderr, "mg_disc_check: FAILED: %s\n", what);
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) return fail("usage: mg_disc_check rows.txt lens.txt l");
  const uint32_t h = (uint32_t)std::atoi(argv[3]) - 1;
  std::vector<mg_edge> rows;
  {
    std::ifstream f(argv[1]);
    uint64_t s, d, o, off;
    while (f >> s >> d >> o >> off) rows.push_back(mg_edge{(uint32_t)s, (uint32_t)d, (uint16_t)off, (uint8_t)o, 0});
  }
  std::vector<uint16_t> lens;
  {
    std::ifstream f(argv[2]);
    uint64_t x;
    while (f >> x) lens.push_back((uint16_t)x);
  }
  const uint64_t N = lens.size();
  if (rows.empty() || !N) return fail("empty input");

  // the lists, restated: key o, window j, order (src, j, dst, o), every second copy of a self row dropped
  static const uint8_t kKey[4] = {1, 3, 2, 0};
  std::vector<Key> keys;
  for (const mg_edge& r : rows) {
    const uint8_t o = kKey[r.orient & 3];
    const uint32_t j = (o == 0 || o == 2) ? r.offset : (uint32_t)(lens[r.src - 1] - h - r.offset);
    keys.push_back(Key{r.src, j, mg_disc{r.dst, r.offset, r.orient, o}});
  }
  std::sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) {
    if (a.src != b.src) return a.src < b.src;
    if (a.j != b.j) return a.j < b.j;
    if (a.d.dst != b.d.dst) return a.d.dst < b.d.dst;
    return a.d.o < b.d.o;
  });
  std::vector<uint64_t> start(N + 2, 0);
  std::vector<mg_disc> disc;
  for (size_t i = 0; i < keys.size(); ++i) {
    if (keys[i].d.dst == keys[i].src) ++i;  // (its identical copy follows)
    if (i >= keys.size()) return fail("unpaired self row in the input");
    disc.push_back(keys[i].d);
    start[keys[i].src + 1]++;
  }
  for (uint64_t a = 1; a <= N + 1; ++a) start[a] += start[a - 1];

  // from_lists + build_from against build from rows
  mg::GraphReplay from_rows, from_lists;
  if (from_rows.build(rows.data(), rows.size(), lens.data(), N, h)) return fail("GraphReplay::build");
  {
    mg::Discoveries D;
    if (D.from_lists(start.data(), disc.data(), disc.size(), lens.data(), N, h)) return fail("from_lists (valid)");
    if (from_lists.build_from(std::move(D), lens.data(), N, h)) return fail("build_from");
  }
  if (from_rows.nodes != from_lists.nodes || from_rows.edges != from_lists.edges ||
      from_rows.lists != from_lists.lists || from_rows.pool.size() != from_lists.pool.size())
    return fail("build_from differs from build");
  for (size_t i = 0; i < from_rows.pool.size(); ++i) {
    const mg::GraphEdge &a = from_rows.pool[i], &b = from_lists.pool[i];
    if (a.src != b.src || a.dst != b.dst || a.offset != b.offset || a.orient != b.orient || a.rev != b.rev)
      return fail("edge pools differ");
  }
  {
    mg::UnitigGraph u;
    u.init(from_lists, N, true);
    if (u.contract() < 0) return fail("contract");
  }

  // malformed lists: each must be rejected (and read nothing out of bounds)
  uint64_t a2 = 0;  // a read with at least two discoveries
  for (uint64_t a = 1; a <= N && !a2; ++a)
    if (start[a + 1] - start[a] >= 2) a2 = a;
  if (!a2) return fail("no list with two records");
  const uint64_t k = start[a2];
  auto rejected = [&](const std::vector<uint64_t>& s, const std::vector<mg_disc>& d, uint64_t nd) {
    mg::Discoveries D;
    return D.from_lists(s.data(), d.data(), nd, lens.data(), N, h) < 0;
  };
  {
    std::vector<uint64_t> s = start;
    s[a2 + 1] = s[a2 + 2] + 1;
    if (!rejected(s, disc, disc.size())) return fail("non-monotone start accepted");
    s = start;
    s[N + 1] -= 1;
    if (!rejected(s, disc, disc.size())) return fail("start[N + 1] != n_disc accepted");
    if (!rejected(start, disc, disc.size() - 1)) return fail("n_disc != start[N + 1] accepted");
    s = start;
    s[0] = 1;
    if (!rejected(s, disc, disc.size())) return fail("start[0] != 0 accepted");
  }
  for (uint32_t bad : {0u, (uint32_t)N + 1}) {
    std::vector<mg_disc> d = disc;
    d[k].dst = bad;
    if (!rejected(start, d, d.size())) return fail("dst out of range accepted");
  }
  for (uint16_t bad : {(uint16_t)0, (uint16_t)65535}) {
    std::vector<mg_disc> d = disc;
    d[k].offset = bad;
    if (!rejected(start, d, d.size())) return fail("j out of range accepted");
  }
  {
    std::vector<mg_disc> d = disc;
    std::swap(d[k], d[k + 1]);
    if (!rejected(start, d, d.size())) return fail("swapped neighbours accepted");
    d = disc;
    d[k + 1] = d[k];
    if (!rejected(start, d, d.size())) return fail("repeated record accepted");
    d = disc;
    d[k].o = 7;
    if (!rejected(start, d, d.size())) return fail("bad key o accepted");
  }
  std::printf("mg_disc_check: ok (%zu rows, %zu list records, %llu reads)\n", rows.size(), disc.size(),
              (unsigned long long)N);
  return 0;
}
