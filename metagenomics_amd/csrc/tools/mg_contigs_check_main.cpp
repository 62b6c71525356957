// mg_contigs_check — a stand-alone host check of the contig code (the mirror of
// getStringInEdge and printGraph's writer, host/mg_contigs.cpp), meant to be
// built with -fsanitize=address,undefined (make contigs_check_asan) and run on
// the CPU (tools/contigs_check.py feeds it every fixture):
//
//   mg_contigs_check reads.txt graph.unitig want.gdl want.fa
//
// reads.txt holds the Dataset's unique reads, one forward string per line in ID
// order.  Packs them, reads the .unitig checkpoint back (readGraphFromFile),
// sortEdges, spells every edge of every list and the contigs with the mirror,
// writes printGraph's two files and requires them equal to want.gdl / want.fa
// byte for byte; then feeds every malformed input (each form of an invalid
// piece, read IDs 0 and N + 1, list ranges outside the lists, inconsistent
// string starts), which must be refused with its code and must not read out of
// range.  Exit status 0 = all checks passed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "mg_contigs.hpp"

namespace {

int fail(const std::string& what) {
  std::fprintf(stderr, "mg_contigs_check: FAILED: %s\n", what.c_str());
  return 1;
}

bool slurp(const std::string& path, std::string* out) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  std::ostringstream s;
  s << f.rdbuf();
  *out = s.str();
  return true;
}

struct OneEdge {
  mg_contig_edge e{};
  std::vector<uint32_t> reads;
  std::vector<uint16_t> offs;
  std::vector<uint8_t> ors;
};

OneEdge edge(uint32_t src, uint32_t dst, uint8_t orient, uint64_t offset, std::vector<uint32_t> reads = {},
             std::vector<uint16_t> offs = {}, std::vector<uint8_t> ors = {}, uint32_t tail = 0) {
  OneEdge x;
  x.e.src = src, x.e.dst = dst, x.e.orient = orient, x.e.offset = offset;
  x.e.n = (uint32_t)reads.size(), x.e.tail = tail;
  x.reads = std::move(reads), x.offs = std::move(offs), x.ors = std::move(ors);
  return x;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 5) return fail("usage: mg_contigs_check reads.txt graph.unitig want.gdl want.fa");
  std::vector<std::string> reads;
  {
    std::ifstream f(argv[1]);
    if (!f) return fail("cannot open the reads");
    std::string line;
    while (std::getline(f, line))
      if (!line.empty()) reads.push_back(line);
  }
  const uint64_t n = reads.size();
  size_t longest = 1;
  for (const std::string& s : reads) longest = std::max(longest, s.size());
  const uint32_t wpr = (uint32_t)((longest + 31) / 32);
  std::vector<uint64_t> words(n * wpr, 0);
  std::vector<uint16_t> lens(n, 0);
  for (uint64_t i = 0; i < n; ++i) {
    lens[i] = (uint16_t)reads[i].size();
    for (size_t p = 0; p < reads[i].size(); ++p) {
      const char c = reads[i][p];
      const uint64_t b = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4;
      if (b > 3) return fail("a read holds a character outside ACGT");
      words[i * wpr + (p >> 5)] |= b << (62 - 2 * (p & 31));
    }
  }

  mg::UnitigGraph g;
  if (g.read_unitig(argv[2], lens.data(), n, true)) return fail("read_unitig");
  g.sort_edges();
  std::vector<uint64_t> start;
  std::string bases, err;
  for (int all = 1; all >= 0; --all) {
    mg::ContigLists c;
    mg::contig_edges(g, all != 0, &c);
    const int rc = mg::contigs_build(words.data(), lens.data(), n, wpr, c.edges.data(), c.edges.size(), c.reads.data(),
                                     c.offs.data(), c.ors.data(), c.reads.size(), &start, &bases, &err);
    if (rc) return fail("contigs_build on the fixture: " + err);
    if (start.size() != c.edges.size() + 1 || start.back() != bases.size()) return fail("starts / bases disagree");
    // every base decodes back to its read: piece 0 of every string is the whole source read
    for (size_t k = 0; k < c.edges.size(); ++k) {
      const std::string& r = reads[c.edges[k].src - 1];
      if (start[k + 1] - start[k] < r.size()) return fail("a string shorter than its source read");
      if ((c.edges[k].orient & 2) && bases.compare(start[k], r.size(), r) != 0)
        return fail("a string does not begin with its forward source read");
    }
    if (all) continue;
    const std::string gdl = std::string(argv[3]) + ".got", fa = std::string(argv[4]) + ".got";
    if (mg::print_graph(g, c, start.data(), bases.data(), gdl.c_str(), fa.c_str())) return fail("print_graph");
    std::string a, b;
    if (!slurp(gdl, &a) || !slurp(argv[3], &b) || a != b) return fail("the .gdl file differs from the golden");
    if (!slurp(fa, &a) || !slurp(argv[4], &b) || a != b) return fail("the FASTA file differs from the golden");
    std::remove(gdl.c_str());
    std::remove(fa.c_str());
    if (mg::print_graph(g, c, start.data(), bases.data(), "/nonexistent-dir/x.gdl", fa.c_str()) != -1)
      return fail("an unwritable path was not reported");
  }

  // malformed input over three reads of 40, 50 and 30 bases
  const std::vector<uint16_t> l3 = {40, 50, 30};
  const std::vector<uint64_t> w3(6, 0x1B1B1B1B1B1B1B1BULL);
  const std::vector<OneEdge> bad = {
      edge(1, 2, 3, 41),                                  // len1 - offset < 0
      edge(1, 2, 3, ~0ull),                               // the same, at the top of the range
      edge(2, 3, 3, 10),                                  // len1 - offset > len2
      edge(1, 2, 3, 60, {3}, {41}, {1}, 5),               // prev - off < 0
      edge(2, 1, 3, 60, {3}, {10}, {1}, 5),               // prev - off > len
      edge(1, 2, 3, 60, {2, 3}, {10, 51}, {1, 0}, 5),     // the second list entry
      edge(1, 3, 3, 60, {2}, {10}, {1}, 31),              // rev.offs[0] > len2
      edge(1, 3, 3, 60, {2}, {10}, {1}, 0xFFFFFFFFu),     // a twin without a list
      edge(0, 2, 3, 10), edge(1, 4, 3, 10), edge(4, 1, 3, 10), edge(1, 0xFFFFFFFFu, 3, 10),
      edge(1, 2, 3, 60, {0}, {10}, {1}, 5), edge(1, 2, 3, 60, {4}, {10}, {1}, 5),
      edge(1, 2, 3, 60, {2, 4}, {10, 10}, {1, 1}, 5),     // a bad ID as the previous read of the tail's list
  };
  for (size_t k = 0; k < bad.size(); ++k) {
    const OneEdge& x = bad[k];
    const int rc = mg::contigs_build(w3.data(), l3.data(), 3, 2, &x.e, 1, x.reads.data(), x.offs.data(), x.ors.data(),
                                     x.reads.size(), &start, &bases, &err);
    if (rc != -2 || err.find("edge 0 (") == std::string::npos || !bases.empty())
      return fail("malformed edge " + std::to_string(k) + " was not refused with -2 and its name");
  }
  {
    OneEdge x = edge(1, 2, 3, 60, {3}, {20}, {1}, 0);
    x.e.first = 1;  // one past the lists
    if (mg::contigs_build(w3.data(), l3.data(), 3, 2, &x.e, 1, x.reads.data(), x.offs.data(), x.ors.data(), 1, &start,
                          &bases, &err) != -1)
      return fail("a list range outside the lists was not refused");
    x.e.first = ~0ull;
    x.e.n = 2;
    if (mg::contigs_build(w3.data(), l3.data(), 3, 2, &x.e, 1, x.reads.data(), x.offs.data(), x.ors.data(), 1, &start,
                          &bases, &err) != -1)
      return fail("a wrapping list range was not refused");
    if (mg::contigs_build(w3.data(), l3.data(), 3, 2, nullptr, 1, nullptr, nullptr, nullptr, 0, &start, &bases, &err) !=
        -1)
      return fail("null edges were not refused");
    // valid edge cases: zero edges, an empty tail, an empty list piece
    if (mg::contigs_build(w3.data(), l3.data(), 3, 2, nullptr, 0, nullptr, nullptr, nullptr, 0, &start, &bases, &err) ||
        start.size() != 1 || !bases.empty())
      return fail("zero edges");
    const OneEdge y = edge(2, 1, 0, 60, {3}, {20}, {0}, 0);
    if (mg::contigs_build(w3.data(), l3.data(), 3, 2, &y.e, 1, y.reads.data(), y.offs.data(), y.ors.data(), 1, &start,
                          &bases, &err) ||
        bases.size() != 50)
      return fail("empty pieces");
  }
  std::printf("mg_contigs_check: ok (%llu reads, %llu edges)\n", (unsigned long long)n, (unsigned long long)g.edges);
  return 0;
}
