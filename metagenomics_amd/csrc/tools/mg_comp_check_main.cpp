// mg_comp_check — a stand-alone host check of the component table and the
// parallel replay (mg::Components::build / from_device, GraphReplay::build_from
// with a table), meant to be built with -fsanitize=address,undefined (make
// comp_check_asan) and with -fsanitize=thread (make comp_check_tsan) and run on
// the CPU:
//
//   mg_comp_check rows.txt lens.txt l
//
// Inputs as for mg_disc_check: rows.txt "src dst orient offset" per line,
// lens.txt one read length per line in ID order.  Builds the lists and the
// components in C++, replays with 1, 2, 4 and 16 threads and requires pool and
// lists identical to the serial replay, then feeds every malformed table, which
// must be rejected with -4 or -1.  Exit status 0 = all checks passed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <utility>
#include <vector>

#include "mg_graph.hpp"

namespace {

int fail(const char* what) {
  std::fprintf(stderr, "mg_comp_check: FAILED: %s\n", what);
  return 1;
}

struct Input {
  std::vector<mg_edge> rows;
  std::vector<uint16_t> lens;
  uint32_t h = 0;
  uint64_t N() const { return lens.size(); }
  int lists(mg::Discoveries* D) const { return D->build(rows.data(), rows.size(), lens.data(), N(), h); }
};

// the code a table gets: from_device, then the replay on `threads` threads
int verdict(const Input& in, const std::vector<uint32_t>& label, const std::vector<mg_comp>& comps, unsigned threads) {
  mg::Discoveries D;
  if (in.lists(&D)) return 1;
  mg::Components C;
  int rc = C.from_device(label.data(), comps.data(), comps.size(), D);
  if (rc) return rc;
  mg::GraphReplay g;
  rc = g.build_from(std::move(D), in.lens.data(), in.N(), in.h, &C, threads);
  if (rc && (!g.pool.empty() || g.nodes || g.edges)) return 2;  // (a refused table leaves no graph)
  return rc;
}

bool rejected(int rc) { return rc == -4 || rc == -1; }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) return fail("usage: mg_comp_check rows.txt lens.txt l");
  Input in;
  in.h = (uint32_t)std::atoi(argv[3]) - 1;
  {
    std::ifstream f(argv[1]);
    uint64_t s, d, o, off;
    while (f >> s >> d >> o >> off) in.rows.push_back(mg_edge{(uint32_t)s, (uint32_t)d, (uint16_t)off, (uint8_t)o, 0});
  }
  {
    std::ifstream f(argv[2]);
    uint64_t x;
    while (f >> x) in.lens.push_back((uint16_t)x);
  }
  const uint64_t N = in.N();
  if (in.rows.empty() || !N) return fail("empty input");

  mg::Discoveries D0;
  if (in.lists(&D0)) return fail("Discoveries::build");
  mg::Components C;
  if (C.build(D0)) return fail("Components::build");
  const std::vector<uint64_t> start = D0.start;
  if (C.label.size() != N + 1 || C.comps.empty()) return fail("no components");
  {  // the host table passes the validation meant for the device's
    mg::Components V;
    if (V.from_device(C.label.data(), C.comps.data(), C.comps.size(), D0)) return fail("from_device (valid)");
    if (V.label != C.label || V.comps.size() != C.comps.size()) return fail("from_device changed the table");
  }

  // the serial replay, then the same with 1, 2, 4 and 16 threads
  mg::GraphReplay serial;
  {
    mg::Discoveries D;
    in.lists(&D);
    if (serial.build_from(std::move(D), in.lens.data(), N, in.h)) return fail("serial build_from");
  }
  for (unsigned t : {1u, 2u, 4u, 16u}) {
    mg::GraphReplay par;
    mg::Discoveries D;
    in.lists(&D);
    if (par.build_from(std::move(D), in.lens.data(), N, in.h, &C, t)) return fail("parallel build_from");
    if (par.nodes != serial.nodes || par.edges != serial.edges || par.lists != serial.lists ||
        par.pool.size() != serial.pool.size())
      return fail("parallel replay differs from the serial one");
    for (size_t i = 0; i < serial.pool.size(); ++i) {
      const mg::GraphEdge &a = serial.pool[i], &b = par.pool[i];
      if (a.src != b.src || a.dst != b.dst || a.offset != b.offset || a.orient != b.orient || a.trans != b.trans ||
          a.rev != b.rev)
        return fail("edge pools differ");
    }
  }

  // malformed tables
  const std::vector<uint32_t>& label = C.label;
  const std::vector<mg_comp>& comps = C.comps;
  if (verdict(in, label, comps, 4) != 0) return fail("valid table refused");
  const uint32_t ra = comps[0].root;
  std::vector<uint32_t> members;  // of the first component
  for (uint64_t a = 1; a <= N; ++a)
    if (label[a] == ra) members.push_back((uint32_t)a);
  if (members.size() < 2) return fail("first component has one read");
  if (comps.size() >= 2) {
    const uint32_t rb = comps[1].root;
    {  // two components given one label: only the replay can tell
      std::vector<uint32_t> lab = label;
      for (uint64_t a = 1; a <= N; ++a)
        if (lab[a] == rb) lab[a] = ra;
      std::vector<mg_comp> cs = comps;
      cs[0].n_reads += cs[1].n_reads;
      cs[0].n_disc += cs[1].n_disc;
      cs[0].n_self += cs[1].n_self;
      cs.erase(cs.begin() + 1);
      for (unsigned t : {2u, 4u, 16u})
        if (verdict(in, lab, cs, t) != -4) return fail("two components under one label accepted");
    }
    {  // roots not ascending
      std::vector<mg_comp> cs = comps;
      std::swap(cs[0], cs[1]);
      if (verdict(in, label, cs, 4) != -4) return fail("descending roots accepted");
      cs = comps;
      cs[1] = cs[0];
      if (verdict(in, label, cs, 4) != -4) return fail("repeated root accepted");
    }
    {  // a component missing from the table
      std::vector<mg_comp> cs(comps.begin() + 1, comps.end());
      if (verdict(in, label, cs, 4) != -4) return fail("missing component accepted");
    }
  }
  if (members.size() >= 4) {  // one component split in two: closure violated
    const size_t half = members.size() / 2;
    std::vector<uint32_t> lab = label;
    mg_comp second{members[half], 0, 0, 0};
    for (size_t i = half; i < members.size(); ++i) {
      lab[members[i]] = members[half];
      second.n_reads++;
      second.n_disc += (uint32_t)(start[members[i] + 1] - start[members[i]]);
    }
    std::vector<mg_comp> cs = comps;
    cs[0].n_reads -= second.n_reads;
    cs[0].n_disc -= second.n_disc;
    cs.push_back(second);
    std::sort(cs.begin(), cs.end(), [](const mg_comp& a, const mg_comp& b) { return a.root < b.root; });
    if (verdict(in, lab, cs, 4) != -4) return fail("split component accepted");
  }
  {  // a root that is not the minimum
    std::vector<uint32_t> lab = label;
    for (uint32_t m : members) lab[m] = members[1];
    std::vector<mg_comp> cs = comps;
    cs[0].root = members[1];
    if (verdict(in, lab, cs, 4) != -4) return fail("non-minimum root accepted");
  }
  for (int field = 0; field < 3; ++field)
    for (int d : {1, -1}) {
      std::vector<mg_comp> cs = comps;
      uint32_t& x = field == 0 ? cs[0].n_reads : field == 1 ? cs[0].n_disc : cs[0].n_self;
      if (d < 0 && !x) continue;
      x += (uint32_t)d;
      if (verdict(in, label, cs, 4) != -4) return fail("count off by one accepted");
    }
  {  // label[A] > A
    std::vector<uint32_t> lab = label;
    lab[ra] = members[1];
    if (verdict(in, lab, comps, 4) != -4) return fail("label[A] > A accepted");
  }
  for (uint32_t bad : {0u, (uint32_t)N + 1}) {  // IDs out of range
    std::vector<uint32_t> lab = label;
    lab[members[1]] = bad;
    if (!rejected(verdict(in, lab, comps, 4))) return fail("label out of range accepted");
    std::vector<mg_comp> cs = comps;
    cs.back().root = bad;
    if (!rejected(verdict(in, label, cs, 4))) return fail("root out of range accepted");
  }
  {  // label[0] != 0
    std::vector<uint32_t> lab = label;
    lab[0] = 1;
    if (verdict(in, lab, comps, 4) != -4) return fail("label[0] != 0 accepted");
  }
  std::printf("mg_comp_check: ok (%zu rows, %llu reads, %zu components, %zu pool entries)\n", in.rows.size(),
              (unsigned long long)N, comps.size(), serial.pool.size());
  return 0;
}
