// mg_paths_check_main.cpp — stand-alone check of the mate-pair path host code
// (host/mg_paths.cpp: mg::mate_paths, mg::path_pairs, mg::merge_supported) over
// built-in cases.  `make paths_check_asan` compiles it with the host sources
// under AddressSanitizer + UBSan and runs it: host code only, from its own
// main, on the CPU.
//
// The graph: a calibration-free chain with a bubble,
//   1 -> 2 -> 3 -> {4, 5} -> 6 -> 7 -> 8     (all orientation 3)
// written as a .unitig text and re-read, so twins, list order and location
// lists are the library's own.  Reads 9, 10, 11 lie on 1 -> 2, reads 12, 13, 14
// on 7 -> 8; mate entries (9, 12), (10, 13), (11, 14) with mean 190, sd 10.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "mg_contigs.hpp"
#include "mg_paths.hpp"
#include "mg_unitig.hpp"

namespace {

int fail(const char* what) {
  std::fprintf(stderr, "paths_check: FAILED: %s\n", what);
  return 1;
}

std::string rec(unsigned s, unsigned d, unsigned offset, std::vector<unsigned> reads = {}, unsigned first = 40) {
  std::string out = std::to_string(s) + "\n" + std::to_string(d) + "\n3\n" + std::to_string(offset) + "\n" +
                    std::to_string(reads.size()) + "\n";
  for (size_t i = 0; i < reads.size(); ++i)
    out += std::to_string(reads[i]) + "\n" + std::to_string(i ? 5u : first) + "\n1\n";
  return out;
}

}  // namespace

int main() {
  const uint64_t n = 14;
  const std::vector<uint16_t> lens(n, 30);
  const std::string text = rec(1, 2, 100, {9, 10, 11}) + rec(2, 3, 20) + rec(3, 4, 20) + rec(4, 6, 20) +
                           rec(3, 5, 25) + rec(5, 6, 20) + rec(6, 7, 20) + rec(7, 8, 100, {12, 13, 14});
  char path[] = "/tmp/mg_paths_check_XXXXXX";
  const int fd = mkstemp(path);
  if (fd < 0) return fail("mkstemp");
  FILE* f = fdopen(fd, "w");
  std::fputs(text.c_str(), f);
  std::fclose(f);
  mg::UnitigGraph u;
  const int rc = u.read_unitig(path, lens.data(), n, true);
  std::remove(path);
  if (rc) return fail("read_unitig");
  u.sort_edges();

  mg::ContigLists c;
  mg::contig_edges(u, true, &c);
  std::vector<uint32_t> index(u.pool.size(), 0xFFFFFFFFu), twin(c.pool.size());
  for (size_t k = 0; k < c.pool.size(); ++k) index[c.pool[k]] = (uint32_t)k;
  for (size_t k = 0; k < c.pool.size(); ++k) twin[k] = index[u.pool[c.pool[k]].rev];
  std::vector<uint64_t> pstart(n + 2, 0), mstart(n + 2, 0);
  std::vector<mg_place> places;
  for (uint64_t r = 1; r <= n; ++r) {
    pstart[r] = places.size();
    for (const mg::ReadLoc& l : u.loc_fwd[r]) places.push_back(mg_place{index[l.edge], 1u, l.loc});
    for (const mg::ReadLoc& l : u.loc_rev[r]) places.push_back(mg_place{index[l.edge], 0u, l.loc});
  }
  pstart[n + 1] = places.size();
  std::vector<mg_mate> mates;
  for (uint64_t r = 1; r <= n; ++r) {
    mstart[r] = mates.size();
    if (r >= 9 && r <= 11) mates.push_back(mg_mate{(uint32_t)r + 3, 2, 0, 0});
    if (r >= 12) mates.push_back(mg_mate{(uint32_t)r - 3, 1, 0, 0});  // skipped: its owner is the higher ID
  }
  mstart[n + 1] = mates.size();
  const uint64_t mean[1] = {190}, sd[1] = {10};

  mg::PathInput in;
  in.n_reads = n;
  in.edges = c.edges.data();
  in.twin = twin.data();
  in.n_edges = c.edges.size();
  in.place_start = pstart.data();
  in.places = places.data();
  in.mate_start = mstart.data();
  in.mates = mates.data();
  in.mean = mean;
  in.sd = sd;
  in.n_datasets = 1;
  std::string err;
  mg::PathEntries full, part, done;
  if (mg::mate_paths(in, 0, nullptr, &full, &err)) return fail(err.c_str());
  int found = 0;
  for (size_t m = 0; m < full.status.size(); ++m) {
    if (full.status[m] != MG_PATH_FOUND) continue;
    ++found;
    if (full.start[m + 1] - full.start[m] != 6) return fail("a path of 6 edges");
    const uint8_t want[6] = {1, 0, 0, 0, 1, 0};  // the pairs inside the bubble are cleared
    for (int k = 0; k < 6; ++k)
      if (full.flags[full.start[m] + k] != want[k]) return fail("bubble flags");
  }
  if (found != 3 || full.status[3] != MG_PATH_SKIPPED) return fail("three paths, three skipped entries");
  std::vector<mg_pair_support> pairs;
  uint64_t counters[3];
  mg::path_pairs(in, full, &pairs, counters);
  if (pairs.size() != 2 || pairs[0].support != 3 || pairs[1].support != 3 || counters[1] != 3 || counters[0] || counters[2])
    return fail("two pairs with support 3");

  // a budget below the search's cost defers it; prior finishes it to the same answer
  if (mg::mate_paths(in, 5, nullptr, &part, &err)) return fail(err.c_str());
  if (part.status[0] != MG_PATH_DEFERRED || part.visits[0] != 6 || part.start.back() != 0) return fail("deferred entries");
  if (mg::mate_paths(in, 0, &part, &done, &err)) return fail(err.c_str());
  if (done.status != full.status || done.path != full.path || done.flags != full.flags || done.start != full.start)
    return fail("prior");

  // every -2 kind
  std::vector<uint32_t> bad_twin = twin;
  bad_twin[2] = (uint32_t)twin.size();
  in.twin = bad_twin.data();
  if (mg::paths_validate(in, &err) != -2 || err.find("edge 2 ") != 0) return fail("twin out of range");
  in.twin = twin.data();
  std::vector<mg_mate> bad_mates = mates;
  bad_mates[1].dataset = 1;
  in.mates = bad_mates.data();
  if (mg::paths_validate(in, &err) != -2 || err.find("mate entry 1:") != 0) return fail("dataset out of range");
  in.mates = mates.data();
  std::vector<mg_place> bad_places = places;
  bad_places.back().edge = 1000;
  in.places = bad_places.data();
  if (mg::paths_validate(in, &err) != -2 || err.find("placement ") != 0) return fail("placement out of range");
  in.places = places.data();

  // the merge: a refused pair leaves the graph alone, then both supported pairs merge
  const uint64_t edges_before = u.edges;
  const mg_pair_support twins[1] = {{pairs[0].edge1, twin[pairs[0].edge1], 3}};
  uint64_t merged = 9;
  if (mg::merge_supported(&u, c.pool, twins, 1, 3, &merged, &err) != -5 || u.edges != edges_before)
    return fail("the twin pair is refused");
  if (mg::merge_supported(&u, c.pool, pairs.data(), pairs.size(), 3, &merged, &err) || merged != 2)
    return fail("two merges");
  if (u.edges != edges_before - 4) return fail("each merge replaces four edges by two");
  std::printf("paths_check: ok (%d paths, %zu pairs, %llu merges)\n", found, pairs.size(), (unsigned long long)merged);
  return 0;
}
