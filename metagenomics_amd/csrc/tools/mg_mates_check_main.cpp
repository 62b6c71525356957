// mg_mates_check — a stand-alone host check of the mate-pair code (the pair
// reader and mg::MatePairs::build, host/mg_mates.cpp), meant to be built with
// -fsanitize=address,undefined (make mates_check_asan) and run on the CPU:
//
//   mg_mates_check l dump.txt pe_file...
//
// dump.txt is a fixture dump (tests/golden/pairs_*.mates.gz, unpacked): "#N n",
// "#R id string", "#S id super", then "#B 1" / "#B 0" blocks of
// "#M id mate orient dataset" lines.  Reads the pairs of the paired-end files,
// builds the lists over the dump's reads with its superReadIDs (block 1) and
// with none (block 0), requires both equal to the dump entry for entry, then
// feeds malformed input (an odd n_raw, dataset counts that do not add up, a
// superReadID out of range, a mate that is in no read), which must be refused
// with its code.  Exit status 0 = all checks passed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "mg_mates.hpp"

namespace {

int fail(const std::string& what) {
  std::fprintf(stderr, "mg_mates_check: FAILED: %s\n", what.c_str());
  return 1;
}

struct Entry {
  uint64_t owner, id, orient, dataset;
};

bool same(const mg::MatePairs& mp, const std::vector<Entry>& want, uint64_t n) {
  if (mp.start.size() != n + 2 || mp.recs.size() != want.size() || mp.start[n + 1] != want.size()) return false;
  uint64_t k = 0;
  for (uint64_t a = 1; a <= n; ++a)
    for (uint64_t i = mp.start[a]; i < mp.start[a + 1]; ++i, ++k) {
      if (k >= want.size()) return false;
      const Entry& e = want[k];
      if (e.owner != a || mp.recs[i].id != e.id || mp.recs[i].orient != e.orient || mp.recs[i].dataset != e.dataset ||
          mp.recs[i].pad != 0)
        return false;
    }
  return k == want.size();
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) return fail("usage: mg_mates_check l dump.txt pe_file...");
  const uint32_t l = (uint32_t)std::atoi(argv[1]);
  uint64_t n = 0;
  std::vector<std::string> reads;
  std::vector<uint32_t> super;
  std::vector<Entry> want[2];
  {
    std::ifstream f(argv[2]);
    if (!f) return fail("cannot open the dump");
    std::string line, tag;
    int block = -1;
    while (std::getline(f, line)) {
      std::istringstream s(line);
      s >> tag;
      if (tag == "#N") {
        s >> n;
        reads.assign(n + 1, "");
        super.assign(n + 1, 0);
      } else if (tag == "#R") {
        uint64_t id;
        s >> id;
        if (id < 1 || id > n) return fail("dump: read ID out of range");
        s >> reads[id];
      } else if (tag == "#S") {
        uint64_t id, sp;
        s >> id >> sp;
        if (id < 1 || id > n) return fail("dump: read ID out of range");
        super[id] = (uint32_t)sp;
      } else if (tag == "#B") {
        s >> block;
        if (block != 0 && block != 1) return fail("dump: block");
      } else if (tag == "#M") {
        Entry e;
        s >> e.owner >> e.id >> e.orient >> e.dataset;
        if (block < 0) return fail("dump: #M before #B");
        want[block].push_back(e);
      }
    }
  }
  // the packed reads in ID order
  uint32_t wpr = 1;
  for (uint64_t i = 1; i <= n; ++i) wpr = std::max<uint32_t>(wpr, (uint32_t)((reads[i].size() + 31) / 32));
  std::vector<uint64_t> words(n * wpr + 1, 0);
  std::vector<uint16_t> lens(n + 1, 0);
  for (uint64_t i = 1; i <= n; ++i) {
    const std::string& s = reads[i];
    lens[i - 1] = (uint16_t)s.size();
    for (size_t p = 0; p < s.size(); ++p) {
      const uint64_t c = s[p] == 'A' ? 0 : s[p] == 'C' ? 1 : s[p] == 'G' ? 2 : 3;
      words[(i - 1) * wpr + (p >> 5)] |= c << (62 - 2 * (p & 31));
    }
  }
  // the pairs
  std::string text;
  std::vector<uint64_t> off{0}, ppd;
  for (int a = 3; a < argc; ++a) {
    uint64_t np = 0;
    const int rc = mg::read_pairs_file(argv[a], text, off, &np);
    if (rc) return fail(std::string("read_pairs_file ") + argv[a] + " = " + std::to_string(rc));
    ppd.push_back(np);
  }
  const uint64_t n_raw = off.size() - 1;
  if (n_raw & 1) return fail("the reader gave an odd record count");
  std::string err;
  mg::MatePairs mp;
  int rc = mp.build(words.data(), lens.data(), n, wpr, super.data(), text.data(), off.data(), n_raw, ppd.data(),
                    (uint32_t)ppd.size(), l, &err);
  if (rc) return fail("build with superReadIDs = " + std::to_string(rc) + ": " + err);
  if (!same(mp, want[1], n)) return fail("the lists differ from the dump's block 1");
  if (mp.good_pairs + mp.bad_pairs != n_raw / 2) return fail("good + bad pairs");
  rc = mp.build(words.data(), lens.data(), n, wpr, nullptr, text.data(), off.data(), n_raw, ppd.data(),
                (uint32_t)ppd.size(), l, &err);
  if (rc) return fail("build without superReadIDs = " + std::to_string(rc) + ": " + err);
  if (!same(mp, want[0], n)) return fail("the lists differ from the dump's block 0");

  // malformed input
  if (n_raw >= 2) {
    rc = mp.build(words.data(), lens.data(), n, wpr, nullptr, text.data(), off.data(), n_raw - 1, ppd.data(),
                  (uint32_t)ppd.size(), l, &err);
    if (rc != -1) return fail("an odd n_raw was not refused");
    std::vector<uint64_t> p2 = ppd;
    p2[0] += 1;
    rc = mp.build(words.data(), lens.data(), n, wpr, nullptr, text.data(), off.data(), n_raw, p2.data(),
                  (uint32_t)p2.size(), l, &err);
    if (rc != -1) return fail("dataset counts above n_raw / 2 were not refused");
    p2[0] = ppd[0] ? ppd[0] - 1 : 0;
    if (ppd[0]) {
      rc = mp.build(words.data(), lens.data(), n, wpr, nullptr, text.data(), off.data(), n_raw, p2.data(),
                    (uint32_t)p2.size(), l, &err);
      if (rc != -1) return fail("dataset counts below n_raw / 2 were not refused");
    }
    rc = mp.build(words.data(), lens.data(), n, wpr, nullptr, text.data(), off.data(), n_raw, ppd.data(), 0, l, &err);
    if (rc != -1) return fail("no datasets for pairs was not refused");
  }
  if (n) {
    std::vector<uint32_t> s2 = super;
    s2[1] = (uint32_t)n + 1;
    rc = mp.build(words.data(), lens.data(), n, wpr, s2.data(), text.data(), off.data(), n_raw, ppd.data(),
                  (uint32_t)ppd.size(), l, &err);
    if (rc != -1) return fail("a superReadID out of range was not refused");
  }
  if (mp.good_pairs && n > 1) {
    // without its last read a good mate is missing, or every good pair avoids it
    const uint64_t had = want[0].size();
    rc = mp.build(words.data(), lens.data(), n - 1, wpr, nullptr, text.data(), off.data(), n_raw, ppd.data(),
                  (uint32_t)ppd.size(), l, &err);
    if (rc == -2 && mp.not_found < 0) return fail("-2 without the raw index");
    if (rc != -2 && rc != 0) return fail("a missing read gave neither -2 nor lists");
    if (rc == 0 && mp.recs.size() > had) return fail("fewer reads gave more entries");
  }
  // empty input
  rc = mp.build(words.data(), lens.data(), n, wpr, nullptr, nullptr, nullptr, 0, nullptr, 0, l, &err);
  if (rc || !mp.recs.empty() || mp.start.size() != n + 2) return fail("empty input");
  std::printf("mg_mates_check: ok (%llu reads, %llu raw mates, %zu + %zu entries)\n", (unsigned long long)n,
              (unsigned long long)n_raw, want[1].size(), want[0].size());
  return 0;
}
