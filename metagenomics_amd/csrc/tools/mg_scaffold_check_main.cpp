// mg_scaffold_check_main.cpp — stand-alone check of the scaffolder host code
// (host/mg_scaffold.cpp: mg::scaffold_validate, mg::scaffold_pairs,
// mg::merge_scaffold with UnitigGraph::merge_edges_disconnected) over built-in
// cases.  `make scaffold_check_asan` compiles it with the host source
// under AddressSanitizer + UBSan and runs it: host code only, from its own
// main, on the CPU.
//
// A hand case whose answer is written out, random cases against a plain
// restatement that keeps the reference's linear list (OverlapGraph.cpp:2166-2191),
// every malformed input, and the merge loop on a re-read .unitig text: a
// disconnected merge, a connected one, a freed pair and the -5 dry run.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "mg_scaffold.hpp"
#include "mg_unitig.hpp"

namespace {

int fail(const char* what) {
  std::fprintf(stderr, "scaffold_check: FAILED: %s\n", what);
  return 1;
}

struct Case {
  uint64_t n = 0;
  std::vector<uint32_t> twin;
  std::vector<uint64_t> pstart, mstart, mean, sd;
  std::vector<mg_place> places;
  std::vector<mg_mate> mates;
  mg::ScaffoldInput input() const {
    mg::ScaffoldInput in;
    in.n_reads = n;
    in.twin = twin.data();
    in.n_edges = twin.size();
    in.place_start = pstart.data();
    in.places = places.data();
    in.mate_start = mstart.data();
    in.mates = mates.data();
    in.mean = mean.data();
    in.sd = sd.data();
    in.n_datasets = (uint32_t)mean.size();
    return in;
  }
};

// the reference's loop with its linear list
void plain(const Case& c, std::vector<uint8_t>* status, std::vector<mg_scaffold_pair>* pairs) {
  status->clear();
  pairs->clear();
  for (uint64_t a = 1; a <= c.n; ++a)
    for (uint64_t m = c.mstart[a]; m < c.mstart[a + 1]; ++m) {
      const mg_mate& mt = c.mates[m];
      if (a > mt.id) {
        status->push_back(MG_SCAF_SKIPPED);
        continue;
      }
      const bool f1 = mt.orient == 0 || mt.orient == 1, f2 = mt.orient == 0 || mt.orient == 2;
      std::vector<mg_place> l1, l2;
      for (uint64_t p = c.pstart[a]; p < c.pstart[a + 1]; ++p)
        if (((c.places[p].flags & 1u) != 0) == f1) l1.push_back(c.places[p]);
      for (uint64_t p = c.pstart[mt.id]; p < c.pstart[mt.id + 1]; ++p)
        if (((c.places[p].flags & 1u) != 0) == f2) l2.push_back(c.places[p]);
      if (l1.size() != 1 || l2.size() != 1) {
        status->push_back(MG_SCAF_NOT_UNIQUE);
        continue;
      }
      const uint64_t dist = l1[0].distance + l2[0].distance;
      if (!(dist < c.mean[mt.dataset] + 3 * c.sd[mt.dataset])) {
        status->push_back(MG_SCAF_FAR);
        continue;
      }
      const uint32_t e1 = l1[0].edge, e2 = l2[0].edge;
      if (e1 == e2 || e1 == c.twin[e2]) {
        status->push_back(MG_SCAF_SAME_EDGE);
        continue;
      }
      status->push_back(MG_SCAF_COUNTED);
      size_t k = 0;
      for (; k < pairs->size(); ++k)
        if (((*pairs)[k].edge1 == c.twin[e1] && (*pairs)[k].edge2 == e2) ||
            ((*pairs)[k].edge1 == c.twin[e2] && (*pairs)[k].edge2 == e1)) {
          (*pairs)[k].support += 1;
          (*pairs)[k].distance += dist;
          break;
        }
      if (k == pairs->size()) pairs->push_back(mg_scaffold_pair{c.twin[e1], e2, 1, dist});
    }
}

Case random_case(std::mt19937_64& rng, uint64_t n, uint32_t half_edges, uint32_t max_mates) {
  Case c;
  c.n = n;
  c.twin.resize(2 * half_edges);
  for (uint32_t k = 0; k < 2 * half_edges; ++k) c.twin[k] = k ^ 1u;
  c.mean = {200, 0};
  c.sd = {10, 0};
  c.pstart.assign(n + 2, 0);
  c.mstart.assign(n + 2, 0);
  for (uint64_t r = 1; r <= n; ++r) {
    c.pstart[r] = c.places.size();
    const int k = (int)(rng() % 8 == 0 ? rng() % 4 : 1 + rng() % 2);
    for (int i = 0; i < k; ++i)
      c.places.push_back(mg_place{(uint32_t)(rng() % (2 * half_edges)), (uint32_t)(rng() % 2), rng() % 160});
  }
  c.pstart[n + 1] = c.places.size();
  for (uint64_t r = 1; r <= n; ++r) {
    c.mstart[r] = c.mates.size();
    const uint32_t k = (uint32_t)(rng() % (max_mates + 1));
    for (uint32_t i = 0; i < k; ++i)
      c.mates.push_back(mg_mate{(uint32_t)(1 + rng() % n), (uint8_t)(rng() % 4), (uint8_t)(rng() % 16 == 0), 0});
  }
  c.mstart[n + 1] = c.mates.size();
  return c;
}

bool same(const std::vector<mg_scaffold_pair>& a, const std::vector<mg_scaffold_pair>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].edge1 != b[i].edge1 || a[i].edge2 != b[i].edge2 || a[i].support != b[i].support ||
        a[i].distance != b[i].distance)
      return false;
  return true;
}

std::string rec(unsigned s, unsigned d, unsigned offset, std::vector<unsigned> reads) {
  std::string out = std::to_string(s) + "\n" + std::to_string(d) + "\n3\n" + std::to_string(offset) + "\n" +
                    std::to_string(reads.size()) + "\n";
  for (size_t i = 0; i < reads.size(); ++i) out += std::to_string(reads[i]) + "\n" + std::to_string(i ? 5u : 40u) + "\n1\n";
  return out;
}

uint32_t edge_of(const mg::UnitigGraph& u, uint32_t s, uint32_t d) {
  for (uint32_t e = 0; e < u.pool.size(); ++e)
    if (u.pool[e].alive && u.pool[e].src == s && u.pool[e].dst == d) return e;
  return UINT32_MAX;
}

// 1 -> 2, 3 -> 4 (disconnected), 5 -> 6 -> 7 (connected), 12 reads of 30 bp
int check_merge() {
  const uint64_t n = 12;
  const std::vector<uint16_t> lens(n, 30);
  std::mt19937_64 rng(7);
  std::vector<uint64_t> words(n);
  for (auto& w : words) w = rng() & ~0xFull;  // 30 bases in the high 60 bits
  const std::string text = rec(1, 2, 100, {8, 9}) + rec(3, 4, 100, {10}) + rec(5, 6, 100, {11}) + rec(6, 7, 100, {12});
  char path[] = "/tmp/mg_scaffold_check_XXXXXX";
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
  std::vector<uint32_t> pool_of(u.pool.size());
  for (uint32_t e = 0; e < pool_of.size(); ++e) pool_of[e] = e;
  const uint32_t e12 = edge_of(u, 1, 2), e34 = edge_of(u, 3, 4), e56 = edge_of(u, 5, 6), e67 = edge_of(u, 6, 7);
  const uint64_t edges_before = u.edges;
  std::string lines, err;
  uint64_t merged = 0;
  const mg_scaffold_pair twice[2] = {{e12, e34, 3, 300}, {e56, e56, 4, 4}};
  if (mg::merge_scaffold(&u, pool_of, twice, 2, 3, words.data(), lens.data(), n, 1, &lines, &merged, &err) != -5 ||
      u.edges != edges_before || err.find("one edge twice") == std::string::npos)
    return fail("the dry run");
  const mg_scaffold_pair pairs[4] = {{e12, e34, 4, 402}, {e56, e67, 3, 10}, {u.pool[e34].rev, e56, 3, 3}, {e12, e67, 2, 2}};
  if (mg::merge_scaffold(&u, pool_of, pairs, 4, 3, words.data(), lens.data(), n, 1, &lines, &merged, &err) || merged != 2)
    return fail("merge_scaffold");  // the third pair is freed by the first two, the fourth is below the support
  if (lines.find("   1 (         1,         2) Length:      100 Flow:   0 and (         3,         4) Length:      100 "
                 "Flow:   0 are supported    4 times. Average distance:  100\n") != 0)
    return fail("the line");
  const uint32_t e14 = edge_of(u, 1, 4), e57 = edge_of(u, 5, 7);
  if (e14 == UINT32_MAX || e57 == UINT32_MAX || u.edges != edges_before - 4) return fail("the merged edges");
  if (u.pool[e14].offset < 201 || u.pool[e14].offset > 230 || u.reads[e14]->reads.size() != 5 || u.pool[e57].offset != 200 ||
      u.reads[e57]->reads.size() != 3)
    return fail("the merged lists");
  return 0;
}

}  // namespace

int main() {
  if (check_merge()) return 1;
  // edges 0/1 and 2/3 are twins.  Reads 1..3 lie forward on edge 0 at 10, 20, 30;
  // reads 4..6 reverse on edge 2 at 5, 6, 7; read 7 forward on edges 0 and 2.
  Case c;
  c.n = 7;
  c.twin = {1, 0, 3, 2};
  c.mean = {100};
  c.sd = {5};
  c.pstart = {0, 0, 1, 2, 3, 4, 5, 6, 8};
  c.places = {{0, 1, 10}, {0, 1, 20}, {0, 1, 30}, {2, 0, 5}, {2, 0, 6}, {2, 0, 7}, {0, 1, 1}, {2, 1, 2}};
  // orient 1: A forward, B reverse
  c.mstart = {0, 0, 2, 3, 4, 5, 5, 5, 5};
  c.mates = {{4, 1, 0, 0}, {7, 1, 0, 0}, {5, 1, 0, 0}, {6, 1, 0, 0}, {1, 2, 0, 0}};
  std::vector<uint8_t> st, st2;
  std::vector<mg_scaffold_pair> pr, pr2;
  uint64_t cnt[5];
  std::string err;
  if (mg::scaffold_pairs(c.input(), &st, &pr, cnt, &err)) return fail("hand case refused");
  const std::vector<uint8_t> want = {MG_SCAF_COUNTED, MG_SCAF_NOT_UNIQUE, MG_SCAF_COUNTED, MG_SCAF_COUNTED,
                                     MG_SCAF_SKIPPED};
  if (st != want) return fail("hand case statuses");
  if (pr.size() != 1 || pr[0].edge1 != 1 || pr[0].edge2 != 2 || pr[0].support != 3 || pr[0].distance != 78)
    return fail("hand case record");
  if (cnt[MG_SCAF_COUNTED] != 3 || cnt[MG_SCAF_SKIPPED] != 1 || cnt[MG_SCAF_NOT_UNIQUE] != 1 || cnt[MG_SCAF_FAR] ||
      cnt[MG_SCAF_SAME_EDGE])
    return fail("hand case counters");
  c.mean[0] = 20;  // bound 35: 10 + 5 and 20 + 6 count, 30 + 7 is far
  if (mg::scaffold_pairs(c.input(), &st, &pr, cnt, &err) || st[3] != MG_SCAF_FAR || pr[0].support != 2 ||
      pr[0].distance != 41)
    return fail("the bound");
  c.mean[0] = 0;
  c.sd[0] = 0;
  if (mg::scaffold_pairs(c.input(), &st, &pr, cnt, &err) || !pr.empty() || cnt[MG_SCAF_FAR] != 3)
    return fail("mean 0 and sd 0 count nothing");

  std::mt19937_64 rng(12345);
  uint64_t records = 0, joined = 0;
  for (int i = 0; i < 200; ++i) {
    const Case r = random_case(rng, 20 + rng() % 60, 2 + (uint32_t)(rng() % 6), 4);
    if (mg::scaffold_pairs(r.input(), &st, &pr, cnt, &err)) return fail("random case refused");
    plain(r, &st2, &pr2);
    if (st != st2 || !same(pr, pr2)) return fail("random case differs from the linear list");
    records += pr.size();
    for (const auto& p : pr) joined += p.support - 1;
  }
  if (!records || !joined) return fail("the random cases hold no joined record");

  // malformed inputs: the first offender of each kind, in order
  Case b = random_case(rng, 40, 4, 3);
  b.mates[5].dataset = 9;
  if (mg::scaffold_pairs(b.input(), &st, &pr, cnt, &err) != -2 || err.find("mate entry 5:") != 0) return fail("bad mate");
  b.places[3].edge = 8;
  if (mg::scaffold_pairs(b.input(), &st, &pr, cnt, &err) != -2 || err.find("placement 3:") != 0) return fail("bad placement");
  b.twin[2] = 8;
  if (mg::scaffold_pairs(b.input(), &st, &pr, cnt, &err) != -2 || err.find("edge 2:") != 0) return fail("bad twin");
  b.mstart[4] = b.mstart[5] + 1;
  if (mg::scaffold_pairs(b.input(), &st, &pr, cnt, &err) != -1) return fail("decreasing starts");
  Case e;  // no reads at all
  e.pstart = {0, 0};
  e.mstart = {0, 0};
  if (mg::scaffold_pairs(e.input(), &st, &pr, cnt, &err) || !st.empty() || !pr.empty()) return fail("empty input");
  std::printf("scaffold_check: ok (%llu records, %llu joins over the random cases)\n", (unsigned long long)records,
              (unsigned long long)joined);
  return 0;
}
