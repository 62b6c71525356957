// mg_scaffold.cpp — the scaffolder on the host: the scoring mirror and the merge loop (see mg_scaffold.hpp).
#include "mg_scaffold.hpp"

#include <algorithm>
#include <cstdio>
#include <unordered_map>

namespace mg {

int scaffold_validate(const ScaffoldInput& in, std::string* err) {
  if (err) err->clear();
  if ((in.n_edges && !in.twin) || !in.place_start || !in.mate_start || (in.n_datasets && (!in.mean || !in.sd)) ||
      in.n_datasets > 256 || (in.n_edges >> 31))
    return -1;
  const uint64_t entries = in.n_reads + 2;
  if (in.place_start[0] != 0 || in.mate_start[0] != 0) return -1;
  for (uint64_t a = 0; a + 1 < entries; ++a)
    if (in.place_start[a + 1] < in.place_start[a] || in.mate_start[a + 1] < in.mate_start[a]) return -1;
  const uint64_t P = in.place_start[entries - 1], M = in.mate_start[entries - 1];
  if ((P && !in.places) || (M && !in.mates) || (P >> 31) || (M >> 31)) return -1;
  for (uint64_t k = 0; k < in.n_edges; ++k)
    if (in.twin[k] >= in.n_edges) {
      if (err)
        *err = "edge " + std::to_string(k) + ": its twin " + std::to_string(in.twin[k]) + " is not below " +
               std::to_string(in.n_edges) + " (-2)";
      return -2;
    }
  for (uint64_t p = 0; p < P; ++p)
    if (in.places[p].edge >= in.n_edges) {
      if (err)
        *err = "placement " + std::to_string(p) + ": its edge " + std::to_string(in.places[p].edge) +
               " is not below " + std::to_string(in.n_edges) + " (-2)";
      return -2;
    }
  for (uint64_t a = 0; a + 1 < entries; ++a)
    for (uint64_t m = in.mate_start[a]; m < in.mate_start[a + 1]; ++m)
      if (a < 1 || a > in.n_reads || in.mates[m].id < 1 || in.mates[m].id > in.n_reads ||
          in.mates[m].dataset >= in.n_datasets) {
        if (err)
          *err = "mate entry " + std::to_string(m) + ": its dataset is not below " + std::to_string(in.n_datasets) +
                 " or its owner or mate ID lies outside 1.." + std::to_string(in.n_reads) + " (-2)";
        return -2;
      }
  return 0;
}

namespace {
// the only placement of the wanted strand in read r's segment: its count, capped at 2
uint32_t only_place(const ScaffoldInput& in, uint64_t r, uint32_t want, mg_place* out) {
  uint32_t n = 0;
  for (uint64_t p = in.place_start[r]; p < in.place_start[r + 1] && n < 2; ++p) {
    if ((in.places[p].flags & 1u) != want) continue;
    if (!n) *out = in.places[p];
    ++n;
  }
  return n;
}
}  // namespace

int scaffold_pairs(const ScaffoldInput& in, std::vector<uint8_t>* status, std::vector<mg_scaffold_pair>* pairs,
                   uint64_t* counters, std::string* err) {
  if (!status || !pairs) return -1;
  if (const int rc = scaffold_validate(in, err)) return rc;
  const uint64_t M = in.mate_start[in.n_reads + 1];
  status->assign(M, MG_SCAF_SKIPPED);
  pairs->clear();
  uint64_t cnt[5] = {0, 0, 0, 0, 0};
  std::unordered_map<uint64_t, size_t> where;  // canonical key -> its record
  for (uint64_t a = 1; a <= in.n_reads; ++a)   // :2130
    for (uint64_t m = in.mate_start[a]; m < in.mate_start[a + 1]; ++m) {
      const mg_mate& mt = in.mates[m];
      uint8_t st;
      if (a > mt.id) {  // :2137
        st = MG_SCAF_SKIPPED;
      } else {
        const uint32_t want1 = (mt.orient == 0 || mt.orient == 1) ? 1u : 0u;  // :2149
        const uint32_t want2 = (mt.orient == 0 || mt.orient == 2) ? 1u : 0u;  // :2153
        mg_place pa{0, 0, 0}, pb{0, 0, 0};
        const uint32_t n1 = only_place(in, a, want1, &pa), n2 = only_place(in, mt.id, want2, &pb);
        const uint64_t dist = pa.distance + pb.distance;
        if (n1 != 1 || n2 != 1) {
          st = MG_SCAF_NOT_UNIQUE;
        } else if (!(dist < in.mean[mt.dataset] + 3 * in.sd[mt.dataset])) {  // :2157 (mod 2^64)
          st = MG_SCAF_FAR;
        } else if (pa.edge == pb.edge || pa.edge == in.twin[pb.edge]) {  // :2161
          st = MG_SCAF_SAME_EDGE;
        } else {
          st = MG_SCAF_COUNTED;
          const uint64_t t1 = in.twin[pa.edge], t2 = in.twin[pb.edge];
          const uint64_t key = std::min(t1 * in.n_edges + pb.edge, t2 * in.n_edges + pa.edge);  // :2168, :2174
          const auto it = where.find(key);
          if (it != where.end()) {
            (*pairs)[it->second].support += 1;
            (*pairs)[it->second].distance += dist;
          } else {  // :2184-2190
            where.emplace(key, pairs->size());
            pairs->push_back(mg_scaffold_pair{(uint32_t)t1, pb.edge, 1, dist});
          }
        }
      }
      (*status)[m] = st;
      ++cnt[st];
    }
  if (counters) std::copy(cnt, cnt + 5, counters);
  return 0;
}

namespace {

struct PairedEdges {  // pairedEdges :1874-1886
  uint32_t edge1, edge2;
  uint64_t support, distance;
  bool freed;
  bool operator<(const PairedEdges& rhs) const { return support > rhs.support; }
};

inline bool match_edge_type(uint8_t a, uint8_t b) {  // matchEdgeType :19-26
  return ((a == 1 || a == 3) && (b == 2 || b == 3)) || ((a == 0 || a == 2) && (b == 0 || b == 1));
}

// the 2-bit codes of read `id`: its stored (forward) string, or its reverse complement
std::vector<uint8_t> read_codes(const uint64_t* words, const uint16_t* lens, uint32_t wpr, uint32_t id, bool forward) {
  const uint64_t* w = words + (uint64_t)(id - 1) * wpr;
  const uint32_t n = lens[id - 1];
  std::vector<uint8_t> s(n);
  for (uint32_t p = 0; p < n; ++p) {
    const uint8_t c = (uint8_t)((w[p >> 5] >> (62u - 2u * (p & 31u))) & 3u);
    if (forward) s[p] = c;
    else s[n - 1 - p] = (uint8_t)(3 - c);
  }
  return s;
}

// findOverlap :2368-2379: the longest i in [10, min(len) - 1] at which the
// suffix of a equals the prefix of b, else 0
uint64_t find_overlap(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b) {
  const uint64_t m = std::min(a.size(), b.size());
  for (uint64_t i = m ? m - 1 : 0; i >= 10; --i)
    if (std::equal(a.end() - (ptrdiff_t)i, a.end(), b.begin())) return i;
  return 0;
}

}  // namespace

int merge_scaffold(UnitigGraph* u, const std::vector<uint32_t>& pool_of, const mg_scaffold_pair* pairs, uint64_t n,
                   uint64_t min_support, const uint64_t* words, const uint16_t* lens, uint64_t n_reads,
                   uint32_t words_per_read, std::string* lines, uint64_t* merged, std::string* err) {
  if (err) err->clear();
  if (merged) *merged = 0;
  if (lines) lines->clear();
  if (!u || (n && !pairs) || (n_reads && (!words || !lens)) || !words_per_read) return -1;
  std::vector<PairedEdges> list(n);
  for (uint64_t i = 0; i < n; ++i) {
    if (pairs[i].edge1 >= pool_of.size() || pairs[i].edge2 >= pool_of.size()) {
      if (err) *err = "pair " + std::to_string(i) + ": an edge index outside the graph's " + std::to_string(pool_of.size()) + " edges";
      return -1;
    }
    list[i] = PairedEdges{pool_of[pairs[i].edge1], pool_of[pairs[i].edge2], pairs[i].support, pairs[i].distance, false};
  }
  std::sort(list.begin(), list.end());  // :2197
  const auto in_pair = [&](uint32_t e, const uint32_t (&four)[4]) {
    return e == four[0] || e == four[1] || e == four[2] || e == four[3];
  };
  const auto name = [&](uint32_t e) {
    return "(" + std::to_string(u->pool[e].src) + ", " + std::to_string(u->pool[e].dst) + ")";
  };
  uint64_t count = 0;
  for (int pass = 0; pass < 2; ++pass) {  // a dry run first: a refused pair leaves the graph as it was
    for (auto& p : list) p.freed = false;
    for (uint64_t i = 0; i < n; ++i) {  // :2199-2219
      if (list[i].freed || list[i].support < min_support) continue;
      const uint32_t e1 = list[i].edge1, e2 = list[i].edge2;
      const uint32_t four[4] = {e1, u->pool[e1].rev, e2, u->pool[e2].rev};  // e1f, e1r, e2f, e2r :2206-2207
      const UnitigEdge a = u->pool[e1], b = u->pool[e2];
      const bool connected = a.dst == b.src && match_edge_type(a.orient, b.orient);  // :2388
      if (pass == 0) {
        if (e1 == e2 || e2 == four[1]) {
          if (err)
            *err = "supported pair " + name(e1) + " and " + name(e2) + ", support " + std::to_string(list[i].support) +
                   (e1 == e2 ? ": one edge twice" : ": an edge and its twin") +
                   "; merging it would touch a removed edge (-5)";
          return -5;
        }
        if (a.orient > 3 || b.orient > 3) {
          if (err) *err = "supported pair " + name(e1) + " and " + name(e2) + ": no merged orientation (-4)";
          return -4;
        }
        if (!connected && (a.dst < 1 || a.dst > n_reads || b.src < 1 || b.src > n_reads)) {
          if (err) *err = "supported pair " + name(e1) + " and " + name(e2) + ": a node outside the reads";
          return -1;
        }
      } else {
        ++count;
        list[i].distance /= list[i].support;  // :2204
        if (lines) {
          char buf[256];
          std::snprintf(buf, sizeof buf,
                        "%4llu (%10u,%10u) Length: %8llu Flow: %3u and (%10u,%10u) Length: %8llu Flow: %3u are supported "
                        "%4llu times. Average distance: %4llu\n",
                        (unsigned long long)(i + 1), a.src, a.dst, (unsigned long long)a.offset, (unsigned)a.flow, b.src,
                        b.dst, (unsigned long long)b.offset, (unsigned)b.flow, (unsigned long long)list[i].support,
                        (unsigned long long)list[i].distance);
          *lines += buf;
        }
        if (connected) {
          u->merge_edges(e1, e2);
        } else {
          const std::vector<uint8_t> s1 = read_codes(words, lens, words_per_read, a.dst, a.orient == 1 || a.orient == 3);  // :2396
          const std::vector<uint8_t> s2 = read_codes(words, lens, words_per_read, b.src, b.orient == 2 || b.orient == 3);  // :2397
          const uint64_t ov = find_overlap(s1, s2);
          u->merge_edges_disconnected(e1, e2, s1.size() - ov, s2.size() - ov);  // :2412-2421
        }
        if (u->bad_merge) return -4;
      }
      for (uint64_t j = i + 1; j < n; ++j)  // :2211-2217
        if (in_pair(list[j].edge1, four) || in_pair(list[j].edge2, four)) list[j].freed = true;
    }
  }
  if (merged) *merged = count;
  return 0;
}

}  // namespace mg
