// mg_paths.cpp — mate-pair path support on the host (see mg_paths.hpp).
#include "mg_paths.hpp"

#include <algorithm>
#include <unordered_map>

namespace mg {

namespace {

constexpr int kMaxLevel = 100;  // :1800

inline bool match_edge_type(uint8_t a, uint8_t b) {  // matchEdgeType :19-26
  if ((a == 1 || a == 3) && (b == 2 || b == 3)) return true;
  if ((a == 0 || a == 2) && (b == 0 || b == 1)) return true;
  return false;
}

std::string edge_name(const mg_contig_edge* edges, uint64_t k) {
  return "edge " + std::to_string(k) + " (" + std::to_string(edges[k].src) + ", " + std::to_string(edges[k].dst) + ")";
}

// One mate entry's search: the reference's statics (pathFound, listOfEdges,
// pathLengths) as plain state, the recursion as an explicit stack.
struct Explorer {
  const PathInput& in;
  const std::vector<uint32_t>& lo;  // per edge: graph[dst] = edges [lo, hi)
  const std::vector<uint32_t>& hi;
  uint64_t budget;
  uint64_t visits = 0;
  bool over = false;
  uint32_t stk_e[kMaxLevel + 1], stk_cur[kMaxLevel + 1];
  uint64_t stk_len[kMaxLevel + 1];
  std::vector<uint32_t> fp, cp;  // firstPath, copyOfPath
  std::vector<uint8_t> ff, cf;   // flags, copyOfFlags

  Explorer(const PathInput& i, const std::vector<uint32_t>& l, const std::vector<uint32_t>& h, uint64_t b)
      : in(i), lo(l), hi(h), budget(b) {}

  bool spend() {
    ++visits;
    if (budget && visits > budget) over = true;
    return over;
  }

  // exploreGraph :1781-1870 from level 0; the number of paths found
  uint64_t explore(uint32_t first, uint32_t last, uint64_t d1, uint64_t d2, uint64_t bhi, uint64_t blo) {
    uint64_t found = 0;
    fp.clear();
    ff.clear();
    int level = 0;
    stk_e[0] = first;
    stk_len[0] = d1;
    stk_cur[0] = lo[first];
    for (;;) {
      const uint32_t e = stk_e[level], c = stk_cur[level];
      if (c >= hi[e]) {  // :1863 ends
        if (!level) break;
        --level;
        continue;
      }
      stk_cur[level] = c + 1;
      if (spend()) return 0;
      const uint64_t len = stk_len[level];
      if (!match_edge_type(in.edges[e].orient, in.edges[c].orient) || !(len < bhi)) continue;  // :1866
      const int nl = level + 1;
      if (nl > kMaxLevel) continue;  // :1800
      if (c == last) {               // :1810
        const uint64_t total = d2 + len;
        if (total >= blo && total <= bhi) {  // :1812
          ++found;
          if (found == 1) {  // :1817-1825
            fp.assign(stk_e, stk_e + nl);
            fp.push_back(c);
            ff.assign((size_t)nl, 1);
          } else {  // :1828-1838: the path is stk_e[0 .. level], c
            for (size_t k = 0; k + 1 < fp.size(); ++k) {
              if (spend()) return 0;
              bool adjacent = false;
              for (int j = 0; j < nl && !adjacent; ++j)
                adjacent = fp[k] == stk_e[j] && fp[k + 1] == (j + 1 < nl ? stk_e[j + 1] : c);
              if (!adjacent) ff[k] = 0;
            }
          }
          continue;  // :1848
        }
      }
      stk_e[nl] = c;  // :1852-1859
      stk_len[nl] = in.edges[c].offset + len;
      stk_cur[nl] = lo[c];
      level = nl;
    }
    return found;
  }

  // findPathBetweenMatepairs :1645-1730 for owner a and its entry mt
  uint8_t entry(uint64_t a, const mg_mate& mt) {
    visits = 0;
    over = false;
    cp.clear();
    cf.clear();
    if (a > mt.id || in.mean[mt.dataset] == 0) return MG_PATH_SKIPPED;  // :1911-1914
    const uint32_t want1 = (mt.orient == 2 || mt.orient == 3) ? 1u : 0u;  // :1657
    const uint32_t want2 = (mt.orient == 0 || mt.orient == 2) ? 1u : 0u;  // :1664
    const uint64_t p0 = in.place_start[a], p1 = in.place_start[a + 1];
    const uint64_t q0 = in.place_start[mt.id], q1 = in.place_start[mt.id + 1];
    uint64_t n1 = 0, n2 = 0;
    for (uint64_t p = p0; p < p1; ++p) n1 += (in.places[p].flags & 1u) == want1;
    for (uint64_t q = q0; q < q1; ++q) n2 += (in.places[q].flags & 1u) == want2;
    if (!n1 || !n2) return MG_PATH_SAME_EDGE;  // :1667
    for (uint64_t p = p0; p < p1; ++p) {       // :1673-1684
      if ((in.places[p].flags & 1u) != want1) continue;
      for (uint64_t q = q0; q < q1; ++q) {
        if ((in.places[q].flags & 1u) != want2) continue;
        if (spend()) return MG_PATH_DEFERRED;
        const uint32_t first = in.places[p].edge, last = in.places[q].edge;
        if (first == last || first == in.twin[last]) return MG_PATH_SAME_EDGE;
      }
    }
    const uint64_t mean = in.mean[mt.dataset], sd = in.sd[mt.dataset];
    const uint64_t bhi = mean + 3 * sd, blo = mean - 3 * sd;  // (mod 2^64)
    for (uint64_t p = p0; p < p1; ++p) {                       // :1687-1728
      if ((in.places[p].flags & 1u) != want1) continue;
      for (uint64_t q = q0; q < q1; ++q) {
        if ((in.places[q].flags & 1u) != want2) continue;
        const uint32_t first = in.places[p].edge, last = in.places[q].edge;
        const uint64_t d1 = in.edges[first].offset - in.places[p].distance;  // :1695
        const uint64_t d2 = in.places[q].distance;
        if (!(d1 + d2 < bhi)) continue;  // :1697
        const uint64_t found = explore(first, last, d1, d2, bhi, blo);
        if (over) return MG_PATH_DEFERRED;
        if (!found) continue;
        if (cp.empty()) {  // :1703-1709
          cp = fp;
          cf = ff;
        } else {  // :1713-1722
          for (size_t k = 0; k + 1 < cp.size(); ++k) {
            if (spend()) return MG_PATH_DEFERRED;
            bool kept = false;
            for (size_t l = 0; l + 1 < fp.size() && !kept; ++l)
              kept = cp[k] == fp[l] && cp[k + 1] == fp[l + 1] && ff[l] == 1;
            if (!kept) cf[k] = 0;
          }
        }
      }
    }
    return cp.empty() ? MG_PATH_NONE : MG_PATH_FOUND;
  }
};

}  // namespace

int paths_validate(const PathInput& in, std::string* err) {
  if (err) err->clear();
  if ((in.n_edges && (!in.edges || !in.twin)) || !in.place_start || !in.mate_start ||
      (in.n_datasets && (!in.mean || !in.sd)) || in.n_datasets > 256 || (in.n_edges >> 31))
    return -1;
  const uint64_t entries = in.n_reads + 2;
  if (in.place_start[0] != 0 || in.mate_start[0] != 0) return -1;
  for (uint64_t a = 0; a + 1 < entries; ++a)
    if (in.place_start[a + 1] < in.place_start[a] || in.mate_start[a + 1] < in.mate_start[a]) return -1;
  const uint64_t P = in.place_start[entries - 1], M = in.mate_start[entries - 1];
  if ((P && !in.places) || (M && !in.mates) || (P >> 31) || (M >> 31)) return -1;
  for (uint64_t k = 1; k < in.n_edges; ++k)
    if (in.edges[k].src < in.edges[k - 1].src) {
      if (err) *err = edge_name(in.edges, k) + ": its source ID is below the previous edge's (-2)";
      return -2;
    }
  for (uint64_t k = 0; k < in.n_edges; ++k)
    if (in.twin[k] >= in.n_edges) {
      if (err)
        *err = edge_name(in.edges, k) + ": its twin " + std::to_string(in.twin[k]) + " is not below " +
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

int mate_paths(const PathInput& in, uint64_t budget, const PathEntries* prior, PathEntries* out, std::string* err) {
  if (!out) return -1;
  if (const int rc = paths_validate(in, err)) return rc;
  const uint64_t M = in.mate_start[in.n_reads + 1];
  if (prior && (prior->status.size() != M || prior->visits.size() != M || prior->start.size() != M + 1 ||
                prior->path.size() != prior->start[M] || prior->flags.size() != prior->start[M]))
    return -1;
  // graph[v] = the edges with src == v: lower bounds over src
  std::vector<uint32_t> lo(in.n_edges), hi(in.n_edges);
  for (uint64_t k = 0; k < in.n_edges; ++k) {
    const uint32_t v = in.edges[k].dst;
    auto cmp = [](const mg_contig_edge& e, uint64_t x) { return (uint64_t)e.src < x; };
    lo[k] = (uint32_t)(std::lower_bound(in.edges, in.edges + in.n_edges, (uint64_t)v, cmp) - in.edges);
    hi[k] = (uint32_t)(std::lower_bound(in.edges, in.edges + in.n_edges, (uint64_t)v + 1, cmp) - in.edges);
  }
  out->status.assign(M, MG_PATH_SKIPPED);
  out->visits.assign(M, 0);
  out->start.assign(M + 1, 0);
  out->path.clear();
  out->flags.clear();
  Explorer ex(in, lo, hi, budget);
  for (uint64_t a = 1; a <= in.n_reads; ++a)  // :1904
    for (uint64_t m = in.mate_start[a]; m < in.mate_start[a + 1]; ++m) {
      out->start[m] = out->path.size();
      if (prior && prior->status[m] != MG_PATH_DEFERRED) {
        out->status[m] = prior->status[m];
        out->visits[m] = prior->visits[m];
        out->path.insert(out->path.end(), prior->path.begin() + prior->start[m], prior->path.begin() + prior->start[m + 1]);
        out->flags.insert(out->flags.end(), prior->flags.begin() + prior->start[m],
                          prior->flags.begin() + prior->start[m + 1]);
        continue;
      }
      const uint8_t st = ex.entry(a, in.mates[m]);
      out->status[m] = st;
      out->visits[m] = (uint32_t)std::min<uint64_t>(ex.visits, UINT32_MAX);
      if (st == MG_PATH_FOUND) {
        out->path.insert(out->path.end(), ex.cp.begin(), ex.cp.end());
        out->flags.insert(out->flags.end(), ex.cf.begin(), ex.cf.end());
        out->flags.push_back(0);  // the last edge starts no pair
      }
    }
  out->start[M] = out->path.size();
  return 0;
}

void path_pairs(const PathInput& in, const PathEntries& e, std::vector<mg_pair_support>* pairs, uint64_t* counters) {
  pairs->clear();
  if (counters) counters[0] = counters[1] = counters[2] = 0;
  std::unordered_map<uint64_t, size_t> where;  // canonical (a, b) -> its record
  for (size_t m = 0; m < e.status.size(); ++m) {
    if (counters) {
      if (e.status[m] == MG_PATH_NONE) counters[0]++;       // noPathsFound
      else if (e.status[m] == MG_PATH_FOUND) counters[1]++;  // pathsFound
      else if (e.status[m] == MG_PATH_SAME_EDGE) counters[2]++;
    }
    for (uint64_t p = e.start[m]; p + 1 < e.start[m + 1]; ++p) {  // :1931
      if (e.flags[p] != 1) continue;
      const uint32_t a = e.path[p], b = e.path[p + 1];
      if (in.edges[a].src == in.edges[a].dst && in.edges[b].src == in.edges[b].dst) continue;  // :1951
      const uint64_t k1 = ((uint64_t)a << 32) | b, k2 = ((uint64_t)in.twin[b] << 32) | in.twin[a];
      const auto it = where.find(std::min(k1, k2));
      if (it != where.end()) {
        (*pairs)[it->second].support += 1;
      } else {
        where.emplace(std::min(k1, k2), pairs->size());
        pairs->push_back(mg_pair_support{a, b, 1});
      }
    }
  }
}

namespace {
struct PairedEdges {  // pairedEdges :1874-1886
  uint32_t edge1, edge2;
  uint64_t support;
  bool freed;
  bool operator<(const PairedEdges& rhs) const { return support > rhs.support; }
};
}  // namespace

int merge_supported(UnitigGraph* u, const std::vector<uint32_t>& pool_of, const mg_pair_support* pairs, uint64_t n,
                    uint64_t min_support, uint64_t* merged, std::string* err) {
  if (err) err->clear();
  if (merged) *merged = 0;
  if (!u || (n && !pairs)) return -1;
  std::vector<PairedEdges> list(n);
  for (uint64_t i = 0; i < n; ++i) {
    if (pairs[i].edge1 >= pool_of.size() || pairs[i].edge2 >= pool_of.size()) {
      if (err) *err = "pair " + std::to_string(i) + ": an edge index outside the graph's " + std::to_string(pool_of.size()) + " edges";
      return -1;
    }
    list[i] = PairedEdges{pool_of[pairs[i].edge1], pool_of[pairs[i].edge2], pairs[i].support, false};
  }
  std::sort(list.begin(), list.end());  // :1968
  const auto in_pair = [&](uint32_t e, const uint32_t (&four)[4]) {
    return e == four[0] || e == four[1] || e == four[2] || e == four[3];
  };
  uint64_t count = 0;
  for (int pass = 0; pass < 2; ++pass) {  // a dry run first: a refused pair leaves the graph as it was
    for (auto& p : list) p.freed = false;
    for (uint64_t i = 0; i < n; ++i) {  // :1972-1992
      if (list[i].freed || list[i].support < min_support) continue;
      const uint32_t e1 = list[i].edge1, e2 = list[i].edge2;
      const uint32_t four[4] = {e1, u->pool[e1].rev, e2, u->pool[e2].rev};
      if (pass == 0) {
        if (e1 == e2 || e2 == four[1]) {
          if (err)
            *err = "supported pair (" + std::to_string(u->pool[e1].src) + ", " + std::to_string(u->pool[e1].dst) +
                   ") and (" + std::to_string(u->pool[e2].src) + ", " + std::to_string(u->pool[e2].dst) + "), support " +
                   std::to_string(list[i].support) +
                   (e1 == e2 ? ": one edge twice" : ": an edge and its twin") +
                   "; merging it would touch a removed edge (-5)";
          return -5;
        }
      } else {
        u->merge_edges(e1, e2);
        if (u->bad_merge) return -4;
        ++count;
      }
      for (uint64_t j = i + 1; j < n; ++j)
        if (in_pair(list[j].edge1, four) || in_pair(list[j].edge2, four)) list[j].freed = true;
    }
  }
  if (merged) *merged = count;
  return 0;
}

}  // namespace mg
