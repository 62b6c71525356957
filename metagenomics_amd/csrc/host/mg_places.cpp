// mg_places.cpp — read placements, insert sizes and edge coverage on the host (see mg_places.hpp).
#include "mg_places.hpp"

#include <cmath>

namespace mg {

namespace {

std::string edge_name(const mg_contig_edge* edges, uint64_t k) {
  return "edge " + std::to_string(k) + " (" + std::to_string(edges[k].src) + ", " + std::to_string(edges[k].dst) + ")";
}

int check_lists(const mg_contig_edge* edges, uint64_t n_edges, const uint32_t* reads, const uint16_t* offs,
                const uint8_t* ors, uint64_t n_list, std::string* err) {
  if ((n_edges && !edges) || (n_list && (!reads || !offs || !ors))) return -1;
  for (uint64_t k = 0; k < n_edges; ++k)
    if (edges[k].first > n_list || edges[k].n > n_list - edges[k].first) {
      if (err) *err = edge_name(edges, k) + ": its list range lies outside the " + std::to_string(n_list) + " list entries";
      return -1;
    }
  return 0;
}

}  // namespace

int placements_build(uint64_t n_reads, const mg_contig_edge* edges, uint64_t n_edges, const uint32_t* reads,
                     const uint16_t* offs, const uint8_t* ors, uint64_t n_list, std::vector<uint64_t>* start,
                     std::vector<mg_place>* out, std::vector<uint32_t>* fwd_count, std::string* err) {
  if (err) err->clear();
  if (!start || !out || !fwd_count) return -1;
  if (const int rc = check_lists(edges, n_edges, reads, offs, ors, n_list, err)) return rc;
  start->assign(n_reads + 2, 0);
  fwd_count->assign(n_reads + 2, 0);
  uint64_t total = 0;
  for (uint64_t k = 0; k < n_edges; ++k) {
    for (uint64_t i = 0; i < edges[k].n; ++i) {
      const uint32_t id = reads[edges[k].first + i];
      if (id < 1 || id > n_reads) {
        if (err)
          *err = edge_name(edges, k) + ", list entry " + std::to_string(i) + ": read ID " + std::to_string(id) +
                 " outside 1.." + std::to_string(n_reads) + " (-2)";
        return -2;
      }
      (*start)[id + 1] += 1;
    }
    total += edges[k].n;
  }
  for (uint64_t a = 0; a + 1 < n_reads + 2; ++a) (*start)[a + 1] += (*start)[a];
  out->assign(total, mg_place{0, 0, 0});
  std::vector<uint64_t> cursor(start->begin(), start->end() - 1);
  for (uint64_t k = 0; k < n_edges; ++k) {
    uint64_t distance = 0;  // :1050
    for (uint64_t i = 0; i < edges[k].n; ++i) {
      const uint64_t q = edges[k].first + i;
      distance += offs[q];  // :1053
      const bool fwd = ors[q] == 1;  // :1055
      (*out)[cursor[reads[q]]++] = mg_place{(uint32_t)k, fwd ? 1u : 0u, distance};
      if (fwd) (*fwd_count)[reads[q]] += 1;
    }
  }
  return 0;
}

int insert_sizes(uint64_t n_reads, const uint64_t* place_start, const mg_place* places, const uint64_t* mate_start,
                 const mg_mate* mates, uint32_t n_datasets, uint64_t max_distance, uint64_t* sums, std::string* err) {
  if (err) err->clear();
  if (!place_start || !mate_start || (n_datasets && !sums) || n_datasets > 256) return -1;
  if (mate_start[0] != 0) return -1;
  for (uint64_t a = 0; a + 1 < n_reads + 2; ++a)
    if (mate_start[a + 1] < mate_start[a]) return -1;
  const uint64_t M = mate_start[n_reads + 1];
  if (M && !mates) return -1;
  if (place_start[n_reads + 1] && !places) return -1;
  for (uint64_t a = 0; a < n_reads + 1; ++a)  // every entry is validated before a sum is written
    for (uint64_t m = mate_start[a]; m < mate_start[a + 1]; ++m)
      if (a < 1 || a > n_reads || mates[m].id < 1 || mates[m].id > n_reads || mates[m].dataset >= n_datasets) {
        if (err)
          *err = "mate entry " + std::to_string(m) + ": its dataset is not below " + std::to_string(n_datasets) +
                 " or its owner or mate ID lies outside 1.." + std::to_string(n_reads) + " (-2)";
        return -2;
      }
  for (uint32_t i = 0; i < 3 * n_datasets; ++i) sums[i] = 0;
  for (uint64_t a = 1; a <= n_reads; ++a)                            // :1138 each read1
    for (uint64_t m = mate_start[a]; m < mate_start[a + 1]; ++m) {   // :1142 each mate read2
      const uint64_t b = mates[m].id;
      uint64_t* s = sums + 3 * (uint64_t)mates[m].dataset;           // :1144 (all datasets in one pass)
      for (uint64_t p = place_start[a]; p < place_start[a + 1]; ++p)      // :1162 each edge containing read1
        for (uint64_t q = place_start[b]; q < place_start[b + 1]; ++q)    // :1164 each edge containing read2
          if (places[p].edge == places[q].edge && places[p].distance > places[q].distance) {  // :1166
            const uint64_t x = places[p].distance - places[q].distance;
            if (x < max_distance) {  // :1168
              s[0] += 1;
              s[1] += x;
              s[2] += x * x;
            }
          }
    }
  return 0;
}

int edge_coverage(const uint16_t* lens, uint64_t n_reads, const mg_contig_edge* edges, uint64_t n_edges,
                  const uint32_t* reads, const uint16_t* offs, const uint8_t* ors, uint64_t n_list,
                  const uint32_t* fwd_count, const uint32_t* freq, uint64_t* out, std::string* err) {
  if (err) err->clear();
  if ((n_reads && (!lens || !freq || !fwd_count)) || (n_edges && !out)) return -1;
  if (const int rc = check_lists(edges, n_edges, reads, offs, ors, n_list, err)) return rc;
  for (uint64_t k = 0; k < n_edges; ++k)
    if (edges[k].offset >= (1ull << 40)) {
      if (err) *err = edge_name(edges, k) + ": an offset of 2^40 or more is not supported";
      return -1;
    }
  // where the reference's at() would throw: every edge is checked before a result is written
  for (uint64_t k = 0; k < n_edges; ++k) {
    const mg_contig_edge& e = edges[k];
    if (e.src < 1 || e.src > n_reads || e.dst < 1 || e.dst > n_reads) {
      if (err)
        *err = edge_name(edges, k) + ": its source or destination read ID lies outside 1.." + std::to_string(n_reads) +
               " (-2)";
      return -2;
    }
    const uint64_t L = e.offset + lens[e.dst - 1];
    uint64_t d = 0;
    for (uint64_t i = 0; i < e.n; ++i) {
      const uint32_t id = reads[e.first + i];
      if (id < 1 || id > n_reads) {
        if (err)
          *err = edge_name(edges, k) + ", list entry " + std::to_string(i) + ": read ID " + std::to_string(id) +
                 " outside 1.." + std::to_string(n_reads) + " (-2)";
        return -2;
      }
      d += offs[e.first + i];
      if (d + lens[id - 1] > L + 1) {
        if (err)
          *err = edge_name(edges, k) + ", list entry " + std::to_string(i) +
                 ": the read ends beyond the edge's counters (vector::at would throw) (-2)";
        return -2;
      }
    }
    if (lens[e.src - 1] > L + 1) {
      if (err)
        *err = edge_name(edges, k) + ": the source read is longer than the edge's counters (vector::at would throw) (-2)";
      return -2;
    }
  }
  std::vector<uint64_t> c;
  for (uint64_t k = 0; k < n_edges; ++k) {
    const mg_contig_edge& e = edges[k];
    uint64_t* o = out + 3 * k;
    o[0] = o[1] = o[2] = 0;
    if (!e.n) continue;  // all counters stay 0
    const uint64_t length = e.offset + lens[e.dst - 1];  // :2725
    c.assign(length + 1, 0);                             // :2726-2729
    uint64_t off = 0;
    for (uint64_t i = 0; i < e.n; ++i) {                 // :2731
      const uint32_t id = reads[e.first + i];
      off += offs[e.first + i];                          // :2734
      for (uint64_t j = off; j < off + lens[id - 1]; ++j) c[j] += freq[id - 1];  // :2736-2739
    }
    off = 0;
    for (uint64_t i = 0; i < e.n; ++i) {                 // :2743
      const uint32_t id = reads[e.first + i];
      off += offs[e.first + i];
      if (fwd_count[id] > 1)                             // :2748 (the forward list only)
        for (uint64_t j = off; j < off + lens[id - 1]; ++j) c[j] = 0;
    }
    for (uint64_t i = 0; i < lens[e.src - 1]; ++i) c[i] = 0;                 // :2756-2759
    for (uint64_t i = 0; i < lens[e.dst - 1]; ++i) c[c.size() - 1 - i] = 0;  // :2761-2764
    for (uint64_t x : c)                                 // :2768-2775 and the variance's terms
      if (x) {
        o[0] += 1;
        o[1] += x;
        o[2] += x * x;
      }
  }
  return 0;
}

void mean_sd(uint64_t count, uint64_t sum, uint64_t sumsq, uint64_t* mean, uint64_t* sd) {
  *mean = *sd = 0;
  if (!count) return;
  const uint64_t m = sum / count;
  const uint64_t variance = sumsq - 2 * m * sum + count * m * m;  // (mod 2^64)
  *mean = m;
  *sd = (uint64_t)std::sqrt((double)(variance / count));
}

}  // namespace mg
