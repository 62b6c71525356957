// mg_contigs.cpp — getStringInEdge as pieces, and printGraph's writer (see mg_contigs.hpp).
#include "mg_contigs.hpp"

#include <algorithm>
#include <cstdio>

namespace mg {

namespace {

struct Piece {
  uint32_t id = 0;   // read ID
  uint32_t pos = 0;  // first base of the chosen strand that is written
  bool fwd = false, n = false, ok = false;
};

inline bool id_ok(uint64_t id, uint64_t n_reads) { return id >= 1 && id <= n_reads; }

// piece i of edge e (0 = source read, 1..n = list entries, n + 1 = tail)
Piece piece_of(const mg_contig_edge& e, uint64_t i, const uint16_t* lens, uint64_t n_reads, const uint32_t* reads,
               const uint16_t* offs, const uint8_t* ors) {
  Piece p;
  const uint32_t o = e.orient;
  if (i == 0) {
    p.id = e.src;
    p.fwd = o == 2 || o == 3;
    p.ok = id_ok(p.id, n_reads);
    return p;
  }
  if (i <= e.n) {
    const uint64_t q = e.first + i - 1;
    p.id = reads[q];
    p.fwd = ors[q] == 1;
    const uint32_t prev_id = i == 1 ? e.src : reads[q - 1];
    if (!id_ok(p.id, n_reads) || !id_ok(prev_id, n_reads)) return p;
    const uint32_t prev = lens[prev_id - 1], len = lens[p.id - 1], off = offs[q];
    if (off > prev || prev - off > len) return p;  // substr position outside [0, len]
    p.pos = prev - off;
    p.n = off == prev;
    p.ok = true;
    return p;
  }
  p.id = e.dst;
  p.fwd = o == 1 || o == 3;
  if (!id_ok(p.id, n_reads)) return p;
  const uint32_t len2 = lens[p.id - 1];
  if (e.n == 0) {
    if (!id_ok(e.src, n_reads)) return p;
    const uint32_t len1 = lens[e.src - 1];
    if (e.offset > len1 || len1 - e.offset > len2) return p;
    p.pos = len1 - (uint32_t)e.offset;
  } else {
    if (e.tail > len2) return p;
    p.pos = len2 - e.tail;
  }
  p.ok = true;
  return p;
}

inline uint32_t base_at(const uint64_t* w, uint32_t p) { return (uint32_t)(w[p >> 5] >> (62u - 2u * (p & 31u))) & 3u; }

}  // namespace

int contigs_build(const uint64_t* words, const uint16_t* lens, uint64_t n_reads, uint32_t wpr,
                  const mg_contig_edge* edges, uint64_t n_edges, const uint32_t* reads, const uint16_t* offs,
                  const uint8_t* ors, uint64_t n_list, std::vector<uint64_t>* start, std::string* out,
                  std::string* err, bool fill) {
  if (err) err->clear();
  if (out) out->clear();
  if ((n_edges && !edges) || (n_list && (!reads || !offs || !ors)) || (n_reads && (!lens || (fill && !words))) ||
      !start)
    return -1;
  start->assign(n_edges + 1, 0);
  // sizes first: every piece is validated before a base is read
  uint64_t total = 0;
  for (uint64_t k = 0; k < n_edges; ++k) {
    const mg_contig_edge& e = edges[k];
    if (e.first > n_list || e.n > n_list - e.first) {
      if (err)
        *err = "edge " + std::to_string(k) + " (" + std::to_string(e.src) + ", " + std::to_string(e.dst) +
               "): its list range lies outside the " + std::to_string(n_list) + " list entries";
      return -1;
    }
    (*start)[k] = total;
    for (uint64_t i = 0; i < (uint64_t)e.n + 2; ++i) {
      const Piece p = piece_of(e, i, lens, n_reads, reads, offs, ors);
      if (!p.ok) {
        if (err)
          *err = "edge " + std::to_string(k) + " (" + std::to_string(e.src) + ", " + std::to_string(e.dst) +
                 "), piece " + std::to_string(i) + " (" +
                 (i == 0 ? std::string("the source read")
                         : i <= e.n ? "list entry " + std::to_string(i - 1) : std::string("the destination read")) +
                 "): a read ID outside 1.." + std::to_string(n_reads) +
                 " or a substring position outside its read (std::string::substr would throw) (-2)";
        return -2;
      }
      total += (uint64_t)lens[p.id - 1] - p.pos + (p.n ? 1 : 0);
    }
  }
  (*start)[n_edges] = total;
  if (!fill || !out) return 0;
  out->resize(total);
  char* dst = total ? &(*out)[0] : nullptr;
  for (uint64_t k = 0; k < n_edges; ++k) {
    const mg_contig_edge& e = edges[k];
    for (uint64_t i = 0; i < (uint64_t)e.n + 2; ++i) {
      const Piece p = piece_of(e, i, lens, n_reads, reads, offs, ors);
      const uint64_t* w = words + (uint64_t)(p.id - 1) * wpr;
      const uint32_t len = lens[p.id - 1];
      if (p.n) *dst++ = 'N';
      if (p.fwd)
        for (uint32_t q = p.pos; q < len; ++q) *dst++ = "ACGT"[base_at(w, q)];
      else
        for (uint32_t q = p.pos; q < len; ++q) *dst++ = "ACGT"[3u - base_at(w, len - 1 - q)];
    }
  }
  return 0;
}

void contig_edges(const UnitigGraph& u, bool all, ContigLists* out) {
  *out = ContigLists();
  for (size_t v = 1; v < u.lists.size(); ++v) {
    for (uint32_t e : u.lists[v]) {
      const UnitigEdge& x = u.pool[e];
      if (!all && !(x.src < x.dst || (x.src == x.dst && e < x.rev))) continue;
      const EdgeReads* lr = u.reads[e].get();
      const EdgeReads* rr = u.reads[x.rev].get();
      mg_contig_edge c{};
      c.src = x.src;
      c.dst = x.dst;
      c.offset = x.offset;
      c.first = out->reads.size();
      c.n = lr ? (uint32_t)lr->reads.size() : 0;
      // the reverse edge's first offset; a composite edge whose twin has no list gets an
      // invalid tail (the reference's at(0) would throw)
      c.tail = c.n ? (rr && !rr->offs.empty() ? rr->offs[0] : 0xFFFFFFFFu) : 0;
      c.orient = x.orient;
      if (lr) {
        out->reads.insert(out->reads.end(), lr->reads.begin(), lr->reads.end());
        out->offs.insert(out->offs.end(), lr->offs.begin(), lr->offs.end());
        out->ors.insert(out->ors.end(), lr->ors.begin(), lr->ors.end());
      }
      out->edges.push_back(c);
      out->pool.push_back(e);
    }
  }
}

int print_graph(const UnitigGraph& u, const ContigLists& c, const uint64_t* start, const char* bases,
                const char* gdl_path, const char* fasta_path) {
  FILE* fg = std::fopen(gdl_path, "w");
  if (!fg) return -1;
  FILE* ff = std::fopen(fasta_path, "w");
  if (!ff) {
    std::fclose(fg);
    return -1;
  }
  std::string g =
      "graph: {\nlayoutalgorithm :forcedir\nfdmax:704\ntempmax:254\ntempmin:0\ntemptreshold:3\ntempscheme:3\n"
      "tempfactor:1.08\nrandomfactor:100\ngravity:0.0\nrepulsion:161\nattraction:43\nignore_singles:yes\n"
      "node.fontname:\"helvB10\"\nedge.fontname:\"helvB10\"\nnode.shape:box\nnode.width:80\nnode.height:20\n"
      "node.borderwidth:1\nnode.bordercolor:31\n";
  for (size_t i = 1; i < u.lists.size(); ++i)
    if (!u.lists[i].empty()) {
      const std::string s = std::to_string(i);
      g += "node: { title:\"" + s + "\" label: \"" + s + "\" }\n";
    }
  static const char* const kStyle[4] = {" arrowstyle: none backarrowstyle: solid color: red label: \"(",
                                        " backarrowstyle:solid arrowstyle:solid color: green label: \"(",
                                        " arrowstyle: none color: blue label: \"(",
                                        " arrowstyle:solid color: red label: \"("};
  for (size_t k = 0; k < c.edges.size(); ++k) {
    const mg_contig_edge& e = c.edges[k];
    if (e.orient > 3) continue;
    g += "edge: { source:\"" + std::to_string(e.src) + "\" target:\"" + std::to_string(e.dst) + "\" thickness: " +
         (e.n ? "3" : "1") + kStyle[e.orient] + std::to_string(u.pool[c.pool[k]].flow) + ",0x," +
         std::to_string(e.offset) + "," + std::to_string(e.n) + ")\" }\n";
  }
  g += "}";
  bool ok = std::fwrite(g.data(), 1, g.size(), fg) == g.size();
  ok = std::fclose(fg) == 0 && ok;

  std::vector<uint32_t> order(c.edges.size());
  for (size_t k = 0; k < order.size(); ++k) order[k] = (uint32_t)k;
  std::sort(order.begin(), order.end(),
            [&](uint32_t a, uint32_t b) { return c.edges[a].offset < c.edges[b].offset; });  // compareEdges
  std::reverse(order.begin(), order.end());
  std::string rec;
  for (size_t i = 0; i < order.size() && ok; ++i) {
    const uint32_t k = order[i];
    const mg_contig_edge& e = c.edges[k];
    const uint64_t len = start[k + 1] - start[k];
    char head[200];
    std::snprintf(head, sizeof head,
                  ">contig_%zu Flow: %10u Edge  (%10u, %10u) String Length: %10llu Coverage: %10u\n", i + 1,
                  (unsigned)u.pool[c.pool[k]].flow, e.src, e.dst, (unsigned long long)len, 0u);
    rec = head;
    uint64_t at = 0;
    do {  // 100 bases per line; an empty string still gives one empty line
      const uint64_t n = std::min<uint64_t>(100, len - at);
      if (n) rec.append(bases + start[k] + at, n);
      rec += '\n';
      at += 100;
    } while (at < len);
    ok = std::fwrite(rec.data(), 1, rec.size(), ff) == rec.size();
  }
  ok = std::fclose(ff) == 0 && ok;
  return ok ? 0 : -1;
}

}  // namespace mg
