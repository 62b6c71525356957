// mg_mates.cpp — host mirror of the mate-pair path (see mg_mates.hpp).
#include "mg_mates.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mg_host.h"

namespace mg {

namespace {

// an ifstream reduced to what the reference's loop observes
struct Stream {
  const char* p;
  uint64_t n, pos = 0;
  bool eof = false, fail = false;
  // std::getline: a stream that is not good only gains failbit and the string
  // keeps its text; else the string is cleared, characters up to the delimiter
  // (consumed, not stored) or the end of the file (eofbit; failbit as well when
  // nothing was extracted) are stored
  void getline(std::string& s, char delim = '\n') {
    if (eof || fail) {
      fail = true;
      return;
    }
    s.clear();
    const void* q = pos < n ? std::memchr(p + pos, delim, n - pos) : nullptr;
    if (q) {
      const uint64_t e = (uint64_t)(static_cast<const char*>(q) - p);
      s.assign(p + pos, e - pos);
      pos = e + 1;
    } else {
      s.assign(p + pos, n - pos);
      pos = n;
      eof = true;
      if (s.empty()) fail = true;
    }
  }
};

void erase_newlines(std::string& s) { s.erase(std::remove(s.begin(), s.end(), '\n'), s.end()); }

// Dataset::testRead (Dataset.cpp:398-413) on an upper-cased string
bool test_read(const std::string& read) {
  uint64_t cnt[4] = {0, 0, 0, 0};
  for (char c : read) {
    if (c != 'A' && c != 'C' && c != 'G' && c != 'T') return false;
    cnt[(c >> 1) & 3]++;
  }
  const uint64_t threshold = (uint64_t)(read.length() * .8);
  return !(cnt[0] >= threshold || cnt[1] >= threshold || cnt[2] >= threshold || cnt[3] >= threshold);
}

// Dataset::reverseComplement (Dataset.cpp:463-475)
std::string reverse_complement(const std::string& read) {
  const size_t n = read.length();
  std::string r(n, '0');
  for (size_t i = 0; i < n; ++i) r[n - i - 1] = (read[i] & 0x02) ? (char)(read[i] ^ 0x04) : (char)(read[i] ^ 0x15);
  return r;
}

inline uint64_t code_of(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3; }

std::string decode(const uint64_t* w, uint32_t len) {
  std::string s(len, 'A');
  for (uint32_t p = 0; p < len; ++p) s[p] = "ACGT"[(w[p >> 5] >> (62 - 2 * (p & 31))) & 3];
  return s;
}

std::string upper(const char* p, uint64_t n) {
  std::string s(p, n);
  for (char& c : s) c = (char)toupper((unsigned char)c);
  return s;
}

}  // namespace

int read_pairs_buffer(const char* buf, uint64_t n, std::string& text, std::vector<uint64_t>& offsets,
                      uint64_t* n_pairs) {
  if (offsets.empty()) offsets.push_back(0);
  if (n_pairs) *n_pairs = 0;
  Stream f{buf, n};
  std::string t, line[8];
  enum { FASTA, FASTQ, UNDEFINED } type = UNDEFINED;
  uint64_t pairs = 0;
  auto push = [&](const std::string& s) {
    text += s;
    offsets.push_back(text.size());
  };
  while (!f.eof) {
    if (type == UNDEFINED) {  // Dataset.cpp:231-241
      f.getline(t);
      if (!t.empty() && t[0] == '>') type = FASTA;
      else if (!t.empty() && t[0] == '@') type = FASTQ;
      else return -2;
      f.pos = 0;  // seekg(0, ios::beg) (clears eofbit)
      f.eof = false;
    }
    if (type == FASTA) {  // :243-257
      f.getline(t);
      f.getline(t, '>');
      line[1] = t;
      f.getline(t);
      f.getline(t, '>');
      line[3] = t;
      erase_newlines(line[1]);
      erase_newlines(line[3]);
      push(line[1]);
      push(line[3]);
    } else {  // :258-267
      for (int i = 0; i < 8; ++i) {
        f.getline(t);
        line[i] = t;
      }
      push(line[1]);
      push(line[5]);
    }
    ++pairs;
  }
  if (n_pairs) *n_pairs = pairs;
  return 0;
}

int read_pairs_file(const std::string& path, std::string& text, std::vector<uint64_t>& offsets, uint64_t* n_pairs) {
  if (n_pairs) *n_pairs = 0;
  FILE* fp = std::fopen(path.c_str(), "rb");
  if (!fp) return -1;
  std::string data;
  char chunk[1 << 16];
  size_t got;
  while ((got = std::fread(chunk, 1, sizeof(chunk), fp)) > 0) data.append(chunk, got);
  std::fclose(fp);
  return read_pairs_buffer(data.data(), data.size(), text, offsets, n_pairs);
}

uint64_t find_packed_read(const uint64_t* words, const uint16_t* lens, uint64_t n_reads, uint32_t wpr,
                          const std::string& read) {
  // the strand getReadFromString searches for (Dataset.cpp:424-427, :440-445)
  const std::string rev = reverse_complement(read);
  const std::string& s = read.compare(rev) < 0 ? read : rev;
  if (!n_reads || s.size() > 32ull * wpr) return 0;
  std::vector<uint64_t> q(wpr, 0);
  for (size_t p = 0; p < s.size(); ++p) q[p >> 5] |= code_of(s[p]) << (62 - 2 * (p & 31));
  // std::string::compare on the packed reads: words first (zero padding reads
  // as 'A'), then length
  uint64_t lo = 0, hi = n_reads;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) / 2;
    const uint64_t* r = words + mid * wpr;
    int c = 0;
    for (uint32_t k = 0; k < wpr && !c; ++k)
      if (r[k] != q[k]) c = r[k] < q[k] ? -1 : 1;
    if (!c) c = lens[mid] < s.size() ? -1 : lens[mid] > s.size() ? 1 : 0;
    if (!c) return mid + 1;
    if (c < 0) lo = mid + 1;
    else hi = mid;
  }
  return 0;
}

int MatePairs::build(const uint64_t* words, const uint16_t* lens, uint64_t n_reads, uint32_t wpr,
                     const uint32_t* super, const char* concat, const uint64_t* offsets, uint64_t n_raw,
                     const uint64_t* pairs_per_dataset, uint32_t n_datasets, uint32_t min_overlap, std::string* err) {
  auto bad = [&](const char* m) {
    if (err) *err = m;
    return -1;
  };
  start.assign(n_reads + 2, 0);
  recs.clear();
  good_pairs = bad_pairs = 0;
  not_found = -1;
  if (n_raw & 1) return bad("n_raw must be even (two mates per pair)");
  if (n_raw && (!concat || !offsets)) return bad("null argument");
  if (n_reads && (!words || !lens || !wpr)) return bad("null argument");
  if (n_datasets > 256) return bad("more than 256 datasets (datasetNumber is UINT8)");
  if (n_datasets && !pairs_per_dataset) return bad("null argument");
  const uint64_t n_pairs = n_raw / 2;
  uint64_t sum = 0;
  for (uint32_t d = 0; d < n_datasets; ++d) {
    if (pairs_per_dataset[d] > n_pairs - sum) return bad("pairs_per_dataset does not add up to n_raw / 2");
    sum += pairs_per_dataset[d];
  }
  if (sum != n_pairs) return bad("pairs_per_dataset does not add up to n_raw / 2");
  if (super)
    for (uint64_t a = 1; a <= n_reads; ++a)
      if (super[a] > n_reads) return bad("a superReadID is outside 0..n_reads");

  std::vector<std::vector<mg_mate>> lists(n_reads + 1);
  // Read::addMatePair (Read.cpp:132-166)
  auto add_mate_pair = [&](uint64_t owner, uint64_t id, uint8_t orientation, uint8_t dataset) {
    std::vector<mg_mate>& l = lists[owner];
    size_t i = 0;
    for (; i < l.size(); ++i)
      if (l[i].id == id && l[i].orient == orientation && l[i].dataset == dataset) break;
    if (i == l.size()) l.push_back(mg_mate{(uint32_t)id, orientation, dataset, 0});
  };
  uint64_t p = 0;
  for (uint32_t d = 0; d < n_datasets; ++d) {
    for (uint64_t k = 0; k < pairs_per_dataset[d]; ++k, ++p) {
      const uint64_t i1 = 2 * p, i2 = 2 * p + 1;
      if (offsets[i1 + 1] < offsets[i1] || offsets[i2 + 1] < offsets[i2]) return bad("record offsets must not decrease");
      const uint64_t n1 = offsets[i1 + 1] - offsets[i1], n2 = offsets[i2 + 1] - offsets[i2];
      // the length test first, as :275 does (the UINT16 bound is the ingest's)
      if (!(n1 > min_overlap && n2 > min_overlap && n1 <= 65535 && n2 <= 65535)) {
        ++bad_pairs;
        continue;
      }
      const std::string line1 = upper(concat + offsets[i1], n1), line2 = upper(concat + offsets[i2], n2);
      if (!(test_read(line1) && test_read(line2))) {
        ++bad_pairs;
        continue;
      }
      ++good_pairs;
      uint64_t r1 = find_packed_read(words, lens, n_reads, wpr, line1);
      uint64_t r2 = find_packed_read(words, lens, n_reads, wpr, line2);
      if (!r1 || !r2) {
        if (not_found < 0) not_found = (int64_t)(!r1 ? i1 : i2);
        continue;
      }
      if (super && super[r1]) r1 = super[r1];  // once, not transitively (:280-284)
      if (super && super[r2]) r2 = super[r2];
      const std::string f1 = decode(words + (r1 - 1) * wpr, lens[r1 - 1]);
      const std::string f2 = decode(words + (r2 - 1) * wpr, lens[r2 - 1]);
      const uint8_t orient1 = f1.find(line1) != std::string::npos ? 1 : 0;  // :291-292
      const uint8_t orient2 = f2.find(line2) != std::string::npos ? 1 : 0;
      add_mate_pair(r1, r2, (uint8_t)(orient1 * 2 + orient2), (uint8_t)d);  // :294-295
      add_mate_pair(r2, r1, (uint8_t)(orient1 + orient2 * 2), (uint8_t)d);
    }
  }
  if (not_found >= 0) {
    if (err) *err = "String not found in Dataset: raw record " + std::to_string(not_found);
    return -2;
  }
  for (uint64_t a = 1; a <= n_reads; ++a) start[a + 1] = start[a] + lists[a].size();
  recs.reserve(start[n_reads + 1]);
  for (uint64_t a = 1; a <= n_reads; ++a) recs.insert(recs.end(), lists[a].begin(), lists[a].end());
  return 0;
}

}  // namespace mg

namespace {
template <typename T>
T* to_malloc(const T* src, size_t n) {
  T* p = static_cast<T*>(std::malloc(std::max<size_t>(n, 1) * sizeof(T)));
  if (p && n) std::memcpy(p, src, n * sizeof(T));
  return p;
}
}  // namespace

extern "C" {

int mgh_read_pairs(const char* const* paths, int nfiles, char** text, uint64_t** offsets, uint64_t* n_records,
                   uint64_t* pairs_per_file, double* seconds) {
  if (!text || !offsets || !n_records || nfiles < 0 || (nfiles && !paths)) return -3;
  const auto t0 = std::chrono::steady_clock::now();
  std::string t;
  std::vector<uint64_t> o{0};
  for (int f = 0; f < nfiles; ++f) {
    uint64_t np = 0;
    const int rc = mg::read_pairs_file(paths[f], t, o, &np);
    if (rc) return rc;
    if (pairs_per_file) pairs_per_file[f] = np;
  }
  *text = to_malloc(t.data(), t.size());
  *offsets = to_malloc(o.data(), o.size());
  if (!*text || !*offsets) {
    std::free(*text);
    std::free(*offsets);
    return -3;
  }
  *n_records = o.size() - 1;
  if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

int mgh_read_pairs_buffer(const char* buf, uint64_t n, char** text, uint64_t** offsets, uint64_t* n_records) {
  if (!text || !offsets || !n_records || (n && !buf)) return -3;
  std::string t;
  std::vector<uint64_t> o{0};
  const int rc = mg::read_pairs_buffer(buf, n, t, o, nullptr);
  if (rc) return rc;
  *text = to_malloc(t.data(), t.size());
  *offsets = to_malloc(o.data(), o.size());
  if (!*text || !*offsets) {
    std::free(*text);
    std::free(*offsets);
    return -3;
  }
  *n_records = o.size() - 1;
  return 0;
}

int mgh_mate_pairs_build(const uint64_t* words, const uint16_t* lens, uint64_t n_reads, uint32_t words_per_read,
                         const uint32_t* super, const char* concat, const uint64_t* offsets, uint64_t n_raw,
                         const uint64_t* pairs_per_dataset, uint32_t n_datasets, uint32_t min_overlap,
                         uint64_t* start, mg_mate* out, uint64_t cap, uint64_t* n_records, uint64_t* good_bad_pairs,
                         int64_t* not_found) {
  mg::MatePairs mp;
  const int rc = mp.build(words, lens, n_reads, words_per_read, super, concat, offsets, n_raw, pairs_per_dataset,
                          n_datasets, min_overlap, nullptr);
  if (n_records) *n_records = mp.recs.size();
  if (good_bad_pairs) {
    good_bad_pairs[0] = mp.good_pairs;
    good_bad_pairs[1] = mp.bad_pairs;
  }
  if (not_found) *not_found = mp.not_found;
  if (rc) return rc;
  if (start) std::copy(mp.start.begin(), mp.start.end(), start);
  if (out) std::copy(mp.recs.begin(), mp.recs.begin() + std::min<uint64_t>(cap, mp.recs.size()), out);
  return 0;
}

}  // extern "C"
