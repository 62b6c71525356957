// mg_mates.hpp — host mirror of the reference's mate-pair path: the pair reader
// and the per-read mate lists (paths relative to the reference's MetaGenomics directory):
//   storeMatePairInformation   Dataset.cpp:208-310
//   getReadFromString          Dataset.cpp:421-455
//   Read::addMatePair          Read.cpp:132-166
// The device versions are mg_find_reads / mg_build_mate_pairs
// (include/mg_overlap.h); MatePairs::build is their checker, as
// Discoveries::build is for mg_build_discoveries.  No device is needed.
#ifndef MG_MATES_HPP_
#define MG_MATES_HPP_
#include <cstdint>
#include <string>
#include <vector>

#include "mg_overlap.h"

namespace mg {

// The mates of every pair of a paired-end file, as storeMatePairInformation's
// own loop extracts them (NOT readDataset's loop): the type from the first
// byte, then per iteration of while(!eof()) FASTQ = eight getlines (mates on
// lines 1 and 5), FASTA = getline, getline(.., '>'), getline, getline(.., '>')
// with only '\n' erased.  getline's rule is kept: the string is cleared only
// while the stream is good, so after the end of the file every further getline
// leaves the previous text.  Consequences: a FASTQ file that ends in a newline
// gives one more pair of two empty mates; a FASTA file with an odd record count
// pairs its last sequence with itself; CRLF leaves '\r' in the mates.
// Records 2p and 2p + 1 (bytes as in the file, case kept) are appended to
// text / offsets (offsets holds one leading 0 when empty).
// 0 = ok, -1 = cannot open, -2 = unknown format (first byte not '>' / '@').
int read_pairs_buffer(const char* buf, uint64_t n, std::string& text, std::vector<uint64_t>& offsets,
                      uint64_t* n_pairs);
int read_pairs_file(const std::string& path, std::string& text, std::vector<uint64_t>& offsets, uint64_t* n_pairs);

struct MatePairs {
  std::vector<uint64_t> start;  // n_reads + 2: the list of read A = recs[start[A] .. start[A + 1])
  std::vector<mg_mate> recs;    // every list in addMatePair's order
  uint64_t good_pairs = 0, bad_pairs = 0;
  int64_t not_found = -1;  // first raw index of a good mate without a read (build returned -2)

  // The per-pair body of storeMatePairInformation (Dataset.cpp:269-301) and
  // addMatePair over the packed unique reads in ID order (words_per_read words
  // each, lens[ID - 1]); super = superReadID per ID (n_reads + 1 entries) or
  // nullptr (every superReadID 0: OverlapGraph::setDataset's case).  Raw
  // record i = concat[offsets[i], offsets[i + 1]); records 2p, 2p + 1 = pair p;
  // pairs_per_dataset[d] pairs belong to paired-end file d.
  // 0 = ok; -1 = bad arguments (n_raw odd, counts that do not add up, more than
  // 256 datasets, a superReadID out of range); -2 = a good mate has no read
  // (the reference exits with "String not found in Dataset").
  int build(const uint64_t* words, const uint16_t* lens, uint64_t n_reads, uint32_t words_per_read,
            const uint32_t* super, const char* concat, const uint64_t* offsets, uint64_t n_raw,
            const uint64_t* pairs_per_dataset, uint32_t n_datasets, uint32_t min_overlap, std::string* err);
};

// Dataset::getReadFromString on the packed reads: the ID of the read equal to
// min(s, revcomp s) for an upper-case ACGT string, 0 when absent.
uint64_t find_packed_read(const uint64_t* words, const uint16_t* lens, uint64_t n_reads, uint32_t words_per_read,
                          const std::string& s);

}  // namespace mg
#endif  // MG_MATES_HPP_
