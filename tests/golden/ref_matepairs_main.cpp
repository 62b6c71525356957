// ref_matepairs_main.cpp — FIXTURE GENERATION ONLY (tests/golden/). Never linked
// into the product, never run by a test.
//
// Driver that runs the *reference* mate-pair path (the reference's own sources,
// compiled in place by make_matepair_golden.py into oracle/_ref/) and dumps
// every Read::getMatePairList().  No reference source is copied: this file only
// #includes the reference headers where they lie, as oracle/ref_harness.cpp does.
//
//   ref_matepairs <l> <out> <n_pe> <pe files...> <se files...>
//
// Block 1 (the build path, OverlapGraph.cpp:142): Dataset(pe, se, l) ->
//   HashTable::insertDataset -> markContainedReads -> readMatePairsFromFile().
// Block 0 (the resume path, OverlapGraph.h:79 setDataset): a fresh Dataset(pe,
//   se, l) whose superReadIDs are all zero -> readMatePairsFromFile().
// Output: "#N <unique reads>", "#R <id> <forward string>", "#S <id> <super>"
// for every contained read, then per block "#B <1|0>" and one
// "#M <id> <mate> <orient> <dataset>" line per list entry, reads in ID order,
// entries in list order.
#define private public
#include "Dataset.h"
#include "HashTable.h"
#include "OverlapGraph.h"
#undef private

#include <cstdio>
#include <cstdlib>

// the reference's progress chatter goes to std::cout
struct NullBuf : std::streambuf {
  int overflow(int c) { return c; }
};

static void dump_lists(FILE* f, Dataset* ds, int block) {
  fprintf(f, "#B %d\n", block);
  for (UINT64 i = 1; i <= ds->getNumberOfUniqueReads(); i++) {
    vector<MPlist>* l = ds->getReadFromID(i)->getMatePairList();
    for (UINT64 j = 0; j < l->size(); j++)
      fprintf(f, "#M %llu %llu %d %d\n", (unsigned long long)i, (unsigned long long)l->at(j).matePairID,
              (int)l->at(j).matePairOrientation, (int)l->at(j).datasetNumber);
  }
}

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s <l> <out> <n_pe> <pe files...> <se files...>\n", argv[0]);
    return 2;
  }
  const UINT64 l = strtoull(argv[1], NULL, 10);
  const int n_pe = atoi(argv[3]);
  vector<string> pe, se;
  for (int i = 4; i < argc; i++) (i - 4 < n_pe ? pe : se).push_back(argv[i]);
  FILE* f = fopen(argv[2], "w");
  if (!f) return 1;
  NullBuf nb;
  std::streambuf* old = cout.rdbuf(&nb);
  {
    Dataset* ds = new Dataset(pe, se, l);
    HashTable* ht = new HashTable();
    ht->insertDataset(ds, l);
    OverlapGraph* og = new OverlapGraph();
    og->hashTable = ht;
    og->dataSet = ds;
    og->graph = new vector<vector<Edge*>*>;
    for (UINT64 i = 0; i <= ds->getNumberOfUniqueReads(); i++) og->graph->push_back(new vector<Edge*>);
    og->markContainedReads();
    ds->readMatePairsFromFile();
    fprintf(f, "#N %llu\n", (unsigned long long)ds->getNumberOfUniqueReads());
    for (UINT64 i = 1; i <= ds->getNumberOfUniqueReads(); i++)
      fprintf(f, "#R %llu %s\n", (unsigned long long)i, ds->getReadFromID(i)->getStringForward().c_str());
    for (UINT64 i = 1; i <= ds->getNumberOfUniqueReads(); i++)
      if (ds->getReadFromID(i)->superReadID)
        fprintf(f, "#S %llu %llu\n", (unsigned long long)i, (unsigned long long)ds->getReadFromID(i)->superReadID);
    dump_lists(f, ds, 1);
  }
  {
    Dataset* ds = new Dataset(pe, se, l);
    ds->readMatePairsFromFile();
    dump_lists(f, ds, 0);
  }
  cout.rdbuf(old);
  fclose(f);
  return 0;
}
