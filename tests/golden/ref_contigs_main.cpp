// ref_contigs_main.cpp — FIXTURE GENERATION ONLY (tests/golden/). Never linked
// into the product, never run by a test.
//
// Driver that runs the *reference* printGraph / getStringInEdge (the reference's
// own sources, compiled in place by make_contig_golden.py into oracle/_ref/) and
// dumps what they give.  No reference source is copied: this file only
// #includes the reference headers where they lie, as oracle/ref_harness.cpp does.
//
//   ref_contigs build  <l> <out prefix> <fasta>...          main.cpp:45-55 without calculateFlow:
//        Dataset -> HashTable -> OverlapGraph(ht) -> sortEdges -> printGraph
//   ref_contigs resume <l> <out prefix> <unitig> <fasta>... main.cpp:38-41, then printGraph:
//        OverlapGraph() -> setDataset -> readGraphFromFile -> sortEdges -> printGraph
// Writes <prefix>.gdl and <prefix>.fa (printGraph's two files verbatim),
// <prefix>.estrings: one line "src dst orient offset nreads string" per edge of
// every list in list order (getStringInEdge of every edge, both directions; a
// string that throws is written as "!"), and <prefix>.loops: one line
// "src list-position" per self-loop edge the reference listed as a contig (:460
// compares two pointers, so which twin it lists depends on the allocator).
#define private public
#include "Dataset.h"
#include "HashTable.h"
#include "OverlapGraph.h"
#undef private

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

struct NullBuf : std::streambuf {
  int overflow(int c) { return c; }
};

int main(int argc, char** argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: %s build|resume <l> <out prefix> [<unitig>] <fasta>...\n", argv[0]);
    return 2;
  }
  const bool resume = !strcmp(argv[1], "resume");
  const UINT64 l = strtoull(argv[2], NULL, 10);
  const string prefix = argv[3];
  vector<string> pe, se;
  for (int i = resume ? 5 : 4; i < argc; i++) se.push_back(argv[i]);
  NullBuf nb;
  std::streambuf* old = cout.rdbuf(&nb);
  Dataset* ds = new Dataset(pe, se, l);
  OverlapGraph* og;
  if (resume) {
    og = new OverlapGraph();
    og->setDataset(ds);
    og->readGraphFromFile(argv[4]);
  } else {
    HashTable* ht = new HashTable();
    ht->insertDataset(ds, l);
    og = new OverlapGraph(ht);
  }
  og->sortEdges();
  FILE* f = fopen((prefix + ".estrings").c_str(), "w");
  FILE* fl = fopen((prefix + ".loops").c_str(), "w");
  if (!f || !fl) return 1;
  bool any = false;
  for (UINT64 i = 1; i <= ds->getNumberOfUniqueReads(); i++) {
    for (UINT64 j = 0; j < og->graph->at(i)->size(); j++) {
      Edge* e = og->graph->at(i)->at(j);
      any = true;
      string s;
      try {
        s = og->getStringInEdge(e);
      } catch (const std::exception&) {
        s = "!";
      }
      fprintf(f, "%llu %llu %d %llu %llu %s\n", (unsigned long long)e->getSourceRead()->getReadNumber(),
              (unsigned long long)e->getDestinationRead()->getReadNumber(), (int)e->getOrientation(),
              (unsigned long long)e->getOverlapOffset(), (unsigned long long)e->getListOfReads()->size(), s.c_str());
      if (e->getSourceRead() == e->getDestinationRead() && e < e->getReverseEdge())
        fprintf(fl, "%llu %llu\n", (unsigned long long)i, (unsigned long long)j);
    }
  }
  fclose(f);
  fclose(fl);
  // printGraph's closing statistics read graph->at(highestDegreeNode), which is
  // uninitialised for a graph without edges: the files are complete before that
  if (any) {
    og->printGraph(prefix + ".gdl", prefix + ".fa");
  } else {
    try {
      og->printGraph(prefix + ".gdl", prefix + ".fa");
    } catch (const std::exception&) {
    }
  }
  cout.rdbuf(old);
  return 0;
}
