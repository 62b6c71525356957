// ref_places_main.cpp — FIXTURE GENERATION ONLY (tests/golden/). Never linked
// into the product, never run by a test.
//
// Driver that runs the *reference* read-location, insert-size and coverage path
// (the reference's own sources, compiled in place by make_places_golden.py into
// oracle/_ref/) and dumps what it leaves.  No reference source is copied: this
// file only #includes the reference headers where they lie, as
// oracle/ref_harness.cpp does.
//
//   ref_places build  <l> <out> <n_pe> <pe files...> <se files...>
//        main.cpp:45-49: Dataset -> HashTable -> OverlapGraph(ht) -> sortEdges
//   ref_places resume <l> <out> <unitig> <n_pe> <pe files...> <se files...>
//        main.cpp:38-41: OverlapGraph() -> setDataset -> readGraphFromFile -> sortEdges
// then calculateMeanAndSdOfInsertSize() (main.cpp:59) and getBaseByBaseCoverage
// of every edge.  Output, one record per line:
//   #N <unique reads>
//   #R <id> <frequency> <length>
//   #M <id> <mate> <orient> <dataset>        every mate list, reads in ID order
//   #E <k> <src> <dst> <orient> <offset> <n> <read:offset:orient>...
//                                            every edge of every list in list order
//   #L <F|R> <read> <k> <location>           the four location lists of every read
//   #O <line>                                the statistic's own stdout lines
//   #D <d> <mean> <sd> <insert sizes>
//   #C <k> <coverageDepth> <SD>              or "#C <k> !" where the reference throws
#define private public
#include "Dataset.h"
#include "HashTable.h"
#include "OverlapGraph.h"
#undef private

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <stdexcept>

struct NullBuf : std::streambuf {
  int overflow(int c) { return c; }
};

int main(int argc, char** argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: %s build|resume <l> <out> [<unitig>] <n_pe> <pe files...> <se files...>\n", argv[0]);
    return 2;
  }
  const bool resume = !strcmp(argv[1], "resume");
  const UINT64 l = strtoull(argv[2], NULL, 10);
  const int at = resume ? 5 : 4;
  const int n_pe = atoi(argv[at]);
  vector<string> pe, se;
  for (int i = at + 1; i < argc; i++) (i - at - 1 < n_pe ? pe : se).push_back(argv[i]);
  FILE* f = fopen(argv[3], "w");
  if (!f) return 1;
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
  const UINT64 n = ds->getNumberOfUniqueReads();
  fprintf(f, "#N %llu\n", (unsigned long long)n);
  for (UINT64 i = 1; i <= n; i++)
    fprintf(f, "#R %llu %llu %llu\n", (unsigned long long)i, (unsigned long long)ds->getReadFromID(i)->getFrequency(),
            (unsigned long long)ds->getReadFromID(i)->getReadLength());
  for (UINT64 i = 1; i <= n; i++) {
    vector<MPlist>* m = ds->getReadFromID(i)->getMatePairList();
    for (UINT64 j = 0; j < m->size(); j++)
      fprintf(f, "#M %llu %llu %d %d\n", (unsigned long long)i, (unsigned long long)m->at(j).matePairID,
              (int)m->at(j).matePairOrientation, (int)m->at(j).datasetNumber);
  }
  std::map<Edge*, UINT64> index;
  vector<Edge*> all;
  for (UINT64 i = 1; i <= n; i++)
    for (UINT64 j = 0; j < og->graph->at(i)->size(); j++) {
      Edge* e = og->graph->at(i)->at(j);
      index[e] = all.size();
      fprintf(f, "#E %llu %llu %llu %d %llu %llu", (unsigned long long)all.size(),
              (unsigned long long)e->getSourceRead()->getReadNumber(),
              (unsigned long long)e->getDestinationRead()->getReadNumber(), (int)e->getOrientation(),
              (unsigned long long)e->getOverlapOffset(), (unsigned long long)e->getListOfReads()->size());
      for (UINT64 k = 0; k < e->getListOfReads()->size(); k++)
        fprintf(f, " %llu:%d:%d", (unsigned long long)e->getListOfReads()->at(k),
                (int)e->getListOfOverlapOffsets()->at(k), (int)e->getListOfOrientations()->at(k));
      fprintf(f, "\n");
      all.push_back(e);
    }
  for (UINT64 i = 1; i <= n; i++) {
    Read* r = ds->getReadFromID(i);
    for (UINT64 j = 0; j < r->getListOfEdgesForward()->size(); j++)
      fprintf(f, "#L F %llu %llu %llu\n", (unsigned long long)i,
              (unsigned long long)index[r->getListOfEdgesForward()->at(j)],
              (unsigned long long)r->getLocationOnEdgeForward()->at(j));
    for (UINT64 j = 0; j < r->getListOfEdgesReverse()->size(); j++)
      fprintf(f, "#L R %llu %llu %llu\n", (unsigned long long)i,
              (unsigned long long)index[r->getListOfEdgesReverse()->at(j)],
              (unsigned long long)r->getLocationOnEdgeReverse()->at(j));
  }
  std::ostringstream said;
  cout.rdbuf(said.rdbuf());
  og->calculateMeanAndSdOfInsertSize();
  cout.rdbuf(&nb);
  {
    std::istringstream in(said.str());
    string line;
    vector<UINT64> count(pe.size(), 0);
    long d = -1;
    while (getline(in, line)) {
      const bool keep = !line.compare(0, 12, "Mean set to:") || !line.compare(0, 10, "SD set to:") ||
                        !line.compare(0, 19, "Reads on same edge:") || !line.compare(0, 21, "No insert-size found ");
      if (!line.compare(0, 36, "Calculating mean and SD of dataset: ")) d = atol(line.c_str() + 36);
      if (!line.compare(0, 19, "Reads on same edge:") && d >= 0) count[d] = strtoull(line.c_str() + 19, NULL, 10);
      if (keep) fprintf(f, "#O %s\n", line.c_str());
    }
    for (UINT64 k = 0; k < og->meanOfInsertSizes.size(); k++)
      fprintf(f, "#D %llu %llu %llu %llu\n", (unsigned long long)k, (unsigned long long)og->meanOfInsertSizes.at(k),
              (unsigned long long)og->sdOfInsertSizes.at(k), (unsigned long long)count[k]);
  }
  for (UINT64 k = 0; k < all.size(); k++) {
    try {
      og->getBaseByBaseCoverage(all[k]);
      fprintf(f, "#C %llu %llu %llu\n", (unsigned long long)k, (unsigned long long)all[k]->coverageDepth,
              (unsigned long long)all[k]->SD);
    } catch (const std::exception&) {
      fprintf(f, "#C %llu !\n", (unsigned long long)k);
    }
  }
  cout.rdbuf(old);
  fclose(f);
  return 0;
}
