// ref_scaffold_main.cpp — FIXTURE GENERATION ONLY (tests/golden/). Never linked
// into the product, never run by a test.
//
// Driver that runs the *reference* scaffolder (the reference's own sources,
// compiled in place by make_scaffold_golden.py into oracle/_ref/) and dumps
// what it computes.  No reference source is copied: this file only #includes
// the reference headers where they lie, as tests/golden/ref_paths_main.cpp does.
//
//   ref_scaffold build  <l> <out> <n_pe> <pe files...> <se files...>
//        main.cpp:45-49: Dataset -> HashTable -> OverlapGraph(ht) -> sortEdges
//   ref_scaffold resume <l> <out> <unitig> <n_pe> <pe files...> <se files...>
//        main.cpp:38-41: OverlapGraph() -> setDataset -> readGraphFromFile -> sortEdges
// then calculateMeanAndSdOfInsertSize() (main.cpp:59; no calculateFlow) and the
// real scaffolder() (main.cpp:85).  Output, one record per line, in the layout
// of ref_paths_main.cpp's dump:
//   #N <unique reads>
//   #R <id> <frequency> <length>
//   #M <id> <mate> <orient> <dataset>        every mate list, reads in ID order
//   #E <k> <src> <dst> <orient> <offset> <n> <read:offset:orient>...
//   #T <k> <twin>
//   #L <F|R> <read> <k> <location>           the four location lists of every read, in list order
//   #D <d> <mean> <sd>
//   #O <line>                                every "are supported" line of the real call
//   #X <return value>
//   #G <src> <dst> <orient> <offset> <n> <read:offset:orient>...   every edge after the merge
// and <out>.unitig: saveGraphToFile after the merge.
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

struct NullBuf : std::streambuf {
  int overflow(int c) { return c; }
};

static void edge_row(FILE* f, Edge* e) {
  fprintf(f, "%llu %llu %d %llu %llu", (unsigned long long)e->getSourceRead()->getReadNumber(),
          (unsigned long long)e->getDestinationRead()->getReadNumber(), (int)e->getOrientation(),
          (unsigned long long)e->getOverlapOffset(), (unsigned long long)e->getListOfReads()->size());
  for (UINT64 k = 0; k < e->getListOfReads()->size(); k++)
    fprintf(f, " %llu:%d:%d", (unsigned long long)e->getListOfReads()->at(k), (int)e->getListOfOverlapOffsets()->at(k),
            (int)e->getListOfOrientations()->at(k));
  fprintf(f, "\n");
}

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
      fprintf(f, "#E %llu ", (unsigned long long)all.size());
      edge_row(f, e);
      all.push_back(e);
    }
  for (UINT64 k = 0; k < all.size(); k++)
    fprintf(f, "#T %llu %llu\n", (unsigned long long)k, (unsigned long long)index[all[k]->getReverseEdge()]);
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
  og->calculateMeanAndSdOfInsertSize();
  for (UINT64 k = 0; k < og->meanOfInsertSizes.size(); k++)
    fprintf(f, "#D %llu %llu %llu\n", (unsigned long long)k, (unsigned long long)og->meanOfInsertSizes.at(k),
            (unsigned long long)og->sdOfInsertSizes.at(k));
  std::ostringstream said;
  cout.rdbuf(said.rdbuf());
  const UINT64 merged = og->scaffolder();
  cout.rdbuf(&nb);
  {
    std::istringstream in(said.str());
    string line;
    while (getline(in, line))
      if (line.find(" are supported ") != string::npos) fprintf(f, "#O %s\n", line.c_str());
  }
  fprintf(f, "#X %llu\n", (unsigned long long)merged);
  for (UINT64 i = 1; i < og->graph->size(); i++)
    for (UINT64 j = 0; j < og->graph->at(i)->size(); j++) {
      fprintf(f, "#G ");
      edge_row(f, og->graph->at(i)->at(j));
    }
  og->saveGraphToFile(string(argv[3]) + ".unitig");
  cout.rdbuf(old);
  fclose(f);
  return 0;
}
