// mg_api.hpp — drop-in C++ surface for the reference's overlap path.
//
// Same class names, method names and argument meaning as the reference's
// Read / Edge / Dataset / HashTable / OverlapGraph (Read.h:31-72,
// Edge.h:16-61, Dataset.h:18-51, HashTable.h:16-36, OverlapGraph.h:32-100 in
// /root/reference/MetaGenomics), so main.cpp:33,45-47 compiles against it:
//
//     Dataset *dataSet = new Dataset(pairedEndFileNames, singleEndFileNames, l);
//     HashTable *hashTable = new HashTable();
//     hashTable->insertDataset(dataSet, l);              // GPU index build
//     OverlapGraph *g = new OverlapGraph(hashTable);     // GPU discovery, deletes hashTable
//
// Differences, all deliberate:
//  * errors throw mg::Error instead of MYEXIT's exit(0) (Common.h:47);
//  * reads are stored 2-bit packed; getStringForward/Reverse decode on demand;
//  * the mate lists of all reads are one CSR array; Read::getMatePairList()
//    returns a view with vector's read interface (size, at, [], begin, end);
//  * OverlapGraph(ht) returns the reference's graph: discovery on the device,
//    then the reference's exploration order and transitive reduction
//     and its contraction loop (OverlapGraph.cpp:211-215,
//    row 3) replayed on the host; flow and scaffolding are out of scope
//    (SURVEY §2 rows 8-13);
//  * HashTable/OverlapGraph run on a HIP device through include/mg_overlap.h
//    and throw if no device is available (there is no CPU fallback).
#ifndef MG_API_HPP_
#define MG_API_HPP_

#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "mg_overlap.h"

// The reference's integer names (Common.h:31-37); UINT32 is 64-bit on LP64 there.
typedef unsigned char UINT8;
typedef unsigned short UINT16;
typedef unsigned long UINT32;
typedef unsigned long long UINT64;
typedef long long INT64;

namespace mg {
class UnitigGraph;
struct Error : std::runtime_error {
  explicit Error(const std::string& s) : std::runtime_error(s) {}
};
struct PackedReads;
}  // namespace mg

class Dataset;
class Edge;

// The exploration state and the transitive-reduction marks (OverlapGraph.h:20-30).
enum nodeType { UNEXPLORED = 0, EXPLORED = 1, EXPLORED_AND_TRANSITIVE_EDGES_MARKED = 2 };
enum markType { VACANT = 0, INPLAY = 1, ELIMINATED = 2 };

// One entry of a read's mate list (Read.h:16-27).
struct MPlist {
  UINT64 matePairID;          // ID of the mate
  UINT8 matePairOrientation;  // 0 = 00 reverse/reverse, 1 = 01 reverse/forward, 2 = 10, 3 = 11 forward/forward
  UINT8 datasetNumber;        // index of the paired-end file
};

// Read::getMatePairList()'s result: the read's slice of the Dataset's CSR array,
// used as the reference uses its vector<MPlist>* (list->size(), list->at(j)).
class MatePairList {
 public:
  MatePairList(const MPlist* b, const MPlist* e) : b_(b), e_(e) {}
  size_t size() const { return (size_t)(e_ - b_); }
  bool empty() const { return b_ == e_; }
  const MPlist& at(size_t i) const {
    if (i >= size()) throw std::out_of_range("MatePairList::at");
    return b_[i];
  }
  const MPlist& operator[](size_t i) const { return b_[i]; }
  const MPlist* begin() const { return b_; }
  const MPlist* end() const { return e_; }
  const MatePairList* operator->() const { return this; }

 private:
  const MPlist* b_;
  const MPlist* e_;
};

class Read {
 public:
  UINT64 superReadID = 0;      // 0 = not contained, else ID of the super read (Read.h:50)
  bool isContainedRead = false;
  std::string getStringForward();
  std::string getStringReverse();
  UINT16 getReadLength();
  UINT64 getReadNumber() { return readNumber; }
  UINT32 getFrequency();
  // the mates Dataset::readMatePairsFromFile() stored for this read, in
  // addMatePair's order (Read.h:65, Read.cpp:132-166); empty before that call
  MatePairList getMatePairList();
  // composite edges holding this read's forward / reverse string and the read's
  // distance on each (Read.h:39-42, maintained by OverlapGraph.cpp:1048-1115)
  std::vector<Edge*>* getListOfEdgesForward() { return &locations().edgesForward; }
  std::vector<UINT64>* getLocationOnEdgeForward() { return &locations().locationForward; }
  std::vector<Edge*>* getListOfEdgesReverse() { return &locations().edgesReverse; }
  std::vector<UINT64>* getLocationOnEdgeReverse() { return &locations().locationReverse; }

 private:
  friend class Dataset;
  friend class OverlapGraph;
  struct Locations {
    std::vector<Edge*> edgesForward, edgesReverse;
    std::vector<UINT64> locationForward, locationReverse;
  };
  Locations& locations() {
    if (!loc) loc.reset(new Locations());
    return *loc;
  }
  const Dataset* owner = nullptr;
  UINT64 readNumber = 0;
  std::unique_ptr<Locations> loc;  // allocated on first use (most reads are on no composite edge)
};

class Edge {
 public:
  Edge(Read* from, Read* to, UINT64 orient, UINT64 length)
      : source(from), destination(to), overlapOrientation((UINT8)orient), overlapOffset(length) {}
  Read* getSourceRead() { return source; }
  Read* getDestinationRead() { return destination; }
  UINT8 getOrientation() { return overlapOrientation; }
  UINT64 getOverlapOffset() { return overlapOffset; }
  Edge* getReverseEdge() { return reverseEdge; }
  bool setReverseEdge(Edge* e) {
    reverseEdge = e;
    return true;
  }
  // ordered reads inside a composite edge (Edge.h:30-32; empty for a simple edge)
  std::vector<UINT64>* getListOfReads() { return &listOfReads; }
  std::vector<UINT16>* getListOfOverlapOffsets() { return &listOfOverlapOffsets; }
  std::vector<UINT8>* getListOfOrientations() { return &listOfOrientations; }
  bool transitiveRemovalFlag = false;
  UINT16 flow = 0;  // Edge.h:42 (0 until flow is computed)
  UINT64 coverageDepth = 0;  // Edge.h:43 (0 until getBaseByBaseCoverage / calculateCoverageOfAllEdges)
  UINT64 SD = 0;             // Edge.h:44: standard deviation of the per-base coverage

 private:
  friend class OverlapGraph;
  UINT64 serial = 0;  // creation order (insertEdge(Read*,...) makes the edge before its twin)
  Read* source;
  Read* destination;
  UINT8 overlapOrientation;  // 0 = u<---<v, 1 = u<--->v, 2 = u>---<v, 3 = u>--->v
  UINT64 overlapOffset;      // start of v relative to u
  Edge* reverseEdge = nullptr;
  std::vector<UINT64> listOfReads;
  std::vector<UINT16> listOfOverlapOffsets;
  std::vector<UINT8> listOfOrientations;
};

class Dataset {
 public:
  std::vector<std::string> pairedEndDatasetFileNames;
  std::vector<std::string> singleEndDatasetFileNames;
  UINT64 shortestReadLength = ~0ULL;
  UINT64 longestReadLength = 0;

  Dataset(std::vector<std::string> pairedEndFileNames, std::vector<std::string> singleEndFileNames,
          UINT64 minOverlap);
  ~Dataset();
  UINT64 getNumberOfReads() { return numberOfReads; }
  UINT64 getNumberOfUniqueReads() { return numberOfUniqueReads; }
  Read* getReadFromString(const std::string& read);
  Read* getReadFromID(UINT64 ID);
  void saveReads(std::string fileName);
  // storeMatePairInformation for every paired-end file (Dataset.cpp:97-104,
  // 208-310): fills every read's mate list.  Nothing to do without paired-end
  // files.  While an OverlapGraph build holds the device context the lists are
  // built there (mg_build_mate_pairs; MG_DEVICE_MATES=0: on the host), else by
  // the host mirror (mg::MatePairs::build).  Same lists either way.
  void readMatePairsFromFile();

  // --- packed view (device upload) and bulk construction (bench / Python) ---
  static Dataset* fromCodes(const uint8_t* codes, uint64_t n, uint64_t stride, const uint16_t* lens,
                            UINT64 minOverlap, int nthreads);
  const uint64_t* packedWords() const;
  const uint16_t* packedLengths() const;
  uint32_t wordsPerRead() const;
  uint32_t frequencyOf(UINT64 id) const;
  std::string decode(UINT64 id, bool reverse) const;
  UINT64 minimumOverlapLength() const { return minOverlapLength; }

 private:
  friend class Read;
  friend class OverlapGraph;
  Dataset() = default;
  void finalize(mg::PackedReads&& pr);
  mg::PackedReads* packed = nullptr;
  std::vector<Read> reads;
  mg_ctx* mateCtx = nullptr;        // the device context of a running OverlapGraph build (not owned)
  std::vector<uint64_t> mateStart;  // n + 2 entries once readMatePairsFromFile ran: the list of read A is
  std::vector<MPlist> mates;        //   mates[mateStart[A] .. mateStart[A + 1])
  UINT64 numberOfReads = 0, numberOfUniqueReads = 0, minOverlapLength = 0;
};

class HashTable {
 public:
  HashTable();
  explicit HashTable(Dataset* d) : HashTable() { dataSet = d; }
  ~HashTable();
  bool insertDataset(Dataset* d, UINT64 minOverlapLength);
  std::vector<UINT64>* getListOfReads(std::string subString);
  UINT64 hashFunction(std::string subString);  // the reference's index function (HashTable.cpp:135-155)
  UINT64 getHashTableSize() { return hashTableSize; }
  UINT64 getHashStringLength() { return hashStringLength; }
  Dataset* getDataset() { return dataSet; }

  // --- device controls (not in the reference) ---
  static void setDefaultDevice(int device);
  static void setDefaultSeedK(uint32_t k);
  mg_ctx* context() { return ctx; }

 private:
  Dataset* dataSet = nullptr;
  mg_ctx* ctx = nullptr;
  UINT64 hashTableSize = 0;
  UINT16 hashStringLength = 0;
  std::vector<std::vector<UINT64>*> lookups;  // lists handed out by getListOfReads
};

class OverlapGraph {
 public:
  OverlapGraph();
  explicit OverlapGraph(HashTable* ht);
  ~OverlapGraph();
  bool buildOverlapGraphFromHashTable(HashTable* ht);
  void markContainedReads();
  bool insertEdge(Edge* edge);
  bool insertEdge(Read* read1, Read* read2, UINT8 orient, UINT16 overlapOffset);

  // --- the reference's per-read build steps (OverlapGraph.h:54,64-68), for a
  // caller that drives its own exploration as buildOverlapGraphFromHashTable
  // does (OverlapGraph.cpp:144-204).  beginBuildFromHashTable(ht) does that
  // function's set-up (:111-142): counters, the N + 1 empty lists,
  // markContainedReads on the device, and the device discovery of every read's
  // D(A) (mg_find_overlaps), kept on the host in insertAllEdgesOfRead's loop
  // order; the caller keeps ownership of ht.  Then:
  //  * insertAllEdgesOfRead (:529-565) inserts D(readNumber) in that order,
  //    skipping partners that are not UNEXPLORED (:546), and sorts the list by
  //    overlap offset with the reference's comparator (:563);
  //  * markTransitiveEdges (:574-615) / removeTransitiveEdges (:623-661) on
  //    the Edge objects, statement for statement;
  //  * checkOverlap (:354-383) / checkOverlapForContainedRead (:302-340) are
  //    the reference's string predicates for any pair (the device answers the
  //    same questions in bulk);
  //  * the contraction steps, sortEdges and saveGraphToFile then apply to the
  //    caller-built graph as to buildOverlapGraphFromHashTable's.
  bool beginBuildFromHashTable(HashTable* ht);
  bool insertAllEdgesOfRead(UINT64 readNumber, std::vector<nodeType>* exploredReads);
  bool markTransitiveEdges(UINT64 readNumber, std::vector<markType>* markedNodes);
  bool removeTransitiveEdges(UINT64 readNumber);
  bool checkOverlap(Read* read1, Read* read2, UINT64 orient, UINT64 start);
  bool checkOverlapForContainedRead(Read* read1, Read* read2, UINT64 orient, UINT64 start);
  // the .unitig checkpoint back into the graph (:1270-1367; main.cpp:36-42's
  // -s resume: OverlapGraph() -> setDataset -> readGraphFromFile -> sortEdges)
  bool readGraphFromFile(const std::string& fileName);
  UINT64 getNumberOfEdges() { return numberOfEdges; }
  UINT64 getNumberOfNodes() { return numberOfNodes; }
  bool setDataset(Dataset* d) {  // OverlapGraph.h:79
    dataSet = d;
    dataSet->readMatePairsFromFile();
    return true;
  }
  // graph[u] of the reference (private there): edges of read u, sorted by offset (:563)
  const std::vector<Edge*>* getEdges(UINT64 readNumber) const;
  // current edges as "u v orient offset" lines, sorted (checkpoint/parity dump)
  bool saveRawEdges(const std::string& fileName) const;
  // every graph[u] list in list order after "#C numberOfNodes numberOfEdges"
  bool saveGraphLists(const std::string& fileName) const;
  // true (default): buildOverlapGraphFromHashTable replays the reference's
  // exploration order and transitive reduction (OverlapGraph.cpp:144-204,
  // 574-661) on the device's discoveries; false: keep the raw discovery multiset.
  static bool replayExploration;
  // true (default, as the reference): then run the contraction loop
  // (OverlapGraph.cpp:211-215); false: stop just before it
  static bool contractPaths;
  // D(A) of every read grouped on the device (mg_build_discoveries; default)
  // or, off, on the host from the downloaded rows (mg_copy_rows +
  // Discoveries::build).  Same lists either way.  Until this is called the
  // environment variable MG_DEVICE_DISC decides (0 = host grouping).
  static void setDeviceDiscoveries(bool on);
  // Connected components of the lists (mg_build_components on the device
  // lists, a host union-find with host grouping; default on): they are
  // replayed in parallel by min(16, hardware threads) host threads
  // (MG_REPLAY_THREADS) unless one component holds 90 % of the records.  Off:
  // always the serial replay.  The same graph either way.  Until this is
  // called the environment variable MG_DEVICE_COMP decides (0 = serial).
  static void setDeviceComponents(bool on);
  // The contraction loop that ends buildOverlapGraphFromHashTable: the safe
  // chains of the replayed graph are found on the device (mg_build_chains, list
  // ranking) and contracted first, then the loop runs unchanged; the same
  // graph, lists, locations and counters.  Off: the loop alone.
  // Until this is called the environment variable MG_DEVICE_CHAINS decides
  // (0 = off).  The caller-driven contractCompositePaths() is not affected.
  static void setDeviceChains(bool on);
  // the contraction loop's steps (:669-696, :931-988) on the current graph
  // (available once the graph was built with replayExploration)
  UINT64 contractCompositePaths();
  UINT64 removeDeadEndNodes();
  void sortEdges();                                // :2799-2808
  bool saveGraphToFile(const std::string& fileName);  // the .unitig checkpoint (:1219-1261)
  // getStringInEdge (:2009-2041): the sequence the edge spells, by the host
  // mirror (mg::contigs_build); where the reference's substr would throw this
  // throws std::out_of_range naming the piece
  std::string getStringInEdge(Edge* edge);
  // printGraph (:428-520): the .gdl file and the contigs as FASTA (main.cpp:55
  // passes <prefix>graph1.gdl, <prefix>contigs1.fasta); the cout statistics
  // (:495-514) are not reproduced.  The strings of all contigs are built on the
  // device in one call (mg_build_contigs): in the hash table's context while a
  // caller-driven build still holds one, else (new OverlapGraph(ht) has freed
  // the table, :210) in a context of its own that uploads the Dataset's packed
  // reads.  Without a HIP device, or with device contigs off, the host mirror
  // spells them.  The same two files either way.
  bool printGraph(std::string graphFileName, std::string contigFileName);
  // Until this is called the environment variable MG_DEVICE_CONTIGS decides (0 = host mirror).
  static void setDeviceContigs(bool on);
  // calculateMeanAndSdOfInsertSize (:1124-1211): mean and SD of the insert sizes
  // of every paired-end dataset over the current edges; true at once when there
  // is no paired-end file.  The placements of every read (updateReadLocations of
  // every edge) and the sums are built on the device (mg_build_placements,
  // mg_insert_sizes) in the hash table's context while a build holds one, else
  // in a context of its own; without a HIP device, or with device placements
  // off, by the host mirrors (mg::placements_build, mg::insert_sizes).  The same
  // values either way.  The reference's cout lines are not printed here
  // (mg_overlap -insert prints them).
  bool calculateMeanAndSdOfInsertSize();
  UINT64 getMean(UINT64 datasetNumber) { return meanOfInsertSizes.at(datasetNumber); }  // OverlapGraph.h:62
  UINT64 getSD(UINT64 datasetNumber) { return sdOfInsertSizes.at(datasetNumber); }      // OverlapGraph.h:63
  // not in the reference: the number of insert sizes behind getMean(d) ("Reads on same edge: ")
  UINT64 getNumberOfInsertSizes(UINT64 datasetNumber) { return numberOfInsertSizes.at(datasetNumber); }
  // getBaseByBaseCoverage (:2722-2792): sets edge->coverageDepth and edge->SD,
  // by the host mirror (mg::edge_coverage); where the reference's at() would
  // throw this throws std::out_of_range naming the entry
  void getBaseByBaseCoverage(Edge* edge);
  // not in the reference: getBaseByBaseCoverage of every edge of the graph in
  // one device call (mg_edge_coverage; contexts and fall-back as above)
  void calculateCoverageOfAllEdges();
  // Until this is called the environment variable MG_DEVICE_PLACES decides (0 = host mirrors).
  static void setDevicePlacements(bool on);
  // findSupportByMatepairsAndMerge (:1892-2002): every mate entry's bounded
  // search between its two reads' edges (findPathBetweenMatepairs), the list of
  // supported edge pairs, then the merge of every pair with support >= 3 in
  // the order of the reference's sort; returns the number of pairs merged, and
  // 0 at once when there is no paired-end file (:1897).  Needs
  // calculateMeanAndSdOfInsertSize first (main.cpp:59 before :71).  The search
  // runs in one device call (mg_mate_paths; contexts as above) and the host
  // mirror (mg::mate_paths) finishes the entries the device deferred; without
  // a HIP device, or with device paths off, the mirror searches them all.  The
  // same graph either way.  The reference's cout lines are not printed here (mg_overlap
  // -support prints the counts); the three counters are kept.
  UINT64 findSupportByMatepairsAndMerge();
  UINT64 getNoPathsFound() const { return pathCounters[0]; }
  UINT64 getPathsFound() const { return pathCounters[1]; }
  UINT64 getMatepairsOnSameEdge() const { return pathCounters[2]; }
  // not in the reference: the size of listOfPairedEdges ("... merged out of N")
  UINT64 getNumberOfPairedEdges() const { return pathCounters[3]; }
  // Until this is called the environment variable MG_DEVICE_PATHS decides (0 = host mirror).
  static void setDevicePaths(bool on);
  // scaffolder (:2120-2223, main.cpp:85): every mate entry whose two reads lie
  // uniquely on two different edges within mean + 3 SD supports that pair of
  // edges; the pairs are sorted by support and every pair with support >= 3
  // that no earlier merge freed is merged by mergeEdgesDisconnected.  Returns
  // the number of pairs merged and writes the reference's line per merged pair
  // to cout.  Needs calculateMeanAndSdOfInsertSize() first.  Twins and location
  // lists come from the list state, as for findSupportByMatepairsAndMerge();
  // the scoring runs in one device call (mg_scaffold_pairs), the merge loop on
  // the host, and the Edge objects are rebuilt.  Without a HIP device, or with
  // the device scaffolder off, the host mirror scores.  The same graph either way.
  UINT64 scaffolder();
  // Until this is called the environment variable MG_DEVICE_SCAFFOLD decides (0 = host mirror).
  static void setDeviceScaffold(bool on);
  const mg_timings& timings() const { return lastTimings; }

 private:
  Dataset* dataSet = nullptr;
  HashTable* hashTable = nullptr;
  std::vector<std::vector<Edge*>*>* graph = nullptr;
  UINT64 numberOfNodes = 0, numberOfEdges = 0;
  std::vector<UINT64> meanOfInsertSizes, sdOfInsertSizes, numberOfInsertSizes;  // OverlapGraph.h:38-39
  UINT64 pathCounters[4] = {0, 0, 0, 0};  // noPathsFound, pathsFound, mpOnSameEdge, paired edges
  bool containedDone = false;
  mg_timings lastTimings{};
  mg::UnitigGraph* unitig = nullptr;  // the list state the contraction steps work on
  struct Manual;                      // a caller-driven build: D(A) lists + the hash string length
  Manual* manual = nullptr;
  UINT64 nextSerial = 0;
  void clear();
  void materialize();  // graph / Edge objects / read locations from `unitig`
  void adoptEdgeLists();  // `unitig` from the Edge lists of a caller-driven build
};

#endif  // MG_API_HPP_
