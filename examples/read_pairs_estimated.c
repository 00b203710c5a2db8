/*
 * read_pairs_estimated.c -- read_pairs.c for a caller who does not know the library's insert distribution, against the two public
 * headers only.  The same path -- index, the pairs put on one strand, longest matches, located, candidate loci and chains with
 * SLOTS - 1 slots in a table of stride SLOTS, slot scores -- and then, instead of an interval from the command line, "insert
 * size": the HISTOGRAM of the template lengths of the pairs whose best slots agree (awfmInsertHistogram /
 * awfmGpuInsertHistogram) over a wide range, the INTERVAL from its quartiles (awfmInsertInterval / awfmGpuInsertInterval), and
 * both pairings with that interval: on the host awfmPairMates with the estimate's minInsert and maxInsert, on the device
 * awfmGpuPairMatesEstimated, which reads them where awfmGpuInsertInterval left them -- no wait in between.  Then window scores,
 * slot scores, pairing, affine alignment as in read_pairs.c, and the same line per pair:
 *     pair <tab> proper <tab> T <tab> MAPQ1 <tab> pos1 <tab> CIGAR1 <tab> MAPQ2 <tab> pos2 <tab> CIGAR2
 * The estimate goes to stderr.  The program runs the host twins and, when a GPU is present, the device calls as well; it refuses
 * to print when the two estimates or any other value differ.
 *
 *   cc -std=gnu11 -O2 examples/read_pairs_estimated.c -Iinclude -Lavxwindowfmindex_amd -lawfmindex_amd \
 *      -Wl,-rpath,$PWD/avxwindowfmindex_amd -o read_pairs_estimated &&
 *      ./read_pairs_estimated strands.fa pairs.txt lowTemplate highTemplate fallbackMin fallbackMax [step [minLength [cap
 *                   [maxHitsPerSeed [band [minVotes [lookback [gapPenalty [bandPad [maxDrift [maxOps [match [mismatch [gapOpen [gapExtend
 *                   [minScore [unpairedPenalty [windowPad [mapqCap [minQuality [spread [minSamples]]]]]]]]]]]]]]]]]]]]]]
 *
 * lowTemplate .. highTemplate: the histogram's range, at most 65536 bins: make it wide, what falls outside is counted and not
 * used.  fallbackMin, fallbackMax: the interval of a batch with fewer than minSamples samples.  pairs.txt: two lines per pair,
 * mate 1 and then mate 2.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "AwFmIndex.h"
#include "awfm_gpu.h"

enum { SLOTS = 4, THREADS = 4 };

struct Params {
  uint64_t step, cap;
  uint32_t minLength, maxHitsPerSeed, band, minVotes, lookback, gapPenalty, bandPad, maxDrift, maxOps, mapqCap;
  struct AwFmAlignScoring scoring;
  struct AwFmPairParams pairing; /* (minInsert and maxInsert come from the estimate) */
  struct AwFmInsertParams insert;
};

struct Batch { /* the reads as sequenced, interleaved: 2p is mate 1, 2p + 1 mate 2; and the windows of the longest-match search */
  uint64_t numReads, numChars, numWindows;
  uint8_t *sequenced;
  uint64_t *readOffsets, *readSeedOffsets, *starts, *ends;
  uint32_t *seedEnds;
};

struct Result { /* per pair, then per read */
  uint8_t *proper, *qualities;
  int64_t *lengths;
  uint32_t *sequences, *scores, *numOps, *ops;
  uint64_t *begins;
  uint64_t numProper, numWindows, numFound, numOutside;
  struct AwFmInsertEstimate estimate;
};

static int onDevice; /* which allocator the side at work uses */

static void *buffer(uint64_t bytes) {
  void *p = onDevice ? awfmGpuHostAlloc(bytes ? bytes : 1) : calloc(bytes ? bytes : 1, 1);
  if (!p) {
    fprintf(stderr, "out of memory: %s\n", onDevice ? awfmGpuLastError() : "host");
    exit(3);
  }
  return p;
}

static void release(void *p) {
  if (onDevice) awfmGpuHostFree(p);
  else free(p);
}

static void check(enum AwFmReturnCode rc, const char *what) {
  if (awFmReturnCodeIsFailure(rc)) {
    fprintf(stderr, "%s failed: %d: %s\n", what, rc, awfmGpuLastError());
    exit(3);
  }
}

/* everything from the reads as sequenced to the alignments of the paired slots; image == NULL: the host twins */
static void run(const struct AwFmIndex *index, AwFmGpuIndex *image, const uint8_t *genome, uint64_t genomeLength, const uint64_t *recordEnds,
                uint64_t numRecords, const struct Batch *in, const struct Params *p, struct Result *out) {
  onDevice = image != NULL;
  const uint64_t numReads = in->numReads, numPairs = numReads / 2, numWindows = in->numWindows, numSlots = numReads * SLOTS;
  struct Batch b = *in;
  if (onDevice) { /* the same arrays where the device reads them */
    b.sequenced = memcpy(buffer(in->numChars), in->sequenced, in->numChars);
    b.readOffsets = memcpy(buffer((numReads + 1) * 8), in->readOffsets, (numReads + 1) * 8);
    b.readSeedOffsets = memcpy(buffer((numReads + 1) * 8), in->readSeedOffsets, (numReads + 1) * 8);
    b.starts = memcpy(buffer(numWindows * 8), in->starts, numWindows * 8);
    b.ends = memcpy(buffer(numWindows * 8), in->ends, numWindows * 8);
    b.seedEnds = memcpy(buffer(numWindows * 4), in->seedEnds, numWindows * 4);
  }
  uint8_t *chars = buffer(in->numChars); /* the reads on one strand */
  uint32_t *lengths = buffer(numWindows * 4), *counts = buffer(numWindows * 4), *one = buffer(4);
  struct AwFmSearchRange *ranges = buffer(numWindows * sizeof *ranges);
  uint64_t *hitOffsets = buffer((numWindows + 1) * 8), *waitOffsets = buffer(16), *counters = buffer(64), totalHits = 0, waited = 0;
  void *scan = onDevice ? buffer(awfmGpuScanScratchBytes(numWindows ? numWindows : 1)) : NULL;
  *one = 1;
  hitOffsets[0] = 0;
  memset(counters, 0, 64);
  /* call 1: mate 2 of every pair onto mate 1's strand */
  if (numReads != 0) {
    if (onDevice) check(awfmGpuReverseComplementReads(image, b.sequenced, in->numChars, b.readOffsets, numReads, AWFM_COMPLEMENT_ODD, chars, &counters[0], NULL), "reverse complement");
    else check(awfmReverseComplementReads(b.sequenced, in->numChars, b.readOffsets, numReads, AWFM_COMPLEMENT_ODD, chars, &counters[0], THREADS), "reverse complement");
  }
  if (numWindows != 0) {
    if (onDevice) {
      check(awfmGpuLongestSuffixMatches(image, chars, b.starts, b.ends, 0, numWindows, p->minLength, lengths, ranges, counts, NULL), "search");
      /* (waits for the stream: the total comes back to the host) */
      check(awfmGpuHitOffsetsFromCounts(image, counts, numWindows, hitOffsets, scan, &totalHits, NULL), "scan");
    } else {
      check(awfmLongestSuffixMatches(index, chars, b.starts, b.ends, 0, numWindows, p->minLength, lengths, ranges, counts, THREADS), "search");
      for (uint64_t w = 0; w < numWindows; w++) hitOffsets[w + 1] = hitOffsets[w] + counts[w];
      totalHits = hitOffsets[numWindows];
    }
  }
  uint64_t *positions = buffer(totalHits * 8);
  uint32_t *sequenceNumbers = buffer(totalHits * 4);
  if (totalHits != 0) {
    if (onDevice) {
      check(awfmGpuLocate(image, ranges, hitOffsets, numWindows, totalHits, positions, NULL), "locate");
      check(awfmGpuLocalPositions(image, positions, totalHits, NULL, sequenceNumbers, positions /* in place */, NULL, NULL), "local positions");
    } else {
      enum AwFmReturnCode rc = AwFmSuccess;
      for (uint64_t w = 0; w < numWindows; w++)
        for (uint64_t k = 0; k < counts[w]; k++) positions[hitOffsets[w] + k] = awFmFindDatabaseHitPositionSingle(index, ranges[w].startPtr + k, &rc);
      check(awfmLocalPositions(index, positions, totalHits, sequenceNumbers, positions /* in place */, NULL, THREADS), "local positions");
    }
  }
  /* candidates and chains with SLOTS - 1 slots a read ... */
  const uint32_t narrow = SLOTS - 1;
  uint32_t *candSequences = buffer(numReads * narrow * 4), *candSpans = buffer(numReads * narrow * 4);
  int64_t *candDiagonals = buffer(numReads * narrow * 8);
  uint32_t *narrowAnchors = buffer(numReads * narrow * 4), *narrowBegins = buffer(numReads * narrow * 4), *narrowEnds = buffer(numReads * narrow * 4);
  int64_t *narrowBeginDiagonals = buffer(numReads * narrow * 8), *narrowEndDiagonals = buffer(numReads * narrow * 8);
  /* ... and the slot table of stride SLOTS: its last column is the window call's */
  uint32_t *sequences = buffer(numSlots * 4), *chainAnchors = buffer(numSlots * 4), *chainBegins = buffer(numSlots * 4), *chainEnds = buffer(numSlots * 4);
  int64_t *chainBeginDiagonals = buffer(numSlots * 8), *chainEndDiagonals = buffer(numSlots * 8);
  uint32_t *slotScores = buffer(numSlots * 4), *slotReadEnds = buffer(numSlots * 4);
  uint64_t *slotTextEnds = buffer(numSlots * 8);
  uint8_t *qualities = buffer(numReads), *proper = buffer(numPairs);
  uint32_t *pairSlots = buffer(numReads * 4), *windowSequences = buffer(numReads * 4);
  uint64_t *windowBegins = buffer(numReads * 8), *windowEnds = buffer(numReads * 8);
  int64_t *templateLengths = buffer(numPairs * 8);
  uint32_t *scores = buffer(numReads * 4), *numOps = buffer(numReads * 4), *ops = buffer(numReads * p->maxOps * 4);
  uint64_t *begins = buffer(numReads * 8);
  const uint64_t bins = (uint64_t)(p->insert.highTemplate - p->insert.lowTemplate) + 1;
  uint64_t *histogram = buffer(bins * 8);
  struct AwFmInsertEstimate *estimate = buffer(sizeof *estimate);
  memset(histogram, 0, bins * 8); /* the histogram is added to: the caller zeroes it */
  memset(estimate, 0, sizeof *estimate);
  if (numReads != 0) {
    const struct AwFmCandidateInputs cin = {.readSeedOffsets = b.readSeedOffsets, .numSeeds = numWindows, .seedEnds = b.seedEnds,
                                            .seedLengths = lengths, .fixedLength = 0, .hitOffsets = hitOffsets, .numHits = totalHits,
                                            .positions = positions, .sequenceNumbers = sequenceNumbers};
    const struct AwFmCandidateOutputs cout = {.sequences = candSequences, .diagonals = candDiagonals, .diagonalSpans = candSpans};
    const struct AwFmChainOutputs chains = {.chainAnchors = narrowAnchors, .chainReadBegins = narrowBegins, .chainReadEnds = narrowEnds,
                                            .chainBeginDiagonals = narrowBeginDiagonals, .chainEndDiagonals = narrowEndDiagonals};
    const struct AwFmVerifyInputs vin = {.readChars = chars, .numReadChars = in->numChars, .readOffsets = b.readOffsets, .sequences = sequences,
                                         .chainAnchors = chainAnchors, .chainReadBegins = chainBegins, .chainReadEnds = chainEnds,
                                         .chainBeginDiagonals = chainBeginDiagonals, .chainEndDiagonals = chainEndDiagonals};
    const struct AwFmSlotScoreOutputs scored = {.slotScores = slotScores, .slotReadEnds = slotReadEnds, .slotTextEnds = slotTextEnds,
                                                .mappingQualities = qualities};
    const struct AwFmPairInputs mates = {.readOffsets = b.readOffsets, .sequences = sequences, .slotScores = slotScores,
                                         .slotReadEnds = slotReadEnds, .slotTextEnds = slotTextEnds, .mappingQualities = qualities};
    /* (the qualities are raised in place; the counters of the first pairing are not kept) */
    const struct AwFmPairOutputs firstPairing = {.windowSequences = windowSequences, .windowBegins = windowBegins, .windowEnds = windowEnds};
    const struct AwFmPairOutputs paired = {.properPairs = proper, .pairSlots = pairSlots, .templateLengths = templateLengths,
                                           .mappingQualities = qualities, .numProper = &counters[1], .numWindows = &counters[2]};
    const struct AwFmWindowInputs win = {.readChars = chars, .numReadChars = in->numChars, .readOffsets = b.readOffsets,
                                         .windowSequences = windowSequences, .windowBegins = windowBegins, .windowEnds = windowEnds};
    const struct AwFmWindowOutputs placed = {.sequences = sequences, .chainAnchors = chainAnchors, .chainReadBegins = chainBegins,
                                             .chainReadEnds = chainEnds, .chainBeginDiagonals = chainBeginDiagonals,
                                             .chainEndDiagonals = chainEndDiagonals, .numFound = &counters[3]};
    const struct AwFmAffineOutputs aligned = {.scores = scores, .textBegins = begins, .numOps = numOps, .ops = ops};
    uint32_t maxLength = 1;
    for (uint64_t r = 0; r < numReads; r++)
      if (in->readOffsets[r + 1] - in->readOffsets[r] > maxLength) maxLength = (uint32_t)(in->readOffsets[r + 1] - in->readOffsets[r]);
    if (maxLength > AWFM_WINDOW_MAX_LENGTH) maxLength = AWFM_WINDOW_MAX_LENGTH; /* (longer reads are reported as too long) */
    void *candScratch = NULL, *chainScratch = NULL, *trace = NULL, *arena = NULL;
    if (onDevice) {
      candScratch = buffer(awfmGpuReadCandidatesScratchBytes(numReads));
      chainScratch = buffer(awfmGpuReadChainsScratchBytes(numReads));
      trace = buffer(awfmGpuAlignChainsAffineScratchBytes(image, maxLength));
      arena = buffer(awfmGpuScoreWindowsAffineScratchBytes(image, maxLength));
      check(awfmGpuReadCandidates(image, &cin, numReads, p->maxHitsPerSeed, p->band, p->minVotes, narrow, &cout, candScratch, NULL), "candidates");
      check(awfmGpuReadChains(image, &cin, numReads, p->maxHitsPerSeed, p->band, narrow, candSequences, candDiagonals, candSpans, p->lookback,
                              p->gapPenalty, &chains, chainScratch, NULL), "chains");
      /* with only the two headers, the scan that returns its total to the host is the call that waits for the stream */
      check(awfmGpuHitOffsetsFromCounts(image, one, 1, waitOffsets, scan, &waited, NULL), "wait");
    } else {
      check(awfmReadCandidates(&cin, numReads, p->maxHitsPerSeed, p->band, p->minVotes, narrow, &cout, THREADS), "candidates");
      check(awfmReadChains(&cin, numReads, p->maxHitsPerSeed, p->band, narrow, candSequences, candDiagonals, candSpans, p->lookback, p->gapPenalty,
                           &chains, THREADS), "chains");
    }
    /* the chains into the table of stride SLOTS (a caller with its own kernels writes them there at once) */
    for (uint64_t r = 0; r < numReads; r++)
      for (uint32_t j = 0; j < SLOTS; j++) {
        const uint64_t to = r * SLOTS + j, from = r * narrow + j;
        const int used = j < narrow;
        sequences[to] = used ? candSequences[from] : AWFM_CANDIDATES_NONE;
        chainAnchors[to] = used ? narrowAnchors[from] : 0;
        chainBegins[to] = used ? narrowBegins[from] : 0;
        chainEnds[to] = used ? narrowEnds[from] : 0;
        chainBeginDiagonals[to] = used ? narrowBeginDiagonals[from] : 0;
        chainEndDiagonals[to] = used ? narrowEndDiagonals[from] : 0;
      }
    if (onDevice) { /* one stream, no wait from here to the end: every call's arrays are written before the next one reads them */
      check(awfmGpuScoreChainsAffine(image, &vin, numReads, SLOTS, p->bandPad, p->maxDrift, &p->scoring, p->pairing.minScore, p->mapqCap, &scored, NULL), "slot scores");
      /* the interval goes from the one kernel to the other through device-visible memory: the host does not look at it here */
      check(awfmGpuInsertHistogram(image, &mates, numPairs, SLOTS, &p->insert, histogram, &counters[4], &counters[5], NULL), "insert histogram");
      check(awfmGpuInsertInterval(image, histogram, &p->insert, estimate, NULL), "insert interval");
      check(awfmGpuPairMatesEstimated(image, &mates, numPairs, SLOTS, &p->pairing, estimate, &firstPairing, NULL), "pairing");
      check(awfmGpuScoreWindowsAffine(image, &win, numReads, &p->scoring, p->pairing.minScore, SLOTS, SLOTS - 1, maxLength, &placed, arena, NULL), "window scores");
      check(awfmGpuScoreChainsAffine(image, &vin, numReads, SLOTS, p->bandPad, p->maxDrift, &p->scoring, p->pairing.minScore, p->mapqCap, &scored, NULL), "slot scores");
      check(awfmGpuPairMatesEstimated(image, &mates, numPairs, SLOTS, &p->pairing, estimate, &paired, NULL), "pairing");
      check(awfmGpuAlignChainsAffine(image, &vin, pairSlots, numReads, SLOTS, p->bandPad, p->maxDrift, &p->scoring, p->maxOps, maxLength, &aligned, trace, NULL), "alignment");
      check(awfmGpuHitOffsetsFromCounts(image, one, 1, waitOffsets, scan, &waited, NULL), "wait");
    } else {
      check(awfmScoreChainsAffine(&vin, numReads, SLOTS, p->bandPad, p->maxDrift, &p->scoring, p->pairing.minScore, p->mapqCap, genome, genomeLength, recordEnds,
                                  numRecords, AwFmAlphabetDna, &scored, THREADS), "slot scores");
      check(awfmInsertHistogram(&mates, numPairs, SLOTS, &p->insert, histogram, &counters[4], &counters[5], THREADS), "insert histogram");
      check(awfmInsertInterval(histogram, &p->insert, estimate), "insert interval");
      struct AwFmPairParams pairing = p->pairing; /* the host reads the struct and passes the interval on */
      pairing.minInsert = estimate->minInsert;
      pairing.maxInsert = estimate->maxInsert;
      check(awfmPairMates(&mates, numPairs, SLOTS, &pairing, &firstPairing, THREADS), "pairing");
      check(awfmScoreWindowsAffine(&win, numReads, &p->scoring, p->pairing.minScore, SLOTS, SLOTS - 1, genome, genomeLength, recordEnds, numRecords, AwFmAlphabetDna,
                                   &placed, THREADS), "window scores");
      check(awfmScoreChainsAffine(&vin, numReads, SLOTS, p->bandPad, p->maxDrift, &p->scoring, p->pairing.minScore, p->mapqCap, genome, genomeLength, recordEnds,
                                  numRecords, AwFmAlphabetDna, &scored, THREADS), "slot scores");
      check(awfmPairMates(&mates, numPairs, SLOTS, &pairing, &paired, THREADS), "pairing");
      check(awfmAlignChainsAffine(&vin, pairSlots, numReads, SLOTS, p->bandPad, p->maxDrift, &p->scoring, p->maxOps, genome, genomeLength, recordEnds, numRecords,
                                  AwFmAlphabetDna, &aligned, THREADS), "alignment");
    }
    void *scratches[] = {candScratch, chainScratch, trace, arena};
    for (size_t i = 0; i < sizeof scratches / sizeof *scratches; i++)
      if (scratches[i]) release(scratches[i]);
  }
  out->proper = malloc(numPairs + 1);
  out->lengths = malloc((numPairs + 1) * 8);
  out->qualities = malloc(numReads + 1);
  out->sequences = malloc((numReads + 1) * 4);
  out->scores = malloc((numReads + 1) * 4);
  out->numOps = malloc((numReads + 1) * 4);
  out->begins = malloc((numReads + 1) * 8);
  out->ops = malloc((numReads * p->maxOps + 1) * 4);
  memcpy(out->proper, proper, numPairs);
  memcpy(out->lengths, templateLengths, numPairs * 8);
  for (uint64_t r = 0; r < numReads; r++) {
    const int has = scores[r] != 0 && scores[r] < AWFM_VERIFY_TOO_LONG;
    out->qualities[r] = has ? qualities[r] : 0;
    out->sequences[r] = has ? sequences[r * SLOTS + pairSlots[r]] : 0;
    out->scores[r] = scores[r];
    out->numOps[r] = has ? numOps[r] : 0;
    out->begins[r] = has ? begins[r] : 0;
    /* (a truncated row has no specified content: it is printed as * and not compared) */
    memset(out->ops + r * p->maxOps, 0, (size_t)p->maxOps * 4);
    if (has && numOps[r] <= p->maxOps) memcpy(out->ops + r * p->maxOps, ops + r * p->maxOps, (size_t)numOps[r] * 4);
  }
  out->numProper = counters[1];
  out->numWindows = counters[2];
  out->numFound = counters[3];
  out->numOutside = counters[5];
  out->estimate = *estimate;
  void *all[] = {chars, lengths, counts, one, ranges, hitOffsets, waitOffsets, counters, scan, positions, sequenceNumbers, candSequences, candSpans,
                 candDiagonals, narrowAnchors, narrowBegins, narrowEnds, narrowBeginDiagonals, narrowEndDiagonals, sequences, chainAnchors, chainBegins,
                 chainEnds, chainBeginDiagonals, chainEndDiagonals, slotScores, slotReadEnds, slotTextEnds, qualities, proper, pairSlots,
                 windowSequences, windowBegins, windowEnds, templateLengths, scores, numOps, ops, begins, histogram, estimate};
  for (size_t i = 0; i < sizeof all / sizeof *all; i++)
    if (all[i]) release(all[i]);
  if (onDevice) {
    void *copies[] = {b.sequenced, b.readOffsets, b.readSeedOffsets, b.starts, b.ends, b.seedEnds};
    for (size_t i = 0; i < sizeof copies / sizeof *copies; i++) release(copies[i]);
  }
}

/* one mate: its quality, header:position and script; * for none or for a row that did not hold the runs */
static int printMate(const struct AwFmIndex *index, const struct Result *shown, uint64_t r, uint32_t maxOps) {
  static const char letters[16] = {'?', 'I', 'D', '?', 'S', '?', '?', '=', 'X', '?', '?', '?', '?', '?', '?', '?'};
  if (shown->scores[r] == 0 || shown->scores[r] >= AWFM_VERIFY_TOO_LONG) {
    printf("\t0\t*\t*");
    return 0;
  }
  char *header = NULL;
  size_t headerLength = 0;
  if (awFmGetHeaderStringFromSequenceNumber(index, shown->sequences[r], &header, &headerLength) != AwFmSuccess) exit(4);
  printf("\t%u\t%.*s:%" PRIu64 "\t", (unsigned)shown->qualities[r], (int)headerLength, header, shown->begins[r]);
  const uint32_t numOps = shown->numOps[r];
  if (numOps > maxOps || numOps == 0) printf("*");
  for (uint32_t k = 0; k < numOps && numOps <= maxOps; k++) printf("%" PRIu32 "%c", shown->ops[r * maxOps + k] >> 4, letters[shown->ops[r * maxOps + k] & 15u]);
  return 1;
}

static uint32_t argument(int argc, char **argv, int at, uint32_t otherwise) { return argc > at ? (uint32_t)strtoul(argv[at], NULL, 10) : otherwise; }

int main(int argc, char **argv) {
  if (argc < 7) {
    fprintf(stderr, "usage: %s strands.fa pairs.txt lowTemplate highTemplate fallbackMin fallbackMax [step [minLength [cap [maxHitsPerSeed [band [minVotes [lookback [gapPenalty [bandPad [maxDrift [maxOps [match [mismatch [gapOpen [gapExtend [minScore [unpairedPenalty [windowPad [mapqCap [minQuality [spread [minSamples]]]]]]]]]]]]]]]]]]]]]]\n", argv[0]);
    return 1;
  }
  struct Params p = {.step = argument(argc, argv, 7, 4), .minLength = argument(argc, argv, 8, 16), .cap = argument(argc, argv, 9, 64),
                     .maxHitsPerSeed = argument(argc, argv, 10, 16), .band = argument(argc, argv, 11, 2), .minVotes = argument(argc, argv, 12, 2),
                     .lookback = argument(argc, argv, 13, AWFM_CHAINS_MAX_LOOKBACK), .gapPenalty = argument(argc, argv, 14, 1),
                     .bandPad = argument(argc, argv, 15, 8), .maxDrift = argument(argc, argv, 16, 15), .maxOps = argument(argc, argv, 17, 32),
                     .scoring = {.match = argument(argc, argv, 18, 1), .mismatch = argument(argc, argv, 19, 4), .gapOpen = argument(argc, argv, 20, 6),
                                 .gapExtend = argument(argc, argv, 21, 1)},
                     .pairing = {.minScore = argument(argc, argv, 22, 30),
                                 .unpairedPenalty = argument(argc, argv, 23, 17), .windowPad = argument(argc, argv, 24, 50),
                                 .mapqCap = argument(argc, argv, 25, 60)},
                     .insert = {.lowTemplate = strtoll(argv[3], NULL, 10), .highTemplate = strtoll(argv[4], NULL, 10),
                                .fallbackMin = strtoll(argv[5], NULL, 10), .fallbackMax = strtoll(argv[6], NULL, 10),
                                .minQuality = argument(argc, argv, 26, 1), .spread = argument(argc, argv, 27, 2),
                                .minSamples = argument(argc, argv, 28, 16)}};
  p.mapqCap = p.pairing.mapqCap;
  p.insert.minScore = p.pairing.minScore;
  if (p.insert.lowTemplate > p.insert.highTemplate || p.insert.highTemplate - p.insert.lowTemplate >= (int64_t)AWFM_INSERT_MAX_BINS) {
    fprintf(stderr, "the histogram's range is lowTemplate <= highTemplate, at most %u bins\n", AWFM_INSERT_MAX_BINS);
    return 1;
  }
  if (p.step == 0 || p.cap == 0 || p.maxOps == 0 || p.maxOps > AWFM_ALIGN_MAX_OPS) return 1;

  struct AwFmIndexConfiguration config = {.suffixArrayCompressionRatio = 8,
                                          .kmerLengthInSeedTable = 8,
                                          .alphabetType = AwFmAlphabetDna,
                                          .keepSuffixArrayInMemory = true,
                                          .storeOriginalSequence = false};
  struct AwFmIndex *index = NULL;
  enum AwFmReturnCode rc = awFmCreateIndexFromFasta(&index, &config, argv[1], "read_pairs_estimated.awfmi");
  if (awFmReturnCodeIsFailure(rc)) {
    fprintf(stderr, "awFmCreateIndexFromFasta failed: %d\n", rc);
    return 2;
  }

  /* the indexed text: the records' residues, each record followed by a NUL terminator; and where each record ends */
  FILE *fasta = fopen(argv[1], "r");
  if (!fasta) return 1;
  size_t genomeCap = 1 << 16, genomeLength = 0, numRecords = 0, endsCap = 1024, lineCap = 0;
  uint8_t *genome = malloc(genomeCap);
  uint64_t *recordEnds = malloc(endsCap * 8);
  char *line = NULL; /* (getline: a line of any length is one line) */
  while (getline(&line, &lineCap, fasta) >= 0) {
    const size_t length = line[0] == '>' ? 0 : strcspn(line, "\r\n");
    while (genomeLength + length + 1 > genomeCap) genome = realloc(genome, genomeCap *= 2);
    if (line[0] == '>') {
      if (numRecords == endsCap) recordEnds = realloc(recordEnds, (endsCap *= 2) * 8);
      if (numRecords++) {
        recordEnds[numRecords - 2] = genomeLength;
        genome[genomeLength++] = 0; /* the terminator of the record before */
      }
    } else {
      memcpy(genome + genomeLength, line, length);
      genomeLength += length;
    }
  }
  fclose(fasta);
  if (numRecords) {
    recordEnds[numRecords - 1] = genomeLength;
    genome[genomeLength++] = 0;
  }

  /* the reads as sequenced, interleaved, and where each begins */
  FILE *file = fopen(argv[2], "r");
  if (!file) {
    fprintf(stderr, "cannot read %s\n", argv[2]);
    return 1;
  }
  struct Batch in = {0};
  size_t readCap = 1024, charCap = 1 << 16;
  in.sequenced = malloc(charCap);
  in.readOffsets = malloc((readCap + 1) * 8);
  in.readOffsets[0] = 0;
  while (getline(&line, &lineCap, file) >= 0) {
    const size_t length = strcspn(line, "\r\n");
    if (in.numReads == readCap) in.readOffsets = realloc(in.readOffsets, ((readCap *= 2) + 1) * 8);
    while (in.numChars + length > charCap) in.sequenced = realloc(in.sequenced, charCap *= 2);
    memcpy(in.sequenced + in.numChars, line, length);
    in.numChars += length;
    in.readOffsets[++in.numReads] = in.numChars;
    in.numWindows += length / p.step;
  }
  free(line);
  fclose(file);
  if (in.numReads & 1) {
    fprintf(stderr, "%s: a mate 1 without its mate 2\n", argv[2]);
    return 1;
  }
  /* window w: the characters before end position e = step, 2 step, ... of its read, `cap` at the most */
  in.starts = malloc((in.numWindows + 1) * 8);
  in.ends = malloc((in.numWindows + 1) * 8);
  in.seedEnds = malloc((in.numWindows + 1) * 4);
  in.readSeedOffsets = malloc((in.numReads + 1) * 8); /* the windows of a read are contiguous: its seeds */
  size_t w = 0;
  for (size_t r = 0; r < in.numReads; r++) {
    in.readSeedOffsets[r] = w;
    for (uint64_t e = p.step; e <= in.readOffsets[r + 1] - in.readOffsets[r]; e += p.step, w++) {
      in.starts[w] = in.readOffsets[r] + (e > p.cap ? e - p.cap : 0);
      in.ends[w] = in.readOffsets[r] + e;
      in.seedEnds[w] = (uint32_t)e;
    }
  }
  in.readSeedOffsets[in.numReads] = w;

  struct Result host = {0}, device = {0}, *shown = &host;
  run(index, NULL, genome, genomeLength, recordEnds, numRecords, &in, &p, &host);
  const int haveDevice = awfmGpuDeviceCount() > 0;
  const uint64_t numPairs = in.numReads / 2;
  if (haveDevice) {
    AwFmGpuIndex *image = awfmGpuIndexAcquire(index); /* carries the record table of the FASTA file */
    if (!image) {
      fprintf(stderr, "no device image: %s\n", awfmGpuLastError());
      return 3;
    }
    check(awfmGpuIndexSetText(image, genome, genomeLength), "awfmGpuIndexSetText");
    run(index, image, genome, genomeLength, recordEnds, numRecords, &in, &p, &device);
    shown = &device;
    uint64_t different = host.numProper != device.numProper || host.numWindows != device.numWindows || host.numFound != device.numFound;
    different += host.numOutside != device.numOutside || memcmp(&host.estimate, &device.estimate, sizeof host.estimate) != 0;
    for (size_t q = 0; q < numPairs; q++) different += host.proper[q] != device.proper[q] || host.lengths[q] != device.lengths[q];
    for (size_t r = 0; r < in.numReads; r++)
      different += host.scores[r] != device.scores[r] || host.qualities[r] != device.qualities[r] || host.begins[r] != device.begins[r] ||
                   host.numOps[r] != device.numOps[r] || host.sequences[r] != device.sequences[r] ||
                   memcmp(host.ops + r * p.maxOps, device.ops + r * p.maxOps, (size_t)p.maxOps * 4) != 0;
    fprintf(stderr, "device and host twins: %" PRIu64 " values differ\n", different);
    if (different) return 4;
  }

  const struct AwFmInsertEstimate *e = &shown->estimate;
  fprintf(stderr, "insert estimate: valid %" PRIu64 " interval %" PRId64 " %" PRId64 " quartiles %" PRId64 " %" PRId64 " %" PRId64 " mean %" PRId64 " samples %" PRIu64 " outside %" PRIu64 "\n",
          e->valid, e->minInsert, e->maxInsert, e->quartiles[0], e->quartiles[1], e->quartiles[2], e->mean, e->numSamples, shown->numOutside);
  uint64_t numAligned = 0;
  for (size_t q = 0; q < numPairs; q++) {
    printf("%zu\t%u\t%" PRId64, q, (unsigned)shown->proper[q], shown->lengths[q]);
    numAligned += (uint64_t)printMate(index, shown, 2 * q, p.maxOps);
    numAligned += (uint64_t)printMate(index, shown, 2 * q + 1, p.maxOps);
    printf("\n");
  }
  fprintf(stderr, "pairs %" PRIu64 " windows %" PRIu64 " proper %" PRIu64 " rescue windows left %" PRIu64 " found in windows %" PRIu64 " aligned %" PRIu64 " on the %s\n",
          numPairs, in.numWindows, shown->numProper, shown->numWindows, shown->numFound, numAligned, haveDevice ? "device" : "host");

  awFmDeallocIndex(index);
  remove("read_pairs_estimated.awfmi");
  return 0;
}
