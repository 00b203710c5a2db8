/*
 * read_rescued.c -- a mate that the seeds cannot place, placed in the window its mate names, against the two public headers only:
 * read_clipped.c for mate 1 of every pair, and for mate 2 the stage without seeds.  A FASTA file -> index
 * (awFmCreateIndexFromFasta) -> MATE 1 through the whole path of read_clipped.c: longest matches, located, mapped to sequence
 * coordinates, candidate loci, chains, verification, local affine alignment -> MATE 2 aligned over its full width against the
 * window [mate 1's textBegin, + width) of mate 1's sequence (awfmScoreWindowsAffine / awfmGpuScoreWindowsAffine: no seeds, no
 * chain; a pair whose mate 1 has no alignment is not looked at) -> the slot that call wrote aligned by awfmAlignChainsAffine /
 * awfmGpuAlignChainsAffine as it is -> one line per pair, the digest
 *     pair <tab> header <tab> pos1 <tab> score1 <tab> CIGAR1 <tab> pos2 <tab> windowScore <tab> score2 <tab> CIGAR2
 * with pos the sequence-local position of the first aligned character and the CIGARs in text form (S = X I D); `*` and zeros
 * stand for a mate without an alignment.  Both mates are given on the strand of the records: strands, insert sizes and any
 * pairing rule are the caller's business.
 *
 * The program runs the whole path through the host twins and, when a GPU is present, through the device calls as well (the text
 * on the device: awfmGpuIndexSetText); it then prints the device's lines and says on stderr whether the two agree.
 *
 *   cc -std=gnu11 -O2 examples/read_rescued.c -Iinclude -Lavxwindowfmindex_amd -lawfmindex_amd \
 *      -Wl,-rpath,$PWD/avxwindowfmindex_amd -o read_rescued &&
 *      ./read_rescued genome.fa pairs.txt width [step [minLength [cap [maxHitsPerSeed [band [minVotes [lookback [gapPenalty [bandPad [maxDrift
 *                     [maxOps [match [mismatch [gapOpen [gapExtend [minScore]]]]]]]]]]]]]]]]
 *
 * pairs.txt: two lines per pair, mate 1 and then mate 2.  On the device the buffers are page-locked host memory
 * (awfmGpuHostAlloc), which the device reads and writes in place: a program that keeps its reads on the device passes its own
 * device pointers instead.
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
  uint32_t minLength, maxHitsPerSeed, band, minVotes, lookback, gapPenalty, bandPad, maxDrift, maxOps, minScore;
  uint64_t width; /* of mate 2's window, from mate 1's textBegin on */
  struct AwFmAlignScoring scoring;
};

struct Batch { /* mate 1 of every pair with its windows, and mate 2; on the device side the same arrays in page-locked memory */
  uint64_t numReads, numChars, numWindows, numMateChars;
  uint8_t *chars, *mateChars;
  uint64_t *readOffsets, *readSeedOffsets, *starts, *ends, *mateOffsets;
  uint32_t *seedEnds;
};

struct Result { /* per pair: mate 1, then mate 2 */
  uint32_t *sequences, *scores, *distances, *numOps, *ops;
  uint64_t *begins, *ends;
  uint32_t *windowScores, *mateScores, *mateNumOps, *mateOps;
  uint64_t *mateBegins;
  uint64_t numUnaligned, numTruncated, numFound;
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

/* mate 2's window: from mate 1's first aligned position on, in mate 1's sequence; a pair whose mate 1 has no alignment is not
 * looked at, and its slot -- which the window call then leaves alone -- is the unused one */
static void mateWindows(uint64_t numReads, uint64_t width, const uint32_t *scores, const uint32_t *candSequences, const uint32_t *best,
                        const uint64_t *begins, uint32_t *windowSequences, uint64_t *windowBegins, uint64_t *windowEnds, uint32_t *slotSequences) {
  for (uint64_t r = 0; r < numReads; r++) {
    const int has = scores[r] != 0 && scores[r] < AWFM_VERIFY_TOO_LONG;
    windowSequences[r] = has ? candSequences[r * SLOTS + best[r]] : AWFM_CANDIDATES_NONE;
    windowBegins[r] = has ? begins[r] : 0;
    windowEnds[r] = has ? begins[r] + width : 0;
    slotSequences[r] = AWFM_CANDIDATES_NONE;
  }
}

/* everything from the seeds of mate 1 to the alignment of mate 2; image == NULL: the host twins */
static void run(const struct AwFmIndex *index, AwFmGpuIndex *image, const uint8_t *genome, uint64_t genomeLength, const uint64_t *recordEnds,
                uint64_t numRecords, const struct Batch *in, const struct Params *p, struct Result *out) {
  onDevice = image != NULL;
  const uint64_t numReads = in->numReads, numWindows = in->numWindows;
  struct Batch b = *in;
  if (onDevice) { /* the same arrays where the device reads them */
    b.chars = memcpy(buffer(in->numChars), in->chars, in->numChars);
    b.readOffsets = memcpy(buffer((numReads + 1) * 8), in->readOffsets, (numReads + 1) * 8);
    b.readSeedOffsets = memcpy(buffer((numReads + 1) * 8), in->readSeedOffsets, (numReads + 1) * 8);
    b.starts = memcpy(buffer(numWindows * 8), in->starts, numWindows * 8);
    b.ends = memcpy(buffer(numWindows * 8), in->ends, numWindows * 8);
    b.seedEnds = memcpy(buffer(numWindows * 4), in->seedEnds, numWindows * 4);
    b.mateChars = memcpy(buffer(in->numMateChars), in->mateChars, in->numMateChars);
    b.mateOffsets = memcpy(buffer((numReads + 1) * 8), in->mateOffsets, (numReads + 1) * 8);
  }
  uint32_t *lengths = buffer(numWindows * 4), *counts = buffer(numWindows * 4);
  struct AwFmSearchRange *ranges = buffer(numWindows * sizeof *ranges);
  uint64_t *hitOffsets = buffer((numWindows + 1) * 8), totalHits = 0;
  void *scan = onDevice ? buffer(awfmGpuScanScratchBytes(numWindows ? numWindows : 1)) : NULL;
  hitOffsets[0] = 0;
  if (numWindows != 0) {
    if (onDevice) {
      check(awfmGpuLongestSuffixMatches(image, b.chars, b.starts, b.ends, 0, numWindows, p->minLength, lengths, ranges, counts, NULL), "search");
      /* (waits for the stream: the total comes back to the host) */
      check(awfmGpuHitOffsetsFromCounts(image, counts, numWindows, hitOffsets, scan, &totalHits, NULL), "scan");
    } else {
      check(awfmLongestSuffixMatches(index, b.chars, b.starts, b.ends, 0, numWindows, p->minLength, lengths, ranges, counts, THREADS), "search");
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
  const uint64_t numSlots = numReads * SLOTS;
  uint32_t *candSequences = buffer(numSlots * 4), *candSpans = buffer(numSlots * 4);
  int64_t *candDiagonals = buffer(numSlots * 8);
  uint32_t *chainAnchors = buffer(numSlots * 4), *chainBegins = buffer(numSlots * 4), *chainEnds = buffer(numSlots * 4);
  int64_t *chainBeginDiagonals = buffer(numSlots * 8), *chainEndDiagonals = buffer(numSlots * 8);
  uint32_t *bestVerified = buffer(numReads * 4), *distances = buffer(numReads * 4), *numOps = buffer(numReads * 4), *scores = buffer(numReads * 4);
  uint32_t *ops = buffer(numReads * p->maxOps * 4);
  uint64_t *begins = buffer(numReads * 8), *ends = buffer(numReads * 8), *counters = buffer(40), *waitOffsets = buffer(16), waited = 0;
  /* mate 2: its window, what the window call says, the slot it writes (one column), and the alignment of that slot */
  uint32_t *windowSequences = buffer(numReads * 4), *windowScores = buffer(numReads * 4), *zeros = buffer(numReads * 4);
  uint64_t *windowBegins = buffer(numReads * 8), *windowEnds = buffer(numReads * 8), *mateBegins = buffer(numReads * 8);
  uint32_t *slotSequences = buffer(numReads * 4), *slotAnchors = buffer(numReads * 4), *slotBegins = buffer(numReads * 4), *slotEnds = buffer(numReads * 4);
  int64_t *slotBeginDiagonals = buffer(numReads * 8), *slotEndDiagonals = buffer(numReads * 8);
  uint32_t *mateScores = buffer(numReads * 4), *mateNumOps = buffer(numReads * 4), *mateOps = buffer(numReads * p->maxOps * 4);
  memset(zeros, 0, numReads * 4); /* slot 0 of every mate 2 */
  uint32_t *one = buffer(4);
  *one = 1;
  counters[0] = counters[1] = counters[2] = counters[3] = counters[4] = 0;
  if (numReads != 0) {
    const struct AwFmCandidateInputs cin = {.readSeedOffsets = b.readSeedOffsets, .numSeeds = numWindows, .seedEnds = b.seedEnds,
                                            .seedLengths = lengths, .fixedLength = 0, .hitOffsets = hitOffsets, .numHits = totalHits,
                                            .positions = positions, .sequenceNumbers = sequenceNumbers};
    const struct AwFmCandidateOutputs cout = {.sequences = candSequences, .diagonals = candDiagonals, .diagonalSpans = candSpans};
    const struct AwFmChainOutputs chains = {.chainAnchors = chainAnchors, .chainReadBegins = chainBegins, .chainReadEnds = chainEnds,
                                            .chainBeginDiagonals = chainBeginDiagonals, .chainEndDiagonals = chainEndDiagonals};
    const struct AwFmVerifyInputs vin = {.readChars = b.chars, .numReadChars = in->numChars, .readOffsets = b.readOffsets,
                                         .sequences = candSequences, .chainAnchors = chainAnchors, .chainReadBegins = chainBegins,
                                         .chainReadEnds = chainEnds, .chainBeginDiagonals = chainBeginDiagonals,
                                         .chainEndDiagonals = chainEndDiagonals};
    const struct AwFmVerifyOutputs verified = {.bestSlots = bestVerified};
    const struct AwFmAffineOutputs aligned = {.scores = scores, .editDistances = distances, .textBegins = begins, .textEnds = ends,
                                              .numOps = numOps, .ops = ops, .numUnaligned = &counters[0], .numTruncated = &counters[1]};
    const struct AwFmWindowInputs win = {.readChars = b.mateChars, .numReadChars = in->numMateChars, .readOffsets = b.mateOffsets,
                                         .windowSequences = windowSequences, .windowBegins = windowBegins, .windowEnds = windowEnds};
    const struct AwFmWindowOutputs placed = {.scores = windowScores, .sequences = slotSequences, .chainAnchors = slotAnchors,
                                             .chainReadBegins = slotBegins, .chainReadEnds = slotEnds, .chainBeginDiagonals = slotBeginDiagonals,
                                             .chainEndDiagonals = slotEndDiagonals, .numUnscored = &counters[2], .numFound = &counters[3]};
    const struct AwFmVerifyInputs mateIn = {.readChars = b.mateChars, .numReadChars = in->numMateChars, .readOffsets = b.mateOffsets,
                                            .sequences = slotSequences, .chainAnchors = slotAnchors, .chainReadBegins = slotBegins,
                                            .chainReadEnds = slotEnds, .chainBeginDiagonals = slotBeginDiagonals,
                                            .chainEndDiagonals = slotEndDiagonals};
    const struct AwFmAffineOutputs mateAligned = {.scores = mateScores, .textBegins = mateBegins, .numOps = mateNumOps, .ops = mateOps,
                                                  .numUnaligned = &counters[4]};
    if (onDevice) { /* one stream: every call's arrays are written before the next one reads them; nothing comes home in between */
      uint32_t maxRows = 1;
      for (uint64_t r = 0; r < numReads; r++)
        if (in->readOffsets[r + 1] - in->readOffsets[r] > maxRows) maxRows = (uint32_t)(in->readOffsets[r + 1] - in->readOffsets[r]);
      if (maxRows > AWFM_ALIGN_MAX_LENGTH) maxRows = AWFM_ALIGN_MAX_LENGTH; /* (longer reads are reported as too long) */
      void *candScratch = buffer(awfmGpuReadCandidatesScratchBytes(numReads)), *chainScratch = buffer(awfmGpuReadChainsScratchBytes(numReads));
      void *trace = buffer(awfmGpuAlignChainsAffineScratchBytes(image, maxRows));
      check(awfmGpuReadCandidates(image, &cin, numReads, p->maxHitsPerSeed, p->band, p->minVotes, SLOTS, &cout, candScratch, NULL), "candidates");
      check(awfmGpuReadChains(image, &cin, numReads, p->maxHitsPerSeed, p->band, SLOTS, candSequences, candDiagonals, candSpans, p->lookback,
                              p->gapPenalty, &chains, chainScratch, NULL), "chains");
      check(awfmGpuVerifyChains(image, &vin, numReads, SLOTS, p->bandPad, p->maxDrift, &verified, NULL), "verification");
      check(awfmGpuAlignChainsAffine(image, &vin, bestVerified, numReads, SLOTS, p->bandPad, p->maxDrift, &p->scoring, p->maxOps, maxRows, &aligned,
                                     trace, NULL), "alignment");
      /* all of it is asynchronous; with only the two headers, the scan that returns its total to the host is the call that
       * waits for the stream */
      check(awfmGpuHitOffsetsFromCounts(image, one, 1, waitOffsets, scan, &waited, NULL), "wait");
      mateWindows(numReads, p->width, scores, candSequences, bestVerified, begins, windowSequences, windowBegins, windowEnds, slotSequences);
      uint32_t maxLength = 1;
      for (uint64_t r = 0; r < numReads; r++)
        if (in->mateOffsets[r + 1] - in->mateOffsets[r] > maxLength) maxLength = (uint32_t)(in->mateOffsets[r + 1] - in->mateOffsets[r]);
      if (maxLength > AWFM_WINDOW_MAX_LENGTH) maxLength = AWFM_WINDOW_MAX_LENGTH; /* (longer mates are reported as too long) */
      void *arena = buffer(awfmGpuScoreWindowsAffineScratchBytes(image, maxLength)), *mateTrace = buffer(awfmGpuAlignChainsAffineScratchBytes(image, maxLength));
      check(awfmGpuScoreWindowsAffine(image, &win, numReads, &p->scoring, p->minScore, 1, 0, maxLength, &placed, arena, NULL), "window scores");
      check(awfmGpuAlignChainsAffine(image, &mateIn, zeros, numReads, 1, p->bandPad, p->maxDrift, &p->scoring, p->maxOps, maxLength, &mateAligned,
                                     mateTrace, NULL), "alignment of mate 2");
      check(awfmGpuHitOffsetsFromCounts(image, one, 1, waitOffsets, scan, &waited, NULL), "wait");
      release(arena);
      release(mateTrace);
      release(candScratch);
      release(chainScratch);
      release(trace);
    } else {
      check(awfmReadCandidates(&cin, numReads, p->maxHitsPerSeed, p->band, p->minVotes, SLOTS, &cout, THREADS), "candidates");
      check(awfmReadChains(&cin, numReads, p->maxHitsPerSeed, p->band, SLOTS, candSequences, candDiagonals, candSpans, p->lookback, p->gapPenalty,
                           &chains, THREADS), "chains");
      check(awfmVerifyChains(&vin, numReads, SLOTS, p->bandPad, p->maxDrift, genome, genomeLength, recordEnds, numRecords, AwFmAlphabetDna,
                             &verified, THREADS), "verification");
      check(awfmAlignChainsAffine(&vin, bestVerified, numReads, SLOTS, p->bandPad, p->maxDrift, &p->scoring, p->maxOps, genome, genomeLength,
                                  recordEnds, numRecords, AwFmAlphabetDna, &aligned, THREADS), "alignment");
      mateWindows(numReads, p->width, scores, candSequences, bestVerified, begins, windowSequences, windowBegins, windowEnds, slotSequences);
      check(awfmScoreWindowsAffine(&win, numReads, &p->scoring, p->minScore, 1, 0, genome, genomeLength, recordEnds, numRecords, AwFmAlphabetDna,
                                   &placed, THREADS), "window scores");
      check(awfmAlignChainsAffine(&mateIn, zeros, numReads, 1, p->bandPad, p->maxDrift, &p->scoring, p->maxOps, genome, genomeLength, recordEnds,
                                  numRecords, AwFmAlphabetDna, &mateAligned, THREADS), "alignment of mate 2");
    }
  }
  out->sequences = malloc((numReads + 1) * 4);
  out->distances = malloc((numReads + 1) * 4);
  out->scores = malloc((numReads + 1) * 4);
  out->numOps = malloc((numReads + 1) * 4);
  out->ops = malloc((numReads * p->maxOps + 1) * 4);
  out->begins = malloc((numReads + 1) * 8);
  out->ends = malloc((numReads + 1) * 8);
  out->windowScores = malloc((numReads + 1) * 4);
  out->mateScores = malloc((numReads + 1) * 4);
  out->mateNumOps = malloc((numReads + 1) * 4);
  out->mateOps = malloc((numReads * p->maxOps + 1) * 4);
  out->mateBegins = malloc((numReads + 1) * 8);
  for (uint64_t r = 0; r < numReads; r++) {
    const int has = scores[r] != 0 && scores[r] < AWFM_VERIFY_TOO_LONG;
    out->sequences[r] = has ? candSequences[r * SLOTS + bestVerified[r]] : 0;
    out->distances[r] = distances[r];
    out->scores[r] = scores[r];
    out->numOps[r] = numOps[r];
    out->begins[r] = begins[r];
    out->ends[r] = ends[r];
    /* (a truncated row has no specified content: it is printed as * and not compared) */
    memset(out->ops + r * p->maxOps, 0, (size_t)p->maxOps * 4);
    if (has && numOps[r] <= p->maxOps) memcpy(out->ops + r * p->maxOps, ops + r * p->maxOps, (size_t)numOps[r] * 4);
    const int mateHas = mateScores[r] != 0 && mateScores[r] < AWFM_VERIFY_TOO_LONG;
    out->windowScores[r] = windowScores[r];
    out->mateScores[r] = mateScores[r];
    out->mateNumOps[r] = mateNumOps[r];
    out->mateBegins[r] = mateBegins[r];
    memset(out->mateOps + r * p->maxOps, 0, (size_t)p->maxOps * 4);
    if (mateHas && mateNumOps[r] <= p->maxOps) memcpy(out->mateOps + r * p->maxOps, mateOps + r * p->maxOps, (size_t)mateNumOps[r] * 4);
  }
  out->numFound = counters[3];
  out->numUnaligned = counters[0];
  out->numTruncated = counters[1];
  void *all[] = {lengths,     counts,       ranges,      hitOffsets,          scan,              positions, sequenceNumbers, candSequences,
                 candSpans,   candDiagonals, chainAnchors, chainBegins,        chainEnds,         chainBeginDiagonals, chainEndDiagonals,
                 bestVerified, distances,   numOps,      scores,      ops,                 begins,            ends,      counters,        waitOffsets, one,
                 windowSequences, windowScores, zeros, windowBegins, windowEnds, mateBegins, slotSequences, slotAnchors, slotBegins, slotEnds,
                 slotBeginDiagonals, slotEndDiagonals, mateScores, mateNumOps, mateOps};
  for (size_t i = 0; i < sizeof all / sizeof *all; i++)
    if (all[i]) release(all[i]);
  if (onDevice) {
    void *copies[] = {b.chars, b.readOffsets, b.readSeedOffsets, b.starts, b.ends, b.seedEnds, b.mateChars, b.mateOffsets};
    for (size_t i = 0; i < sizeof copies / sizeof *copies; i++) release(copies[i]);
  }
}

/* the runs of a script in text form, * for none or for a row that did not hold them */
static void printScript(const uint32_t *ops, uint32_t numOps, uint32_t maxOps) {
  static const char letters[16] = {'?', 'I', 'D', '?', 'S', '?', '?', '=', 'X', '?', '?', '?', '?', '?', '?', '?'};
  if (numOps > maxOps || numOps == 0) printf("*");
  for (uint32_t k = 0; k < numOps && numOps <= maxOps; k++) printf("%" PRIu32 "%c", ops[k] >> 4, letters[ops[k] & 15u]);
}

int main(int argc, char **argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s records.fa pairs.txt width [step [minLength [cap [maxHitsPerSeed [band [minVotes [lookback [gapPenalty [bandPad [maxDrift [maxOps [match [mismatch [gapOpen [gapExtend [minScore]]]]]]]]]]]]]]]]\n", argv[0]);
    return 1;
  }
  struct Params p = {.step = argc > 4 ? strtoull(argv[4], NULL, 10) : 4, .cap = argc > 6 ? strtoull(argv[6], NULL, 10) : 64,
                     .minLength = argc > 5 ? (uint32_t)strtoul(argv[5], NULL, 10) : 16,
                     .maxHitsPerSeed = argc > 7 ? (uint32_t)strtoul(argv[7], NULL, 10) : 16, .band = argc > 8 ? (uint32_t)strtoul(argv[8], NULL, 10) : 2,
                     .minVotes = argc > 9 ? (uint32_t)strtoul(argv[9], NULL, 10) : 2,
                     .lookback = argc > 10 ? (uint32_t)strtoul(argv[10], NULL, 10) : AWFM_CHAINS_MAX_LOOKBACK,
                     .gapPenalty = argc > 11 ? (uint32_t)strtoul(argv[11], NULL, 10) : 1, .bandPad = argc > 12 ? (uint32_t)strtoul(argv[12], NULL, 10) : 8,
                     .maxDrift = argc > 13 ? (uint32_t)strtoul(argv[13], NULL, 10) : 15, .maxOps = argc > 14 ? (uint32_t)strtoul(argv[14], NULL, 10) : 32,
                     .scoring = {.match = argc > 15 ? (uint32_t)strtoul(argv[15], NULL, 10) : 1, .mismatch = argc > 16 ? (uint32_t)strtoul(argv[16], NULL, 10) : 4,
                                 .gapOpen = argc > 17 ? (uint32_t)strtoul(argv[17], NULL, 10) : 6,
                                 .gapExtend = argc > 18 ? (uint32_t)strtoul(argv[18], NULL, 10) : 1},
                     .minScore = argc > 19 ? (uint32_t)strtoul(argv[19], NULL, 10) : 30, .width = strtoull(argv[3], NULL, 10)};
  if (p.step == 0 || p.cap == 0 || p.maxOps == 0 || p.maxOps > AWFM_ALIGN_MAX_OPS) return 1;

  struct AwFmIndexConfiguration config = {.suffixArrayCompressionRatio = 8,
                                          .kmerLengthInSeedTable = 8,
                                          .alphabetType = AwFmAlphabetDna,
                                          .keepSuffixArrayInMemory = true,
                                          .storeOriginalSequence = false};
  struct AwFmIndex *index = NULL;
  enum AwFmReturnCode rc = awFmCreateIndexFromFasta(&index, &config, argv[1], "read_rescued.awfmi");
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

  /* the mates, concatenated per side, and where each begins: the odd lines are mate 1, the even ones mate 2 */
  FILE *file = fopen(argv[2], "r");
  if (!file) {
    fprintf(stderr, "cannot read %s\n", argv[2]);
    return 1;
  }
  struct Batch in = {0};
  size_t readCap = 1024, charCap = 1 << 16;
  in.chars = malloc(charCap);
  in.readOffsets = malloc((readCap + 1) * 8);
  in.readOffsets[0] = 0;
  size_t mateCap = 1 << 16, numMates = 0;
  in.mateChars = malloc(mateCap);
  in.mateOffsets = malloc((readCap + 1) * 8);
  in.mateOffsets[0] = 0;
  for (size_t lineNumber = 0; getline(&line, &lineCap, file) >= 0; lineNumber++) {
    const size_t length = strcspn(line, "\r\n");
    if (lineNumber & 1) {
      while (in.numMateChars + length > mateCap) in.mateChars = realloc(in.mateChars, mateCap *= 2);
      memcpy(in.mateChars + in.numMateChars, line, length);
      in.numMateChars += length;
      in.mateOffsets[++numMates] = in.numMateChars;
      continue;
    }
    if (in.numReads == readCap) {
      in.readOffsets = realloc(in.readOffsets, ((readCap *= 2) + 1) * 8);
      in.mateOffsets = realloc(in.mateOffsets, (readCap + 1) * 8);
    }
    while (in.numChars + length > charCap) in.chars = realloc(in.chars, charCap *= 2);
    memcpy(in.chars + in.numChars, line, length);
    in.numChars += length;
    in.readOffsets[++in.numReads] = in.numChars;
    in.numWindows += length / p.step;
  }
  free(line);
  fclose(file);
  if (numMates != in.numReads) {
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
  if (haveDevice) {
    AwFmGpuIndex *image = awfmGpuIndexAcquire(index); /* carries the record table of the FASTA file */
    if (!image) {
      fprintf(stderr, "no device image: %s\n", awfmGpuLastError());
      return 3;
    }
    check(awfmGpuIndexSetText(image, genome, genomeLength), "awfmGpuIndexSetText");
    run(index, image, genome, genomeLength, recordEnds, numRecords, &in, &p, &device);
    shown = &device;
    uint64_t different = 0;
    for (size_t r = 0; r < in.numReads; r++)
      different += host.scores[r] != device.scores[r] || host.distances[r] != device.distances[r] || host.begins[r] != device.begins[r] || host.ends[r] != device.ends[r] ||
                   host.numOps[r] != device.numOps[r] || host.sequences[r] != device.sequences[r] ||
                   memcmp(host.ops + r * p.maxOps, device.ops + r * p.maxOps, (size_t)p.maxOps * 4) != 0 ||
                   host.windowScores[r] != device.windowScores[r] || host.mateScores[r] != device.mateScores[r] ||
                   host.mateBegins[r] != device.mateBegins[r] || host.mateNumOps[r] != device.mateNumOps[r] ||
                   memcmp(host.mateOps + r * p.maxOps, device.mateOps + r * p.maxOps, (size_t)p.maxOps * 4) != 0;
    fprintf(stderr, "device and host twins: %" PRIu64 " pairs differ\n", different);
    if (different) return 4;
  }

  uint64_t numAligned = 0, numRescued = 0;
  for (size_t r = 0; r < in.numReads; r++) {
    if (shown->scores[r] == 0 || shown->scores[r] >= AWFM_VERIFY_TOO_LONG) { /* no mate 1, hence no window */
      printf("%zu\t*\t0\t0\t*\t0\t0\t0\t*\n", r);
      continue;
    }
    char *header = NULL;
    size_t headerLength = 0;
    if (awFmGetHeaderStringFromSequenceNumber(index, shown->sequences[r], &header, &headerLength) != AwFmSuccess) return 4;
    printf("%zu\t%.*s\t%" PRIu64 "\t%" PRIu32 "\t", r, (int)headerLength, header, shown->begins[r], shown->scores[r]);
    printScript(shown->ops + r * p.maxOps, shown->numOps[r], p.maxOps);
    numAligned++;
    const int rescued = shown->mateScores[r] != 0 && shown->mateScores[r] < AWFM_VERIFY_TOO_LONG;
    const uint32_t windowScore = shown->windowScores[r] < AWFM_VERIFY_TOO_LONG ? shown->windowScores[r] : 0;
    printf("\t%" PRIu64 "\t%" PRIu32 "\t%" PRIu32 "\t", rescued ? shown->mateBegins[r] : 0, windowScore, rescued ? shown->mateScores[r] : 0);
    printScript(shown->mateOps + r * p.maxOps, rescued ? shown->mateNumOps[r] : 0, p.maxOps);
    printf("\n");
    numRescued += (uint64_t)rescued;
  }
  fprintf(stderr, "pairs %" PRIu64 " windows %" PRIu64 " aligned %" PRIu64 " found %" PRIu64 " rescued %" PRIu64 " on the %s\n", in.numReads, in.numWindows,
          numAligned, shown->numFound, numRescued, haveDevice ? "device" : "host");

  awFmDeallocIndex(index);
  remove("read_rescued.awfmi");
  return 0;
}
