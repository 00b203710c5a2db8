/*
 * read_verified.c -- where each read lies and how well it fits there, against the two public headers only: read_chains.c with
 * the stage that follows.  A FASTA file -> index (awFmCreateIndexFromFasta) and its text on the device (awfmGpuIndexSetText: the
 * records concatenated with their NUL terminators) -> for every read the longest match that ends at every s-th position
 * (awfmGpuLongestSuffixMatches) -> located (awfmGpuHitOffsetsFromCounts, awfmGpuLocate) -> mapped to sequence coordinates
 * (awfmGpuLocalPositions) -> grouped (awfmGpuReadCandidates) -> chained (awfmGpuReadChains) -> every chain compared with the text
 * it names (awfmGpuVerifyChains, with the arrays of the two calls before passed straight in) -> one line
 * `read:header:begin:end:score:distance` per read that has a verified chain: the text interval of the slot with the smallest
 * banded edit distance, that chain's score, and the distance.  Only chains and distances come home.
 *
 *   cc -std=gnu11 -O2 examples/read_verified.c -Iinclude -Lavxwindowfmindex_amd -lawfmindex_amd \
 *      -Wl,-rpath,$PWD/avxwindowfmindex_amd -o read_verified &&
 *      ./read_verified genome.fa reads.txt [step [minLength [cap [maxHitsPerSeed [band [minVotes [lookback [gapPenalty [bandPad [maxDrift]]]]]]]]]]
 *
 * reads.txt: one read per line.  The buffers are page-locked host memory (awfmGpuHostAlloc), which the device reads and writes
 * in place: a program that keeps its reads on the device passes its own device pointers instead.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "AwFmIndex.h"
#include "awfm_gpu.h"

static void *pinned(uint64_t bytes) {
  void *p = awfmGpuHostAlloc(bytes ? bytes : 1);
  if (!p) {
    fprintf(stderr, "no page-locked memory: %s\n", awfmGpuLastError());
    exit(3);
  }
  return p;
}

int main(int argc, char **argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s records.fa reads.txt [step [minLength [cap [maxHitsPerSeed [band [minVotes [lookback [gapPenalty [bandPad [maxDrift]]]]]]]]]]\n", argv[0]);
    return 1;
  }
  const uint64_t step = argc > 3 ? strtoull(argv[3], NULL, 10) : 4, cap = argc > 5 ? strtoull(argv[5], NULL, 10) : 64;
  const uint32_t minLength = argc > 4 ? (uint32_t)strtoul(argv[4], NULL, 10) : 16;
  const uint32_t maxHitsPerSeed = argc > 6 ? (uint32_t)strtoul(argv[6], NULL, 10) : 16, band = argc > 7 ? (uint32_t)strtoul(argv[7], NULL, 10) : 2;
  const uint32_t minVotes = argc > 8 ? (uint32_t)strtoul(argv[8], NULL, 10) : 2, slots = 4;
  const uint32_t lookback = argc > 9 ? (uint32_t)strtoul(argv[9], NULL, 10) : AWFM_CHAINS_MAX_LOOKBACK;
  const uint32_t gapPenalty = argc > 10 ? (uint32_t)strtoul(argv[10], NULL, 10) : 1;
  const uint32_t bandPad = argc > 11 ? (uint32_t)strtoul(argv[11], NULL, 10) : 8, maxDrift = argc > 12 ? (uint32_t)strtoul(argv[12], NULL, 10) : 15;
  if (step == 0 || cap == 0) return 1;

  struct AwFmIndexConfiguration config = {.suffixArrayCompressionRatio = 8,
                                          .kmerLengthInSeedTable = 8,
                                          .alphabetType = AwFmAlphabetDna,
                                          .keepSuffixArrayInMemory = true,
                                          .storeOriginalSequence = false};
  struct AwFmIndex *index = NULL;
  enum AwFmReturnCode rc = awFmCreateIndexFromFasta(&index, &config, argv[1], "read_verified.awfmi");
  if (awFmReturnCodeIsFailure(rc)) {
    fprintf(stderr, "awFmCreateIndexFromFasta failed: %d\n", rc);
    return 2;
  }
  AwFmGpuIndex *image = awfmGpuIndexAcquire(index); /* carries the record table of the FASTA file */
  if (!image) {
    fprintf(stderr, "no device image: %s\n", awfmGpuLastError());
    return 3;
  }

  /* the indexed text: the records' residues, each record followed by a NUL terminator */
  FILE *fasta = fopen(argv[1], "r");
  if (!fasta) return 1;
  size_t genomeCap = 1 << 16, genomeLength = 0, numRecords = 0, lineCap = 0;
  uint8_t *genome = malloc(genomeCap);
  char *line = NULL; /* (getline: a line of any length is one line) */
  while (getline(&line, &lineCap, fasta) >= 0) {
    const size_t length = line[0] == '>' ? (numRecords++ ? 1 : 0) : strcspn(line, "\r\n");
    while (genomeLength + length + 1 > genomeCap) genome = realloc(genome, genomeCap *= 2);
    if (line[0] == '>') {
      if (length) genome[genomeLength++] = 0; /* the terminator of the record before */
    } else {
      memcpy(genome + genomeLength, line, length);
      genomeLength += length;
    }
  }
  fclose(fasta);
  if (numRecords) genome[genomeLength++] = 0;
  rc = awfmGpuIndexSetText(image, genome, genomeLength);
  if (awFmReturnCodeIsFailure(rc)) {
    fprintf(stderr, "awfmGpuIndexSetText failed: %d: %s\n", rc, awfmGpuLastError());
    return 3;
  }
  free(genome);

  /* the reads, concatenated, and where each begins */
  FILE *in = fopen(argv[2], "r");
  if (!in) {
    fprintf(stderr, "cannot read %s\n", argv[2]);
    return 1;
  }
  size_t numReads = 0, readCap = 1024, charCap = 1 << 16, numChars = 0, numWindows = 0;
  char *text = malloc(charCap);
  uint64_t *readAt = malloc((readCap + 1) * sizeof *readAt);
  readAt[0] = 0;
  while (getline(&line, &lineCap, in) >= 0) {
    const size_t length = strcspn(line, "\r\n");
    if (length == 0) continue;
    if (numReads == readCap) readAt = realloc(readAt, ((readCap *= 2) + 1) * sizeof *readAt);
    while (numChars + length > charCap) text = realloc(text, charCap *= 2);
    memcpy(text + numChars, line, length);
    numChars += length;
    readAt[++numReads] = numChars;
    numWindows += length / step;
  }
  free(line);
  fclose(in);

  /* window w: the characters before end position e = step, 2 step, ... of its read, `cap` at the most */
  uint8_t *chars = pinned(numChars);
  uint64_t *starts = pinned(numWindows * 8), *ends = pinned(numWindows * 8);
  uint64_t *readSeedOffsets = pinned((numReads + 1) * 8); /* the windows of a read are contiguous: its seeds */
  uint64_t *readOffsets = pinned((numReads + 1) * 8);
  memcpy(readOffsets, readAt, (numReads + 1) * 8);
  uint32_t *seedEnds = pinned(numWindows * 4);
  memcpy(chars, text, numChars);
  size_t w = 0;
  for (size_t r = 0; r < numReads; r++) {
    readSeedOffsets[r] = w;
    for (uint64_t e = step; e <= readAt[r + 1] - readAt[r]; e += step, w++) {
      starts[w] = readAt[r] + (e > cap ? e - cap : 0);
      ends[w] = readAt[r] + e;
      seedEnds[w] = (uint32_t)e;
    }
  }
  readSeedOffsets[numReads] = w;

  uint32_t *lengths = pinned(numWindows * 4), *counts = pinned(numWindows * 4);
  struct AwFmSearchRange *ranges = pinned(numWindows * sizeof *ranges);
  uint64_t *hitOffsets = pinned((numWindows + 1) * 8), totalHits = 0;
  void *scratch = pinned(awfmGpuScanScratchBytes(numWindows ? numWindows : 1));
  hitOffsets[numWindows] = 0;
  if (numWindows != 0) {
    rc = awfmGpuLongestSuffixMatches(image, chars, starts, ends, 0, numWindows, minLength, lengths, ranges, counts, NULL);
    if (!awFmReturnCodeIsFailure(rc)) /* (waits for the stream: the total comes back to the host) */
      rc = awfmGpuHitOffsetsFromCounts(image, counts, numWindows, hitOffsets, scratch, &totalHits, NULL);
    if (awFmReturnCodeIsFailure(rc)) {
      fprintf(stderr, "search failed: %d: %s\n", rc, awfmGpuLastError());
      return 3;
    }
  }
  uint64_t *positions = pinned(totalHits * 8), *waitOffsets = pinned(16), waited = 0;
  uint32_t *sequenceNumbers = pinned(totalHits * 4), *one = pinned(4);
  *one = 1;
  /* the candidates: what names a slot is all the chains need of them */
  uint32_t *candSequences = pinned(numReads * slots * 4), *candSpans = pinned(numReads * slots * 4);
  int64_t *candDiagonals = pinned(numReads * slots * 8);
  void *candScratch = pinned(awfmGpuReadCandidatesScratchBytes(numReads ? numReads : 1));
  /* the chains: six values per slot, the best slot per read, one counter */
  uint32_t *chainScores = pinned(numReads * slots * 4), *chainAnchors = pinned(numReads * slots * 4);
  uint32_t *chainBegins = pinned(numReads * slots * 4), *chainEnds = pinned(numReads * slots * 4), *bestSlots = pinned(numReads * 4);
  int64_t *chainBeginDiagonals = pinned(numReads * slots * 8), *chainEndDiagonals = pinned(numReads * slots * 8);
  uint64_t *numOverflowed = pinned(8), *numUnverified = pinned(8), numVerified = 0;
  uint32_t *editDistances = pinned(numReads * slots * 4), *bestVerified = pinned(numReads * 4);
  *numUnverified = 0;
  void *chainScratch = pinned(awfmGpuReadChainsScratchBytes(numReads ? numReads : 1));
  *numOverflowed = 0;
  if (totalHits != 0) {
    rc = awfmGpuLocate(image, ranges, hitOffsets, numWindows, totalHits, positions, NULL);
    if (!awFmReturnCodeIsFailure(rc))
      rc = awfmGpuLocalPositions(image, positions, totalHits, NULL, sequenceNumbers, positions /* in place */, NULL, NULL);
  }
  if (numReads != 0 && !awFmReturnCodeIsFailure(rc)) {
    const struct AwFmCandidateInputs in = {.readSeedOffsets = readSeedOffsets, .numSeeds = numWindows, .seedEnds = seedEnds,
                                           .seedLengths = lengths, /* as awfmGpuLongestSuffixMatches left them */
                                           .fixedLength = 0, .hitOffsets = hitOffsets, .numHits = totalHits, .positions = positions,
                                           .sequenceNumbers = sequenceNumbers};
    const struct AwFmCandidateOutputs out = {.sequences = candSequences, .diagonals = candDiagonals, .diagonalSpans = candSpans};
    const struct AwFmChainOutputs chains = {.chainScores = chainScores, .chainAnchors = chainAnchors, .chainReadBegins = chainBegins,
                                            .chainReadEnds = chainEnds, .chainBeginDiagonals = chainBeginDiagonals,
                                            .chainEndDiagonals = chainEndDiagonals, .bestSlots = bestSlots, .numOverflowed = numOverflowed};
    rc = awfmGpuReadCandidates(image, &in, numReads, maxHitsPerSeed, band, minVotes, slots, &out, candScratch, NULL);
    if (!awFmReturnCodeIsFailure(rc)) /* (the same stream: the slots are written before they are read) */
      rc = awfmGpuReadChains(image, &in, numReads, maxHitsPerSeed, band, slots, candSequences, candDiagonals, candSpans, lookback, gapPenalty,
                             &chains, chainScratch, NULL);
    if (!awFmReturnCodeIsFailure(rc)) { /* (the same stream again: the chains are written before they are read) */
      const struct AwFmVerifyInputs verify = {.readChars = chars, .numReadChars = numChars, .readOffsets = readOffsets,
                                              .sequences = candSequences, .chainAnchors = chainAnchors, .chainReadBegins = chainBegins,
                                              .chainReadEnds = chainEnds, .chainBeginDiagonals = chainBeginDiagonals,
                                              .chainEndDiagonals = chainEndDiagonals};
      const struct AwFmVerifyOutputs verified = {.editDistances = editDistances, .bestSlots = bestVerified, .numUnverified = numUnverified};
      rc = awfmGpuVerifyChains(image, &verify, numReads, slots, bandPad, maxDrift, &verified, NULL);
    }
    /* all of it is asynchronous.  A program with a stream of its own waits for it with its runtime (hipStreamSynchronize); this
     * one has only the two headers, in which the scan that returns its total to the host is the call that waits for the stream */
    if (!awFmReturnCodeIsFailure(rc)) rc = awfmGpuHitOffsetsFromCounts(image, one, 1, waitOffsets, scratch, &waited, NULL);
  }
  if (awFmReturnCodeIsFailure(rc)) {
    fprintf(stderr, "locate, candidates, chains or verification failed: %d: %s\n", rc, awfmGpuLastError());
    return 3;
  }

  for (size_t r = 0; r < numReads; r++) {
    if (bestVerified[r] == AWFM_CHAINS_NO_SLOT) continue;
    const size_t at = r * slots + bestVerified[r];
    char *header = NULL;
    size_t headerLength = 0;
    if (awFmGetHeaderStringFromSequenceNumber(index, candSequences[at], &header, &headerLength) != AwFmSuccess) return 4;
    printf("%zu:%.*s:%" PRId64 ":%" PRId64 ":%" PRIu32 ":%" PRIu32 "\n", r, (int)headerLength, header,
           (int64_t)chainBegins[at] + chainBeginDiagonals[at], (int64_t)chainEnds[at] + chainEndDiagonals[at], chainScores[at], editDistances[at]);
    numVerified++;
  }
  fprintf(stderr, "reads %zu windows %zu occurrences %" PRIu64 " verified %" PRIu64 " overflowed %" PRIu64 " unverified %" PRIu64 "\n", numReads,
          numWindows, totalHits, numVerified, *numOverflowed, *numUnverified);

  void *all[] = {chars,         starts,      ends,         lengths,      counts,          ranges,       hitOffsets,
                 scratch,       positions,   waitOffsets,  sequenceNumbers, one,          readSeedOffsets, seedEnds,
                 candSequences, candSpans,   candDiagonals, candScratch,  chainScores,     chainAnchors, chainBegins,
                 chainEnds,     bestSlots,   chainBeginDiagonals, chainEndDiagonals, numOverflowed, chainScratch,
                 readOffsets,   numUnverified, editDistances, bestVerified};
  for (size_t i = 0; i < sizeof all / sizeof *all; i++) awfmGpuHostFree(all[i]);
  free(readAt);
  free(text);
  awFmDeallocIndex(index);
  remove("read_verified.awfmi");
  return 0;
}
