/*
 * read_strands.c -- paired reads of BOTH strands on an index of ONE strand, from seeds to SAM lines, against the two public
 * headers only.  A FASTA file as it is (no reverse complements of the records) -> index (awFmCreateIndexFromFasta) -> the pairs
 * AS SEQUENCED, an inward-facing library -> ONE batch of 2R rows: the reads, then their reverse complements
 * (awfmReverseComplementReads with AWFM_COMPLEMENT_ALL into the second half of the buffer) -> the path of read_mapped.c for every
 * row: longest matches, located, mapped to sequence coordinates, candidate loci and chains with SLOTS - 1 slots in a slot table
 * of stride SLOTS -> slot scores (awfmScoreChainsAffine) on the 2R rows -> STRAND CHOICE (awfmChooseStrands, paired) -> window
 * scores on the windows it names, by row, into the free column -> slot scores and strand choice again -> ORIENT
 * (awfmOrientReads): the chosen strand of every read, R rows -> affine alignment with strandSlots, the classic CIGAR and MD:Z
 * (awfmAlignmentStrings), SAM records (awfmSamRecords) with baseFlags, properPairs, mappingQualities and secondScores as the
 * strand choice left them -> the header lines and one SAM line per read on the standard output.
 *
 * The program runs the host twins, which are the definition; the device calls take the same structs with device pointers and
 * a stream (tests/test_gpu_strands.py runs this loop on the device and compares).
 *
 *   cc -std=gnu11 -O2 examples/read_strands.c -Iinclude -Lavxwindowfmindex_amd -lawfmindex_amd \
 *      -Wl,-rpath,$PWD/avxwindowfmindex_amd -o read_strands &&
 *      ./read_strands genome.fa pairs.txt minInsert maxInsert [step [minLength [cap [maxHitsPerSeed [band [minVotes [lookback [gapPenalty
 *                     [bandPad [maxDrift [maxOps [match [mismatch [gapOpen [gapExtend [minScore [unpairedPenalty [windowPad [mapqCap]]]]]]]]]]]]]]]]]]]
 *
 * pairs.txt: two lines per pair, mate 1 and then mate 2, as sequenced.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "AwFmIndex.h"
#include "awfm_gpu.h"

enum { SLOTS = 4, THREADS = 4 };

static void *buffer(uint64_t bytes) {
  void *p = calloc(bytes ? bytes : 1, 1);
  if (!p) {
    fprintf(stderr, "out of memory\n");
    exit(3);
  }
  return p;
}

static void check(enum AwFmReturnCode rc, const char *what) {
  if (awFmReturnCodeIsFailure(rc)) {
    fprintf(stderr, "%s failed: %d: %s\n", what, rc, awfmGpuLastError());
    exit(3);
  }
}

static uint32_t argument(int argc, char **argv, int at, uint32_t otherwise) { return argc > at ? (uint32_t)strtoul(argv[at], NULL, 10) : otherwise; }

int main(int argc, char **argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: %s genome.fa pairs.txt minInsert maxInsert [step [minLength [cap [maxHitsPerSeed [band [minVotes [lookback [gapPenalty [bandPad [maxDrift [maxOps [match [mismatch [gapOpen [gapExtend [minScore [unpairedPenalty [windowPad [mapqCap]]]]]]]]]]]]]]]]]]]\n", argv[0]);
    return 1;
  }
  const uint64_t step = argument(argc, argv, 5, 4), cap = argument(argc, argv, 7, 64);
  const uint32_t minLength = argument(argc, argv, 6, 16), maxHitsPerSeed = argument(argc, argv, 8, 16), band = argument(argc, argv, 9, 2);
  const uint32_t minVotes = argument(argc, argv, 10, 2), lookback = argument(argc, argv, 11, AWFM_CHAINS_MAX_LOOKBACK), gapPenalty = argument(argc, argv, 12, 1);
  const uint32_t bandPad = argument(argc, argv, 13, 8), maxDrift = argument(argc, argv, 14, 15), maxOps = argument(argc, argv, 15, 32);
  const struct AwFmAlignScoring scoring = {.match = argument(argc, argv, 16, 1), .mismatch = argument(argc, argv, 17, 4),
                                           .gapOpen = argument(argc, argv, 18, 6), .gapExtend = argument(argc, argv, 19, 1)};
  const struct AwFmPairParams pairing = {.minInsert = strtoll(argv[3], NULL, 10), .maxInsert = strtoll(argv[4], NULL, 10),
                                         .minScore = argument(argc, argv, 20, 30), .unpairedPenalty = argument(argc, argv, 21, 17),
                                         .windowPad = argument(argc, argv, 22, 50), .mapqCap = argument(argc, argv, 23, 60)};
  if (step == 0 || cap == 0 || maxOps == 0 || maxOps > AWFM_ALIGN_MAX_OPS) return 1;

  struct AwFmIndexConfiguration config = {.suffixArrayCompressionRatio = 8,
                                          .kmerLengthInSeedTable = 8,
                                          .alphabetType = AwFmAlphabetDna,
                                          .keepSuffixArrayInMemory = true,
                                          .storeOriginalSequence = false};
  struct AwFmIndex *index = NULL;
  enum AwFmReturnCode rc = awFmCreateIndexFromFasta(&index, &config, argv[1], "read_strands.awfmi");
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

  /* the reads as sequenced, interleaved, in the FIRST HALF of a buffer of twice their size; no qualities in this file format:
   * a constant one, so that QUAL shows the orientation's effect on nothing but stays a legal column */
  FILE *file = fopen(argv[2], "r");
  if (!file) {
    fprintf(stderr, "cannot read %s\n", argv[2]);
    return 1;
  }
  uint64_t numReads = 0, numChars = 0;
  size_t readCap = 1024, charCap = 1 << 16;
  uint8_t *sequenced = malloc(charCap);
  uint64_t *lengthsOfReads = malloc(readCap * 8);
  while (getline(&line, &lineCap, file) >= 0) {
    const size_t length = strcspn(line, "\r\n");
    if (numReads == readCap) lengthsOfReads = realloc(lengthsOfReads, (readCap *= 2) * 8);
    while (numChars + length > charCap) sequenced = realloc(sequenced, charCap *= 2);
    memcpy(sequenced + numChars, line, length);
    numChars += length;
    lengthsOfReads[numReads++] = length;
  }
  free(line);
  fclose(file);
  if (numReads & 1) {
    fprintf(stderr, "%s: a mate 1 without its mate 2\n", argv[2]);
    return 1;
  }
  /* the 2R rows: row r the read as sequenced, row R + r its reverse complement */
  const uint64_t R = numReads, numRows = 2 * R, numRowChars = 2 * numChars, numSlots = numRows * SLOTS;
  uint8_t *chars = buffer(numRowChars), *qualities = buffer(numRowChars);
  uint64_t *rowOffsets = buffer((numRows + 1) * 8), malformed = 0;
  memcpy(chars, sequenced, numChars);
  memset(qualities, 'I', numRowChars);
  for (uint64_t row = 0; row < numRows; row++) rowOffsets[row + 1] = rowOffsets[row] + lengthsOfReads[row % (R ? R : 1)];
  if (R) check(awfmReverseComplementReads(chars, numChars, rowOffsets, R, AWFM_COMPLEMENT_ALL, chars + numChars, &malformed, THREADS), "reverse complement");

  /* window w: the characters before end position e = step, 2 step, ... of its row, `cap` at the most */
  uint64_t numWindows = 0;
  for (uint64_t row = 0; row < numRows; row++) numWindows += (rowOffsets[row + 1] - rowOffsets[row]) / step;
  uint64_t *starts = buffer(numWindows * 8), *ends = buffer(numWindows * 8), *rowSeedOffsets = buffer((numRows + 1) * 8);
  uint32_t *seedEnds = buffer(numWindows * 4);
  uint64_t w = 0;
  for (uint64_t row = 0; row < numRows; row++) {
    rowSeedOffsets[row] = w;
    for (uint64_t e = step; e <= rowOffsets[row + 1] - rowOffsets[row]; e += step, w++) {
      starts[w] = rowOffsets[row] + (e > cap ? e - cap : 0);
      ends[w] = rowOffsets[row] + e;
      seedEnds[w] = (uint32_t)e;
    }
  }
  rowSeedOffsets[numRows] = w;

  /* seeds, hits and sequence coordinates of every row */
  uint32_t *lengths = buffer(numWindows * 4), *counts = buffer(numWindows * 4);
  struct AwFmSearchRange *ranges = buffer(numWindows * sizeof *ranges);
  uint64_t *hitOffsets = buffer((numWindows + 1) * 8), totalHits = 0;
  if (numWindows) check(awfmLongestSuffixMatches(index, chars, starts, ends, 0, numWindows, minLength, lengths, ranges, counts, THREADS), "search");
  for (uint64_t k = 0; k < numWindows; k++) hitOffsets[k + 1] = hitOffsets[k] + counts[k];
  totalHits = hitOffsets[numWindows];
  uint64_t *positions = buffer(totalHits * 8);
  uint32_t *sequenceNumbers = buffer(totalHits * 4);
  for (uint64_t k = 0; k < numWindows; k++)
    for (uint64_t h = 0; h < counts[k]; h++) positions[hitOffsets[k] + h] = awFmFindDatabaseHitPositionSingle(index, ranges[k].startPtr + h, &rc);
  if (totalHits) check(awfmLocalPositions(index, positions, totalHits, sequenceNumbers, positions /* in place */, NULL, THREADS), "local positions");

  /* candidates and chains with SLOTS - 1 slots a row, then the slot table of stride SLOTS: its last column is the window call's */
  const uint32_t narrow = SLOTS - 1;
  uint32_t *candSequences = buffer(numRows * narrow * 4), *candSpans = buffer(numRows * narrow * 4);
  int64_t *candDiagonals = buffer(numRows * narrow * 8);
  uint32_t *narrowAnchors = buffer(numRows * narrow * 4), *narrowBegins = buffer(numRows * narrow * 4), *narrowEnds = buffer(numRows * narrow * 4);
  int64_t *narrowBeginDiagonals = buffer(numRows * narrow * 8), *narrowEndDiagonals = buffer(numRows * narrow * 8);
  uint32_t *sequences = buffer(numSlots * 4), *chainAnchors = buffer(numSlots * 4), *chainBegins = buffer(numSlots * 4), *chainEnds = buffer(numSlots * 4);
  int64_t *chainBeginDiagonals = buffer(numSlots * 8), *chainEndDiagonals = buffer(numSlots * 8);
  uint32_t *slotScores = buffer(numSlots * 4), *slotReadEnds = buffer(numSlots * 4);
  uint64_t *slotTextEnds = buffer(numSlots * 8);
  if (R == 0) {
    awFmDeallocIndex(index);
    remove("read_strands.awfmi");
    return 0;
  }
  const struct AwFmCandidateInputs cin = {.readSeedOffsets = rowSeedOffsets, .numSeeds = numWindows, .seedEnds = seedEnds, .seedLengths = lengths,
                                          .fixedLength = 0, .hitOffsets = hitOffsets, .numHits = totalHits, .positions = positions,
                                          .sequenceNumbers = sequenceNumbers};
  const struct AwFmCandidateOutputs cout = {.sequences = candSequences, .diagonals = candDiagonals, .diagonalSpans = candSpans};
  const struct AwFmChainOutputs chains = {.chainAnchors = narrowAnchors, .chainReadBegins = narrowBegins, .chainReadEnds = narrowEnds,
                                          .chainBeginDiagonals = narrowBeginDiagonals, .chainEndDiagonals = narrowEndDiagonals};
  check(awfmReadCandidates(&cin, numRows, maxHitsPerSeed, band, minVotes, narrow, &cout, THREADS), "candidates");
  check(awfmReadChains(&cin, numRows, maxHitsPerSeed, band, narrow, candSequences, candDiagonals, candSpans, lookback, gapPenalty, &chains, THREADS), "chains");
  for (uint64_t row = 0; row < numRows; row++)
    for (uint32_t j = 0; j < SLOTS; j++) {
      const uint64_t to = row * SLOTS + j, from = row * narrow + j;
      const int used = j < narrow;
      sequences[to] = used ? candSequences[from] : AWFM_CANDIDATES_NONE;
      chainAnchors[to] = used ? narrowAnchors[from] : 0;
      chainBegins[to] = used ? narrowBegins[from] : 0;
      chainEnds[to] = used ? narrowEnds[from] : 0;
      chainBeginDiagonals[to] = used ? narrowBeginDiagonals[from] : 0;
      chainEndDiagonals[to] = used ? narrowEndDiagonals[from] : 0;
    }

  /* THE LOOP on the 2R rows: slot scores, strand choice, window scores on the windows it names, slot scores, strand choice */
  uint8_t *strands = buffer(R), *mappingQualities = buffer(R), *properPairs = buffer(R / 2);
  uint16_t *baseFlags = buffer(R * 2);
  uint32_t *strandSlots = buffer(R * 4), *secondScores = buffer(R * 4), *windowSequences = buffer(numRows * 4);
  uint64_t *windowBegins = buffer(numRows * 8), *windowEnds = buffer(numRows * 8), counters[8] = {0};
  const struct AwFmVerifyInputs rows = {.readChars = chars, .numReadChars = numRowChars, .readOffsets = rowOffsets, .sequences = sequences,
                                        .chainAnchors = chainAnchors, .chainReadBegins = chainBegins, .chainReadEnds = chainEnds,
                                        .chainBeginDiagonals = chainBeginDiagonals, .chainEndDiagonals = chainEndDiagonals};
  const struct AwFmSlotScoreOutputs scored = {.slotScores = slotScores, .slotReadEnds = slotReadEnds, .slotTextEnds = slotTextEnds};
  const struct AwFmStrandInputs both = {.readOffsets = rowOffsets, .sequences = sequences, .slotScores = slotScores, .slotReadEnds = slotReadEnds,
                                        .slotTextEnds = slotTextEnds};
  const struct AwFmStrandOutputs firstChoice = {.windowSequences = windowSequences, .windowBegins = windowBegins, .windowEnds = windowEnds};
  const struct AwFmStrandOutputs chosen = {.strands = strands, .strandSlots = strandSlots, .secondScores = secondScores,
                                           .mappingQualities = mappingQualities, .baseFlags = baseFlags, .properPairs = properPairs,
                                           .numReverse = &counters[0], .numProper = &counters[1], .numWindows = &counters[2],
                                           .numMalformed = &counters[3]};
  const struct AwFmWindowInputs win = {.readChars = chars, .numReadChars = numRowChars, .readOffsets = rowOffsets, .windowSequences = windowSequences,
                                       .windowBegins = windowBegins, .windowEnds = windowEnds};
  const struct AwFmWindowOutputs placed = {.sequences = sequences, .chainAnchors = chainAnchors, .chainReadBegins = chainBegins,
                                           .chainReadEnds = chainEnds, .chainBeginDiagonals = chainBeginDiagonals,
                                           .chainEndDiagonals = chainEndDiagonals, .numFound = &counters[4]};
  check(awfmScoreChainsAffine(&rows, numRows, SLOTS, bandPad, maxDrift, &scoring, pairing.minScore, pairing.mapqCap, genome, genomeLength, recordEnds,
                              numRecords, AwFmAlphabetDna, &scored, THREADS), "slot scores");
  check(awfmChooseStrands(&both, R, SLOTS, AWFM_STRANDS_PAIRED, &pairing, &firstChoice, THREADS), "strand choice");
  check(awfmScoreWindowsAffine(&win, numRows, &scoring, pairing.minScore, SLOTS, SLOTS - 1, genome, genomeLength, recordEnds, numRecords, AwFmAlphabetDna,
                               &placed, THREADS), "window scores");
  check(awfmScoreChainsAffine(&rows, numRows, SLOTS, bandPad, maxDrift, &scoring, pairing.minScore, pairing.mapqCap, genome, genomeLength, recordEnds,
                              numRecords, AwFmAlphabetDna, &scored, THREADS), "slot scores");
  check(awfmChooseStrands(&both, R, SLOTS, AWFM_STRANDS_PAIRED, &pairing, &chosen, THREADS), "strand choice");

  /* ORIENT: the chosen strand of every read, R rows; SEQ and QUAL come out as SAM wants them */
  uint8_t *orientedChars = buffer(numChars), *orientedQualities = buffer(numChars);
  uint64_t *readOffsets = buffer((R + 1) * 8);
  uint32_t *oSequences = buffer(R * SLOTS * 4), *oAnchors = buffer(R * SLOTS * 4), *oBegins = buffer(R * SLOTS * 4), *oEnds = buffer(R * SLOTS * 4);
  int64_t *oBeginDiagonals = buffer(R * SLOTS * 8), *oEndDiagonals = buffer(R * SLOTS * 8);
  const struct AwFmOrientInputs oin = {.rows = rows, .qualities = qualities, .strands = strands};
  const struct AwFmOrientOutputs oout = {.readChars = orientedChars, .capacity = numChars, .readOffsets = readOffsets, .qualities = orientedQualities,
                                         .sequences = oSequences, .chainAnchors = oAnchors, .chainReadBegins = oBegins, .chainReadEnds = oEnds,
                                         .chainBeginDiagonals = oBeginDiagonals, .chainEndDiagonals = oEndDiagonals, .numMalformed = &counters[5]};
  check(awfmOrientReads(&oin, R, SLOTS, &oout, THREADS), "orient");

  /* affine alignment with strandSlots, the strings, the records: R rows, unchanged calls */
  uint32_t *scores = buffer(R * 4), *editDistances = buffer(R * 4), *numOps = buffer(R * 4), *ops = buffer(R * maxOps * 4);
  uint64_t *textBegins = buffer(R * 8), *textEnds = buffer(R * 8);
  const struct AwFmVerifyInputs oriented = {.readChars = orientedChars, .numReadChars = numChars, .readOffsets = readOffsets, .sequences = oSequences,
                                            .chainAnchors = oAnchors, .chainReadBegins = oBegins, .chainReadEnds = oEnds,
                                            .chainBeginDiagonals = oBeginDiagonals, .chainEndDiagonals = oEndDiagonals};
  const struct AwFmAffineOutputs aligned = {.scores = scores, .editDistances = editDistances, .textBegins = textBegins, .textEnds = textEnds,
                                            .numOps = numOps, .ops = ops};
  check(awfmAlignChainsAffine(&oriented, strandSlots, R, SLOTS, bandPad, maxDrift, &scoring, maxOps, genome, genomeLength, recordEnds, numRecords,
                              AwFmAlphabetDna, &aligned, THREADS), "alignment");
  const struct AwFmStringInputs sin = {.sequences = oSequences, .slots = strandSlots, .textBegins = textBegins, .numOps = numOps, .ops = ops};
  uint64_t *cigarOffsets = buffer((R + 1) * 8), *mdOffsets = buffer((R + 1) * 8);
  struct AwFmStringOutputs strings = {.cigarOffsets = cigarOffsets, .mdOffsets = mdOffsets};
  check(awfmAlignmentStrings(&sin, R, SLOTS, maxOps, AWFM_STRINGS_CIGAR_M, genome, genomeLength, recordEnds, numRecords, AwFmAlphabetDna, &strings, THREADS),
        "string lengths"); /* (offsets alone size the arenas) */
  strings.cigarCapacity = cigarOffsets[R];
  strings.mdCapacity = mdOffsets[R];
  strings.cigarChars = buffer(strings.cigarCapacity);
  strings.mdChars = buffer(strings.mdCapacity);
  check(awfmAlignmentStrings(&sin, R, SLOTS, maxOps, AWFM_STRINGS_CIGAR_M, genome, genomeLength, recordEnds, numRecords, AwFmAlphabetDna, &strings, THREADS),
        "strings");
  uint64_t *nameOffsets = buffer((numRecords + 1) * 8);
  check(awfmRecordNames(index, nameOffsets, NULL, 0), "record names");
  uint8_t *nameChars = buffer(nameOffsets[numRecords]);
  check(awfmRecordNames(index, nameOffsets, nameChars, nameOffsets[numRecords]), "record names");
  const struct AwFmSamInputs sam = {.readChars = orientedChars, .numReadChars = numChars, .readOffsets = readOffsets, .qualities = orientedQualities,
                                    .recordNameOffsets = nameOffsets, .recordNameChars = nameChars, .numRecordNames = (uint32_t)numRecords,
                                    .sequences = oSequences, .slots = strandSlots, .scores = scores, .editDistances = editDistances,
                                    .textBegins = textBegins, .textEnds = textEnds, .cigarOffsets = cigarOffsets, .cigarChars = strings.cigarChars,
                                    .mdOffsets = mdOffsets, .mdChars = strings.mdChars, .mappingQualities = mappingQualities,
                                    .secondScores = secondScores, .baseFlags = baseFlags, .properPairs = properPairs};
  uint64_t *lineOffsets = buffer((R + 1) * 8);
  struct AwFmSamOutputs lines = {.lineOffsets = lineOffsets, .numUnaligned = &counters[6], .numOverflow = &counters[7]};
  check(awfmSamRecords(&sam, R, SLOTS, AWFM_SAM_PAIRED, &lines, THREADS), "line lengths");
  counters[6] = 0;
  lines.lineCapacity = lineOffsets[R];
  lines.lineChars = buffer(lines.lineCapacity);
  check(awfmSamRecords(&sam, R, SLOTS, AWFM_SAM_PAIRED, &lines, THREADS), "records");

  const uint64_t headerLength = awfmSamHeader(index, NULL, 0);
  uint8_t *header = buffer(headerLength);
  awfmSamHeader(index, header, headerLength);
  fwrite(header, 1, headerLength, stdout);
  fwrite(lines.lineChars, 1, lines.lineCapacity, stdout);
  fprintf(stderr, "reads %" PRIu64 " on the reverse strand %" PRIu64 " proper pairs %" PRIu64 " rescue windows left %" PRIu64 " found in windows %" PRIu64
                  " malformed %" PRIu64 " unaligned %" PRIu64 "\n",
          R, counters[0], counters[1], counters[2], counters[4], counters[3] + counters[5] + malformed, counters[6]);
  awFmDeallocIndex(index);
  remove("read_strands.awfmi");
  return 0;
}
