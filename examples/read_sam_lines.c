/*
 * read_sam_lines.c -- a SAM file for a batch of reads, against the two public headers only: read_sam.c's pipeline with the slot
 * scores in the place of verification, then the call that writes the records.  A FASTA file -> index (awFmCreateIndexFromFasta)
 * -> for every read the longest match that ends at every s-th position -> located -> mapped to sequence coordinates -> grouped
 * into candidate loci -> chained -> every chain slot scored with affine gap costs: the best slot, the second score and the
 * mapping quality of every read (awfmScoreChainsAffine / awfmGpuScoreChainsAffine) -> the best slot aligned locally -> the
 * classic CIGAR and the MD:Z string of every aligned read, packed -> one SAM line per read, packed behind offsets
 * (awfmSamRecords / awfmGpuSamRecords, fed with the arrays of the calls before as they are: first for the offsets alone, which
 * size the arena, then for the bytes).  QNAME is the read's number, one strand, no qualities.
 *
 * The program runs the whole path through the host twins and, when a GPU is present, through the device calls as well (the text
 * on the device: awfmGpuIndexSetText); it compares the two arenas byte for byte, refuses to print when they differ, and writes the
 * header lines (awfmSamHeader) and the arena with ONE fwrite: no line is formatted on the host.
 *
 *   cc -std=gnu11 -O2 examples/read_sam_lines.c -Iinclude -Lavxwindowfmindex_amd -lawfmindex_amd \
 *      -Wl,-rpath,$PWD/avxwindowfmindex_amd -o read_sam_lines &&
 *      ./read_sam_lines genome.fa reads.txt [step [minLength [cap [maxHitsPerSeed [band [minVotes [lookback [gapPenalty [bandPad [maxDrift [maxOps
 *                       [match [mismatch [gapOpen [gapExtend]]]]]]]]]]]]]]] > reads.sam
 *
 * reads.txt: one read per line.  On the device the buffers are page-locked host memory (awfmGpuHostAlloc), which the device
 * reads and writes in place: a program that keeps its reads on the device passes its own device pointers instead.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "AwFmIndex.h"
#include "awfm_gpu.h"

enum { SLOTS = 4, THREADS = 4, MAPQ_CAP = 60 };

struct Params {
  uint64_t step, cap;
  uint32_t minLength, maxHitsPerSeed, band, minVotes, lookback, gapPenalty, bandPad, maxDrift, maxOps;
  struct AwFmAlignScoring scoring;
};

struct Batch { /* the reads and their windows; on the device side the same arrays in page-locked memory */
  uint64_t numReads, numChars, numWindows;
  uint8_t *chars;
  uint64_t *readOffsets, *readSeedOffsets, *starts, *ends;
  uint32_t *seedEnds;
};

struct Result { /* per read */
  uint32_t *sequences, *scores, *distances, *numOps, *ops;
  uint64_t *begins, *ends;
  uint64_t numUnaligned, numTruncated;
  uint64_t *cigarOffsets, *mdOffsets; /* [numReads + 1]: read r's strings are the bytes [offsets[r], offsets[r + 1]) */
  uint8_t *cigarChars, *mdChars;
  uint64_t numSkipped, numOverflow;
  uint64_t *lineOffsets; /* [numReads + 1]: read r's line is the bytes [lineOffsets[r], lineOffsets[r + 1]) */
  uint8_t *lineChars;
  uint64_t samUnaligned, samOverflow;
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

/* everything from the windows to the alignment; image == NULL: the host twins */
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
  uint64_t *begins = buffer(numReads * 8), *ends = buffer(numReads * 8), *counters = buffer(48), *waitOffsets = buffer(16), waited = 0;
  uint64_t *cigarOffsets = buffer((numReads + 1) * 8), *mdOffsets = buffer((numReads + 1) * 8);
  uint8_t *cigarChars = NULL, *mdChars = NULL;
  uint32_t *secondScores = buffer(numReads * 4);
  uint8_t *mappingQualities = buffer(numReads);
  uint64_t *lineOffsets = buffer((numReads + 1) * 8);
  uint8_t *lineChars = NULL;
  /* the records' names: the first word of every header, packed (host only: the device gets a copy) */
  uint64_t *nameOffsets = buffer((numRecords + 1) * 8);
  check(awfmRecordNames(index, nameOffsets, NULL, 0), "record names");
  uint8_t *nameChars = buffer(nameOffsets[numRecords]);
  check(awfmRecordNames(index, nameOffsets, nameChars, nameOffsets[numRecords]), "record names");
  uint32_t *one = buffer(4);
  *one = 1;
  counters[0] = counters[1] = counters[2] = counters[3] = counters[4] = counters[5] = 0;
  cigarOffsets[numReads] = mdOffsets[numReads] = lineOffsets[numReads] = 0;
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
    const struct AwFmSlotScoreOutputs scored = {.bestSlots = bestVerified, .secondScores = secondScores, .mappingQualities = mappingQualities};
    const struct AwFmAffineOutputs aligned = {.scores = scores, .editDistances = distances, .textBegins = begins, .textEnds = ends,
                                              .numOps = numOps, .ops = ops, .numUnaligned = &counters[0], .numTruncated = &counters[1]};
    /* the strings' inputs are the alignment's arrays as they are */
    const struct AwFmStringInputs sin = {.sequences = candSequences, .slots = bestVerified, .textBegins = begins, .numOps = numOps, .ops = ops};
    struct AwFmStringOutputs strings = {.cigarOffsets = cigarOffsets, .mdOffsets = mdOffsets};
    /* the records' inputs are the arrays of the calls before as they are; the arenas are filled in below */
    struct AwFmSamInputs sam = {.readChars = b.chars, .numReadChars = in->numChars, .readOffsets = b.readOffsets, .recordNameOffsets = nameOffsets,
                                .recordNameChars = nameChars, .numRecordNames = (uint32_t)numRecords, .sequences = candSequences,
                                .slots = bestVerified, .scores = scores, .editDistances = distances, .textBegins = begins, .textEnds = ends,
                                .cigarOffsets = cigarOffsets, .mdOffsets = mdOffsets, .mappingQualities = mappingQualities,
                                .secondScores = secondScores};
    struct AwFmSamOutputs lines = {.lineOffsets = lineOffsets};
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
      check(awfmGpuScoreChainsAffine(image, &vin, numReads, SLOTS, p->bandPad, p->maxDrift, &p->scoring, 0, MAPQ_CAP, &scored, NULL), "slot scores");
      check(awfmGpuAlignChainsAffine(image, &vin, bestVerified, numReads, SLOTS, p->bandPad, p->maxDrift, &p->scoring, p->maxOps, maxRows, &aligned,
                                     trace, NULL), "alignment");
      /* the strings: the offsets alone size the arenas (the one value that comes home), then the bytes */
      void *stringScratch = buffer(awfmGpuAlignmentStringsScratchBytes(image, numReads));
      check(awfmGpuAlignmentStrings(image, &sin, numReads, SLOTS, p->maxOps, AWFM_STRINGS_CIGAR_M, &strings, stringScratch, NULL), "string offsets");
      check(awfmGpuHitOffsetsFromCounts(image, one, 1, waitOffsets, scan, &waited, NULL), "wait");
      strings.cigarCapacity = cigarOffsets[numReads];
      strings.mdCapacity = mdOffsets[numReads];
      strings.cigarChars = cigarChars = buffer(strings.cigarCapacity);
      strings.mdChars = mdChars = buffer(strings.mdCapacity);
      strings.numSkipped = &counters[2];
      strings.numOverflow = &counters[3];
      check(awfmGpuAlignmentStrings(image, &sin, numReads, SLOTS, p->maxOps, AWFM_STRINGS_CIGAR_M, &strings, stringScratch, NULL), "strings");
      /* all of it is asynchronous; with only the two headers, the scan that returns its total to the host is the call that
       * waits for the stream */
      /* the records: again the offsets alone first, then the bytes */
      void *samScratch = buffer(awfmGpuSamRecordsScratchBytes(image, numReads));
      sam.cigarChars = cigarChars;
      sam.mdChars = mdChars;
      check(awfmGpuSamRecords(image, &sam, numReads, SLOTS, 0, &lines, samScratch, NULL), "line offsets");
      check(awfmGpuHitOffsetsFromCounts(image, one, 1, waitOffsets, scan, &waited, NULL), "wait");
      lines.lineCapacity = lineOffsets[numReads];
      lines.lineChars = lineChars = buffer(lines.lineCapacity);
      lines.numUnaligned = &counters[4];
      lines.numOverflow = &counters[5];
      check(awfmGpuSamRecords(image, &sam, numReads, SLOTS, 0, &lines, samScratch, NULL), "records");
      check(awfmGpuHitOffsetsFromCounts(image, one, 1, waitOffsets, scan, &waited, NULL), "wait");
      release(samScratch);
      release(stringScratch);
      release(candScratch);
      release(chainScratch);
      release(trace);
    } else {
      check(awfmReadCandidates(&cin, numReads, p->maxHitsPerSeed, p->band, p->minVotes, SLOTS, &cout, THREADS), "candidates");
      check(awfmReadChains(&cin, numReads, p->maxHitsPerSeed, p->band, SLOTS, candSequences, candDiagonals, candSpans, p->lookback, p->gapPenalty,
                           &chains, THREADS), "chains");
      check(awfmScoreChainsAffine(&vin, numReads, SLOTS, p->bandPad, p->maxDrift, &p->scoring, 0, MAPQ_CAP, genome, genomeLength, recordEnds,
                                  numRecords, AwFmAlphabetDna, &scored, THREADS), "slot scores");
      check(awfmAlignChainsAffine(&vin, bestVerified, numReads, SLOTS, p->bandPad, p->maxDrift, &p->scoring, p->maxOps, genome, genomeLength,
                                  recordEnds, numRecords, AwFmAlphabetDna, &aligned, THREADS), "alignment");
      check(awfmAlignmentStrings(&sin, numReads, SLOTS, p->maxOps, AWFM_STRINGS_CIGAR_M, genome, genomeLength, recordEnds, numRecords,
                                 AwFmAlphabetDna, &strings, THREADS), "string offsets");
      strings.cigarCapacity = cigarOffsets[numReads];
      strings.mdCapacity = mdOffsets[numReads];
      strings.cigarChars = cigarChars = buffer(strings.cigarCapacity);
      strings.mdChars = mdChars = buffer(strings.mdCapacity);
      strings.numSkipped = &counters[2];
      strings.numOverflow = &counters[3];
      check(awfmAlignmentStrings(&sin, numReads, SLOTS, p->maxOps, AWFM_STRINGS_CIGAR_M, genome, genomeLength, recordEnds, numRecords,
                                 AwFmAlphabetDna, &strings, THREADS), "strings");
      sam.cigarChars = cigarChars;
      sam.mdChars = mdChars;
      check(awfmSamRecords(&sam, numReads, SLOTS, 0, &lines, THREADS), "line offsets");
      lines.lineCapacity = lineOffsets[numReads];
      lines.lineChars = lineChars = buffer(lines.lineCapacity);
      lines.numUnaligned = &counters[4];
      lines.numOverflow = &counters[5];
      check(awfmSamRecords(&sam, numReads, SLOTS, 0, &lines, THREADS), "records");
    }
  }
  out->sequences = malloc((numReads + 1) * 4);
  out->distances = malloc((numReads + 1) * 4);
  out->scores = malloc((numReads + 1) * 4);
  out->numOps = malloc((numReads + 1) * 4);
  out->ops = malloc((numReads * p->maxOps + 1) * 4);
  out->begins = malloc((numReads + 1) * 8);
  out->ends = malloc((numReads + 1) * 8);
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
  }
  out->numUnaligned = counters[0];
  out->numTruncated = counters[1];
  out->numSkipped = counters[2];
  out->numOverflow = counters[3];
  out->cigarOffsets = memcpy(malloc((numReads + 1) * 8), cigarOffsets, (numReads + 1) * 8);
  out->mdOffsets = memcpy(malloc((numReads + 1) * 8), mdOffsets, (numReads + 1) * 8);
  out->cigarChars = malloc(cigarOffsets[numReads] + 1);
  out->mdChars = malloc(mdOffsets[numReads] + 1);
  if (cigarChars) memcpy(out->cigarChars, cigarChars, cigarOffsets[numReads]);
  if (mdChars) memcpy(out->mdChars, mdChars, mdOffsets[numReads]);
  out->samUnaligned = counters[4];
  out->samOverflow = counters[5];
  out->lineOffsets = memcpy(malloc((numReads + 1) * 8), lineOffsets, (numReads + 1) * 8);
  out->lineChars = malloc(lineOffsets[numReads] + 1);
  if (lineChars) memcpy(out->lineChars, lineChars, lineOffsets[numReads]);
  void *all[] = {lengths,     counts,       ranges,      hitOffsets,          scan,              positions, sequenceNumbers, candSequences,
                 candSpans,   candDiagonals, chainAnchors, chainBegins,        chainEnds,         chainBeginDiagonals, chainEndDiagonals,
                 bestVerified, distances,   numOps,      scores,      ops,                 begins,            ends,      counters,        waitOffsets, one,
                 cigarOffsets, mdOffsets, cigarChars, mdChars, secondScores, mappingQualities, lineOffsets, lineChars, nameOffsets, nameChars};
  for (size_t i = 0; i < sizeof all / sizeof *all; i++)
    if (all[i]) release(all[i]);
  if (onDevice) {
    void *copies[] = {b.chars, b.readOffsets, b.readSeedOffsets, b.starts, b.ends, b.seedEnds};
    for (size_t i = 0; i < sizeof copies / sizeof *copies; i++) release(copies[i]);
  }
}

int main(int argc, char **argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s records.fa reads.txt [step [minLength [cap [maxHitsPerSeed [band [minVotes [lookback [gapPenalty [bandPad [maxDrift [maxOps [match [mismatch [gapOpen [gapExtend]]]]]]]]]]]]]]]\n", argv[0]);
    return 1;
  }
  struct Params p = {.step = argc > 3 ? strtoull(argv[3], NULL, 10) : 4, .cap = argc > 5 ? strtoull(argv[5], NULL, 10) : 64,
                     .minLength = argc > 4 ? (uint32_t)strtoul(argv[4], NULL, 10) : 16,
                     .maxHitsPerSeed = argc > 6 ? (uint32_t)strtoul(argv[6], NULL, 10) : 16, .band = argc > 7 ? (uint32_t)strtoul(argv[7], NULL, 10) : 2,
                     .minVotes = argc > 8 ? (uint32_t)strtoul(argv[8], NULL, 10) : 2,
                     .lookback = argc > 9 ? (uint32_t)strtoul(argv[9], NULL, 10) : AWFM_CHAINS_MAX_LOOKBACK,
                     .gapPenalty = argc > 10 ? (uint32_t)strtoul(argv[10], NULL, 10) : 1, .bandPad = argc > 11 ? (uint32_t)strtoul(argv[11], NULL, 10) : 8,
                     .maxDrift = argc > 12 ? (uint32_t)strtoul(argv[12], NULL, 10) : 15, .maxOps = argc > 13 ? (uint32_t)strtoul(argv[13], NULL, 10) : 32,
                     .scoring = {.match = argc > 14 ? (uint32_t)strtoul(argv[14], NULL, 10) : 1, .mismatch = argc > 15 ? (uint32_t)strtoul(argv[15], NULL, 10) : 4,
                                 .gapOpen = argc > 16 ? (uint32_t)strtoul(argv[16], NULL, 10) : 6,
                                 .gapExtend = argc > 17 ? (uint32_t)strtoul(argv[17], NULL, 10) : 1}};
  if (p.step == 0 || p.cap == 0 || p.maxOps == 0 || p.maxOps > AWFM_ALIGN_MAX_OPS) return 1;

  struct AwFmIndexConfiguration config = {.suffixArrayCompressionRatio = 8,
                                          .kmerLengthInSeedTable = 8,
                                          .alphabetType = AwFmAlphabetDna,
                                          .keepSuffixArrayInMemory = true,
                                          .storeOriginalSequence = false};
  struct AwFmIndex *index = NULL;
  enum AwFmReturnCode rc = awFmCreateIndexFromFasta(&index, &config, argv[1], "read_sam_lines.awfmi");
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

  /* the reads, concatenated, and where each begins */
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
  while (getline(&line, &lineCap, file) >= 0) {
    const size_t length = strcspn(line, "\r\n");
    if (length == 0) continue;
    if (in.numReads == readCap) in.readOffsets = realloc(in.readOffsets, ((readCap *= 2) + 1) * 8);
    while (in.numChars + length > charCap) in.chars = realloc(in.chars, charCap *= 2);
    memcpy(in.chars + in.numChars, line, length);
    in.numChars += length;
    in.readOffsets[++in.numReads] = in.numChars;
    in.numWindows += length / p.step;
  }
  free(line);
  fclose(file);
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
                   host.cigarOffsets[r + 1] != device.cigarOffsets[r + 1] || host.mdOffsets[r + 1] != device.mdOffsets[r + 1];
    if (!different) /* the offsets agree: the arenas are compared byte for byte */
      different += memcmp(host.cigarChars, device.cigarChars, host.cigarOffsets[in.numReads]) != 0 ||
                   memcmp(host.mdChars, device.mdChars, host.mdOffsets[in.numReads]) != 0 || host.numSkipped != device.numSkipped ||
                   host.numOverflow != device.numOverflow;
    /* the records: offsets, counters, and the arena byte for byte */
    different += memcmp(host.lineOffsets, device.lineOffsets, (in.numReads + 1) * 8) != 0 || host.samUnaligned != device.samUnaligned ||
                 host.samOverflow != device.samOverflow;
    if (!different) different += memcmp(host.lineChars, device.lineChars, host.lineOffsets[in.numReads]) != 0;
    fprintf(stderr, "device and host twins: %" PRIu64 " reads differ\n", different);
    if (different) return 4;
  }

  /* the header lines and the arena, as they are, with one fwrite */
  const uint64_t headerBytes = awfmSamHeader(index, NULL, 0), lineBytes = shown->lineOffsets[in.numReads];
  uint8_t *sam = malloc(headerBytes + lineBytes + 1);
  awfmSamHeader(index, sam, headerBytes);
  memcpy(sam + headerBytes, shown->lineChars, lineBytes);
  if (fwrite(sam, 1, headerBytes + lineBytes, stdout) != headerBytes + lineBytes) return 4;
  free(sam);
  const uint64_t numAligned = in.numReads - shown->samUnaligned;
  fprintf(stderr, "reads %" PRIu64 " windows %" PRIu64 " aligned %" PRIu64 " unaligned %" PRIu64 " truncated %" PRIu64 " skipped %" PRIu64
                  " overflow %" PRIu64 " bytes %" PRIu64 " on the %s\n", in.numReads, in.numWindows, numAligned, shown->samUnaligned, shown->numTruncated,
          shown->numSkipped, shown->numOverflow + shown->samOverflow, headerBytes + lineBytes, haveDevice ? "device" : "host");

  awFmDeallocIndex(index);
  remove("read_sam_lines.awfmi");
  return 0;
}
