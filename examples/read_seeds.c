/*
 * read_seeds.c -- variable-length seeds of reads, against the two public headers only: a FASTA file -> index
 * (awFmCreateIndexFromFasta) -> for every read the longest match that ends at every s-th position, at most `cap` characters
 * long (awfmGpuLongestSuffixMatches over overlapping (start, end) windows into the read buffer, matches shorter than minLength
 * dropped) -> located (awfmGpuHitOffsetsFromCounts, awfmGpuLocate) -> mapped to sequence coordinates on the device
 * (awfmGpuLocalPositions) -> one line `read:end:length:header:offset` per occurrence, windows in order, the occurrences of a
 * window in BWT order.  An occurrence that starts on a record's terminator prints `*` for the header and its global position.
 *
 *   cc -std=gnu11 -O2 examples/read_seeds.c -Iinclude -Lavxwindowfmindex_amd -lawfmindex_amd \
 *      -Wl,-rpath,$PWD/avxwindowfmindex_amd -o read_seeds && ./read_seeds genome.fa reads.txt [step [minLength [cap]]]
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
    fprintf(stderr, "usage: %s records.fa reads.txt [step [minLength [cap]]]\n", argv[0]);
    return 1;
  }
  const uint64_t step = argc > 3 ? strtoull(argv[3], NULL, 10) : 4, cap = argc > 5 ? strtoull(argv[5], NULL, 10) : 64;
  const uint32_t minLength = argc > 4 ? (uint32_t)strtoul(argv[4], NULL, 10) : 16;
  if (step == 0 || cap == 0) return 1;

  struct AwFmIndexConfiguration config = {.suffixArrayCompressionRatio = 8,
                                          .kmerLengthInSeedTable = 8,
                                          .alphabetType = AwFmAlphabetDna,
                                          .keepSuffixArrayInMemory = true,
                                          .storeOriginalSequence = false};
  struct AwFmIndex *index = NULL;
  enum AwFmReturnCode rc = awFmCreateIndexFromFasta(&index, &config, argv[1], "read_seeds.awfmi");
  if (awFmReturnCodeIsFailure(rc)) {
    fprintf(stderr, "awFmCreateIndexFromFasta failed: %d\n", rc);
    return 2;
  }
  AwFmGpuIndex *image = awfmGpuIndexAcquire(index); /* carries the record table of the FASTA file */
  if (!image) {
    fprintf(stderr, "no device image: %s\n", awfmGpuLastError());
    return 3;
  }

  /* the reads, concatenated, and where each begins */
  FILE *in = fopen(argv[2], "r");
  if (!in) {
    fprintf(stderr, "cannot read %s\n", argv[2]);
    return 1;
  }
  size_t numReads = 0, readCap = 1024, charCap = 1 << 16, numChars = 0, numWindows = 0;
  char *text = malloc(charCap);
  uint64_t *readAt = malloc((readCap + 1) * sizeof *readAt);
  char *line = NULL; /* (getline: a read of any length is one read) */
  size_t lineCap = 0;
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
  uint32_t *readOf = malloc((numWindows ? numWindows : 1) * sizeof *readOf);
  memcpy(chars, text, numChars);
  size_t w = 0;
  for (size_t r = 0; r < numReads; r++)
    for (uint64_t e = step; e <= readAt[r + 1] - readAt[r]; e += step, w++) {
      starts[w] = readAt[r] + (e > cap ? e - cap : 0);
      ends[w] = readAt[r] + e;
      readOf[w] = (uint32_t)r;
    }

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
  uint64_t *positions = pinned(totalHits * 8), *waitOffsets = pinned(16), waited = 0, numIllegal = 0;
  uint32_t *sequenceNumbers = pinned(totalHits * 4), *one = pinned(4);
  *one = 1;
  if (totalHits != 0) {
    rc = awfmGpuLocate(image, ranges, hitOffsets, numWindows, totalHits, positions, NULL);
    if (!awFmReturnCodeIsFailure(rc))
      rc = awfmGpuLocalPositions(image, positions, totalHits, NULL, sequenceNumbers, positions /* in place */, NULL, NULL);
    /* both are asynchronous.  A program with a stream of its own waits for it with its runtime (hipStreamSynchronize); this one
     * has only the two headers, in which the scan that returns its total to the host is the call that waits for the stream */
    if (!awFmReturnCodeIsFailure(rc)) rc = awfmGpuHitOffsetsFromCounts(image, one, 1, waitOffsets, scratch, &waited, NULL);
    if (awFmReturnCodeIsFailure(rc)) {
      fprintf(stderr, "locate failed: %d: %s\n", rc, awfmGpuLastError());
      return 3;
    }
  }

  for (w = 0; w < numWindows; w++)
    for (uint64_t h = hitOffsets[w]; h < hitOffsets[w + 1]; h++) {
      const uint64_t end = ends[w] - readAt[readOf[w]];
      if (sequenceNumbers[h] == 0xFFFFFFFFu) {
        numIllegal++;
        printf("%" PRIu32 ":%" PRIu64 ":%" PRIu32 ":*:%" PRIu64 "\n", readOf[w], end, lengths[w], positions[h]);
        continue;
      }
      char *header = NULL;
      size_t headerLength = 0;
      if (awFmGetHeaderStringFromSequenceNumber(index, sequenceNumbers[h], &header, &headerLength) != AwFmSuccess) return 4;
      printf("%" PRIu32 ":%" PRIu64 ":%" PRIu32 ":%.*s:%" PRIu64 "\n", readOf[w], end, lengths[w], (int)headerLength, header, positions[h]);
    }
  fprintf(stderr, "reads %zu windows %zu occurrences %" PRIu64 " illegal %" PRIu64 "\n", numReads, numWindows, totalHits, numIllegal);

  void *all[] = {chars, starts, ends, lengths, counts, ranges, hitOffsets, scratch, positions, waitOffsets, sequenceNumbers, one};
  for (size_t i = 0; i < sizeof all / sizeof *all; i++) awfmGpuHostFree(all[i]);
  free(readOf);
  free(readAt);
  free(text);
  awFmDeallocIndex(index);
  remove("read_seeds.awfmi");
  return 0;
}
