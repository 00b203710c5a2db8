/*
 * kmer_neighbours.c -- where the strings at Hamming distance at most 1 of a list of k-mers occur, against the two public headers
 * only: a FASTA file -> index (awFmCreateIndexFromFasta) -> awfmGpuOneSubstitutionSearch over the k-mers (once for the number of
 * records, once for the records) -> located (awfmGpuHitOffsets, awfmGpuLocate: the record list goes in as if it were a batch)
 * -> mapped to sequence coordinates on the device (awfmGpuLocalPositions) -> one line `kmer:edit:header:offset` per occurrence.
 * kmer: the k-mer's number in the list; edit: `=` for the k-mer as it is, otherwise the position and the letter that replaces
 * the one there (`7g`).  Records in the order of (k-mer, edit) -- the device appends them in whatever order its waves come, the
 * program sorts an index over them --, the occurrences of a record in BWT order.  An occurrence that starts on a record's
 * terminator prints `*` for the header and its global position.
 *
 *   cc -std=gnu11 -O2 examples/kmer_neighbours.c -Iinclude -Lavxwindowfmindex_amd -lawfmindex_amd \
 *      -Wl,-rpath,$PWD/avxwindowfmindex_amd -o kmer_neighbours && ./kmer_neighbours genome.fa kmers.txt
 *
 * kmers.txt: one k-mer per line, of any lengths.  The buffers are page-locked host memory (awfmGpuHostAlloc), which the device
 * reads and writes in place: a program that keeps its k-mers on the device passes its own device pointers instead.
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

static const uint32_t *sortQueries, *sortEdits;
static int byQueryThenEdit(const void *a, const void *b) {
  const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
  if (sortQueries[x] != sortQueries[y]) return sortQueries[x] < sortQueries[y] ? -1 : 1;
  return sortEdits[x] < sortEdits[y] ? -1 : (sortEdits[x] > sortEdits[y] ? 1 : 0);
}

int main(int argc, char **argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s records.fa kmers.txt\n", argv[0]);
    return 1;
  }
  struct AwFmIndexConfiguration config = {.suffixArrayCompressionRatio = 8,
                                          .kmerLengthInSeedTable = 8,
                                          .alphabetType = AwFmAlphabetDna,
                                          .keepSuffixArrayInMemory = true,
                                          .storeOriginalSequence = false};
  struct AwFmIndex *index = NULL;
  enum AwFmReturnCode rc = awFmCreateIndexFromFasta(&index, &config, argv[1], "kmer_neighbours.awfmi");
  if (awFmReturnCodeIsFailure(rc)) {
    fprintf(stderr, "awFmCreateIndexFromFasta failed: %d\n", rc);
    return 2;
  }
  AwFmGpuIndex *image = awfmGpuIndexAcquire(index); /* carries the record table of the FASTA file */
  if (!image) {
    fprintf(stderr, "no device image: %s\n", awfmGpuLastError());
    return 3;
  }

  /* the k-mers, concatenated, and where each begins */
  FILE *in = fopen(argv[2], "r");
  if (!in) {
    fprintf(stderr, "cannot read %s\n", argv[2]);
    return 1;
  }
  size_t numKmers = 0, kmerCap = 1024, charCap = 1 << 16, numChars = 0;
  char *text = malloc(charCap);
  uint64_t *kmerAt = malloc((kmerCap + 1) * sizeof *kmerAt);
  char *line = NULL;
  size_t lineCap = 0;
  kmerAt[0] = 0;
  while (getline(&line, &lineCap, in) >= 0) {
    const size_t length = strcspn(line, "\r\n");
    if (length == 0) continue;
    if (numKmers == kmerCap) kmerAt = realloc(kmerAt, ((kmerCap *= 2) + 1) * sizeof *kmerAt);
    while (numChars + length > charCap) text = realloc(text, charCap *= 2);
    memcpy(text + numChars, line, length);
    numChars += length;
    kmerAt[++numKmers] = numChars;
  }
  free(line);
  fclose(in);

  uint8_t *chars = pinned(numChars);
  uint64_t *offsets = pinned((numKmers + 1) * 8);
  memcpy(chars, text, numChars);
  memcpy(offsets, kmerAt, (numKmers + 1) * 8);

  /* the calls are asynchronous.  A program with a stream of its own waits for it with its runtime (hipStreamSynchronize); this one
   * has only the two headers, in which a scan that returns its total to the host is the call that waits for the stream */
  uint64_t *numRecords = pinned(8), *waitOffsets = pinned(16), waited = 0, totalHits = 0, numIllegal = 0;
  uint32_t *one = pinned(4);
  void *waitScratch = pinned(awfmGpuScanScratchBytes(1));
  *numRecords = 0;
  *one = 1;
  if (numKmers != 0) { /* how many records: the lists' capacity */
    rc = awfmGpuOneSubstitutionSearch(image, chars, offsets, 0, numKmers, 1, NULL, NULL, NULL, 0, numRecords, NULL, NULL, NULL);
    if (!awFmReturnCodeIsFailure(rc)) rc = awfmGpuHitOffsetsFromCounts(image, one, 1, waitOffsets, waitScratch, &waited, NULL);
    if (awFmReturnCodeIsFailure(rc)) {
      fprintf(stderr, "search failed: %d: %s\n", rc, awfmGpuLastError());
      return 3;
    }
  }
  const uint64_t capacity = *numRecords;
  uint32_t *hitKmers = pinned(capacity * 4), *hitEdits = pinned(capacity * 4);
  struct AwFmSearchRange *hitRanges = pinned(capacity * sizeof *hitRanges);
  uint64_t *hitOffsets = pinned((capacity + 1) * 8);
  void *scratch = pinned(awfmGpuScanScratchBytes(capacity ? capacity : 1));
  hitOffsets[capacity] = 0;
  if (capacity != 0) {
    rc = awfmGpuOneSubstitutionSearch(image, chars, offsets, 0, numKmers, 1, hitKmers, hitEdits, hitRanges, capacity, numRecords, NULL,
                                      NULL, NULL);
    if (!awFmReturnCodeIsFailure(rc)) rc = awfmGpuHitOffsets(image, hitRanges, capacity, hitOffsets, scratch, &totalHits, NULL);
    if (awFmReturnCodeIsFailure(rc)) {
      fprintf(stderr, "search failed: %d: %s\n", rc, awfmGpuLastError());
      return 3;
    }
  }
  uint64_t *positions = pinned(totalHits * 8);
  uint32_t *sequenceNumbers = pinned(totalHits * 4);
  if (totalHits != 0) {
    rc = awfmGpuLocate(image, hitRanges, hitOffsets, capacity, totalHits, positions, NULL);
    if (!awFmReturnCodeIsFailure(rc))
      rc = awfmGpuLocalPositions(image, positions, totalHits, NULL, sequenceNumbers, positions /* in place */, NULL, NULL);
    if (!awFmReturnCodeIsFailure(rc)) rc = awfmGpuHitOffsetsFromCounts(image, one, 1, waitOffsets, waitScratch, &waited, NULL);
    if (awFmReturnCodeIsFailure(rc)) {
      fprintf(stderr, "locate failed: %d: %s\n", rc, awfmGpuLastError());
      return 3;
    }
  }

  uint64_t *order = malloc((capacity ? capacity : 1) * sizeof *order);
  for (uint64_t i = 0; i < capacity; i++) order[i] = i;
  sortQueries = hitKmers;
  sortEdits = hitEdits;
  qsort(order, capacity, sizeof *order, byQueryThenEdit);
  for (uint64_t i = 0; i < capacity; i++) {
    const uint64_t r = order[i];
    char edit[16] = "=";
    /* (a nucleotide index: the letter index in the edit's low five bits is 0..3, a c g t) */
    if (hitEdits[r] != AWFM_EDIT_NONE) snprintf(edit, sizeof edit, "%" PRIu32 "%c", hitEdits[r] >> 5, "acgt"[hitEdits[r] & 3u]);
    for (uint64_t h = hitOffsets[r]; h < hitOffsets[r + 1]; h++) {
      if (sequenceNumbers[h] == 0xFFFFFFFFu) {
        numIllegal++;
        printf("%" PRIu32 ":%s:*:%" PRIu64 "\n", hitKmers[r], edit, positions[h]);
        continue;
      }
      char *header = NULL;
      size_t headerLength = 0;
      if (awFmGetHeaderStringFromSequenceNumber(index, sequenceNumbers[h], &header, &headerLength) != AwFmSuccess) return 4;
      printf("%" PRIu32 ":%s:%.*s:%" PRIu64 "\n", hitKmers[r], edit, (int)headerLength, header, positions[h]);
    }
  }
  fprintf(stderr, "kmers %zu records %" PRIu64 " occurrences %" PRIu64 " illegal %" PRIu64 "\n", numKmers, capacity, totalHits, numIllegal);

  void *all[] = {chars, offsets, numRecords, waitOffsets, one, waitScratch, hitKmers, hitEdits, hitRanges, hitOffsets, scratch, positions,
                 sequenceNumbers};
  for (size_t i = 0; i < sizeof all / sizeof *all; i++) awfmGpuHostFree(all[i]);
  free(order);
  free(kmerAt);
  free(text);
  awFmDeallocIndex(index);
  remove("kmer_neighbours.awfmi");
  return 0;
}
