/*
 * kmer_locate_fasta.c -- sequence coordinates end to end, against the two public headers only: a multi-record FASTA file ->
 * index (awFmCreateIndexFromFasta) -> locate a batch of k-mers with the hits mapped to (record, offset) on the device
 * (awfmGpuLocateHostLocal) -> one line `kmer <tab> header:offset` per hit, in batch order, the hits of a k-mer in BWT order.
 * A hit on a record's terminator (only a k-mer of ambiguity letters has those) prints as `kmer <tab> *:global position`.
 *
 *   cc -std=gnu11 -O2 examples/kmer_locate_fasta.c -Iinclude -Lavxwindowfmindex_amd -lawfmindex_amd \
 *      -Wl,-rpath,$PWD/avxwindowfmindex_amd -o kmer_locate_fasta && ./kmer_locate_fasta genome.fa kmers.txt [dna|amino]
 *
 * kmers.txt: one k-mer per line (any lengths).
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "AwFmIndex.h"
#include "awfm_gpu.h"

int main(int argc, char **argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s records.fa kmers.txt [dna|amino]\n", argv[0]);
    return 1;
  }
  const int amino = argc > 3 && strcmp(argv[3], "amino") == 0;

  /* the batch, flat: characters and CSR offsets */
  FILE *in = fopen(argv[2], "r");
  if (!in) {
    fprintf(stderr, "cannot read %s\n", argv[2]);
    return 1;
  }
  size_t numKmers = 0, kmerCap = 1024, charCap = 1 << 16;
  uint8_t *chars = malloc(charCap);
  uint64_t *offsets = malloc((kmerCap + 1) * sizeof *offsets);
  char line[4096];
  offsets[0] = 0;
  while (fgets(line, sizeof line, in)) {
    size_t length = strcspn(line, "\r\n");
    if (length == 0) continue;
    if (numKmers == kmerCap) offsets = realloc(offsets, ((kmerCap *= 2) + 1) * sizeof *offsets);
    while (offsets[numKmers] + length > charCap) chars = realloc(chars, charCap *= 2);
    memcpy(chars + offsets[numKmers], line, length);
    offsets[numKmers + 1] = offsets[numKmers] + length;
    numKmers++;
  }
  fclose(in);

  struct AwFmIndexConfiguration config = {.suffixArrayCompressionRatio = 8,
                                          .kmerLengthInSeedTable = amino ? 2 : 8,
                                          .alphabetType = amino ? AwFmAlphabetAmino : AwFmAlphabetDna,
                                          .keepSuffixArrayInMemory = true,
                                          .storeOriginalSequence = false};
  struct AwFmIndex *index = NULL;
  enum AwFmReturnCode rc = awFmCreateIndexFromFasta(&index, &config, argv[1], "kmer_locate_fasta.awfmi");
  if (awFmReturnCodeIsFailure(rc)) {
    fprintf(stderr, "awFmCreateIndexFromFasta failed: %d\n", rc);
    return 2;
  }

  /* the index's device image (the one awFmParallelSearch* use); it carries the record table of the FASTA file */
  AwFmGpuIndex *image = awfmGpuIndexAcquire(index);
  if (!image) {
    fprintf(stderr, "no device image: %s\n", awfmGpuLastError());
    return 3;
  }
  uint64_t *hitOffsets = malloc((numKmers + 1) * sizeof *hitOffsets), *localPositions = NULL, numIllegal = 0;
  uint32_t *sequenceNumbers = NULL;
  rc = awfmGpuLocateHostLocal(image, chars, offsets, 0, numKmers, NULL, hitOffsets, &sequenceNumbers, &localPositions, &numIllegal);
  if (awFmReturnCodeIsFailure(rc)) {
    fprintf(stderr, "awfmGpuLocateHostLocal failed: %d: %s\n", rc, awfmGpuLastError());
    return 3;
  }
  for (size_t i = 0; i < numKmers; i++)
    for (uint64_t h = hitOffsets[i]; h < hitOffsets[i + 1]; h++) {
      fwrite(chars + offsets[i], 1, (size_t)(offsets[i + 1] - offsets[i]), stdout);
      if (sequenceNumbers[h] == 0xFFFFFFFFu) { /* an illegal position keeps its place in the concatenated text */
        printf("\t*:%" PRIu64 "\n", localPositions[h]);
        continue;
      }
      char *header = NULL;
      size_t headerLength = 0;
      if (awFmGetHeaderStringFromSequenceNumber(index, sequenceNumbers[h], &header, &headerLength) != AwFmSuccess) return 4;
      printf("\t%.*s:%" PRIu64 "\n", (int)headerLength, header, localPositions[h]);
    }
  fprintf(stderr, "kmers %zu hits %" PRIu64 " illegal %" PRIu64 " records %" PRIu32 "\n", numKmers, hitOffsets[numKmers], numIllegal,
          awfmGpuIndexNumRecords(image));
  free(sequenceNumbers);
  free(localPositions);
  free(hitOffsets);
  free(offsets);
  free(chars);
  awFmDeallocIndex(index);
  remove("kmer_locate_fasta.awfmi");
  return 0;
}
