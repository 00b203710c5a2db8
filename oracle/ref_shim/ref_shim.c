/* The functions FastaVector.h and divsufsort64.h of this directory declare.  TEST INFRASTRUCTURE ONLY. */
#include <stdlib.h>
#include <string.h>
#include "FastaVector.h"
#include "divsufsort64.h"

/* avxwindowfmindex_amd/csrc/awfm_suffix_sort.c, compiled into the same library */
int awfmSuffixSort(const uint8_t *s, uint64_t n, uint64_t *sa);

int64_t divsufsort64(const uint8_t *text, int64_t *suffixArray, int64_t length) {
  if (!text || !suffixArray || length < 0) return -1;
  return awfmSuffixSort(text, (uint64_t)length, (uint64_t *)suffixArray) == 0 ? 0 : -2;
}

enum FastaVectorReturnCode fastaVectorInit(struct FastaVector *fastaVector) {
  memset(fastaVector, 0, sizeof *fastaVector);
  return FASTA_VECTOR_OK;
}

/* FASTA input is out of scope: every file "fails to open" */
enum FastaVectorReturnCode fastaVectorReadFasta(const char *fileSrc, struct FastaVector *fastaVector) {
  (void)fileSrc;
  (void)fastaVector;
  return FASTA_VECTOR_FILE_OPEN_FAIL;
}

void fastaVectorStringDealloc(struct FastaVectorString *string) {
  free(string->charData);
  string->charData = NULL;
  string->capacity = string->count = 0;
}

void fastaVectorDealloc(struct FastaVector *fastaVector) {
  fastaVectorStringDealloc(&fastaVector->sequence);
  fastaVectorStringDealloc(&fastaVector->header);
  free(fastaVector->metadata.data);
  memset(&fastaVector->metadata, 0, sizeof fastaVector->metadata);
}

bool fastaVectorGetLocalSequencePositionFromGlobal(const struct FastaVector *fastaVector, size_t globalPosition,
                                                   struct FastaVectorLocalPosition *localPosition) {
  (void)fastaVector;
  (void)globalPosition;
  (void)localPosition;
  return false;
}

void fastaVectorGetHeader(const struct FastaVector *fastaVector, size_t sequenceNumber, char **headerBuffer,
                          size_t *headerLength) {
  (void)fastaVector;
  (void)sequenceNumber;
  *headerBuffer = NULL;
  *headerLength = 0;
}
