/* Stand-in for the FastaVector header the reference's sources include: exactly the names those sources use, declared
 * from how they use them (struct members read and written in AwFmFile.c / AwFmCreate.c / AwFmIndexStruct.c, the calls
 * in AwFmSearch.c).  TEST INFRASTRUCTURE ONLY: it lets oracle/Makefile compile the reference's src directory into
 * _ref/libawfm_ref.so.  FASTA reading, headers and local positions are not implemented behind it (ref_shim.c): the
 * reference has no code of its own for them, so there is nothing of the reference to check there. */
#ifndef AWFM_REF_SHIM_FASTA_VECTOR_H
#define AWFM_REF_SHIM_FASTA_VECTOR_H
#include <stdbool.h>
#include <stddef.h>

enum FastaVectorReturnCode { FASTA_VECTOR_OK = 0, FASTA_VECTOR_FILE_OPEN_FAIL = 1, FASTA_VECTOR_ALLOCATION_FAIL = 2 };

struct FastaVectorString {
  char *charData;
  size_t capacity;
  size_t count;
};

struct FastaVectorMetadata {
  size_t headerEndPosition;
  size_t sequenceEndPosition;
};

struct FastaVectorMetadataVector {
  struct FastaVectorMetadata *data;
  size_t capacity;
  size_t count;
};

struct FastaVector {
  struct FastaVectorString sequence;
  struct FastaVectorString header;
  struct FastaVectorMetadataVector metadata;
};

struct FastaVectorLocalPosition {
  size_t sequenceIndex;
  size_t positionInSequence;
};

enum FastaVectorReturnCode fastaVectorInit(struct FastaVector *fastaVector);
enum FastaVectorReturnCode fastaVectorReadFasta(const char *fileSrc, struct FastaVector *fastaVector);
void fastaVectorDealloc(struct FastaVector *fastaVector);
void fastaVectorStringDealloc(struct FastaVectorString *string);
bool fastaVectorGetLocalSequencePositionFromGlobal(const struct FastaVector *fastaVector, size_t globalPosition,
                                                   struct FastaVectorLocalPosition *localPosition);
void fastaVectorGetHeader(const struct FastaVector *fastaVector, size_t sequenceNumber, char **headerBuffer,
                          size_t *headerLength);

#endif
