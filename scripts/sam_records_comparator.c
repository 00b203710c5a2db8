/*
 * sam_records_comparator.c -- what a caller did for a SAM line before awfmSamRecords existed, as a shared object that
 * scripts/sam_records_timing.py compiles and times: the loop at the end of examples/read_sam.c -- one read at a time, the
 * record's header looked up per read, FLAG 0 or 4, MAPQ 255, no mates, the line made by snprintf --, spread over `threads`
 * threads, each over a contiguous share of the reads and into its own part of `out` (`stride` bytes a read).  It uses nothing of
 * the library.  lookup(user, s, &header, &length) is the per-read header lookup: the timing script's index is built from a
 * synthetic text and has no FASTA trailer, so the script passes samComparatorTableLookup over a table of names, which does what
 * awFmGetHeaderStringFromSequenceNumber does (a bounds check, two table reads, a pointer and a length).
 *
 *   cc -std=gnu11 -O2 -fPIC -shared -pthread scripts/sam_records_comparator.c -o sam_records_comparator.so
 */
#include <inttypes.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

typedef int (*HeaderLookup)(const void *user, size_t sequenceNumber, const char **header, size_t *length);

struct SamComparatorInputs {
  const uint8_t *readChars;
  const uint64_t *readOffsets;
  const uint32_t *sequences, *slots, *scores, *editDistances;
  const uint64_t *textBegins, *cigarOffsets;
  const uint8_t *cigarChars;
  const uint64_t *mdOffsets;
  const uint8_t *mdChars;
  uint64_t numReads;
  uint32_t maxCandidates;
  HeaderLookup lookup;
  const void *lookupUser;
  char *out;          /* numReads * stride bytes */
  uint64_t stride;    /* room per read */
  uint64_t *written;  /* [threads]: the bytes of thread t, which begin at out + (its first read) * stride */
  uint64_t *firstRead; /* [threads] */
};

struct NameTable {
  const uint64_t *offsets;
  const char *chars;
  uint64_t numRecords;
};

int samComparatorTableLookup(const void *user, size_t sequenceNumber, const char **header, size_t *length) {
  const struct NameTable *table = user;
  if (sequenceNumber >= table->numRecords) return 0;
  *header = table->chars + table->offsets[sequenceNumber];
  *length = table->offsets[sequenceNumber + 1] - table->offsets[sequenceNumber];
  return 1;
}

struct Share {
  const struct SamComparatorInputs *in;
  uint64_t begin, end, written;
  int failed;
};

#define PUT(...)                                                      \
  do {                                                                \
    const int k = snprintf(at, (size_t)(limit - at), __VA_ARGS__);    \
    if (k < 0 || k >= limit - at) {                                   \
      share->failed = 1;                                              \
      return NULL;                                                    \
    }                                                                 \
    at += k;                                                          \
  } while (0)

static void *samComparatorShare(void *p) {
  struct Share *share = p;
  const struct SamComparatorInputs *in = share->in;
  char *const first = in->out + share->begin * in->stride, *at = first, *const limit = in->out + share->end * in->stride;
  for (uint64_t r = share->begin; r < share->end; r++) {
    const uint8_t *read = in->readChars + in->readOffsets[r];
    const int readLength = (int)(in->readOffsets[r + 1] - in->readOffsets[r]);
    if (in->scores[r] == 0 || in->scores[r] >= 0xFFFFFFFCu) {
      PUT("%" PRIu64 "\t4\t*\t0\t0\t*\t*\t0\t0\t%.*s\t*\n", r, readLength, (const char *)read);
      continue;
    }
    const char *header = NULL;
    size_t headerLength = 0;
    if (!in->lookup(in->lookupUser, in->sequences[r * in->maxCandidates + in->slots[r]], &header, &headerLength)) {
      share->failed = 1;
      return NULL;
    }
    const uint64_t cigarLength = in->cigarOffsets[r + 1] - in->cigarOffsets[r], mdLength = in->mdOffsets[r + 1] - in->mdOffsets[r];
    PUT("%" PRIu64 "\t0\t%.*s\t%" PRIu64 "\t255\t", r, (int)headerLength, header, in->textBegins[r] + 1);
    if (cigarLength) PUT("%.*s", (int)cigarLength, (const char *)in->cigarChars + in->cigarOffsets[r]);
    else PUT("*");
    PUT("\t*\t0\t0\t%.*s\t*\tNM:i:%" PRIu32 "\tAS:i:%" PRIu32, readLength, (const char *)read, in->editDistances[r], in->scores[r]);
    if (mdLength) PUT("\tMD:Z:%.*s", (int)mdLength, (const char *)in->mdChars + in->mdOffsets[r]);
    PUT("\n");
  }
  share->written = (uint64_t)(at - first);
  return NULL;
}

/* 1: every line was written; 0: a lookup failed or a share's room ran out */
int samComparator(const struct SamComparatorInputs *in, unsigned threads) {
  if (threads == 0 || threads > 64) return 0;
  pthread_t ids[64];
  struct Share shares[64];
  for (unsigned t = 0; t < threads; t++) {
    shares[t] = (struct Share){in, in->numReads * t / threads, in->numReads * (t + 1) / threads, 0, 0};
    if (pthread_create(&ids[t], NULL, samComparatorShare, &shares[t]) != 0) return 0;
  }
  int ok = 1;
  for (unsigned t = 0; t < threads; t++) {
    pthread_join(ids[t], NULL);
    ok = ok && !shares[t].failed;
    in->written[t] = shares[t].written;
    in->firstRead[t] = shares[t].begin;
  }
  return ok;
}
