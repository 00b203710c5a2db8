/*
 * awfm_matrix.c -- the two makers of a struct AwFmMatrixScoring (include/awfm_gpu.h, "substitution matrices"):
 * awfmMatrixScoringUniform, the matrix that scores as a struct AwFmAlignScoring does, and awfmMatrixScoringFromText, the parser of
 * the usual matrix text format from memory.  Neither does I/O, allocates or keeps anything.  The calls that score with a matrix
 * sit beside their affine siblings (awfm_score_affine.c, awfm_align_affine.c) and share their rows (awfm_band.h).  The reference
 * has no analogue (it stops at positions: ref src/AwFmParallelSearch.c:315-365).
 */
#include <string.h>

#include "awfm_band.h"

enum { AWFM_MATRIX_MAX_COLUMNS = 64, AWFM_MATRIX_SKIP = 255 };

static int awfmAlphabetOk(enum AwFmAlphabetType alphabet) {
  return alphabet == AwFmAlphabetAmino || alphabet == AwFmAlphabetDna || alphabet == AwFmAlphabetRna;
}

enum AwFmReturnCode awfmMatrixScoringUniform(enum AwFmAlphabetType alphabet, const struct AwFmAlignScoring *scoring,
                                             struct AwFmMatrixScoring *out) {
  if (!scoring || !out) return AwFmNullPtrError;
  if (!awfmAlphabetOk(alphabet) || !awfmScoringOk(scoring) || scoring->match > 127 || scoring->mismatch > 128) return AwFmIllegalPositionError;
  const uint32_t proper = alphabet == AwFmAlphabetAmino ? 20u : 4u;
  for (uint32_t a = 0; a < AWFM_MATRIX_CLASSES; a++)
    for (uint32_t b = 0; b < AWFM_MATRIX_CLASSES; b++)
      out->substitution[a * AWFM_MATRIX_CLASSES + b] = (int8_t)(a == b && a < proper ? (int32_t)scoring->match : -(int32_t)scoring->mismatch);
  out->gapOpen = scoring->gapOpen;
  out->gapExtend = scoring->gapExtend;
  return AwFmSuccess;
}

static int awfmIsBlank(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f'; }

/* the class a row or column letter stands for: 0 .. proper - 1, `proper` for X (amino) or N (nucleotide), AWFM_MATRIX_SKIP for
 * every other single character; -1: not a single character */
static int awfmMatrixLetterClass(int amino, const char *token, uint64_t length) {
  if (length != 1) return -1;
  const uint8_t c = (uint8_t)token[0], l = c | 0x20;
  if (l < 'a' || l > 'z') return AWFM_MATRIX_SKIP;
  const uint32_t proper = amino ? 20u : 4u, x = amino ? awfmAminoAsciiToIndex(c) : awfmNucAsciiToIndex(c);
  if (x < proper) return (int)x;
  return l == (amino ? 'x' : 'n') ? (int)proper : AWFM_MATRIX_SKIP;
}

/* the next token of [*at, end): 0 when the line holds no more */
static int awfmMatrixToken(const char **at, const char *end, const char **token, uint64_t *length) {
  const char *p = *at;
  while (p < end && awfmIsBlank(*p)) p++;
  *token = p;
  while (p < end && !awfmIsBlank(*p)) p++;
  *length = (uint64_t)(p - *token);
  *at = p;
  return *length != 0;
}

/* a decimal integer with an optional sign; 0: the token is none.  Values beyond +-1000 stay beyond it */
static int awfmMatrixInteger(const char *token, uint64_t length, int32_t *value) {
  uint64_t q = 0;
  int negative = 0;
  if (token[0] == '-' || token[0] == '+') {
    negative = token[0] == '-';
    q = 1;
  }
  if (q == length) return 0;
  int32_t v = 0;
  for (; q < length; q++) {
    if (token[q] < '0' || token[q] > '9') return 0;
    v = v * 10 + (token[q] - '0');
    if (v > 1000) v = 1000;
  }
  *value = negative ? -v : v;
  return 1;
}

enum AwFmReturnCode awfmMatrixScoringFromText(enum AwFmAlphabetType alphabet, const char *text, uint64_t bytes, uint32_t gapOpen,
                                              uint32_t gapExtend, struct AwFmMatrixScoring *out) {
  if (!out || (!text && bytes != 0)) return AwFmNullPtrError;
  if (!awfmAlphabetOk(alphabet) || gapOpen > 255 || gapExtend < 1 || gapExtend > 255) return AwFmIllegalPositionError;
  if (bytes == 0) return AwFmFileFormatError;
  const int amino = alphabet == AwFmAlphabetAmino;
  const uint32_t proper = amino ? 20u : 4u, classes = proper + 1u;
  struct AwFmMatrixScoring result;
  uint8_t given[AWFM_MATRIX_CLASSES * AWFM_MATRIX_CLASSES], columns[AWFM_MATRIX_MAX_COLUMNS];
  uint32_t numColumns = 0, columnSeen = 0, rowSeen = 0;
  int haveColumns = 0;
  memset(&result, 0, sizeof result);
  memset(given, 0, sizeof given);
  const char *line = text, *const end = text + bytes;
  while (line < end) {
    const char *lineEnd = memchr(line, '\n', (size_t)(end - line));
    if (!lineEnd) lineEnd = end;
    const char *at = line, *token;
    uint64_t length;
    line = lineEnd < end ? lineEnd + 1 : end;
    if (!awfmMatrixToken(&at, lineEnd, &token, &length) || token[0] == '#') continue;
    if (!haveColumns) { /* the column letters */
      do {
        const int c = awfmMatrixLetterClass(amino, token, length);
        if (c < 0 || numColumns == AWFM_MATRIX_MAX_COLUMNS) return AwFmFileFormatError;
        if (c != AWFM_MATRIX_SKIP) {
          if (columnSeen >> c & 1u) return AwFmFileFormatError; /* repeated */
          columnSeen |= 1u << c;
        }
        columns[numColumns++] = (uint8_t)c;
      } while (awfmMatrixToken(&at, lineEnd, &token, &length));
      haveColumns = 1;
      continue;
    }
    const int r = awfmMatrixLetterClass(amino, token, length);
    if (r < 0) return AwFmFileFormatError;
    if (r != AWFM_MATRIX_SKIP) {
      if (rowSeen >> r & 1u) return AwFmFileFormatError; /* repeated */
      rowSeen |= 1u << r;
    }
    uint32_t numValues = 0;
    while (awfmMatrixToken(&at, lineEnd, &token, &length)) {
      int32_t value;
      if (numValues == numColumns || !awfmMatrixInteger(token, length, &value)) return AwFmFileFormatError;
      if (value < -128 || value > 127) return AwFmIllegalPositionError;
      const uint32_t c = columns[numValues++];
      if (r == AWFM_MATRIX_SKIP || c == AWFM_MATRIX_SKIP) continue;
      result.substitution[(uint32_t)r * AWFM_MATRIX_CLASSES + c] = (int8_t)value;
      given[(uint32_t)r * AWFM_MATRIX_CLASSES + c] = 1;
    }
    if (numValues != numColumns) return AwFmFileFormatError; /* a short row, also the one the text ends in */
  }
  const uint32_t all = (1u << proper) - 1u;
  if ((columnSeen & all) != all || (rowSeen & all) != all) return AwFmFileFormatError; /* a proper letter is missing */
  int32_t smallest = 127;
  for (uint32_t a = 0; a < proper; a++)
    for (uint32_t b = 0; b < proper; b++)
      if (result.substitution[a * AWFM_MATRIX_CLASSES + b] < smallest) smallest = result.substitution[a * AWFM_MATRIX_CLASSES + b];
  /* what the text does not give of the last class's row and column */
  for (uint32_t a = 0; a < classes; a++)
    for (uint32_t b = 0; b < classes; b++)
      if (!given[a * AWFM_MATRIX_CLASSES + b]) result.substitution[a * AWFM_MATRIX_CLASSES + b] = (int8_t)smallest;
  result.gapOpen = gapOpen;
  result.gapExtend = gapExtend;
  *out = result;
  return AwFmSuccess;
}
