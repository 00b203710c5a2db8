/*
 * awfm_score_affine_kernel.h -- scoreChainsAffineKernel<G>, the kernel of "slot scores and mapping quality" (include/awfm_gpu.h):
 * the banded local affine score and end cell of every slot of every read, and per read the best slot, the runner-up and the
 * mapping quality.  The definition is the header's; the host twin and checker is awfm_score_affine.c.
 *
 * A wave takes a read (persistent grid over reads), its 64 / G groups of G lanes take the read's slots in turn, lane k of a
 * group is diagonal lo + k of the band in sequence-local coordinates, the rows go in chunks of kVerifyChunk.  The classification
 * of a slot, the band, the staging of a chunk's read and text characters into the group's words of LDS, the row and the end
 * cell are awfm_band_kernel.h's (classifySlot, readBand, stageChunk, affineRow, affineEndCell), the same calls as in
 * alignChainsAffineKernel -- EVERY LOAD OF TEXT OR READ is an aligned dword that holds a byte the slot owns, and the record is
 * checked against the text's length before anything is read; a slot with a status or without an existing cell loads no text.
 * Of the row this kernel keeps nothing but the call: no ballot, no store and no other shuffle per row.  The end cell -- largest
 * H, then smallest i, then smallest k -- is each lane's own best (strict-greater update) and one butterfly over the group.
 *
 * THE READ'S RULES.  Lane 0 of a group leaves the slot's value, readEnd, textEnd and sequence in the wave's kScoreSlotWords words
 * of LDS; behind a wave barrier lane j < C holds slot j, stores the three per-slot outputs (one coalesced store each) and
 * enters the keyed maxima over the wave's first sixteen lanes: score << 4 | 15 - slot among the slots that count gives the best
 * slot with ties to the lowest, the same among those that are neither the best nor its duplicate gives the second.  Lane 0
 * stores the per-read outputs.  Counters take one atomic per wave.  Vector loads and stores only.
 */
#ifndef AWFM_SCORE_AFFINE_KERNEL_H
#define AWFM_SCORE_AFFINE_KERNEL_H

#include "awfm_band_kernel.h"

namespace {

constexpr unsigned kScoreThreads = 256;    /* per workgroup: four waves, each with reads of its own */
constexpr unsigned kScoreSlotWords = 80;   /* per wave: value, readEnd, the two halves of textEnd and the sequence of sixteen slots */
constexpr unsigned kScoreLdsBytes = 4640;  /* static LDS at G = 16: 16 x 52 staging words, the letter table, four waves' slot words */
constexpr unsigned kScoreBlocksPerCU = 7;  /* up to 72 VGPRs: seven waves per SIMD, i.e. seven workgroups of four waves per CU */
static_assert(kScoreSlotWords == 5u * AWFM_CANDIDATES_MAX_SLOTS, "five words a slot");
static_assert(kScoreLdsBytes == (kScoreThreads / 16u) * kVerifyGroupWords * 4u + 32u + (kScoreThreads / 64u) * kScoreSlotWords * 4u,
              "the staging words of sixteen groups, the letter table and the slot words of four waves");

struct DevScoreParams {
  struct AwFmVerifyInputs in;
  struct AwFmSlotScoreOutputs out;
  const unsigned char *text;
  unsigned long long length;
  const unsigned long long *ends; /* the image's record table; numRecords == 0: one sequence [0, length) */
  unsigned numRecords;
  unsigned long long numReads;
  unsigned slots, pad, drift, amino, floor, cap; /* floor: max(minScore, 1) */
  int match, mismatch, open, extend;             /* open: what the first character of a gap costs, o + e */
};

/* the launch's parameters where the launch left them, in the kernel's argument segment: a field is loaded where it is used
 * instead of living in a register from the kernel's first instruction to its last */
typedef const __attribute__((address_space(4))) DevScoreParams *ScoreParamsRef;

/* the value of slot `at` of read r (header: UNUSED .. TOO LONG, else the score) with its end cell; every lane of the group
 * returns the same.  Ref: ScoreParamsRef, or such a pointer to a struct that begins with a DevScoreParams; score: the diagonal's,
 * IdentityScore or MatrixScore (awfm_band_kernel.h) */
template <int G, typename Ref, typename S>
__device__ __forceinline__ unsigned scoreSlot(const Ref p, const S &score, const unsigned long long at, const unsigned s,
                                              const unsigned long long readBegin, const unsigned long long n64, const bool readOk,
                                              unsigned *sRead, unsigned *sText, const unsigned char *sAmino, const unsigned k,
                                              unsigned &endRead, unsigned long long &endText) {
  endRead = 0u;
  endText = 0ull;
  SlotBand slot;
  const unsigned status = classifySlot(*p, at, s, n64, readOk, slot);
  if (status != kSlotHasBand) return status;
  if (n64 > (unsigned long long)AWFM_ALIGN_MAX_LENGTH) return AWFM_VERIFY_TOO_LONG;
  const int n = (int)n64; /* <= 2^16 */
  const ReadBand band = readBand(slot, p->pad);
  if (n == 0 || (long long)n + band.hi < 0 || band.lo + 1 > slot.L) return 0u; /* no existing cell with i >= 1: nothing is aligned, nothing is read */
  /* here -n - 63 <= lo <= L - 1, so uMin <= n + 63 and uMax >= 1 */
  const bool inBand = (int)k < band.width;
  const unsigned char *R = p->in.readChars + readBegin, *T = p->text + slot.S;
  const int kExtend = (int)k * p->extend;
  const int bonus = score.endBonus(); /* the constant 0 but for "end bonus" */
  int prevH = inBand && (int)k >= band.uMin && (int)k <= band.uMax ? bonus : kBandNeg, prevF = kBandNeg; /* row 0: H(0, t) = B */
  int bestH = 0, bestI = 0;
  for (int i0 = 0; i0 < n; i0 += (int)kVerifyChunk) {
    const int rows = n - i0 < (int)kVerifyChunk ? n - i0 : (int)kVerifyChunk;
    const StagedChunk chunk = stageChunk<G>(R, T, band, i0, rows, sRead, sText, k);
    for (int q = 0; q < rows; q++) {
      const int u = i0 + q + 1 + (int)k;
      const bool inMatrix = inBand && u >= band.uMin && u <= band.uMax;
      const StagedLetters letters = stagedLetters(chunk, band, sRead, sText, sAmino, p->amino, q, u, inMatrix);
      const AffineCell c = affineRow<G>(*p, prevH, prevF, score(*p, letters, lettersSub(letters, p->amino)), inMatrix, kExtend, k);
      if (c.h > bestH) { /* (strictly: the smallest i of the lane's largest H) */
        bestH = c.h;
        bestI = i0 + q + 1;
      }
      prevH = c.h;
      prevF = inMatrix ? c.F : kBandNeg;
    }
  }
  /* V: a cell of row n reaches the read's end and is worth H + B when H > 0.  prevH is the lane's H(n, .) now, and bestH is at
   * least that: taking row n's value behind the loop gives the lane's largest V and its smallest i, as the update on V in
   * every row would, and costs the rows nothing */
  if (bonus != 0) {
    const int v = prevH > 0 ? prevH + bonus : prevH;
    if (v > bestH) {
      bestH = v;
      bestI = n;
    }
  }
  const AffineEnd end = affineEndCell<G>(bestH, bestI, k);
  if (end.score == 0u) return 0u;
  endRead = end.i;
  endText = (unsigned long long)(band.lo + (long long)end.i + (long long)end.k);
  return end.score;
}

/* the largest key of the wave's first sixteen lanes, in each of them */
__device__ __forceinline__ unsigned scoreMaxOfSixteen(unsigned key) {
#pragma unroll
  for (int step = 1; step < 16; step <<= 1) {
    const unsigned other = (unsigned)__shfl_xor((int)key, step, 16);
    key = other > key ? other : key;
  }
  return key;
}

/* The reads of the grid's waves, behind the workgroup's __syncthreads(): sStage is the staging words of its groups, kScoreThreads /
 * G times kVerifyGroupWords, sSlots the slot words of its waves.  Thirty-odd parameters, the nested loops' masks and a slot's own
 * values are more scalar registers than a wave has, and pinned into vector registers they cost a wave its occupancy: the
 * parameters stay in the argument segment (the struct is the kernel's only argument, so it begins the segment) and every trip
 * of the read loop takes the address anew, so that what a field's load yields lives no longer than the trip needs it */
template <int G, typename Ref, typename S>
__device__ __forceinline__ void scoreChainsAffineReads(Ref p, const S &score, unsigned *sStage, unsigned *sSlots, const unsigned char *sAmino) {
  constexpr unsigned kGroupsPerWave = 64u / (unsigned)G;
  const unsigned lane = threadIdx.x & 63u, k = lane % (unsigned)G, groupInWave = lane / (unsigned)G;
  unsigned *sRead = sStage + (threadIdx.x / (unsigned)G) * kVerifyGroupWords, *sText = sRead + kVerifyReadWords;
  unsigned *sValue = sSlots + (threadIdx.x / 64u) * kScoreSlotWords, *sEndRead = sValue + 16, *sEndLow = sValue + 32, *sEndHigh = sValue + 48,
           *sSequence = sValue + 64;
  const unsigned long long numWaves = (unsigned long long)gridDim.x * (kScoreThreads / 64u);
  const unsigned long long numReads = p->numReads;
  unsigned unscored = 0, mapped = 0;
  for (unsigned long long r = (unsigned long long)blockIdx.x * (kScoreThreads / 64u) + threadIdx.x / 64u; r < numReads; r += numWaves) {
    asm volatile("" : "+s"(p));
    const unsigned long long readBegin = p->in.readOffsets[r], readEnd = p->in.readOffsets[r + 1ull];
    const bool readOk = readBegin <= readEnd && readEnd <= p->in.numReadChars;
    __builtin_amdgcn_wave_barrier(); /* (the read before has read its slot words) */
    for (unsigned j = groupInWave; j < p->slots; j += kGroupsPerWave) {
      const unsigned long long at = r * p->slots + j;
      const unsigned s = p->in.sequences[at];
      unsigned endRead;
      unsigned long long endText;
      const unsigned value = scoreSlot<G>(p, score, at, s, readBegin, readEnd - readBegin, readOk, sRead, sText, sAmino, k, endRead, endText);
      if (k == 0u) {
        sValue[j] = value;
        sEndRead[j] = endRead;
        sEndLow[j] = (unsigned)endText;
        sEndHigh[j] = (unsigned)(endText >> 32);
        sSequence[j] = s;
      }
    }
    __builtin_amdgcn_wave_barrier();
    /* lane j holds slot j */
    const bool holds = lane < p->slots;
    const unsigned mine = lane & 15u;
    const unsigned value = holds ? sValue[mine] : AWFM_VERIFY_NONE, endRead = holds ? sEndRead[mine] : 0u;
    const unsigned endLow = holds ? sEndLow[mine] : 0u, endHigh = holds ? sEndHigh[mine] : 0u, sequence = holds ? sSequence[mine] : 0u;
    if (holds) {
      const unsigned long long at = r * p->slots + lane;
      if (p->out.slotScores) p->out.slotScores[at] = value;
      if (p->out.slotReadEnds) p->out.slotReadEnds[at] = endRead;
      if (p->out.slotTextEnds) p->out.slotTextEnds[at] = ((unsigned long long)endHigh << 32) | endLow;
    }
    unscored += holds && value >= AWFM_VERIFY_TOO_LONG && value != AWFM_VERIFY_NONE ? 1u : 0u;
    /* a score is below 2^24: score << 4 | 15 - slot orders by score, then by the lowest slot; 0 is "none" */
    const bool counts = holds && value < AWFM_VERIFY_TOO_LONG && value >= p->floor;
    const unsigned key = counts ? (value << 4) | (15u - mine) : 0u;
    const unsigned bestKey = scoreMaxOfSixteen(key);
    const unsigned best = 15u - (bestKey & 15u); /* (slot 15 when there is none: its words are read and not used) */
    const bool duplicate = sequence == sSequence[best] && endRead == sEndRead[best] && endLow == sEndLow[best] && endHigh == sEndHigh[best];
    const unsigned secondKey = scoreMaxOfSixteen(counts && mine != best && !duplicate ? key : 0u);
    if (lane == 0u) {
      const unsigned bestScore = bestKey >> 4, secondScore = secondKey >> 4;
      mapped += bestKey ? 1u : 0u;
      if (p->out.bestSlots) p->out.bestSlots[r] = bestKey ? best : AWFM_CHAINS_NO_SLOT;
      if (p->out.bestScores) p->out.bestScores[r] = bestScore;
      if (p->out.secondSlots) p->out.secondSlots[r] = secondKey ? 15u - (secondKey & 15u) : AWFM_CHAINS_NO_SLOT;
      if (p->out.secondScores) p->out.secondScores[r] = secondScore;
      /* exact in 32 bits: best < 2^24 and cap <= 254 */
      if (p->out.mappingQualities) p->out.mappingQualities[r] = (unsigned char)(bestKey ? p->cap * (bestScore - secondScore) / bestScore : 0u);
    }
  }
  /* one atomic per wave and counter that met any */
#pragma unroll
  for (int offset = 32; offset > 0; offset >>= 1) unscored += (unsigned)__shfl_xor((int)unscored, offset, 64);
  if (lane == 0u && unscored && p->out.numUnscored) atomicAdd((unsigned long long *)p->out.numUnscored, (unsigned long long)unscored);
  if (lane == 0u && mapped && p->out.numMapped) atomicAdd((unsigned long long *)p->out.numMapped, (unsigned long long)mapped);
}

template <int G>
__global__ void __launch_bounds__(kScoreThreads) scoreChainsAffineKernel(const DevScoreParams args) {
  (void)args;
  ScoreParamsRef p = (ScoreParamsRef)__builtin_amdgcn_kernarg_segment_ptr();
  __shared__ unsigned sStage[kScoreThreads / (unsigned)G][kVerifyGroupWords];
  __shared__ unsigned sSlots[kScoreThreads / 64u][kScoreSlotWords];
  __shared__ unsigned char sAmino[32];
  if (threadIdx.x < 32u) sAmino[threadIdx.x] = kAminoTables.letterOfAscii[threadIdx.x];
  __syncthreads();
  scoreChainsAffineReads<G>(p, IdentityScore(), &sStage[0][0], &sSlots[0][0], sAmino);
}

/* ---- the launcher (host side), shared with awfm_gpu_score_matrix.hip ---- */

/* The argument checks of awfmGpuScoreChainsAffine and awfmGpuScoreChainsMatrix after "null image" and numReads == 0, in the
 * header's order, before the device is switched or a lock taken (scoring: the call's scoring or matrix; refused: the call's
 * own check of its ranges, run in its place in that order) */
template <class Refused>
inline enum AwFmReturnCode scoreChainsArgumentsRefused(const char *name, const struct AwFmVerifyInputs *dIn, const void *scoring, Refused refused,
                                                       const uint64_t numReads, const uint32_t maxCandidates, const uint32_t bandPad,
                                                       const uint32_t maxDrift, const uint32_t mapqCap, const struct AwFmSlotScoreOutputs *dOut) {
  const uint64_t band = (uint64_t)maxDrift + 2ull * bandPad + 1ull;
  const enum AwFmReturnCode rc = chainArgumentsRefused(name, dIn, dOut && scoring, numReads, maxCandidates, band);
  if (rc != AwFmSuccess) return rc;
  if (mapqCap > AWFM_SCORE_MAX_MAPQ) {
    setCallError(name, "mapqCap is 0 to 254");
    return AwFmIllegalPositionError;
  }
  return refused();
}

/* The parameters of either call but for the costs, the lanes per group and the grid.  The caller holds image->recordMutex from
 * before this call until after the launch and has seen that the image has a text */
inline void scoreChainsParams(const AwFmGpuIndex *g, const struct AwFmVerifyInputs *dIn, const uint64_t numReads, const uint32_t maxCandidates,
                              const uint32_t bandPad, const uint32_t maxDrift, const uint32_t minScore, const uint32_t mapqCap,
                              const struct AwFmSlotScoreOutputs *dOut, DevScoreParams &p, unsigned &group, dim3 &grid) {
  const AwFmGpuImage *image = g->image;
  p.in = *dIn;
  p.out = *dOut;
  p.text = (const unsigned char *)image->dText;
  p.length = image->textLength;
  p.ends = image->records.ends;
  p.numRecords = image->records.numRecords;
  p.numReads = numReads;
  p.slots = maxCandidates;
  p.pad = bandPad;
  p.drift = maxDrift;
  p.amino = g->amino ? 1u : 0u;
  p.floor = minScore > 1u ? minScore : 1u;
  p.cap = mapqCap;
  group = bandGroup((uint64_t)maxDrift + 2ull * bandPad + 1ull, "score_group");
  /* persistent grid over reads, a wave each */
  const uint64_t perBlock = kScoreThreads / 64u, blocks = (numReads + perBlock - 1u) / perBlock;
  const uint64_t resident = (uint64_t)g->numCUs * kScoreBlocksPerCU;
  grid = dim3((unsigned)(blocks < resident ? blocks : resident));
}

}  // namespace

#endif
