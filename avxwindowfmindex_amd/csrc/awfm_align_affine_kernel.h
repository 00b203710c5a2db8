/*
 * awfm_align_affine_kernel.h -- alignChainsAffineKernel<G>, the kernel of "affine alignment" (include/awfm_gpu.h): the banded local
 * alignment with affine gap costs of every read against the record its chosen slot names, with soft clipping and the walk back
 * that emits the edit script.  The definition is the header's; the host twin and checker is awfm_align_affine.c.
 *
 * A group of G lanes per read (persistent grid over reads), lane k is diagonal lo + k of the band in sequence-local
 * coordinates, the rows go in chunks of kVerifyChunk.  The classification of the slot, the band, the staging of a chunk's read
 * and text characters into the group's words of LDS, the row and the end cell are awfm_band_kernel.h's (classifySlot, readBand,
 * stageChunk, affineRow, affineEndCell) -- EVERY LOAD OF TEXT OR READ is an aligned dword that holds a byte the slot owns, and
 * the record is checked against the text's length before anything is read; only aligned reads load text.  Lanes and rows
 * without a cell carry kBandNeg, and their trace code is "stop".
 *
 * THE TRACE.  Five wave-wide ballots give a row: three bits of the source of H (0 stop, 1 diagonal with equal letters, 2
 * diagonal with a substitution, 3 F, 4 E), "F of this cell opens its gap above" and "E of this cell opens its gap on the
 * left".  A group keeps its G bits of each -- 5 G / 8 bytes a row, kAffineRowBytes = 40 per row and wave whatever G --
 * and lane 0 stores them as row i - 1 of the group's part of the wave's arena in dScratch.  The end cell -- largest H, then
 * smallest i, then smallest k -- is each lane's own best (strict-greater update, no reduction per row) and one butterfly over
 * the group.  A fence orders the stores before the loads of the walk: every lane of the group walks back from the end cell
 * through the arena in the three states H, F, E -- the same addresses and the same state in all of them, neither read nor text
 * --, lane 0 writes the runs, last to first, and turns them round when they fit maxOps.  Counters take one atomic per wave.
 * Vector loads and stores only.
 */
#ifndef AWFM_ALIGN_AFFINE_KERNEL_H
#define AWFM_ALIGN_AFFINE_KERNEL_H

#include "awfm_band_kernel.h"

namespace {

constexpr unsigned kAffineThreads = 256;    /* per workgroup: four waves */
constexpr unsigned kAffineLdsBytes = 3360;  /* static LDS at G = 16, the most groups: 16 x 52 words and the amino letter table */
constexpr unsigned kAffineBlocksPerCU = 4;  /* up to 128 VGPRs: four waves per SIMD, i.e. four workgroups of four waves per CU */
constexpr unsigned kAffineRowBytes = 40;    /* of trace per row and wave: five ballots of 64 lanes, whatever G */
static_assert(kAffineLdsBytes == (kAffineThreads / 16u) * kVerifyGroupWords * 4u + 32u, "the staging words of sixteen groups and the letter table");

struct DevAffineParams {
  struct AwFmVerifyInputs in;
  struct AwFmAffineOutputs out;
  const unsigned *chosen;
  const unsigned char *text;
  unsigned long long length;
  const unsigned long long *ends; /* the image's record table; numRecords == 0: one sequence [0, length) */
  unsigned numRecords;
  unsigned long long numReads;
  unsigned char *arena; /* kAffineRowBytes * maxRows bytes per wave of the grid */
  unsigned slots, pad, drift, amino, maxOps, maxRows;
  int match, mismatch, open, extend; /* open: what the first character of a gap costs, o + e */
};

struct DevAffineAlignment {
  unsigned distance, readBegin, readEnd, numOps;
  unsigned long long textBegin, textEnd;
};

/* a group's G bits of one ballot: five of them make its row of trace */
template <int G>
struct AffineBits {
  typedef unsigned short type;
};
template <>
struct AffineBits<32> {
  typedef unsigned type;
};
template <>
struct AffineBits<64> {
  typedef unsigned long long type;
};

/* the group's bits of ballot q of a row (above bit G - 1: the groups behind this one) */
template <int G>
__device__ __forceinline__ void storeAffineBits(unsigned char *trace, unsigned row, unsigned q, unsigned long long bits) {
  typedef typename AffineBits<G>::type Bits;
  ((Bits *)trace)[row * 5u + q] = (Bits)bits;
}

/* the five bits of lane k's cell in that row: source in bits 0 .. 2, F opens in bit 3, E opens in bit 4 */
template <int G>
__device__ __forceinline__ unsigned loadAffineCode(const unsigned char *trace, unsigned row, unsigned k) {
  typedef typename AffineBits<G>::type Bits;
  const Bits *bits = (const Bits *)trace + row * 5u;
  unsigned code = 0;
#pragma unroll
  for (unsigned q = 0; q < 5u; q++) code |= (unsigned)((bits[q] >> (k & (unsigned)(G - 1))) & 1u) << q;
  return code;
}

/* a run of the script, met last to first: lane 0 stores a finished one */
struct AffineRuns {
  unsigned *ops;
  unsigned maxOps, numOps, run, op;
  bool writer;
  __device__ __forceinline__ void flush() {
    if (!run) return;
    if (ops && writer && numOps < maxOps) ops[numOps] = run << 4 | op;
    numOps++;
    run = 0;
  }
  __device__ __forceinline__ void emit(unsigned now, unsigned count) {
    if (!count) return;
    if (run && now != op) flush();
    op = now;
    run += count;
  }
};

/* the status of read r (header: UNUSED .. TOO LONG) or its score; every lane of the group returns the same.  scorer: the
 * diagonal's, IdentityScore or MatrixScore (awfm_band_kernel.h); '=' and 'X' go by verification's sub under either */
template <int G, typename S>
__device__ __forceinline__ unsigned alignReadAffine(const DevAffineParams &p, const S &scorer, const unsigned long long r, unsigned *sRead,
                                                    unsigned *sText, const unsigned char *sAmino, unsigned char *trace, const unsigned k,
                                                    const unsigned groupShift, DevAffineAlignment &a) {
  const unsigned j = p.chosen[r];
  if (j == AWFM_CHAINS_NO_SLOT) return AWFM_VERIFY_NONE;
  if (j >= p.slots) return AWFM_VERIFY_MALFORMED;
  const unsigned long long at = r * p.slots + j;
  const unsigned long long readBegin = p.in.readOffsets[r], readEnd = p.in.readOffsets[r + 1ull], n64 = readEnd - readBegin;
  SlotBand slot;
  const unsigned status = classifySlot(p, at, p.in.sequences[at], n64, readBegin <= readEnd && readEnd <= p.in.numReadChars, slot);
  if (status != kSlotHasBand) return status;
  if (n64 > (unsigned long long)p.maxRows) return AWFM_VERIFY_TOO_LONG;
  const int n = (int)n64; /* <= 2^16 */
  const ReadBand band = readBand(slot, p.pad);
  const long long lo = band.lo;
  if (n == 0 || (long long)n + band.hi < 0 || lo + 1 > slot.L) return 0u; /* no existing cell with i >= 1: nothing is aligned, nothing is read */
  /* here -n - 63 <= lo <= L - 1, so uMin <= n + 63 and uMax >= 1 */
  const int uMin = band.uMin, uMax = band.uMax;
  const bool inBand = (int)k < band.width;
  const unsigned char *R = p.in.readChars + readBegin, *T = p.text + slot.S;
  const int kExtend = (int)k * p.extend;
  const int bonus = scorer.endBonus(); /* the constant 0 but for "end bonus" */
  int prevH = inBand && (int)k >= uMin && (int)k <= uMax ? bonus : kBandNeg, prevF = kBandNeg; /* row 0: H(0, t) = B */
  int bestH = 0, bestI = 0;
  for (int i0 = 0; i0 < n; i0 += (int)kVerifyChunk) {
    const int rows = n - i0 < (int)kVerifyChunk ? n - i0 : (int)kVerifyChunk;
    const StagedChunk chunk = stageChunk<G>(R, T, band, i0, rows, sRead, sText, k);
    for (int q = 0; q < rows; q++) {
      const int u = i0 + q + 1 + (int)k;
      const bool inMatrix = inBand && u >= uMin && u <= uMax;
      const StagedLetters letters = stagedLetters(chunk, band, sRead, sText, sAmino, p.amino, q, u, inMatrix);
      const bool sub = lettersSub(letters, p.amino);
      const AffineCell c = affineRow<G>(p, prevH, prevF, scorer(p, letters, sub), inMatrix, kExtend, k);
      int leftH = __shfl_up(c.h, 1, G);
      leftH = k == 0u ? kBandNeg : leftH;
      const unsigned source = !inMatrix || c.h == 0 ? 0u : c.M == c.h ? (sub ? 2u : 1u) : c.F == c.h ? 3u : 4u;
      /* the five ballots, each out of the scalar registers and into the arena at once */
      const bool bit[5] = {(source & 1u) != 0u, (source & 2u) != 0u, (source & 4u) != 0u, c.fOpens >= c.fExtends,
                           c.e == leftH - p.open /* e = max(leftH - o - e, E[k - 1] - e) */};
#pragma unroll
      for (unsigned b = 0; b < 5u; b++) {
        unsigned long long bits = __builtin_amdgcn_ballot_w64(bit[b]) >> groupShift;
        asm volatile("" : "+v"(bits));
        if (k == 0u) storeAffineBits<G>(trace, (unsigned)(i0 + q), b, bits);
      }
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
  const unsigned score = end.score;
  if (score == 0u) return 0u;
  int i = (int)end.i;
  unsigned at2 = end.k;
  a.readEnd = (unsigned)i;
  a.textEnd = (unsigned long long)(lo + (long long)i + (long long)at2);
  __threadfence_block(); /* the rows lane 0 stored are read by every lane of the group */
  AffineRuns runs = {p.out.ops ? p.out.ops + r * p.maxOps : nullptr, p.maxOps, 0u, 0u, 0u, k == 0u};
  runs.emit(AWFM_ALIGN_OP_S, (unsigned)(n - i));
  unsigned state = 0u, distance = 0u; /* 0 H, 1 F, 2 E */
  /* (n steps to row 0 and at most n + 63 to the left; the bound only matters to a trace that is not this call's own) */
  for (int budget = 2 * n + 64; i > 0 && budget > 0; budget--) {
    const unsigned code = loadAffineCode<G>(trace, (unsigned)(i - 1), at2);
    if (state == 0u) {
      const unsigned source = code & 7u;
      if (source == 0u || source > 4u) break;
      if (source <= 2u) {
        runs.emit(source == 2u ? 8u : 7u, 1u);
        distance += source == 2u ? 1u : 0u;
        i--;
        continue;
      }
      state = source == 3u ? 1u : 2u;
    }
    distance++;
    if (state == 1u) {
      runs.emit(1u, 1u);
      state = code & 8u ? 0u : 1u;
      i--;
      at2++;
    } else {
      runs.emit(2u, 1u);
      state = code & 16u ? 0u : 2u;
      at2--;
    }
  }
  runs.emit(AWFM_ALIGN_OP_S, (unsigned)i);
  runs.flush();
  a.distance = distance;
  a.readBegin = (unsigned)i;
  a.textBegin = (unsigned long long)(lo + (long long)i + (long long)(int)at2);
  a.numOps = runs.numOps;
  if (runs.ops && k == 0u && runs.numOps <= p.maxOps) /* (the lane that stored them: its loads follow its stores) */
    for (unsigned q = 0; q < runs.numOps / 2u; q++) {
      const unsigned other = runs.ops[runs.numOps - 1u - q];
      runs.ops[runs.numOps - 1u - q] = runs.ops[q];
      runs.ops[q] = other;
    }
  return score;
}

/* the arguments live in vector registers, as in alignChainsKernel: the addresses, the nested loops' masks and five ballots a
 * row are more scalar registers than a wave has, and the compiler would spill some of them into lanes of a vector register */
__device__ __forceinline__ void pinAffineParams(DevAffineParams &p) {
  asm volatile("" : "+v"(p.in.sequences), "+v"(p.in.chainAnchors), "+v"(p.in.chainReadBegins), "+v"(p.in.chainReadEnds));
  asm volatile("" : "+v"(p.in.chainBeginDiagonals), "+v"(p.in.chainEndDiagonals), "+v"(p.out.scores), "+v"(p.out.editDistances));
  asm volatile("" : "+v"(p.out.readBegins), "+v"(p.out.readEnds), "+v"(p.out.textBegins), "+v"(p.out.textEnds));
  asm volatile("" : "+v"(p.out.numOps), "+v"(p.out.ops), "+v"(p.chosen), "+v"(p.in.readOffsets));
  asm volatile("" : "+v"(p.in.readChars), "+v"(p.in.numReadChars), "+v"(p.text), "+v"(p.ends));
  asm volatile("" : "+v"(p.length), "+v"(p.out.numUnaligned), "+v"(p.out.numTruncated), "+v"(p.numReads));
  asm volatile("" : "+v"(p.numRecords), "+v"(p.slots), "+v"(p.pad), "+v"(p.drift), "+v"(p.maxOps), "+v"(p.maxRows));
}

/* the reads of the grid's groups, behind the workgroup's __syncthreads(): sStage is the staging words of its groups, kAffineThreads /
 * G times kVerifyGroupWords */
template <int G, typename S>
__device__ __forceinline__ void alignChainsAffineReads(const DevAffineParams &p, const S &score, unsigned *sStage, const unsigned char *sAmino) {
  constexpr unsigned kGroupsPerWave = 64u / (unsigned)G;
  const unsigned lane = threadIdx.x & 63u, k = lane % (unsigned)G, groupInWave = lane / (unsigned)G;
  unsigned *sRead = sStage + (threadIdx.x / (unsigned)G) * kVerifyGroupWords, *sText = sRead + kVerifyReadWords;
  const unsigned long long wave = (unsigned long long)blockIdx.x * (kAffineThreads / 64u) + threadIdx.x / 64u;
  const unsigned long long numGroups = (unsigned long long)gridDim.x * (kAffineThreads / 64u) * kGroupsPerWave;
  /* the wave's arena, and in it the group's rows */
  unsigned char *trace = p.arena + wave * ((unsigned long long)kAffineRowBytes * p.maxRows) +
                         (unsigned long long)groupInWave * ((unsigned long long)(5 * G / 8) * p.maxRows);
  unsigned unaligned = 0, truncated = 0;
  for (unsigned long long r = wave * kGroupsPerWave + groupInWave; r < p.numReads; r += numGroups) {
    DevAffineAlignment a = {0u, 0u, 0u, 0u, 0ull, 0ull};
    const unsigned value = alignReadAffine<G>(p, score, r, sRead, sText, sAmino, trace, k, groupInWave * (unsigned)G, a);
    if (value >= AWFM_VERIFY_TOO_LONG) {
      unaligned += value != AWFM_VERIFY_NONE && k == 0u ? 1u : 0u;
    } else {
      truncated += a.numOps > p.maxOps && k == 0u ? 1u : 0u;
    }
    if (k == 0u) {
      if (p.out.scores) p.out.scores[r] = value;
      if (p.out.editDistances) p.out.editDistances[r] = a.distance;
      if (p.out.readBegins) p.out.readBegins[r] = a.readBegin;
      if (p.out.readEnds) p.out.readEnds[r] = a.readEnd;
      if (p.out.textBegins) p.out.textBegins[r] = a.textBegin;
      if (p.out.textEnds) p.out.textEnds[r] = a.textEnd;
      if (p.out.numOps) p.out.numOps[r] = a.numOps;
    }
  }
  /* one atomic per wave and counter that met any */
#pragma unroll
  for (int offset = 32; offset > 0; offset >>= 1) {
    unaligned += (unsigned)__shfl_xor((int)unaligned, offset, 64);
    truncated += (unsigned)__shfl_xor((int)truncated, offset, 64);
  }
  if (lane == 0u && unaligned && p.out.numUnaligned) atomicAdd((unsigned long long *)p.out.numUnaligned, (unsigned long long)unaligned);
  if (lane == 0u && truncated && p.out.numTruncated) atomicAdd((unsigned long long *)p.out.numTruncated, (unsigned long long)truncated);
}

template <int G>
__global__ void __launch_bounds__(kAffineThreads, 4) alignChainsAffineKernel(const DevAffineParams args) {
  DevAffineParams p = args;
  pinAffineParams(p);
  __shared__ unsigned sStage[kAffineThreads / (unsigned)G][kVerifyGroupWords];
  __shared__ unsigned char sAmino[32];
  if (threadIdx.x < 32u) sAmino[threadIdx.x] = kAminoTables.letterOfAscii[threadIdx.x];
  __syncthreads();
  alignChainsAffineReads<G>(p, IdentityScore(), &sStage[0][0], sAmino);
}

/* ---- the launcher (host side), shared with awfm_gpu_align_matrix.hip ---- */

/* the waves of the persistent grid: the launch and the arena's size come from this one number */
inline uint64_t affineGridWaves(const AwFmGpuIndex *g) { return (uint64_t)g->numCUs * kAffineBlocksPerCU * (kAffineThreads / 64u); }

/* The argument checks of awfmGpuAlignChainsAffine and awfmGpuAlignChainsMatrix after "null image" and numReads == 0, in the
 * header's order, before the device is switched or a lock taken (scoring: the call's scoring or matrix; refused: the call's
 * own check of its ranges, run in its place in that order) */
template <class Refused>
inline enum AwFmReturnCode alignChainsArgumentsRefused(const char *name, const struct AwFmVerifyInputs *dIn, const uint32_t *dSlots,
                                                       const void *scoring, Refused refused, const uint64_t numReads, const uint32_t maxCandidates,
                                                       const uint32_t bandPad, const uint32_t maxDrift, const uint32_t maxOps,
                                                       const uint32_t maxRows, const struct AwFmAffineOutputs *dOut, const void *dScratch) {
  const uint64_t band = (uint64_t)maxDrift + 2ull * bandPad + 1ull;
  enum AwFmReturnCode rc = chainArgumentsRefused(name, dIn, dOut && dSlots && dScratch && scoring, numReads, maxCandidates, band);
  if (rc != AwFmSuccess) return rc;
  if (maxOps < 1 || maxOps > AWFM_ALIGN_MAX_OPS || maxRows < 1 || maxRows > AWFM_ALIGN_MAX_LENGTH) {
    setCallError(name, "maxOps is 1 to 4096 and maxRows 1 to 65536");
    return AwFmIllegalPositionError;
  }
  if ((rc = refused()) != AwFmSuccess) return rc;
  if ((uintptr_t)dScratch & 15u) {
    setCallError(name, "the scratch is aligned to 16 bytes");
    return AwFmIllegalPositionError;
  }
  return AwFmSuccess;
}

/* The parameters of either call but for the costs, the lanes per group and the grid.  The caller holds image->recordMutex from
 * before this call until after the launch and has seen that the image has a text */
inline void alignChainsParams(const AwFmGpuIndex *g, const struct AwFmVerifyInputs *dIn, const uint32_t *dSlots, const uint64_t numReads,
                              const uint32_t maxCandidates, const uint32_t bandPad, const uint32_t maxDrift, const uint32_t maxOps,
                              const uint32_t maxRows, const struct AwFmAffineOutputs *dOut, void *dScratch, DevAffineParams &p, unsigned &group,
                              dim3 &grid) {
  const AwFmGpuImage *image = g->image;
  p.in = *dIn;
  p.out = *dOut;
  p.chosen = dSlots;
  p.text = (const unsigned char *)image->dText;
  p.length = image->textLength;
  p.ends = image->records.ends;
  p.numRecords = image->records.numRecords;
  p.numReads = numReads;
  p.arena = (unsigned char *)dScratch;
  p.slots = maxCandidates;
  p.pad = bandPad;
  p.drift = maxDrift;
  p.amino = g->amino ? 1u : 0u;
  p.maxOps = maxOps;
  p.maxRows = maxRows;
  group = bandGroup((uint64_t)maxDrift + 2ull * bandPad + 1ull, "affine_group");
  /* persistent grid over reads, a group each: never more waves than the arena has room for */
  const uint64_t perBlock = (uint64_t)(kAffineThreads / group), blocks = (numReads + perBlock - 1u) / perBlock;
  const uint64_t resident = affineGridWaves(g) / (kAffineThreads / 64u);
  grid = dim3((unsigned)(blocks < resident ? blocks : resident));
}

}  // namespace

#endif
