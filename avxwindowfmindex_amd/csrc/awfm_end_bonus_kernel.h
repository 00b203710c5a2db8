/*
 * awfm_end_bonus_kernel.h -- scoreChainsEndBonusKernel<G> and alignChainsEndBonusKernel<G>, the kernels of "end bonus"
 * (include/awfm_gpu.h): slot scores and affine alignment under a substitution matrix in which an alignment that reaches a read
 * end earns B there.  The definition is the header's; the host twins and checkers are awfmScoreChainsEndBonus
 * (awfm_score_affine.c) and awfmAlignChainsEndBonus (awfm_align_affine.c).
 *
 * Each kernel IS its matrix sibling (awfm_matrix_kernel.h) -- scoreChainsAffineReads, alignChainsAffineReads: the same staging,
 * row, E scan, end cell, five trace bits and walk -- called with EndBonusScore in place of MatrixScore.  The scorer's endBonus()
 * is what those bodies put into row 0 (H(0, t) = B) and add to a positive H of row n -- behind the row loop, where the lane still
 * holds its H(n, .): the lane's best over H already is at least that, so one compare there gives the best over V with its
 * smallest i, and the rows cost what the sibling's cost; for every other scorer it is the constant 0 and both places fold away.
 * B travels behind the matrix in the kernel's argument segment.  EVERY LOAD OF TEXT OR READ stays the siblings' aligned dword
 * through stageBytes.  Vector loads and stores only.
 */
#ifndef AWFM_END_BONUS_KERNEL_H
#define AWFM_END_BONUS_KERNEL_H

#include "awfm_matrix_kernel.h"

namespace {

/* MatrixScore's diagonal, and B for a read end that is reached: 0 .. AWFM_END_BONUS_MAX */
struct EndBonusScore : MatrixScore {
  int bonus;
  __device__ __forceinline__ int endBonus() const { return bonus; }
};

/* the matrix sibling's parameters, then B */
struct DevScoreEndBonusParams : DevScoreMatrixParams {
  unsigned endBonus;
};
struct DevAffineEndBonusParams : DevAffineMatrixParams {
  unsigned endBonus;
};
/* the argument segment's layout: the matrix sibling's first, B in its tail or right behind it, nothing else */
static_assert(sizeof(DevScoreEndBonusParams) <= sizeof(DevScoreMatrixParams) + alignof(DevScoreParams) && alignof(DevScoreEndBonusParams) == alignof(DevScoreParams),
              "DevScoreEndBonusParams is DevScoreMatrixParams, then B");
static_assert(sizeof(DevAffineEndBonusParams) <= sizeof(DevAffineMatrixParams) + alignof(DevAffineParams) && alignof(DevAffineEndBonusParams) == alignof(DevAffineParams),
              "DevAffineEndBonusParams is DevAffineMatrixParams, then B");
typedef const __attribute__((address_space(4))) DevScoreEndBonusParams *ScoreEndBonusParamsRef;
typedef const __attribute__((address_space(4))) DevAffineEndBonusParams *AffineEndBonusParamsRef;

template <int G>
__global__ void __launch_bounds__(kScoreThreads) scoreChainsEndBonusKernel(const DevScoreEndBonusParams args) {
  (void)args;
  ScoreEndBonusParamsRef p = (ScoreEndBonusParamsRef)__builtin_amdgcn_kernarg_segment_ptr();
  __shared__ unsigned sStage[kScoreThreads / (unsigned)G][kVerifyGroupWords];
  __shared__ unsigned sSlots[kScoreThreads / 64u][kScoreSlotWords];
  __shared__ unsigned char sAmino[32];
  __shared__ signed char sMatrix[kMatrixLdsBytes];
  if (threadIdx.x < 32u) sAmino[threadIdx.x] = kAminoTables.letterOfAscii[threadIdx.x];
  stageMatrix(p->matrix, sMatrix);
  EndBonusScore score;
  score.sMatrix = sMatrix;
  score.other = p->amino ? 20u : 4u;
  score.bonus = (int)p->endBonus;
  __syncthreads();
  scoreChainsAffineReads<G>(p, score, &sStage[0][0], &sSlots[0][0], sAmino);
}

template <int G>
__global__ void __launch_bounds__(kAffineThreads, 4) alignChainsEndBonusKernel(const DevAffineEndBonusParams args) {
  DevAffineParams p = args;
  pinAffineParams(p);
  __shared__ unsigned sStage[kAffineThreads / (unsigned)G][kVerifyGroupWords];
  __shared__ unsigned char sAmino[32];
  __shared__ signed char sMatrix[kMatrixLdsBytes];
  if (threadIdx.x < 32u) sAmino[threadIdx.x] = kAminoTables.letterOfAscii[threadIdx.x];
  const AffineEndBonusParamsRef whole = (AffineEndBonusParamsRef)__builtin_amdgcn_kernarg_segment_ptr();
  stageMatrix(whole->matrix, sMatrix);
  EndBonusScore score;
  score.sMatrix = sMatrix;
  score.other = p.amino ? 20u : 4u;
  score.bonus = (int)whole->endBonus;
  __syncthreads();
  alignChainsAffineReads<G>(p, score, &sStage[0][0], sAmino);
}

}  // namespace

#endif
