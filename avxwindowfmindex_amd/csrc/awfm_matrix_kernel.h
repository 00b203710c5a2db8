/*
 * awfm_matrix_kernel.h -- scoreChainsMatrixKernel<G> and alignChainsMatrixKernel<G>, the kernels of "substitution matrices"
 * (include/awfm_gpu.h): slot scores and affine alignment with the diagonal's score out of a 21 x 21 table of signed bytes.  The
 * definition is the header's; the host twins and checkers are awfmScoreChainsMatrix (awfm_score_affine.c) and
 * awfmAlignChainsMatrix (awfm_align_affine.c).
 *
 * Each kernel IS its sibling -- scoreChainsAffineReads (awfm_score_affine_kernel.h), alignChainsAffineReads
 * (awfm_align_affine_kernel.h): a wave per read or a group per read, a lane per diagonal, chunks of kVerifyChunk rows, the same
 * staging, row, end cell, trace and walk -- called with MatrixScore in place of IdentityScore (awfm_band_kernel.h).  What is this
 * file's own is the matrix: it travels behind the sibling's parameters in the kernel's argument segment, and the workgroup copies
 * it into kMatrixLdsBytes of LDS before the __syncthreads() that the letter table needs anyway.  Per cell the two staged bytes
 * go through verifyLetter, then the cap to the last class, then one signed byte load from LDS whose row is uniform over a group.
 * EVERY LOAD OF TEXT OR READ stays the siblings' aligned dword through stageBytes.  Vector loads and stores only.
 */
#ifndef AWFM_MATRIX_KERNEL_H
#define AWFM_MATRIX_KERNEL_H

#include "awfm_align_affine_kernel.h"
#include "awfm_score_affine_kernel.h"

namespace {

constexpr unsigned kScoreMatrixLdsBytes = kScoreLdsBytes + kMatrixLdsBytes;   /* static LDS at G = 16 */
constexpr unsigned kAffineMatrixLdsBytes = kAffineLdsBytes + kMatrixLdsBytes; /* static LDS at G = 16 */

/* the sibling's parameters (match and mismatch unused), then the matrix as the caller's struct holds it */
struct DevScoreMatrixParams : DevScoreParams {
  signed char matrix[AWFM_MATRIX_CLASSES * AWFM_MATRIX_CLASSES];
};
struct DevAffineMatrixParams : DevAffineParams {
  signed char matrix[AWFM_MATRIX_CLASSES * AWFM_MATRIX_CLASSES];
};
/* the argument segment's layout, said out loud: the base first and whole, the matrix right behind it, nothing else */
template <class Params, class Base>
constexpr bool matrixBehind() {
  return sizeof(Params) == (sizeof(Base) + sizeof(Params::matrix) + alignof(Base) - 1u) / alignof(Base) * alignof(Base) && alignof(Params) == alignof(Base);
}
static_assert(matrixBehind<DevScoreMatrixParams, DevScoreParams>(), "DevScoreMatrixParams is DevScoreParams, then the matrix");
static_assert(matrixBehind<DevAffineMatrixParams, DevAffineParams>(), "DevAffineMatrixParams is DevAffineParams, then the matrix");
typedef const __attribute__((address_space(4))) DevScoreMatrixParams *ScoreMatrixParamsRef;
typedef const __attribute__((address_space(4))) DevAffineMatrixParams *AffineMatrixParamsRef;

template <int G>
__global__ void __launch_bounds__(kScoreThreads) scoreChainsMatrixKernel(const DevScoreMatrixParams args) {
  (void)args;
  ScoreMatrixParamsRef p = (ScoreMatrixParamsRef)__builtin_amdgcn_kernarg_segment_ptr();
  __shared__ unsigned sStage[kScoreThreads / (unsigned)G][kVerifyGroupWords];
  __shared__ unsigned sSlots[kScoreThreads / 64u][kScoreSlotWords];
  __shared__ unsigned char sAmino[32];
  __shared__ signed char sMatrix[kMatrixLdsBytes];
  if (threadIdx.x < 32u) sAmino[threadIdx.x] = kAminoTables.letterOfAscii[threadIdx.x];
  stageMatrix(p->matrix, sMatrix);
  const MatrixScore score = {sMatrix, p->amino ? 20u : 4u};
  __syncthreads();
  scoreChainsAffineReads<G>(p, score, &sStage[0][0], &sSlots[0][0], sAmino);
}

template <int G>
__global__ void __launch_bounds__(kAffineThreads, 4) alignChainsMatrixKernel(const DevAffineMatrixParams args) {
  DevAffineParams p = args;
  pinAffineParams(p);
  __shared__ unsigned sStage[kAffineThreads / (unsigned)G][kVerifyGroupWords];
  __shared__ unsigned char sAmino[32];
  __shared__ signed char sMatrix[kMatrixLdsBytes];
  if (threadIdx.x < 32u) sAmino[threadIdx.x] = kAminoTables.letterOfAscii[threadIdx.x];
  stageMatrix(((AffineMatrixParamsRef)__builtin_amdgcn_kernarg_segment_ptr())->matrix, sMatrix);
  const MatrixScore score = {sMatrix, p.amino ? 20u : 4u};
  __syncthreads();
  alignChainsAffineReads<G>(p, score, &sStage[0][0], sAmino);
}

}  // namespace

#endif
