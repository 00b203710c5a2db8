"""ctypes loader and struct mirrors for libawfmindex_amd.so (include/AwFmIndex.h, include/awfm_gpu.h)."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AWFM_LIB_PATH") or os.path.join(_HERE, "libawfmindex_amd.so")  # override: A/B builds
_LIB = None

AwFmAlphabetAmino, AwFmAlphabetDna, AwFmAlphabetRna = 1, 2, 3
AwFmSuccess, AwFmFileReadOkay, AwFmFileWriteOkay = 1, 2, 3
AwFmGeneralFailure = -1
AwFmIllegalPositionError = -6
AwFmUnsupportedVersionError = -2
AwFmFileReadFail = -11

# every symbol the two public headers declare
API_SYMBOLS = [
    "awFmCreateIndex", "awFmCreateIndexFromFasta", "awFmDeallocIndex", "awFmWriteIndexToFile",
    "awFmReadIndexFromFile", "awFmCreateKmerSearchList", "awFmDeallocKmerSearchList", "awFmParallelSearchLocate",
    "awFmParallelSearchCount", "awFmFindSearchRangeForString", "awFmReadSequenceFromFile",
    "awFmCreateInitialQueryRange", "awFmCreateInitialQueryRangeFromChar",
    "awFmNucleotideIterativeStepBackwardSearch", "awFmAminoIterativeStepBackwardSearch",
    "awFmFindDatabaseHitPositions", "awFmFindDatabaseHitPositionSingle",
    "awFmGetLocalSequencePositionFromIndexPosition", "awFmNucleotideBacktraceReturnPreviousLetterIndex",
    "awFmAminoBacktraceReturnPreviousLetterIndex", "awFmGetHeaderStringFromSequenceNumber", "awFmSearchRangeLength",
    "awFmReturnCodeIsFailure", "awFmReturnCodeIsSuccess", "awFmGetNumSequences",
]
GPU_SYMBOLS = [
    "awfmGpuDeviceCount", "awfmGpuLastError", "awfmGpuIndexCreate", "awfmGpuIndexDestroy", "awfmGpuIndexAcquire", "awfmGpuIndexAcquireAll",
    "awfmGpuIndexRelease", "awfmGpuIndexDeviceBytes", "awfmGpuIndexDevice", "awfmGpuIndexSetKernel", "awfmGpuIndexSetWide", "awfmGpuIndexIsWide", "awfmGpuLastBatchStatus", "awfmGpuIndexSetDeepSeed", "awfmGpuIndexSetDenseSa", "awfmGpuPinnedBuffer", "awfmGpuLocateHostWindows", "awfmGpuLocateWindow", "awfmGpuAosLock",
    "awfmGpuAosUnlock", "awfmGpuSearch", "awfmGpuSearchHits", "awfmGpuSearchHitsSparse", "awfmGpuIndexSetOrdered", "awfmGpuSearchHitsIsOrdered", "awfmGpuLastOrderedKernelMs", "awfmGpuLastOrderedKernelIsLookup", "awfmGpuLastOrderedKept", "awfmGpuLastSecondWindow",
    "awfmGpuScanScratchBytes", "awfmGpuHitOffsets", "awfmGpuHitOffsetsFromCounts", "awfmGpuLocate", "awfmGpuCountHost", "awfmGpuLocateHost",
    "awfmGpuCreateIndex", "awfmGpuSearchTally", "awfmGpuSynthText", "awfmGpuSynthRandomQueries", "awfmGpuSynthPlantedQueries",
    "awfmGpuSynthMixedLengths", "awfmGpuSynthMixedQueries", "awfmGpuSynthGenomeText", "awfmGpuSynthPlantedQueriesClean",
    "awfmPackKmers", "awfmGpuPackKmers", "awfmGpuUnpackKmers", "awfmGpuHostAlloc", "awfmGpuHostFree", "awfmGpuStreamPacked",
    "awfmGpuStreamChars", "awfmGpuCountPackedHost", "awfmGpuLocatePackedHost", "awfmGpuIndexSetPairImage", "awfmGpuIndexHasPairImage",
    "awfmGpuSearchHitsPacked", "awfmGpuLocateTo", "awfmGpuSearchHitsLineTally", "awfmGpuIndexDeepSeedK", "awfmGpuSearchHitsCompact", "awfmGpuCompactHits", "awfmGpuSortHits",
    "awfmGpuStreamPackedSparse", "awfmGpuStreamCharsSparse", "awfmGpuSearchHitsInOrder", "awfmGpuSearchHitsInOrderCounts",
    "awfmGpuSortHitsOnDevice", "awfmGpuHitOffsetsOnDevice", "awfmGpuLocateOnDevice", "awfmGpuLastOrderedSearchKernelMs", "awfmGpuOrderedKernelLog", "awfmGpuIndexDeepSeedBuildSeconds", "awfmGpuIndexDeepSeedTransientBytes", "awfmGpuIndexHasDenseSa", "awfmGpuIndexDenseSaBuildSeconds", "awfmGpuIndexLengthTableBytes", "awfmGpuIndexLengthTableBuildSeconds", "awfmGpuMixedLookupLineTally",
    "awfmGpuListLocateOnDevice", "awfmGpuLastLookupFront", "awfmGpuLastSearchWasExactLookup", "awfmGpuSynthPlantedQueriesUnique", "awfmGpuStreamRetire", "awfmGpuIndexDescribe", "awfmGpuIndexDeepSeedAllocSeconds", "awfmGpuAosLastStages", "awfmHostCopyGBs",
    "awfmLocalPositions", "awfmGpuIndexSetRecordTable", "awfmGpuIndexNumRecords", "awfmGpuLocalPositions", "awfmGpuLocateHostLocal",
    "awfmLongestSuffixMatches", "awfmGpuLongestSuffixMatches", "awfmOneSubstitutionSearch", "awfmGpuOneSubstitutionSearch",
    "awfmReadCandidates", "awfmGpuReadCandidates", "awfmGpuReadCandidatesScratchBytes",
    "awfmReadChains", "awfmGpuReadChains", "awfmGpuReadChainsScratchBytes",
    "awfmGpuIndexSetText", "awfmGpuIndexTextLength", "awfmTextWindows", "awfmGpuTextWindows", "awfmVerifyChains", "awfmGpuVerifyChains",
    "awfmAlignChains", "awfmGpuAlignChainsScratchBytes", "awfmGpuAlignChains",
    "awfmAlignChainsAffine", "awfmGpuAlignChainsAffineScratchBytes", "awfmGpuAlignChainsAffine",
    "awfmScoreChainsAffine", "awfmGpuScoreChainsAffine",
    "awfmMatrixScoringUniform", "awfmMatrixScoringFromText", "awfmScoreChainsMatrix", "awfmGpuScoreChainsMatrix", "awfmAlignChainsMatrix",
    "awfmGpuAlignChainsMatrix",
    "awfmScoreChainsEndBonus", "awfmGpuScoreChainsEndBonus", "awfmAlignChainsEndBonus", "awfmGpuAlignChainsEndBonus",
    "awfmScoreWindowsAffine", "awfmGpuScoreWindowsAffineScratchBytes", "awfmGpuScoreWindowsAffine",
    "awfmPairMates", "awfmGpuPairMates", "awfmReverseComplementReads", "awfmGpuReverseComplementReads",
    "awfmInsertHistogram", "awfmGpuInsertHistogram", "awfmInsertInterval", "awfmGpuInsertInterval", "awfmGpuPairMatesEstimated",
    "awfmAlignmentStrings", "awfmGpuAlignmentStringsScratchBytes", "awfmGpuAlignmentStrings",
    "awfmSamRecords", "awfmGpuSamRecordsScratchBytes", "awfmGpuSamRecords", "awfmRecordNames", "awfmSamHeader",
    "awfmChooseStrands", "awfmGpuChooseStrands", "awfmOrientReads", "awfmGpuOrientReads",
    "awfmGpuOrderBuckets", "awfmGpuOrderKmers", "awfmGpuSearchOrderedRecords", "awfmGpuSearchOrderedRecordsCounts", "awfmGpuSearchGeneralRecords", "awfmGpuMergeBucketRuns",
]
# int sink(void *user, uint64 firstKmer, uint64 numKmers, const uint32 *counts, const uint64 *positions, uint64 numPositions)
CHUNK_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_uint64)


# int sink(void *user, uint64 firstKmer, uint64 numKmers, uint64 numHitKmers, const uint32 *hitKmers, const uint64 *hitOffsets,
#          const uint64 *positions, uint64 numPositions)
SPARSE_CHUNK_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                C.POINTER(C.c_uint64), C.c_uint64)
# int sink(void *user, uint64 queryBegin, uint64 queryEnd, uint64 hitBegin, uint64 hitEnd, const uint64 *positions)
HIT_WINDOW_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64))


class AwFmIndexConfiguration(C.Structure):
    _fields_ = [("suffixArrayCompressionRatio", C.c_uint8), ("kmerLengthInSeedTable", C.c_uint8),
                ("alphabetType", C.c_int), ("keepSuffixArrayInMemory", C.c_bool), ("storeOriginalSequence", C.c_bool)]


class AwFmCompressedSuffixArray(C.Structure):
    _fields_ = [("valueBitWidth", C.c_uint8), ("values", C.POINTER(C.c_uint8)), ("compressedByteLength", C.c_uint64)]


class AwFmSearchRange(C.Structure):
    _fields_ = [("startPtr", C.c_uint64), ("endPtr", C.c_uint64)]


class AwFmCandidateInputs(C.Structure):
    """struct AwFmCandidateInputs (include/awfm_gpu.h): host or device addresses"""
    _fields_ = [("readSeedOffsets", C.c_void_p), ("numSeeds", C.c_uint64), ("seedEnds", C.c_void_p), ("seedLengths", C.c_void_p),
                ("fixedLength", C.c_uint32), ("hitOffsets", C.c_void_p), ("numHits", C.c_uint64), ("positions", C.c_void_p),
                ("sequenceNumbers", C.c_void_p)]


class AwFmCandidateOutputs(C.Structure):
    """struct AwFmCandidateOutputs (include/awfm_gpu.h): host or device addresses, each may be NULL"""
    _fields_ = [("sequences", C.c_void_p), ("diagonals", C.c_void_p), ("votes", C.c_void_p), ("diagonalSpans", C.c_void_p),
                ("readBegins", C.c_void_p), ("readEnds", C.c_void_p), ("numCandidates", C.c_void_p), ("keptHits", C.c_void_p),
                ("numOverflowed", C.c_void_p)]


class AwFmChainOutputs(C.Structure):
    """struct AwFmChainOutputs (include/awfm_gpu.h): host or device addresses, each may be NULL"""
    _fields_ = [("chainScores", C.c_void_p), ("chainAnchors", C.c_void_p), ("chainReadBegins", C.c_void_p), ("chainReadEnds", C.c_void_p),
                ("chainBeginDiagonals", C.c_void_p), ("chainEndDiagonals", C.c_void_p), ("bestSlots", C.c_void_p), ("keptHits", C.c_void_p),
                ("numOverflowed", C.c_void_p)]


class AwFmVerifyInputs(C.Structure):
    """struct AwFmVerifyInputs (include/awfm_gpu.h): host or device addresses"""
    _fields_ = [("readChars", C.c_void_p), ("numReadChars", C.c_uint64), ("readOffsets", C.c_void_p), ("sequences", C.c_void_p),
                ("chainAnchors", C.c_void_p), ("chainReadBegins", C.c_void_p), ("chainReadEnds", C.c_void_p),
                ("chainBeginDiagonals", C.c_void_p), ("chainEndDiagonals", C.c_void_p)]


class AwFmVerifyOutputs(C.Structure):
    """struct AwFmVerifyOutputs (include/awfm_gpu.h): host or device addresses, each may be NULL"""
    _fields_ = [("editDistances", C.c_void_p), ("bestSlots", C.c_void_p), ("numUnverified", C.c_void_p)]


class AwFmAlignOutputs(C.Structure):
    """struct AwFmAlignOutputs (include/awfm_gpu.h): host or device addresses, each may be NULL"""
    _fields_ = [("editDistances", C.c_void_p), ("textBegins", C.c_void_p), ("textEnds", C.c_void_p), ("numOps", C.c_void_p),
                ("ops", C.c_void_p), ("numUnaligned", C.c_void_p), ("numTruncated", C.c_void_p)]


class AwFmAlignScoring(C.Structure):
    """struct AwFmAlignScoring (include/awfm_gpu.h): match 1..255, mismatch 0..255, gapOpen 0..255, gapExtend 1..255"""
    _fields_ = [("match", C.c_uint32), ("mismatch", C.c_uint32), ("gapOpen", C.c_uint32), ("gapExtend", C.c_uint32)]


class AwFmMatrixScoring(C.Structure):
    """struct AwFmMatrixScoring (include/awfm_gpu.h): 21 x 21 substitution values [class(read) * 21 + class(text)], gapOpen 0..255,
    gapExtend 1..255"""
    _fields_ = [("substitution", C.c_int8 * (21 * 21)), ("gapOpen", C.c_uint32), ("gapExtend", C.c_uint32)]


class AwFmAffineOutputs(C.Structure):
    """struct AwFmAffineOutputs (include/awfm_gpu.h): host or device addresses, each may be NULL"""
    _fields_ = [("scores", C.c_void_p), ("editDistances", C.c_void_p), ("readBegins", C.c_void_p), ("readEnds", C.c_void_p),
                ("textBegins", C.c_void_p), ("textEnds", C.c_void_p), ("numOps", C.c_void_p), ("ops", C.c_void_p),
                ("numUnaligned", C.c_void_p), ("numTruncated", C.c_void_p)]


class AwFmSlotScoreOutputs(C.Structure):
    """struct AwFmSlotScoreOutputs (include/awfm_gpu.h): host or device addresses, each may be NULL"""
    _fields_ = [("slotScores", C.c_void_p), ("slotReadEnds", C.c_void_p), ("slotTextEnds", C.c_void_p), ("bestSlots", C.c_void_p),
                ("bestScores", C.c_void_p), ("secondSlots", C.c_void_p), ("secondScores", C.c_void_p), ("mappingQualities", C.c_void_p),
                ("numUnscored", C.c_void_p), ("numMapped", C.c_void_p)]


class AwFmWindowInputs(C.Structure):
    """struct AwFmWindowInputs (include/awfm_gpu.h): host or device addresses"""
    _fields_ = [("readChars", C.c_void_p), ("numReadChars", C.c_uint64), ("readOffsets", C.c_void_p), ("windowSequences", C.c_void_p),
                ("windowBegins", C.c_void_p), ("windowEnds", C.c_void_p)]


class AwFmWindowOutputs(C.Structure):
    """struct AwFmWindowOutputs (include/awfm_gpu.h): host or device addresses, each may be NULL"""
    _fields_ = [("scores", C.c_void_p), ("readBegins", C.c_void_p), ("readEnds", C.c_void_p), ("textBegins", C.c_void_p),
                ("textEnds", C.c_void_p), ("sequences", C.c_void_p), ("chainAnchors", C.c_void_p), ("chainReadBegins", C.c_void_p),
                ("chainReadEnds", C.c_void_p), ("chainBeginDiagonals", C.c_void_p), ("chainEndDiagonals", C.c_void_p),
                ("numUnscored", C.c_void_p), ("numFound", C.c_void_p)]


class AwFmPairInputs(C.Structure):
    """struct AwFmPairInputs (include/awfm_gpu.h): host or device addresses; mappingQualities may be NULL"""
    _fields_ = [("readOffsets", C.c_void_p), ("sequences", C.c_void_p), ("slotScores", C.c_void_p), ("slotReadEnds", C.c_void_p),
                ("slotTextEnds", C.c_void_p), ("mappingQualities", C.c_void_p)]


class AwFmPairParams(C.Structure):
    """struct AwFmPairParams (include/awfm_gpu.h): minInsert <= maxInsert within +-2^40, mapqCap 0..254"""
    _fields_ = [("minInsert", C.c_int64), ("maxInsert", C.c_int64), ("minScore", C.c_uint32), ("unpairedPenalty", C.c_uint32),
                ("windowPad", C.c_uint32), ("mapqCap", C.c_uint32)]


class AwFmPairOutputs(C.Structure):
    """struct AwFmPairOutputs (include/awfm_gpu.h): host or device addresses, each may be NULL"""
    _fields_ = [("properPairs", C.c_void_p), ("pairSlots", C.c_void_p), ("pairScores", C.c_void_p), ("pairSecondScores", C.c_void_p),
                ("templateLengths", C.c_void_p), ("pairQualities", C.c_void_p), ("mappingQualities", C.c_void_p),
                ("windowSequences", C.c_void_p), ("windowBegins", C.c_void_p), ("windowEnds", C.c_void_p), ("numProper", C.c_void_p),
                ("numWindows", C.c_void_p)]


class AwFmInsertParams(C.Structure):
    """struct AwFmInsertParams (include/awfm_gpu.h, "insert size"): the histogram's range, who qualifies, the spread and the fallback"""
    _fields_ = [("lowTemplate", C.c_int64), ("highTemplate", C.c_int64), ("minScore", C.c_uint32), ("minQuality", C.c_uint32),
                ("spread", C.c_uint32), ("minSamples", C.c_uint32), ("fallbackMin", C.c_int64), ("fallbackMax", C.c_int64)]


class AwFmInsertEstimate(C.Structure):
    """struct AwFmInsertEstimate (include/awfm_gpu.h): 64 bytes, minInsert and maxInsert first"""
    _fields_ = [("minInsert", C.c_int64), ("maxInsert", C.c_int64), ("quartiles", C.c_int64 * 3), ("mean", C.c_int64),
                ("numSamples", C.c_uint64), ("valid", C.c_uint64)]


class AwFmStringInputs(C.Structure):
    """struct AwFmStringInputs (include/awfm_gpu.h, "alignment strings"): host or device addresses"""
    _fields_ = [("sequences", C.c_void_p), ("slots", C.c_void_p), ("textBegins", C.c_void_p), ("numOps", C.c_void_p), ("ops", C.c_void_p)]


class AwFmStringOutputs(C.Structure):
    """struct AwFmStringOutputs (include/awfm_gpu.h): host or device addresses, each may be NULL, and the arenas' capacities"""
    _fields_ = [("cigarOffsets", C.c_void_p), ("cigarChars", C.c_void_p), ("cigarCapacity", C.c_uint64), ("mdOffsets", C.c_void_p),
                ("mdChars", C.c_void_p), ("mdCapacity", C.c_uint64), ("numSkipped", C.c_void_p), ("numOverflow", C.c_void_p)]


class AwFmSamInputs(C.Structure):
    """struct AwFmSamInputs (include/awfm_gpu.h, "SAM records"): host or device addresses; the optional ones may be NULL"""
    _fields_ = [("readChars", C.c_void_p), ("numReadChars", C.c_uint64), ("readOffsets", C.c_void_p), ("qualities", C.c_void_p),
                ("nameOffsets", C.c_void_p), ("nameChars", C.c_void_p), ("recordNameOffsets", C.c_void_p), ("recordNameChars", C.c_void_p),
                ("numRecordNames", C.c_uint32), ("sequences", C.c_void_p), ("slots", C.c_void_p), ("scores", C.c_void_p),
                ("editDistances", C.c_void_p), ("textBegins", C.c_void_p), ("textEnds", C.c_void_p), ("cigarOffsets", C.c_void_p),
                ("cigarChars", C.c_void_p), ("mdOffsets", C.c_void_p), ("mdChars", C.c_void_p), ("mappingQualities", C.c_void_p),
                ("secondScores", C.c_void_p), ("baseFlags", C.c_void_p), ("properPairs", C.c_void_p)]


class AwFmStrandInputs(C.Structure):
    """struct AwFmStrandInputs (include/awfm_gpu.h, "strands"): host or device addresses of the 2R rows"""
    _fields_ = [("readOffsets", C.c_void_p), ("sequences", C.c_void_p), ("slotScores", C.c_void_p), ("slotReadEnds", C.c_void_p),
                ("slotTextEnds", C.c_void_p)]


class AwFmStrandOutputs(C.Structure):
    """struct AwFmStrandOutputs (include/awfm_gpu.h): host or device addresses, each may be NULL"""
    _fields_ = [("strands", C.c_void_p), ("strandSlots", C.c_void_p), ("bestScores", C.c_void_p), ("secondScores", C.c_void_p),
                ("mappingQualities", C.c_void_p), ("baseFlags", C.c_void_p), ("rowSlots", C.c_void_p), ("windowSequences", C.c_void_p),
                ("windowBegins", C.c_void_p), ("windowEnds", C.c_void_p), ("properPairs", C.c_void_p), ("pairScores", C.c_void_p),
                ("pairSecondScores", C.c_void_p), ("templateLengths", C.c_void_p), ("pairQualities", C.c_void_p), ("numReverse", C.c_void_p),
                ("numProper", C.c_void_p), ("numWindows", C.c_void_p), ("numMalformed", C.c_void_p)]


class AwFmOrientInputs(C.Structure):
    """struct AwFmOrientInputs (include/awfm_gpu.h, "strands"): the 2R rows, the optional score columns and qualities, the strands"""
    _fields_ = [("rows", AwFmVerifyInputs), ("slotScores", C.c_void_p), ("slotReadEnds", C.c_void_p), ("slotTextEnds", C.c_void_p),
                ("qualities", C.c_void_p), ("strands", C.c_void_p)]


class AwFmOrientOutputs(C.Structure):
    """struct AwFmOrientOutputs (include/awfm_gpu.h): host or device addresses; a column is given exactly when its input is"""
    _fields_ = [("readChars", C.c_void_p), ("capacity", C.c_uint64), ("readOffsets", C.c_void_p), ("qualities", C.c_void_p),
                ("sequences", C.c_void_p), ("chainAnchors", C.c_void_p), ("chainReadBegins", C.c_void_p), ("chainReadEnds", C.c_void_p),
                ("chainBeginDiagonals", C.c_void_p), ("chainEndDiagonals", C.c_void_p), ("slotScores", C.c_void_p),
                ("slotReadEnds", C.c_void_p), ("slotTextEnds", C.c_void_p), ("numMalformed", C.c_void_p)]


class AwFmSamOutputs(C.Structure):
    """struct AwFmSamOutputs (include/awfm_gpu.h): host or device addresses, each may be NULL, and the arena's capacity"""
    _fields_ = [("lineOffsets", C.c_void_p), ("lineChars", C.c_void_p), ("lineCapacity", C.c_uint64), ("numUnaligned", C.c_void_p),
                ("numOverflow", C.c_void_p)]


class AwFmIndex(C.Structure):
    _fields_ = [("versionNumber", C.c_uint32), ("featureFlags", C.c_uint32), ("bwtLength", C.c_uint64),
                ("bwtBlockList", C.c_void_p), ("prefixSums", C.POINTER(C.c_uint64)),
                ("kmerSeedTable", C.POINTER(AwFmSearchRange)), ("fileHandle", C.c_void_p),
                ("config", AwFmIndexConfiguration), ("fileDescriptor", C.c_int), ("suffixArrayFileOffset", C.c_size_t),
                ("sequenceFileOffset", C.c_size_t), ("fastaVector", C.c_void_p),
                ("suffixArray", AwFmCompressedSuffixArray)]


class AwFmKmerSearchData(C.Structure):
    _fields_ = [("kmerString", C.c_void_p), ("kmerLength", C.c_uint64), ("positionList", C.POINTER(C.c_uint64)),
                ("count", C.c_uint32), ("capacity", C.c_uint32)]


class AwFmKmerSearchList(C.Structure):
    _fields_ = [("capacity", C.c_size_t), ("count", C.c_size_t), ("kmerSearchData", C.POINTER(AwFmKmerSearchData))]


def build(force=False):
    """compile libawfmindex_amd.so in-tree (hipcc --offload-arch=gfx950 + gcc)"""
    src = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", src, "-s", "clean"])
    subprocess.check_call(["make", "-C", src, "-s", "-j4"])
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libawfmindex_amd.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
            "there is no fallback implementation")
    try:  # share torch's HIP runtime when torch is in the process (same SONAME libamdhip64.so.7)
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    IP, LP = C.POINTER(AwFmIndex), C.POINTER(AwFmKmerSearchList)
    RP = C.POINTER(AwFmSearchRange)
    vp, u64 = C.c_void_p, C.c_uint64
    sig = {
        "awFmCreateIndex": (C.c_int, [C.POINTER(IP), C.POINTER(AwFmIndexConfiguration), vp, C.c_size_t, C.c_char_p]),
        "awFmCreateIndexFromFasta": (C.c_int, [C.POINTER(IP), C.POINTER(AwFmIndexConfiguration), C.c_char_p, C.c_char_p]),
        "awFmDeallocIndex": (None, [IP]),
        "awFmWriteIndexToFile": (C.c_int, [IP, vp, u64, C.c_char_p]),
        "awFmReadIndexFromFile": (C.c_int, [C.POINTER(IP), C.c_char_p, C.c_bool]),
        "awFmCreateKmerSearchList": (LP, [C.c_size_t]),
        "awFmDeallocKmerSearchList": (None, [LP]),
        "awFmParallelSearchLocate": (C.c_int, [IP, LP, C.c_uint32]),
        "awFmParallelSearchCount": (None, [IP, LP, C.c_uint32]),
        "awFmFindSearchRangeForString": (AwFmSearchRange, [IP, C.c_char_p, C.c_size_t]),
        "awFmReadSequenceFromFile": (C.c_int, [IP, C.c_size_t, C.c_size_t, C.c_char_p]),
        "awFmCreateInitialQueryRange": (AwFmSearchRange, [IP, C.c_char_p, u64]),
        "awFmCreateInitialQueryRangeFromChar": (AwFmSearchRange, [IP, C.c_char]),
        "awFmNucleotideIterativeStepBackwardSearch": (None, [IP, RP, C.c_uint8]),
        "awFmAminoIterativeStepBackwardSearch": (None, [IP, RP, C.c_uint8]),
        "awFmFindDatabaseHitPositions": (C.POINTER(u64), [IP, RP, C.POINTER(C.c_int)]),
        "awFmFindDatabaseHitPositionSingle": (u64, [IP, u64, C.POINTER(C.c_int)]),
        "awFmNucleotideBacktraceReturnPreviousLetterIndex": (C.c_uint8, [IP, C.POINTER(u64)]),
        "awFmAminoBacktraceReturnPreviousLetterIndex": (C.c_uint8, [IP, C.POINTER(u64)]),
        "awFmGetLocalSequencePositionFromIndexPosition": (C.c_int, [IP, C.c_size_t, C.POINTER(C.c_size_t),
                                                                   C.POINTER(C.c_size_t)]),
        "awFmGetHeaderStringFromSequenceNumber": (C.c_int, [IP, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t)]),
        "awFmSearchRangeLength": (C.c_size_t, [RP]),
        "awFmReturnCodeIsFailure": (C.c_bool, [C.c_int]),
        "awFmReturnCodeIsSuccess": (C.c_bool, [C.c_int]),
        "awFmGetNumSequences": (C.c_uint32, [IP]),
        "awfmGpuDeviceCount": (C.c_int, []),
        "awfmGpuLastError": (C.c_char_p, []),
        "awfmGpuIndexCreate": (C.c_int, [IP, C.c_int, C.POINTER(vp)]),
        "awfmGpuIndexDestroy": (None, [vp]),
        "awfmGpuIndexAcquire": (vp, [IP]),
        "awfmGpuIndexAcquireAll": (C.c_int, [IP, C.POINTER(vp), C.c_int]),
        "awfmGpuIndexRelease": (None, [IP]),
        "awfmGpuIndexDeviceBytes": (u64, [vp]),
        "awfmGpuIndexDevice": (C.c_int, [vp]),
        "awfmGpuIndexSetKernel": (None, [vp, C.c_int]),
        "awfmGpuIndexSetWide": (None, [vp, C.c_int]),
        "awfmGpuIndexIsWide": (C.c_int, [vp]),
        "awfmGpuLastBatchStatus": (C.c_int, []),
        "awfmGpuIndexSetOrdered": (None, [vp, C.c_int]),
        "awfmGpuSearchHitsIsOrdered": (C.c_int, [vp, C.c_int, C.c_uint32, u64]),
        "awfmGpuLastOrderedKernelMs": (C.c_double, [vp]),
        "awfmGpuLastOrderedKernelIsLookup": (C.c_int, [vp]),
        "awfmGpuLastOrderedKept": (C.c_uint64, [vp]),
        "awfmGpuLastSecondWindow": (None, [vp, C.POINTER(C.c_uint64 * 2)]),
        "awfmGpuIndexSetDeepSeed": (C.c_int, [vp, C.c_uint]),
        "awfmGpuIndexSetDenseSa": (C.c_int, [vp, C.c_int]),
        "awfmGpuIndexSetPairImage": (C.c_int, [vp, C.c_int]),
        "awfmGpuIndexHasPairImage": (C.c_int, [vp]),
        "awfmGpuIndexDeepSeedK": (C.c_uint, [vp]),
        "awfmGpuIndexDeepSeedBuildSeconds": (C.c_double, [vp]),
        "awfmGpuIndexDeepSeedTransientBytes": (u64, [vp]),
        "awfmGpuIndexHasDenseSa": (C.c_int, [vp]),
        "awfmGpuIndexDenseSaBuildSeconds": (C.c_double, [vp]),
        "awfmGpuIndexLengthTableBytes": (u64, [vp]),
        "awfmGpuIndexLengthTableBuildSeconds": (C.c_double, [vp]),
        "awfmGpuMixedLookupLineTally": (C.c_int, [vp, vp, vp, u64, C.POINTER(u64 * 8)]),
        "awfmGpuSearch": (C.c_int, [vp, vp, vp, C.c_uint32, u64, vp, vp, vp]),
        "awfmGpuSearchHits": (C.c_int, [vp, vp, vp, C.c_uint32, u64, vp, vp, vp]),
        "awfmGpuSearchHitsSparse": (C.c_int, [vp, vp, vp, C.c_uint32, u64, vp, vp, vp]),
        "awfmGpuSearchHitsCompact": (C.c_int, [vp, vp, vp, C.c_uint32, u64, C.c_int, vp, vp, C.c_uint32, vp, vp]),
        "awfmGpuCompactHits": (C.c_int, [vp, vp, vp, u64, vp, vp, vp, vp, C.c_uint32, vp, vp]),
        "awfmGpuSearchHitsInOrder": (C.c_int, [vp, vp, vp, C.c_uint32, u64, C.c_int, vp, vp, vp]),
        "awfmGpuSearchHitsInOrderCounts": (C.c_int, [vp, vp, vp, C.c_uint32, u64, C.c_int, vp, vp, vp, vp]),
        "awfmGpuOrderBuckets": (C.c_uint32, [vp, C.c_uint32, u64]),
        "awfmGpuOrderKmers": (C.c_int, [vp, vp, C.c_uint32, u64, u64, u64, vp, vp, vp]),
        "awfmGpuSearchOrderedRecords": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, u64, vp, vp, vp]),
        "awfmGpuSearchOrderedRecordsCounts": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, u64, vp, vp, vp, vp]),
        "awfmGpuMergeBucketRuns": (C.c_int, [vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp]),
        "awfmGpuSearchGeneralRecords": (C.c_int, [vp, vp, C.c_uint32, u64, u64, u64, vp, vp, vp, vp, vp]),
        "awfmGpuSortHits": (C.c_int, [vp, vp, vp, C.c_uint32, vp]),
        "awfmGpuSortHitsOnDevice": (C.c_int, [vp, vp, vp, C.c_uint32, vp, u64, vp]),
        "awfmGpuListLocateOnDevice": (C.c_int, [vp, vp, vp, C.c_uint32, vp, u64, vp, vp, vp, u64, vp, vp]),
        "awfmGpuLastLookupFront": (C.c_int, [vp]),
        "awfmGpuLastSearchWasExactLookup": (C.c_int, [vp]),
        "awfmGpuStreamRetire": (None, [vp, vp]),
        "awfmGpuIndexDescribe": (C.c_int, [vp, C.c_char_p, C.c_int]),
        "awfmGpuIndexDeepSeedAllocSeconds": (C.c_double, [vp]),
        "awfmGpuAosLastStages": (None, [C.POINTER(C.c_double * 10)]),
        "awfmHostCopyGBs": (C.c_double, [C.c_uint32, u64]),
        "awfmGpuHitOffsetsOnDevice": (C.c_int, [vp, vp, vp, u64, vp, vp, vp]),
        "awfmGpuLocateOnDevice": (C.c_int, [vp, vp, vp, u64, u64, vp, vp]),
        "awfmGpuLastOrderedSearchKernelMs": (C.c_double, [vp]),
        "awfmGpuOrderedKernelLog": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int]),
        "awfmGpuScanScratchBytes": (u64, [u64]),
        "awfmGpuHitOffsets": (C.c_int, [vp, vp, u64, vp, vp, C.POINTER(u64), vp]),
        "awfmGpuHitOffsetsFromCounts": (C.c_int, [vp, vp, u64, vp, vp, C.POINTER(u64), vp]),
        "awfmGpuLocate": (C.c_int, [vp, vp, vp, u64, u64, vp, vp]),
        "awfmGpuLocateTo": (C.c_int, [vp, vp, vp, u64, u64, vp, vp, vp]),
        "awfmGpuLocateWindow": (C.c_int, [vp, vp, vp, u64, u64, u64, u64, vp, vp, vp]),
        "awfmGpuLocateHostWindows": (C.c_int, [vp, vp, vp, C.c_uint32, u64, vp, vp, HIT_WINDOW_SINK, vp]),
        "awfmGpuCountHost": (C.c_int, [vp, vp, vp, C.c_uint32, u64, vp, vp]),
        "awfmGpuLocateHost": (C.c_int, [vp, vp, vp, C.c_uint32, u64, vp, vp, C.POINTER(C.POINTER(u64))]),
        "awfmLocalPositions": (C.c_int, [IP, vp, u64, vp, vp, C.POINTER(u64), C.c_uint]),
        "awfmLongestSuffixMatches": (C.c_int, [IP, vp, vp, vp, C.c_uint32, u64, C.c_uint32, vp, vp, vp, C.c_uint]),
        "awfmGpuLongestSuffixMatches": (C.c_int, [vp, vp, vp, vp, C.c_uint32, u64, C.c_uint32, vp, vp, vp, vp]),
        "awfmOneSubstitutionSearch": (C.c_int, [IP, vp, vp, C.c_uint32, u64, C.c_int, vp, vp, vp, u64, vp, vp, vp, C.c_uint]),
        "awfmGpuOneSubstitutionSearch": (C.c_int, [vp, vp, vp, C.c_uint32, u64, C.c_int, vp, vp, vp, u64, vp, vp, vp, vp]),
        "awfmReadCandidates": (C.c_int, [C.POINTER(AwFmCandidateInputs), u64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.POINTER(AwFmCandidateOutputs), C.c_uint]),
        "awfmGpuReadCandidatesScratchBytes": (u64, [u64]),
        "awfmGpuReadCandidates": (C.c_int, [vp, C.POINTER(AwFmCandidateInputs), u64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                            C.POINTER(AwFmCandidateOutputs), vp, vp]),
        "awfmReadChains": (C.c_int, [C.POINTER(AwFmCandidateInputs), u64, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint32,
                                     C.c_uint32, C.POINTER(AwFmChainOutputs), C.c_uint]),
        "awfmGpuReadChainsScratchBytes": (u64, [u64]),
        "awfmGpuReadChains": (C.c_int, [vp, C.POINTER(AwFmCandidateInputs), u64, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint32,
                                        C.c_uint32, C.POINTER(AwFmChainOutputs), vp, vp]),
        "awfmGpuIndexSetText": (C.c_int, [vp, vp, u64]),
        "awfmGpuIndexTextLength": (u64, [vp]),
        "awfmTextWindows": (C.c_int, [vp, u64, vp, u64, C.c_uint32, C.c_uint32, vp, C.c_uint]),
        "awfmGpuTextWindows": (C.c_int, [vp, vp, u64, vp, C.c_uint32, C.c_uint32, vp, vp]),
        "awfmVerifyChains": (C.c_int, [C.POINTER(AwFmVerifyInputs), u64, C.c_uint32, C.c_uint32, C.c_uint32, vp, u64, vp, u64, C.c_int,
                                       C.POINTER(AwFmVerifyOutputs), C.c_uint]),
        "awfmGpuVerifyChains": (C.c_int, [vp, C.POINTER(AwFmVerifyInputs), u64, C.c_uint32, C.c_uint32, C.c_uint32,
                                          C.POINTER(AwFmVerifyOutputs), vp]),
        "awfmAlignChains": (C.c_int, [C.POINTER(AwFmVerifyInputs), vp, u64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, u64, vp, u64,
                                      C.c_int, C.POINTER(AwFmAlignOutputs), C.c_uint]),
        "awfmGpuAlignChainsScratchBytes": (u64, [vp, C.c_uint32]),
        "awfmGpuAlignChains": (C.c_int, [vp, C.POINTER(AwFmVerifyInputs), vp, u64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.POINTER(AwFmAlignOutputs), vp, vp]),
        "awfmAlignChainsAffine": (C.c_int, [C.POINTER(AwFmVerifyInputs), vp, u64, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(AwFmAlignScoring),
                                            C.c_uint32, vp, u64, vp, u64, C.c_int, C.POINTER(AwFmAffineOutputs), C.c_uint]),
        "awfmGpuAlignChainsAffineScratchBytes": (u64, [vp, C.c_uint32]),
        "awfmMatrixScoringUniform": (C.c_int, [C.c_int, C.POINTER(AwFmAlignScoring), C.POINTER(AwFmMatrixScoring)]),
        "awfmMatrixScoringFromText": (C.c_int, [C.c_int, vp, u64, C.c_uint32, C.c_uint32, C.POINTER(AwFmMatrixScoring)]),
        "awfmAlignChainsMatrix": (C.c_int, [C.POINTER(AwFmVerifyInputs), vp, u64, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(AwFmMatrixScoring),
                                            C.c_uint32, vp, u64, vp, u64, C.c_int, C.POINTER(AwFmAffineOutputs), C.c_uint]),
        "awfmGpuAlignChainsMatrix": (C.c_int, [vp, C.POINTER(AwFmVerifyInputs), vp, u64, C.c_uint32, C.c_uint32, C.c_uint32,
                                               C.POINTER(AwFmMatrixScoring), C.c_uint32, C.c_uint32, C.POINTER(AwFmAffineOutputs), vp, vp]),
        "awfmScoreChainsMatrix": (C.c_int, [C.POINTER(AwFmVerifyInputs), u64, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(AwFmMatrixScoring),
                                            C.c_uint32, C.c_uint32, vp, u64, vp, u64, C.c_int, C.POINTER(AwFmSlotScoreOutputs), C.c_uint]),
        "awfmGpuScoreChainsMatrix": (C.c_int, [vp, C.POINTER(AwFmVerifyInputs), u64, C.c_uint32, C.c_uint32, C.c_uint32,
                                               C.POINTER(AwFmMatrixScoring), C.c_uint32, C.c_uint32, C.POINTER(AwFmSlotScoreOutputs), vp]),
        "awfmAlignChainsEndBonus": (C.c_int, [C.POINTER(AwFmVerifyInputs), vp, u64, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(AwFmMatrixScoring),
                                              C.c_uint32, C.c_uint32, vp, u64, vp, u64, C.c_int, C.POINTER(AwFmAffineOutputs), C.c_uint]),
        "awfmGpuAlignChainsEndBonus": (C.c_int, [vp, C.POINTER(AwFmVerifyInputs), vp, u64, C.c_uint32, C.c_uint32, C.c_uint32,
                                                 C.POINTER(AwFmMatrixScoring), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(AwFmAffineOutputs),
                                                 vp, vp]),
        "awfmScoreChainsEndBonus": (C.c_int, [C.POINTER(AwFmVerifyInputs), u64, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(AwFmMatrixScoring),
                                              C.c_uint32, C.c_uint32, C.c_uint32, vp, u64, vp, u64, C.c_int, C.POINTER(AwFmSlotScoreOutputs),
                                              C.c_uint]),
        "awfmGpuScoreChainsEndBonus": (C.c_int, [vp, C.POINTER(AwFmVerifyInputs), u64, C.c_uint32, C.c_uint32, C.c_uint32,
                                                 C.POINTER(AwFmMatrixScoring), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(AwFmSlotScoreOutputs),
                                                 vp]),
        "awfmGpuAlignChainsAffine": (C.c_int, [vp, C.POINTER(AwFmVerifyInputs), vp, u64, C.c_uint32, C.c_uint32, C.c_uint32,
                                               C.POINTER(AwFmAlignScoring), C.c_uint32, C.c_uint32, C.POINTER(AwFmAffineOutputs), vp, vp]),
        "awfmScoreChainsAffine": (C.c_int, [C.POINTER(AwFmVerifyInputs), u64, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(AwFmAlignScoring),
                                            C.c_uint32, C.c_uint32, vp, u64, vp, u64, C.c_int, C.POINTER(AwFmSlotScoreOutputs), C.c_uint]),
        "awfmScoreWindowsAffine": (C.c_int, [C.POINTER(AwFmWindowInputs), u64, C.POINTER(AwFmAlignScoring), C.c_uint32, C.c_uint32, C.c_uint32,
                                             vp, u64, vp, u64, C.c_int, C.POINTER(AwFmWindowOutputs), C.c_uint]),
        "awfmGpuScoreWindowsAffineScratchBytes": (u64, [vp, C.c_uint32]),
        "awfmPairMates": (C.c_int, [C.POINTER(AwFmPairInputs), u64, C.c_uint32, C.POINTER(AwFmPairParams), C.POINTER(AwFmPairOutputs), C.c_uint]),
        "awfmGpuPairMates": (C.c_int, [vp, C.POINTER(AwFmPairInputs), u64, C.c_uint32, C.POINTER(AwFmPairParams), C.POINTER(AwFmPairOutputs), vp]),
        "awfmReverseComplementReads": (C.c_int, [vp, u64, vp, u64, C.c_uint32, vp, vp, C.c_uint]),
        "awfmInsertHistogram": (C.c_int, [C.POINTER(AwFmPairInputs), u64, C.c_uint32, C.POINTER(AwFmInsertParams), vp, vp, vp, C.c_uint]),
        "awfmGpuInsertHistogram": (C.c_int, [vp, C.POINTER(AwFmPairInputs), u64, C.c_uint32, C.POINTER(AwFmInsertParams), vp, vp, vp, vp]),
        "awfmInsertInterval": (C.c_int, [vp, C.POINTER(AwFmInsertParams), C.POINTER(AwFmInsertEstimate)]),
        "awfmAlignmentStrings": (C.c_int, [C.POINTER(AwFmStringInputs), u64, C.c_uint32, C.c_uint32, C.c_uint32, vp, u64, vp, u64, C.c_int,
                                           C.POINTER(AwFmStringOutputs), C.c_uint]),
        "awfmGpuAlignmentStringsScratchBytes": (u64, [vp, u64]),
        "awfmGpuAlignmentStrings": (C.c_int, [vp, C.POINTER(AwFmStringInputs), u64, C.c_uint32, C.c_uint32, C.c_uint32,
                                              C.POINTER(AwFmStringOutputs), vp, vp]),
        "awfmSamRecords": (C.c_int, [C.POINTER(AwFmSamInputs), u64, C.c_uint32, C.c_uint32, C.POINTER(AwFmSamOutputs), C.c_uint]),
        "awfmGpuSamRecordsScratchBytes": (u64, [vp, u64]),
        "awfmGpuSamRecords": (C.c_int, [vp, C.POINTER(AwFmSamInputs), u64, C.c_uint32, C.c_uint32, C.POINTER(AwFmSamOutputs), vp, vp]),
        "awfmRecordNames": (C.c_int, [IP, vp, vp, u64]),
        "awfmChooseStrands": (C.c_int, [C.POINTER(AwFmStrandInputs), u64, C.c_uint32, C.c_uint32, C.POINTER(AwFmPairParams),
                                        C.POINTER(AwFmStrandOutputs), C.c_uint]),
        "awfmGpuChooseStrands": (C.c_int, [vp, C.POINTER(AwFmStrandInputs), u64, C.c_uint32, C.c_uint32, C.POINTER(AwFmPairParams),
                                           C.POINTER(AwFmStrandOutputs), vp]),
        "awfmOrientReads": (C.c_int, [C.POINTER(AwFmOrientInputs), u64, C.c_uint32, C.POINTER(AwFmOrientOutputs), C.c_uint]),
        "awfmGpuOrientReads": (C.c_int, [vp, C.POINTER(AwFmOrientInputs), u64, C.c_uint32, C.POINTER(AwFmOrientOutputs), vp]),
        "awfmSamHeader": (u64, [IP, vp, u64]),
        "awfmGpuInsertInterval": (C.c_int, [vp, vp, C.POINTER(AwFmInsertParams), vp, vp]),
        "awfmGpuPairMatesEstimated": (C.c_int, [vp, C.POINTER(AwFmPairInputs), u64, C.c_uint32, C.POINTER(AwFmPairParams), vp,
                                                C.POINTER(AwFmPairOutputs), vp]),
        "awfmGpuReverseComplementReads": (C.c_int, [vp, vp, u64, vp, u64, C.c_uint32, vp, vp, vp]),
        "awfmGpuScoreWindowsAffine": (C.c_int, [vp, C.POINTER(AwFmWindowInputs), u64, C.POINTER(AwFmAlignScoring), C.c_uint32, C.c_uint32,
                                                C.c_uint32, C.c_uint32, C.POINTER(AwFmWindowOutputs), vp, vp]),
        "awfmGpuScoreChainsAffine": (C.c_int, [vp, C.POINTER(AwFmVerifyInputs), u64, C.c_uint32, C.c_uint32, C.c_uint32,
                                               C.POINTER(AwFmAlignScoring), C.c_uint32, C.c_uint32, C.POINTER(AwFmSlotScoreOutputs), vp]),
        "awfmGpuIndexSetRecordTable": (C.c_int, [vp, vp, u64]),
        "awfmGpuIndexNumRecords": (C.c_uint32, [vp]),
        "awfmGpuLocalPositions": (C.c_int, [vp, vp, u64, vp, vp, vp, vp, vp]),
        "awfmGpuLocateHostLocal": (C.c_int, [vp, vp, vp, C.c_uint32, u64, vp, vp, C.POINTER(C.POINTER(C.c_uint32)),
                                             C.POINTER(C.POINTER(u64)), C.POINTER(u64)]),
        "awfmGpuCreateIndex": (C.c_int, [C.POINTER(IP), C.POINTER(AwFmIndexConfiguration), vp, u64, C.c_int,
                                         C.c_char_p, C.c_int]),
        "awfmGpuSearchTally": (C.c_int, [vp, vp, vp, C.c_uint32, u64, C.POINTER(u64 * 4)]),
        "awfmGpuSearchHitsLineTally": (C.c_int, [vp, vp, vp, C.c_uint32, u64, C.POINTER(u64 * 8)]),
        "awfmGpuSynthText": (C.c_int, [vp, u64, u64, u64, C.c_int, vp]),
        "awfmGpuSynthRandomQueries": (C.c_int, [vp, u64, u64, C.c_uint32, u64, C.c_int, vp]),
        "awfmGpuSynthPlantedQueries": (C.c_int, [vp, u64, u64, C.c_uint32, u64, vp, u64, vp]),
        "awfmGpuSynthPlantedQueriesClean": (C.c_int, [vp, u64, u64, C.c_uint32, u64, vp, u64, vp]),
        "awfmGpuSynthPlantedQueriesUnique": (C.c_int, [vp, u64, u64, C.c_uint32, u64, vp, u64, u64, vp, vp]),
        "awfmGpuSynthGenomeText": (C.c_int, [vp, u64, u64, vp]),
        "awfmGpuSynthMixedLengths": (C.c_int, [vp, u64, u64, C.c_uint32, C.c_uint32, u64, vp]),
        "awfmGpuSynthMixedQueries": (C.c_int, [vp, vp, u64, u64, u64, vp, u64, C.c_int, vp]),
        "awfmPackKmers": (C.c_int, [C.c_int, vp, C.c_uint32, u64, vp, C.POINTER(u64)]),
        "awfmGpuPackKmers": (C.c_int, [vp, vp, C.c_uint32, u64, vp, C.POINTER(u64), vp]),
        "awfmGpuUnpackKmers": (C.c_int, [vp, vp, C.c_uint32, u64, vp, vp]),
        "awfmGpuSearchHitsPacked": (C.c_int, [vp, vp, C.c_uint32, u64, vp, vp, vp, vp]),
        "awfmGpuHostAlloc": (vp, [u64]),
        "awfmGpuHostFree": (None, [vp]),
        "awfmGpuStreamPacked": (C.c_int, [vp, vp, C.c_uint32, u64, u64, C.c_int, C.c_uint, CHUNK_SINK, vp]),
        "awfmGpuStreamChars": (C.c_int, [vp, vp, C.c_uint32, u64, u64, C.c_int, C.c_uint, CHUNK_SINK, vp]),
        "awfmGpuStreamPackedSparse": (C.c_int, [vp, vp, C.c_uint32, u64, u64, C.c_int, C.c_uint, SPARSE_CHUNK_SINK, vp]),
        "awfmGpuStreamCharsSparse": (C.c_int, [vp, vp, C.c_uint32, u64, u64, C.c_int, C.c_uint, SPARSE_CHUNK_SINK, vp]),
        "awfmGpuCountPackedHost": (C.c_int, [vp, vp, C.c_uint32, u64, vp]),
        "awfmGpuLocatePackedHost": (C.c_int, [vp, vp, C.c_uint32, u64, vp, C.POINTER(C.POINTER(u64)), C.POINTER(u64)]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    L.free = C.CDLL(None).free
    L.free.argtypes = [vp]
    L.free.restype = None
    _LIB = L
    return L
