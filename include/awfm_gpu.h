/*
 * awfm_gpu.h -- C ABI of the HIP (gfx950) side of libawfmindex_amd.so.
 *
 * This is the thin shim the host C code (and any FFI: ctypes, cgo, JNI ...)
 * calls.  Plain pointers and sizes only; `stream` arguments are hipStream_t
 * passed as void* (NULL = the null stream).  Pointers prefixed `d` are device
 * addresses (hipMalloc or any allocator that shares the HIP context, e.g. a
 * torch tensor's data_ptr()); all others are host addresses.
 *
 * What each entry point replaces in the reference:
 *   awfmGpuSearch          seed + extend phases of awFmParallelSearchCount /
 *                          awFmParallelSearchLocate
 *                          (ref src/AwFmParallelSearch.c:159-220, :222-313) on top of
 *                          the rank primitives (ref src/AwFmOccurrence.c:8-135,
 *                          src/AwFmSimdConfig.c:89-114, src/AwFmSearch.c:42-159,
 *                          :485-520, src/AwFmKmerTable.c:4-51)
 *   awfmGpuLongestSuffixMatches   the loop a seed-and-extend caller writes around
 *                          awFmCreateInitialQueryRangeFromChar and the iterative step
 *                          functions (ref src/AwFmSearch.c:27-159): step until the range
 *                          empties, keep the last range that had hits and its depth
 *   awfmGpuOneSubstitutionSearch  the same caller's next loop: the ranges of every string at Hamming
 *                          distance 1 of a k-mer, from the same two functions (ref src/AwFmSearch.c:27-159,
 *                          :317-358), without enumerating the 3m + 1 strings
 *   awfmGpuHitOffsets      the per-query sizing of setPositionListCount
 *                          (ref src/AwFmParallelSearch.c:327-328, :367-387) as
 *                          one exclusive scan
 *   awfmGpuLocate          parallelSearchTracebackPositionLists
 *                          (ref src/AwFmParallelSearch.c:315-365): LF walk
 *                          (ref src/AwFmSearch.c:369-427, src/AwFmOccurrence.c:170-217)
 *                          + sampled-SA read (ref src/AwFmSuffixArray.c:114-142, :179-191)
 *   awfmGpuCountHost /     the whole of awFmParallelSearchCount / ...Locate
 *   awfmGpuLocateHost      for host-resident flat query buffers
 *   awfmGpuIndexCreate     the reference has no analogue: it builds the
 *                          device image (re-laid-out BWT blocks, seed table,
 *                          sampled SA) of a host AwFmIndex.
 *
 * Results are bit-identical to the reference semantics:
 * a query stops at the first invalid range and keeps it; hits are listed in
 * BWT order sp, sp+1, ..., ep.
 */
#ifndef AWFM_GPU_H
#define AWFM_GPU_H

#include "AwFmIndex.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct AwFmGpuIndex AwFmGpuIndex; /* opaque device image of one index on one GPU */

/* search kernel variants: how many lanes cooperate on one query (AUTO picks the default) */
enum AwFmGpuKernel {
  AWFM_GPU_KERNEL_AUTO = 0,
  AWFM_GPU_KERNEL_GROUP8 = 1, /* 8 lanes x 16 B: one load instruction per 128-B block, 8 queries per wave */
  AWFM_GPU_KERNEL_GROUP4 = 2, /* 4 lanes x 32 B, 16 queries per wave */
  AWFM_GPU_KERNEL_GROUP2 = 3, /* 2 lanes x 64 B, 32 queries per wave (nucleotide only) */
  AWFM_GPU_KERNEL_GROUP1 = 4  /* 1 lane x 128 B, 64 queries per wave (nucleotide only) */
};

/* ---- runtime ---- */
int awfmGpuDeviceCount(void);           /* 0 when no usable HIP device */
const char *awfmGpuLastError(void);     /* thread-local text of the last failure, "" if none */
/* Return code of the calling thread's last awFmParallelSearchCount / awFmParallelSearchLocate.  Count returns void in
 * the reference API (ref src/AwFmIndex.h:400-403) and there is no CPU search path here, so a failed call (no device,
 * allocation or kernel failure) sets the `count` of every k-mer of the failed shard(s) to 0, prints the reason to
 * stderr, and leaves its code here. */
enum AwFmReturnCode awfmGpuLastBatchStatus(void);

/* ---- environment ----
 * The library reads 20 variables, all through csrc/awfm_knobs.h (INTEGRATION.md section 7 explains each); none changes a
 * result.  $AWFM_GPU_DIAG = "key=value,key=value,..." holds the test and diagnostics hooks, none of which selects a faster path:
 *   walk_give_up=N      LF steps after which an ordinary locate's walk is parked for finishKernel to walk on
 *   park_list=N         capacity of the full-suffix-array builder's list of parked walks (0: an entry per position)
 *   build_wide=1        the GPU builder's 64-bit suffix sort on any text
 *   kernel=g1|g2|g4     lanes per k-mer of the general kernel (awfmGpuIndexSetKernel does the same per image)
 *   tally_with_deep=1   awfmGpuSearchTally starts from the deeper table (default: the index's own, the reference's bytes)
 *   nuc_super_shift=13..31|auto   nucleotide superblocks of 2^shift positions: the arithmetic of images of 2^32 positions
 *                       and more on small ones
 *   record_lookup=lds|dir   which lookup a record table gets when it is installed (default: by its size; lds only where it fits)
 *   candidates_tier=wave|group   awfmGpuReadCandidates: group sends every read with a kept hit to the workgroup tier; wave is the
 *                       default (a read of up to 256 kept hits takes the wave tier) and changes nothing
 *   chains_tier=wave|group   awfmGpuReadChains: group sends every read with an anchor to the workgroup tier; wave is the default
 *                       (a read of up to 256 anchors takes the wave tier) and changes nothing
 *   verify_group=16|32|64   awfmGpuVerifyChains: lanes per slot, where that is more than the band's diagonals need (a smaller
 *                       value than the band needs is ignored); the default is the smallest that holds the band
 *   align_group=16|32|64    awfmGpuAlignChains: lanes per read, in the same way
 *   affine_group=32|64      awfmGpuAlignChainsAffine, awfmGpuAlignChainsMatrix, awfmGpuAlignChainsEndBonus: lanes per read, in the
 *                       same way
 *   score_group=32|64       awfmGpuScoreChainsAffine, awfmGpuScoreChainsMatrix, awfmGpuScoreChainsEndBonus: lanes per slot, in the
 *                       same way
 *   window_q=4|8|12         awfmGpuScoreWindowsAffine: columns per lane for every read (narrower column blocks)
 *   pair_group=64           awfmGpuPairMates: a wave per pair also where 16 lanes hold the candidates
 *   strand_group=64         awfmGpuChooseStrands: a wave per pair or per read also where 32 or 16 lanes hold the strand slots
 *   insert_tier=global      awfmGpuInsertHistogram: global atomics at any bin count (default: a private histogram in LDS per
 *                       workgroup up to 8192 bins)
 *   strings_tier=direct     awfmGpuAlignmentStrings: every wave stores its strings read by read in bytes (default: a span that
 *                       fits the LDS tile is formatted there and stored in dwords)
 *   sam_tier=direct         awfmGpuSamRecords: every wave stores its line straight into the arena (default: a line that fits the
 *                       LDS tile is built there and stored in dwords)
 *   second_window=0|1   the lookup kernel's second table window (a survivor's leftmost characters): 0 never, 1 on every trip;
 *                       unset, the kernel's own gate decides trip by trip (the results are the same either way)
 *   stream_trace=1, aos_trace=1  host timelines of the chunked pipelines / the AoS lanes on stderr */

/* ---- device image ---- */
/* Builds the device image of `index` on GPU `device` (-1: current device or
 * $AWFM_GPU_DEVICE).  When the index has no in-memory sampled SA
 * (keepSuffixArrayInMemory == false) it is staged from index->fileDescriptor.  The image is complete when the call returns:
 * its device-only accelerators (deeper seed table, full suffix array: below) are built before it does. */
enum AwFmReturnCode awfmGpuIndexCreate(const struct AwFmIndex *index, int device, AwFmGpuIndex **out);
void awfmGpuIndexDestroy(AwFmGpuIndex *g);
/* Side table used by awFmParallelSearch*: image for a host index, created on first use.  Round 6: the image the drop-in entry
 * points make (awfmGpuIndexAcquireAll) is usable as soon as its blocks, pair image and copied tables are on the device; its
 * deeper table and full suffix array are built by a thread of their own, on a stream of their own, and installed between two
 * calls of the entry points -- the first awFmParallelSearchLocate on a GRCh38-sized index returns after 0.2 s instead of 0.9-7 s,
 * and searches issued meanwhile run on what is there (same results).  awfmGpuIndexAcquire hands over the COMPLETE image: it
 * waits for that thread. */
AwFmGpuIndex *awfmGpuIndexAcquire(const struct AwFmIndex *index);
/* Handles on the device images of a host index for every entry of $AWFM_GPU_DEVICES ("all" or a comma list of
 * ordinals), created on first use; awFmParallelSearch* deal the chunks of a list to them, one host thread each.  A device
 * named again gets a lane: a handle with its own staging buffers and locks on the image that device already
 * has (no second copy of the index), so that its chunks overlap the others' transfers and kernels.  Unset:
 * the default device with three lanes.  Returns how many handles were written to out[0..maxOut). */
int awfmGpuIndexAcquireAll(const struct AwFmIndex *index, AwFmGpuIndex **out, int maxOut);
/* Drops the side-table entries of the index (called by awFmDeallocIndex). */
void awfmGpuIndexRelease(const struct AwFmIndex *index);
uint64_t awfmGpuIndexDeviceBytes(const AwFmGpuIndex *g);
int awfmGpuIndexDevice(const AwFmGpuIndex *g);
/* Optional, nucleotide images: builds a device-only seed table of depth deepK (seedK < deepK <= 16,
 * 4^deepK x 8 bytes of HBM on images below 2^32 positions -- {sp, length}: 2.1 GB at 14, 34 GB at 16 -- and 16 bytes
 * {sp, ep} beyond) whose entries equal what the reference algorithm
 * reaches after the seed lookup plus deepK-seedK extension steps (stopping at the first invalid range), so
 * results stay bit-identical while those steps' block reads disappear.  deepK = 0 drops it.  The host
 * index, its seed table and the .awfmi file are untouched.  When an image is created: $AWFM_GPU_DEEP_SEED_K (0: none)
 * if set; otherwise images of 2^28 positions and more whose own table is shallower get depth 14 when four times the
 * table's 4.3 GB are free on the device. */
enum AwFmReturnCode awfmGpuIndexSetDeepSeed(AwFmGpuIndex *g, unsigned deepK);
unsigned awfmGpuIndexDeepSeedK(const AwFmGpuIndex *g); /* depth of the deeper table the image has, 0: none */
/* reporting: wall seconds the construction of that table took (levels + next-step bits; whoever built it: the automatic
 * choice at awfmGpuIndexCreate / Acquire, or awfmGpuIndexSetDeepSeed), and the device memory the construction held
 * beyond the table itself at its peak (the level below the deepest, 16 B x 4^(k-1)) */
double awfmGpuIndexDeepSeedBuildSeconds(const AwFmGpuIndex *g);
/* ... of which spent inside hipMalloc (a process's first allocation of tens of GB can take seconds on some boxes: device
 * memory handed back from, or scrubbed after, the process before -- not the construction) */
double awfmGpuIndexDeepSeedAllocSeconds(const AwFmGpuIndex *g);
uint64_t awfmGpuIndexDeepSeedTransientBytes(const AwFmGpuIndex *g);
/* The full suffix array on the device (32-bit entries, 4 x bwtLength bytes: 12.4 GB for a GRCh38-sized index),
 * reconstructed once from the sampled SA with the LF-walk kernel (walks capped at 32 x ratio steps; the ones that have
 * not met a sample by then -- positions inside long runs of one letter -- are completed from each other by pointer jumping),
 * so that locating a hit is one read instead of a chain of about ratio-1 dependent block reads.  Positions are bit-identical (the walk wrote them).  Built by default for
 * images of 2^26 .. 2^32 positions with a sampled array when four times its size is free on the device
 * ($AWFM_GPU_DENSE_SA=0|1: never / always); enable = 0 drops it, 1 builds it.  Needs bwtLength < 2^32. */
enum AwFmReturnCode awfmGpuIndexSetDenseSa(AwFmGpuIndex *g, int enable);
int awfmGpuIndexHasDenseSa(const AwFmGpuIndex *g);
/* One line of text about what the image holds: its size, which of the optional accelerators it has (pair image, deeper table
 * and its depth, full suffix array, tables per k-mer length) and which ones its size asked for and it did NOT get, with the
 * reason (every one of them is dropped silently when device memory is short: the searches run without it, results are the
 * same).  Returns the length of the whole text; at most outBytes - 1 characters and a 0 are written. */
int awfmGpuIndexDescribe(const AwFmGpuIndex *g, char *out, int outBytes);
double awfmGpuIndexDenseSaBuildSeconds(const AwFmGpuIndex *g); /* reporting: wall seconds of the automatic construction */
/* Device-only tables per k-mer length (nucleotide images below 2^32 positions with the narrow deeper table of depth D): for
 * every length d = 1 .. D-1 the 8-byte entry {first position, length} of the range of EVERY d-letter string -- what the
 * reference reaches for a k-mer of exactly d characters (ref src/AwFmSearch.c:485-520 below the seed table's length,
 * src/AwFmKmerTable.c:4-51 at it, src/AwFmParallelSearch.c:273-313 above it) -- (4^D - 4) / 3 entries, 11.5 GB for D = 16.
 * Built on the device by the first mixed-length batch (CSR offsets) that takes the lookup-first kernel
 * ($AWFM_GPU_MIXED_LOOKUP=0: never), kept with the image; bytes / wall seconds of that construction (0: none yet).
 * THAT ONE CALL IS NOT ASYNCHRONOUS: the tables are built on the null stream and the call waits for the device (0.02 s for
 * D = 16) before it launches its search on the caller's stream; they are built only when three times their size is free on
 * the device, and a construction that found no room is tried again 64 mixed-length searches later. */
uint64_t awfmGpuIndexLengthTableBytes(const AwFmGpuIndex *g);
double awfmGpuIndexLengthTableBuildSeconds(const AwFmGpuIndex *g);
/* Nucleotide images carry, beside the one-letter blocks, a pair image: for every BWT position the pair of its two
 * preceding text characters, in 128-byte blocks of 128 positions with 16 base counts, so that two backward steps (two
 * LF steps) are one rank over a 16-letter sequence and one block read (csrc/awfm_pair.h).  The searches and the LF
 * walk of awfmGpuLocate use it; results are those of the letter-by-letter steps (ref src/AwFmSearch.c:42-103,
 * :369-427), bit for bit -- awfmGpuSearch's final range of a k-mer without hits included (a k-mer that dies inside a
 * pair step gets the range of the single step that emptied it).  Built with every nucleotide image unless
 * $AWFM_GPU_PAIR=0; enable = 0 drops it (the image then takes one step per read), enable != 0 rebuilds it.  It adds
 * 1 byte per BWT position of device memory; the host index and the .awfmi file are untouched. */
enum AwFmReturnCode awfmGpuIndexSetPairImage(AwFmGpuIndex *g, int enable);
int awfmGpuIndexHasPairImage(const AwFmGpuIndex *g);
/* ---- sequence coordinates: global text position -> (sequence number, position in that sequence) ----
 * The batch forms of awFmGetLocalSequencePositionFromIndexPosition (ref src/AwFmSearch.c:284-301), one definition on both
 * sides: with the records' ends E[0..R) (sequenceEndPosition: terminator excluded) and starts S[0] = 0, S[r] = E[r-1] + 1, a
 * position p belongs to the first record r with E[r] > p, provided p >= S[r]; its local position is p - S[r].  Any other p -- a
 * record's terminator, or anything from E[R-1] on, the sentinel included -- is ILLEGAL: it gets sequence number 0xFFFFFFFF,
 * keeps its global position, is counted, and the batch carries on (ordinary searches reach such positions: terminators are
 * stored as the ambiguity letter, so a query of ambiguity letters hits them).  Empty records own no position.  Only a hit's
 * start is mapped, as in the reference: a k-mer's length plays no part.
 *
 * awfmLocalPositions: on the host, over `threads` threads of the library's pool (a binary search per position: 10^8 positions
 * take 0.16-0.17 s against 640 records and 0.7-0.8 s against 5.7 * 10^5 on 16 threads); what callers of the AoS entry points run on a positionList, and the checker of the
 * device calls.  localPositions may be `positions`.  AwFmUnsupportedVersionError, nothing written, when the index has no
 * record table (it was not made from a FASTA file). */
enum AwFmReturnCode awfmLocalPositions(const struct AwFmIndex *index, const uint64_t *positions, uint64_t numPositions,
                                       uint32_t *sequenceNumbers, uint64_t *localPositions, uint64_t *numIllegalOut,
                                       unsigned threads);
/* The record table of a device image: the records' ends (8 bytes each) and a directory over the positions (4 bytes per bucket;
 * about as many buckets as records, at most 4096 for a table small enough to be looked up from LDS), counted in
 * awfmGpuIndexDeviceBytes and named by awfmGpuIndexDescribe.  An image made from an index that has records (awFmCreateIndexFromFasta
 * on either builder, awFmReadIndexFromFile of such a file) gets it with its blocks.  awfmGpuIndexSetRecordTable installs or
 * replaces it from the caller's array of ends (host; numRecords == 0 drops it) -- for an index made by awFmCreateIndex /
 * awfmGpuCreateIndex from a text the caller concatenated with its own terminators.  The ends must increase (E[r] > E[r-1]) and
 * may lie at and beyond 2^32 whatever the image's width.  Cost: one upload of the table; it waits for the searches on the image
 * like every other change of it, and mapping calls already enqueued finish on the table they were enqueued with.  Refused
 * (AwFmIllegalPositionError) tables leave the old one in place. */
enum AwFmReturnCode awfmGpuIndexSetRecordTable(AwFmGpuIndex *g, const uint64_t *sequenceEndPositions, uint64_t numRecords);
uint32_t awfmGpuIndexNumRecords(const AwFmGpuIndex *g); /* 0: the image has no record table */
/* Selects the search kernel variant for this image (default AUTO). */
void awfmGpuIndexSetKernel(AwFmGpuIndex *g, enum AwFmGpuKernel kernel);
/* The kernels keep BWT positions in 32 bits whenever bwtLength < 2^32 and in 64 bits otherwise (the reference is
 * 64-bit throughout: ref src/AwFmIndex.h:88-91, src/AwFmSuffixArray.c:114-142).  wide != 0 selects the 64-bit
 * instantiations on any image -- same results, used by the parity tests to cover the code indices of 2^32 or more
 * positions run; also read from $AWFM_GPU_FORCE_WIDE when an image is created. */
void awfmGpuIndexSetWide(AwFmGpuIndex *g, int wide);
int awfmGpuIndexIsWide(const AwFmGpuIndex *g); /* 1 when searches on this image run the 64-bit instantiations */

/* ---- index construction on the GPU ---- */
/* Same contract and byte-identical arrays as awFmCreateIndex (ref src/AwFmCreate.c:31-137), built on
 * the device: suffix sort (radix + prefix doubling), BWT bit planes, base counts, seed table, sampled
 * SA.  `sequence` is a host pointer, or a device pointer when sequenceOnDevice != 0.  fileSrc may be
 * NULL (no .awfmi file is written; an extension over the reference).  The device image stays
 * resident and is the one awFmParallelSearch* will use.  Suffix positions and ranks are 32-bit on the device while
 * bwtLength <= 2^32-2 (about 25 bytes of HBM per position at the peak) and 64-bit beyond (about 37 bytes per
 * position: a 4.4 Gbp text builds in 12 s, a two-strand human genome of 6.2 Gbp fits one MI355X);
 * $AWFM_GPU_DIAG build_wide=1 selects the 64-bit suffix sort on any text (tests). */
enum AwFmReturnCode awfmGpuCreateIndex(struct AwFmIndex **index, const struct AwFmIndexConfiguration *config,
                                       const uint8_t *sequence, uint64_t sequenceLength, int sequenceOnDevice,
                                       const char *fileSrc, int device);

/* ---- flat batch API on device buffers ---- */
/* Queries: dChars = concatenated ASCII k-mers; either dOffsets (numQueries+1
 * CSR offsets into dChars) or, with dOffsets == NULL, fixedLength characters
 * per query.  Outputs (each may be NULL): dRanges[numQueries] = final {sp,ep},
 * dCounts[numQueries] = range length truncated to u32
 * (ref src/AwFmIndexStruct.c:126-130).  Asynchronous on `stream`; allocates no table: large batches read the image's
 * device-only tables where it has them (the deeper table; the tables per k-mer length once a hits-only mixed-length batch
 * has built them), and scratch of 8 bytes per k-mer in one of the image's two slots.
 *
 * Which letter a byte is: ref src/AwFmLetter.c over all 256 values (tests/byte_values_common.py states the classes).  An amino
 * byte that is no letter and no ambiguity letter either (j, o, u, '@', NUL, ...: 90 values of letter index 20 that
 * awFmLetterIsAmbiguous lets pass) goes through the index's k-mer table as in the reference: its digit 20 carries into the
 * next digit of the table index (ref src/AwFmKmerTable.c:37-51) and the k-mer starts from the entry that index names.  Where
 * the index so computed is NOT BELOW THE TABLE'S LENGTH (the seed's leading digits are 19 .. 19, 20) the reference reads past
 * its table; the product defines the result as the plain letter-by-letter backward search of the whole k-mer (ref
 * src/AwFmSearch.c:317-358: awFmFindSearchRangeForString), final range included.  The device-only tables are never entered
 * with such a byte among their characters: those k-mers start from the index's own table.  A byte of the sentinel's letter
 * index ('$'; nucleotide 0x04 too) in a query is not defined. */
enum AwFmReturnCode awfmGpuSearch(AwFmGpuIndex *g, const uint8_t *dChars, const uint64_t *dOffsets,
                                  uint32_t fixedLength, uint64_t numQueries, struct AwFmSearchRange *dRanges,
                                  uint32_t *dCounts, void *stream);

/* ---- longest suffix match: how much of a query matches, and where ----
 * The batch form of the walk a caller of the reference's step functions writes by hand (ref src/AwFmIndex.h:477-512): with the
 * library's own letter mapping, r_1 = awFmCreateInitialQueryRangeFromChar(q[m-1]) and r_(l+1) = one backward step of r_l with the
 * letter of q[m-1-l].  The MATCH LENGTH of q[0..m) is the largest l <= m for which r_1 .. r_l are all non-empty (0 when m = 0 or
 * r_1 is empty), the MATCH RANGE is r_l, or {1, 0} when l = 0: the longest suffix of the query that occurs in the text and the
 * BWT interval of its occurrences.  No table, pair image or position width changes an answer.
 *
 * Query i is chars[starts[i] .. ends[i]) (ends[i] <= starts[i]: empty): two arrays, so that queries may overlap -- "the match
 * ending at every 4th position of this read, at most 64 characters long" is a list of (start, end) into the read buffer.  A CSR
 * caller passes offsets and offsets + 1; both NULL: fixedLength characters per query.  Of a query longer than 2^32 - 1
 * characters the last 2^32 - 1 are walked.  minLength (0: none): a query whose match is shorter than max(minLength, 1) gets
 * count 0 and the range {1, 0}, so that awfmGpuHitOffsets / awfmGpuHitOffsetsFromCounts / awfmGpuLocate* skip it; the match
 * length written is the true one either way.  Each output may be NULL; counts[i] = range length truncated to u32.
 *
 * awfmLongestSuffixMatches: the definition, letter by letter on the host over `threads` threads of the library's pool; the
 * checker of the device call.
 * awfmGpuLongestSuffixMatches: one asynchronous kernel on `stream`, no host wait, no allocation and no scratch (csrc/
 * awfm_match_kernel.h).  It starts from the deeper table or the index's own where the entry of the query's last letters is
 * non-empty (an empty entry says only that the match is shorter: the walk then starts from r_1), takes two letters per block
 * read through the pair image, and re-fills its 32-character register window as the walk moves left.  It reads dChars only in
 * aligned 4-byte words that hold at least one byte of the query they are read for: nothing outside an allocation that holds
 * the queries.  numQueries == 0 succeeds and touches nothing. */
enum AwFmReturnCode awfmLongestSuffixMatches(const struct AwFmIndex *index, const uint8_t *chars, const uint64_t *starts,
                                             const uint64_t *ends, uint32_t fixedLength, uint64_t numQueries, uint32_t minLength,
                                             uint32_t *matchLengths, struct AwFmSearchRange *ranges, uint32_t *counts,
                                             unsigned threads);
enum AwFmReturnCode awfmGpuLongestSuffixMatches(AwFmGpuIndex *g, const uint8_t *dChars, const uint64_t *dStarts,
                                                const uint64_t *dEnds, uint32_t fixedLength, uint64_t numQueries,
                                                uint32_t minLength, uint32_t *dMatchLengths, struct AwFmSearchRange *dRanges,
                                                uint32_t *dCounts, void *stream);

/* ---- one substitution: every string at Hamming distance 1 of a query that occurs, and where ----
 * PROPER LETTERS are the letter indices 0 .. sigma-1 of the library's mapping (awfmNucAsciiToIndex / awfmAminoAsciiToIndex):
 * sigma = 4 for nucleotide, 20 for amino.  For a query q[0..m) the VARIANT (p, c) is q with position p replaced by the proper
 * letter c, where c differs from the letter index of q[p] (q[p] an ambiguity letter: all sigma letters qualify).  The RANGE of a
 * string s, R(s), is what awFmFindSearchRangeForString computes: awFmCreateInitialQueryRangeFromChar of its last character,
 * then one backward step per character leftwards until the range is empty.  A non-empty R(s) is unique: no table, pair image
 * or position width changes a result.  A RECORD {query number, edit, range} exists for every variant with a non-empty R, and,
 * with includeExact != 0, for q itself when R(q) is non-empty.  edit = p * 32 + c for a variant and AWFM_EDIT_NONE for the
 * unedited query.  Positions p >= 2^27 are NOT substituted (the edit has 27 bits for p); ambiguity letters elsewhere in q step
 * like any letter, as in awfmGpuSearch; m = 0 gives no records, and so does a query of more than 2^32 - 1 characters.
 *
 * Queries as awfmGpuSearch takes them: offsets[numQueries + 1] into chars, or, offsets NULL, fixedLength characters each.  The
 * records are three parallel arrays (hitQueries, hitEdits, hitRanges) of `capacity` entries; *numHits is the TRUE number of
 * records and may exceed capacity.  variantsPerQuery[i] = the records of query i, occurrencesPerQuery[i] = the sum of their
 * range lengths: both complete whatever the capacity.  Every output may be NULL (capacity 0 with NULL lists: counts only).
 * numQueries == 0 succeeds and touches nothing; numQueries >= 2^32 is refused (AwFmIllegalPositionError: query numbers are
 * 32-bit); missing chars, or neither offsets nor a fixedLength: AwFmNullPtrError.
 *
 * awfmOneSubstitutionSearch: the definition, letter by letter on the host over `threads` threads of the library's pool, no
 * table.  Records sorted by (query, edit) -- the unedited query last among its own --; beyond capacity the first `capacity`
 * records of that order are stored.
 * awfmGpuOneSubstitutionSearch (csrc/awfm_subst_kernel.h): asynchronous on `stream`, no host wait, no allocation, none of the
 * handle's scratch slots: two streams may run it on one image at the same time.  Before the kernel runs the lists are filled up
 * to capacity with {0xFFFFFFFF, 0xFFFFFFFF, {1, 0}} and *dNumHits is zeroed, so that the list AT ITS CAPACITY goes straight into
 * awfmGpuHitOffsetsOnDevice(g, NULL, dHitRanges, capacity, ...) and awfmGpuLocateOnDevice: positions per record, dHitQueries /
 * dHitEdits say whose.  The order of the list is whatever order the waves append in; beyond capacity SOME capacity distinct
 * records of the true set are stored.  WHERE THE DEVICE CALL DIFFERS FROM THE HOST'S: the host fills any one list alone, numHits
 * NULL or not; the device appends through the counter *dNumHits (it allocates nothing, so it has no counter of its own), and a
 * call with a non-zero capacity and any list but without dNumHits is refused (AwFmNullPtrError).  Every other output may be NULL
 * on both sides.  One branch step gives the ranges of all sigma letters from one pair of block reads; a substitution
 * inside the span of the deeper table (or the index's own) costs one gather of the variant's entry.  With awfmGpuIndexSetKernel
 * set to anything but AUTO or GROUP4 the kernel runs letter by letter and reads no table.  dChars is read only in aligned
 * 4-byte words that hold at least one byte of the query they are read for. */
#define AWFM_EDIT_NONE 0xFFFFFFFFu
enum AwFmReturnCode awfmOneSubstitutionSearch(const struct AwFmIndex *index, const uint8_t *chars, const uint64_t *offsets,
                                              uint32_t fixedLength, uint64_t numQueries, int includeExact, uint32_t *hitQueries,
                                              uint32_t *hitEdits, struct AwFmSearchRange *hitRanges, uint64_t capacity,
                                              uint64_t *numHits, uint32_t *variantsPerQuery, uint64_t *occurrencesPerQuery,
                                              unsigned threads);
enum AwFmReturnCode awfmGpuOneSubstitutionSearch(AwFmGpuIndex *g, const uint8_t *dChars, const uint64_t *dOffsets,
                                                 uint32_t fixedLength, uint64_t numQueries, int includeExact,
                                                 uint32_t *dHitQueries, uint32_t *dHitEdits, struct AwFmSearchRange *dHitRanges,
                                                 uint64_t capacity, uint64_t *dNumHits, uint32_t *dVariantsPerQuery,
                                                 uint64_t *dOccurrencesPerQuery, void *stream);

/* Hits-only variant of awfmGpuSearch, for callers that go on to count or locate (what
 * awFmParallelSearchCount/Locate report: ref src/AwFmParallelSearch.c:159-220, :315-365): queries with hits get
 * exactly the range and count awfmGpuSearch gives them; a query WITHOUT hits gets count 0 and some empty range
 * (sp > ep), not necessarily the one the stepping ended in.  That freedom lets large nucleotide batches (>= 2^23
 * k-mers against >= 2^28 positions, fixed length or CSR; $AWFM_GPU_ORDERED=0|1 or awfmGpuIndexSetOrdered override)
 * be searched in seed order: the k-mers are packed into 8- or 16-byte records, partitioned by the leading bits of the
 * string their search starts from, searched in that order so that neighbouring queries read neighbouring blocks out of
 * the L2, and only the non-empty results are stored under their query numbers over a "no hit" fill.
 * Other batches run awfmGpuSearch.  Scratch: 16-36 bytes per query, owned by the image and re-used; searches on one
 * image are ordered across streams.  Every launch is asynchronous on `stream`: a fixed-length ASCII batch of >= 2^20
 * k-mers that starts from the deeper table is sampled first (awfmGpuLastOrderedKernelIsLookup below), and the sample's
 * verdict stays on the device -- the kernels of both front ends are launched and the one it does not choose returns at
 * once ($AWFM_GPU_LOOKUP_FIRST=0|1: no sample). */
enum AwFmReturnCode awfmGpuSearchHits(AwFmGpuIndex *g, const uint8_t *dChars, const uint64_t *dOffsets,
                                      uint32_t fixedLength, uint64_t numQueries, struct AwFmSearchRange *dRanges,
                                      uint32_t *dCounts, void *stream);
/* The same when the caller reads the ranges through the counts, as awfmGpuHitOffsetsFromCounts + awfmGpuLocate do:
 * dCounts[i] (required) is written for every k-mer, dRanges[i] for the k-mers with hits -- the range of a k-mer with
 * dCounts[i] == 0 may be left as the caller passed it (the seed-order path then streams 4 instead of 20 bytes of
 * "no hit" per k-mer over the outputs).  Hit offsets must then come from the counts (awfmGpuHitOffsets reads every
 * range), i.e. from images below 2^32 positions. */
enum AwFmReturnCode awfmGpuSearchHitsSparse(AwFmGpuIndex *g, const uint8_t *dChars, const uint64_t *dOffsets,
                                            uint32_t fixedLength, uint64_t numQueries, struct AwFmSearchRange *dRanges,
                                            uint32_t *dCounts, void *stream);
/* Sparse results: the k-mers with hits as a list instead of a range / count under every query number -- for batches in
 * which few k-mers occur (10^8 random 21-mers against a human-sized text: 7 * 10^4), where writing, scanning and moving
 * 10^8 "no hit" records is most of what happens after the search.  Only batches that take the seed-order path
 * (awfmGpuSearchHitsIsOrdered; AwFmUnsupportedVersionError otherwise -- run awfmGpuSearchHits + awfmGpuCompactHits then).
 * dHitKmers[capacity] / dHitRanges[capacity] are first filled with {0xFFFFFFFF, empty range}; every k-mer with hits then
 * appends {its number in the batch, its range} (order: as the waves come); *dNumHits (device) = how many there are, which
 * may exceed capacity -- the list is then incomplete and the caller repeats densely (a dense batch should not be searched
 * this way in the first place: its appends contend for one counter; capacity = numQueries / 64 keeps a mistaken attempt
 * cheap).  `packed`: dChars is one 64-bit word per k-mer (awfmGpuSearchHitsPacked).  awfmGpuSortHits orders the list by
 * k-mer number (entries beyond the hits sort last); awfmGpuHitOffsets / awfmGpuLocate then take the list as if it were
 * the batch (numQueries = capacity or the number of hits). */
enum AwFmReturnCode awfmGpuSearchHitsCompact(AwFmGpuIndex *g, const uint8_t *dChars, const uint64_t *dOffsets,
                                             uint32_t fixedLength, uint64_t numQueries, int packed, uint32_t *dHitKmers,
                                             struct AwFmSearchRange *dHitRanges, uint32_t capacity, uint32_t *dNumHits,
                                             void *stream);
/* Results IN SEARCH ORDER, for batches in which most k-mers have hits: entry q = {number of the k-mer the seed-order search
 * took q-th, its range (exact when it has hits, empty otherwise)}, every k-mer of the batch exactly once, written as whole
 * lines -- instead of 10^8 partial-line stores under the original k-mer numbers.  awfmGpuHitOffsets / awfmGpuLocate take
 * dOrderRanges as if it were the batch: hit offsets and positions then follow the search order too (neighbouring entries
 * are neighbours in the BWT, which the walk's first steps share), and dOrderKmers says whose they are -- what a consumer
 * that scatters into per-k-mer lists anyway (awFmParallelSearchLocate does: ref src/AwFmParallelSearch.c:327-361) needs.
 * Only batches that take the seed-order path (AwFmUnsupportedVersionError otherwise). */
enum AwFmReturnCode awfmGpuSearchHitsInOrder(AwFmGpuIndex *g, const uint8_t *dChars, const uint64_t *dOffsets,
                                             uint32_t fixedLength, uint64_t numQueries, int packed, uint32_t *dOrderKmers,
                                             struct AwFmSearchRange *dOrderRanges, void *stream);
/* the same with the 32-bit counts in that order as well (dOrderCounts, may be NULL; ref src/AwFmIndexStruct.c:126-130: the
 * list's count is a u32): awfmGpuHitOffsetsOnDevice then scans 4 instead of 16 bytes per k-mer (round 6: 10^8 planted
 * 21-mers, the scan 0.78 -> 0.3 ms) */
enum AwFmReturnCode awfmGpuSearchHitsInOrderCounts(AwFmGpuIndex *g, const uint8_t *dChars, const uint64_t *dOffsets,
                                                   uint32_t fixedLength, uint64_t numQueries, int packed, uint32_t *dOrderKmers,
                                                   struct AwFmSearchRange *dOrderRanges, uint32_t *dOrderCounts, void *stream);
/* the same list from dense results (dCounts / dRanges of awfmGpuSearchHits or awfmGpuSearch), already in k-mer order:
 * dFlagOffsets[numQueries + 1] and dScratch (awfmGpuScanScratchBytes) are work space */
enum AwFmReturnCode awfmGpuCompactHits(AwFmGpuIndex *g, const uint32_t *dCounts, const struct AwFmSearchRange *dRanges,
                                       uint64_t numQueries, uint64_t *dFlagOffsets, void *dScratch, uint32_t *dHitKmers,
                                       struct AwFmSearchRange *dHitRanges, uint32_t capacity, uint32_t *dNumHits, void *stream);
enum AwFmReturnCode awfmGpuSortHits(AwFmGpuIndex *g, uint32_t *dHitKmers, struct AwFmSearchRange *dHitRanges,
                                    uint32_t numEntries, void *stream);
/* The same order without the host knowing the list's length: the first min(*dNumHits, capacity) entries of the list
 * awfmGpuSearchHitsCompact appended (k-mer numbers distinct and below numQueries, the batch's size) are put in k-mer order
 * by ranking them in a bitmap of the batch; *dNumHits is read on the device, every launch is asynchronous on `stream`, and
 * the entries beyond the hits stay {0xFFFFFFFF, empty range}.  With awfmGpuHitOffsetsOnDevice / awfmGpuLocateOnDevice a
 * batch is searched, listed and located without one host wait. */
enum AwFmReturnCode awfmGpuSortHitsOnDevice(AwFmGpuIndex *g, uint32_t *dHitKmers, struct AwFmSearchRange *dHitRanges,
                                            uint32_t capacity, const uint32_t *dNumHits, uint64_t numQueries, void *stream);

/* The whole tail of a step whose results are the list, in one launch (lists of up to 2^18 entries; longer ones through the
 * three calls above): the first min(*dNumHits, capacity) entries of the list awfmGpuSearchHitsCompact appended -- left as
 * they are -- come out in k-mer order in dSortedKmers / dSortedRanges (entries beyond the hits: {0xFFFFFFFF, empty range}),
 * dHitOffsets[0 .. capacity] are the hit offsets over the sorted list (every entry from the list's length on holds the
 * total), and dPositions[0 .. capacityHits) the first capacityHits positions in that order (may be NULL: offsets only) --
 * what awfmGpuSortHitsOnDevice + awfmGpuHitOffsetsOnDevice + awfmGpuLocateOnDevice leave, from seven dependent launches less
 * (ref src/AwFmParallelSearch.c:315-365: the reference sizes and fills one list per k-mer on the host).  Nothing waits for
 * the host; the sorted arrays must not be the unsorted ones. */
enum AwFmReturnCode awfmGpuListLocateOnDevice(AwFmGpuIndex *g, const uint32_t *dHitKmers, const struct AwFmSearchRange *dHitRanges,
                                              uint32_t capacity, const uint32_t *dNumHits, uint64_t numQueries, uint32_t *dSortedKmers,
                                              struct AwFmSearchRange *dSortedRanges, uint64_t *dHitOffsets, uint64_t capacityHits,
                                              uint64_t *dPositions, void *stream);

/* The stage after a locate on the device: dSequenceNumbers[i], dLocalPositions[i] = the sequence coordinates of dPositions[i]
 * (definition: "sequence coordinates" above; dLocalPositions may be dPositions) for the first n entries, n = capacity when
 * dNumPositions is NULL and min(*dNumPositions, capacity) otherwise, the count being read ON THE DEVICE: after
 * awfmGpuLocateOnDevice pass &dHitOffsets[numQueries], after awfmGpuListLocateOnDevice &dHitOffsets[capacity of the list].
 * Entries past the count stay as they were.  *dNumIllegal (device, may be NULL) is ADDED to: zero it first.  One launch,
 * asynchronous on `stream`: no host wait, no allocation; the grid is sized from `capacity` and trimmed by the count.  It reads 8
 * and writes 12 bytes per position and looks the record up in LDS (tables of up to 4096 records: 10^8 positions in 0.35-0.36 ms,
 * the rate of a device-to-device copy of the same bytes) or in a directory in memory (any table; 5.7 * 10^5 records: 2.3 ms).
 * AwFmUnsupportedVersionError when the image has no record table. */
enum AwFmReturnCode awfmGpuLocalPositions(AwFmGpuIndex *g, const uint64_t *dPositions, uint64_t capacity, const uint64_t *dNumPositions,
                                          uint32_t *dSequenceNumbers, uint64_t *dLocalPositions, uint64_t *dNumIllegal, void *stream);

/* ---- candidate loci: the located seeds of a read, grouped by (sequence, diagonal) ----
 * The stage after awfmGpuLocalPositions for a caller that maps reads: one definition on both sides, the host twin being the
 * definition and the checker of the device call.  (The reference stops at positions: ref src/AwFmParallelSearch.c:315-365.)
 *
 * READS AND SEEDS.  The seeds of read r are the seed numbers [readSeedOffsets[r], readSeedOffsets[r + 1]) of numSeeds seeds
 * (windows over reads and the k-mers of reads are contiguous per read in read order).  Seed s ends at seedEnds[s], the offset
 * in its read one past its last character, and is seedLengths[s] characters long (seedLengths NULL: fixedLength each; the
 * dMatchLengths of awfmGpuLongestSuffixMatches go in as they are).  Its ANCHOR is a = seedEnds[s] - length; a seed with
 * length > seedEnds[s] contributes no hit.  Its hits are the entries [hitOffsets[s], hitOffsets[s + 1]) of positions /
 * sequenceNumbers (numHits entries; sequenceNumbers NULL: every hit lies in sequence 0 and positions are global).  A seed with
 * more than maxHitsPerSeed hits contributes none (0: no limit; the usual repeat filter), and hits of sequence 0xFFFFFFFF (the
 * illegal positions of awfmGpuLocalPositions) are dropped.  What remains are the read's KEPT HITS.
 *
 * CLUSTERS.  A kept hit has the diagonal D = (int64_t)position - a (negative where the read overhangs its sequence's start).
 * The kept hits of a read are ordered by (sequence ascending, D ascending as a signed value); a cluster is a maximal run in that
 * order whose neighbours have the same sequence and D[k + 1] - D[k] <= band.  Its votes are the hits of the run -- a seed with
 * two hits inside one band votes twice --, its diagonal is the run's smallest D, its span the largest D minus the smallest,
 * saturated at 2^32 - 1, and its read interval runs from the smallest anchor to the largest seedEnd of the run.
 *
 * CANDIDATES.  A cluster with votes >= max(minVotes, 1) is a candidate; a read's candidates are ordered by (votes descending,
 * sequence ascending, diagonal ascending).  With C = maxCandidates (1..16), the first min(C, number of candidates) candidates of
 * read r are stored at r * C + j in the six per-slot arrays, and the remaining slots of the read hold {sequence 0xFFFFFFFF, 0,
 * 0, 0, 0, 0}.  numCandidates[r] is the true number (it may exceed C), keptHits[r] the read's kept hits.
 *
 * LIMIT.  AWFM_CANDIDATES_MAX_HITS kept hits per read is part of the definition on both sides.  A read with more is
 * OVERFLOWED: no candidates (all slots hold the fill, numCandidates 0), keptHits = the true number saturated at 0xFFFFFFFE, and
 * it is counted in *numOverflowed, which is ADDED to (zero it first); the caller re-runs such reads with a stricter
 * maxHitsPerSeed.  A read is MALFORMED when its seed range is inverted, leaves [0, numSeeds] or holds 2^32 seeds or more, or
 * when the hit range of any of its seeds is inverted or leaves [0, numHits]: it is reported like an overflowed read, with
 * keptHits = 0xFFFFFFFF.  Neither side reads outside the arrays it was given, whatever the offsets say.
 *
 * Every output may be NULL.  numReads == 0 succeeds and touches nothing; a missing input array (sequenceNumbers and seedLengths
 * apart), or neither seedLengths nor a fixedLength: AwFmNullPtrError; numReads >= 2^32 or maxCandidates outside 1..16:
 * AwFmIllegalPositionError.
 *
 * awfmReadCandidates: on the host over `threads` threads of the library's pool, one read at a time: collect, qsort, scan, select.
 * (What a kept hit is, is written once per side for this call and for "read chains": csrc/awfm_hits.h, csrc/awfm_hits_kernel.h.)
 * awfmGpuReadCandidates (csrc/awfm_candidates_kernel.h): the same on device arrays (both structs live on the host and hold
 * device addresses); asynchronous on `stream`, no host wait, no allocation, none of the handle's scratch slots: two streams may
 * run it on one image at once, each with its own dScratch of awfmGpuReadCandidatesScratchBytes(numReads) bytes.  One wave per read
 * gathers the read's stretch of hits, and sorts and scans reads of up to 256 kept hits in LDS; larger reads go onto a worklist
 * in dScratch, which a second launch reads on the device and gives a workgroup each.  `g` names the device and takes the error
 * text; the call reads nothing of the index. */
#define AWFM_CANDIDATES_MAX_HITS 4096u
#define AWFM_CANDIDATES_MAX_SLOTS 16u
#define AWFM_CANDIDATES_NONE 0xFFFFFFFFu /* the sequence of an unused slot */
struct AwFmCandidateInputs {
  const uint64_t *readSeedOffsets; /* [numReads + 1] */
  uint64_t numSeeds;
  const uint32_t *seedEnds;    /* [numSeeds] */
  const uint32_t *seedLengths; /* [numSeeds], or NULL: fixedLength */
  uint32_t fixedLength;
  const uint64_t *hitOffsets; /* [numSeeds + 1] */
  uint64_t numHits;
  const uint64_t *positions;       /* [numHits] */
  const uint32_t *sequenceNumbers; /* [numHits], or NULL: sequence 0 */
};
struct AwFmCandidateOutputs {
  uint32_t *sequences; /* the six per-slot arrays: [numReads * maxCandidates] */
  int64_t *diagonals;
  uint32_t *votes;
  uint32_t *diagonalSpans;
  uint32_t *readBegins;
  uint32_t *readEnds;
  uint32_t *numCandidates; /* [numReads] */
  uint32_t *keptHits;      /* [numReads] */
  uint64_t *numOverflowed; /* one counter, added to */
};
enum AwFmReturnCode awfmReadCandidates(const struct AwFmCandidateInputs *in, uint64_t numReads, uint32_t maxHitsPerSeed, uint32_t band,
                                       uint32_t minVotes, uint32_t maxCandidates, const struct AwFmCandidateOutputs *out,
                                       unsigned threads);
uint64_t awfmGpuReadCandidatesScratchBytes(uint64_t numReads);
enum AwFmReturnCode awfmGpuReadCandidates(AwFmGpuIndex *g, const struct AwFmCandidateInputs *dIn, uint64_t numReads,
                                          uint32_t maxHitsPerSeed, uint32_t band, uint32_t minVotes, uint32_t maxCandidates,
                                          const struct AwFmCandidateOutputs *dOut, void *dScratch, void *stream);

/* ---- read chains: the best colinear chain of the seeds of every candidate locus ----
 * The stage after awfmGpuReadCandidates: votes count hits, a chain counts the read bases that distinct, colinear seeds support,
 * and says where in its sequence the read begins and ends.  One definition on both sides, the host twin being the definition
 * and the checker of the device call.  (The reference has no analogue: ref src/AwFmParallelSearch.c:315-365.)
 *
 * INPUTS.  struct AwFmCandidateInputs, numReads, maxHitsPerSeed, band and C = maxCandidates (1..16) as in "candidate loci": the
 * KEPT HITS of a read are exactly those of that definition, dropped seeds, illegal hits and AWFM_CANDIDATES_MAX_HITS included.
 * The slot arrays sequences, diagonals and diagonalSpans ([numReads * C], read only) name the loci; lookback
 * (1..AWFM_CHAINS_MAX_LOOKBACK) and gapPenalty (per unit of diagonal change, 0 allowed) steer the chaining.
 *
 * ANCHORS.  Slot (r, j) with sequences != AWFM_CANDIDATES_NONE owns the kept hits of read r in its sequence whose diagonal D has
 * 0 <= D - diagonals[slot] <= diagonalSpans[slot], the difference taken exactly (as the candidate definition's keys do: no
 * wrap-around, so a D below the slot's diagonal is never inside).  For slots that awfmReadCandidates wrote with the same band
 * that interval is exactly the cluster (clusters are maximal runs); the call does not otherwise depend on how the slots were
 * made.  Each such hit is an anchor (e, D, len): e = seedEnd, len = the seed's length, a = e - len the read offset of its start.
 * A slot's anchors are ordered by (e ascending, D ascending as a signed value, len ascending); identical triples may stand in
 * any order, the result being a function of the sequence of triples.
 *
 * RECURRENCE, in exact integer arithmetic (everything fits 64 bits signed except g * gapPenalty, which fits 64 bits unsigned; a
 * value that is not above len_i is never taken, so no side needs a negative score).  The predecessors of anchor i are the
 * anchors at the order positions max(0, i - lookback) .. i - 1 of its slot; predecessor j is compatible when
 *   dr = e_i - e_j > 0,   dt = dr + (D_i - D_j) > 0,   g = |D_i - D_j| <= band,   and then
 *   f(i) = max(len_i, max over compatible j of f(j) + min(len_i, dr, dt) - g * gapPenalty),
 * ties among predecessors going to the largest j, and a predecessor being taken only when its value is strictly greater than
 * len_i.  f(j) <= e_j and min(...) <= dr give f(i) <= e_i: SCORES FIT 32 BITS (the host twin asserts it).  An anchor carries
 * the a and the D of the first anchor of its chain and the number of its anchors; nothing is backtraced.  Two hits of one seed
 * share e and are never in one chain.  The BEST CHAIN of a slot ends at the anchor with the largest f, ties to the smallest
 * order position.
 *
 * OUTPUTS (struct AwFmChainOutputs, every pointer may be NULL).  Per slot: chainScores = that f, chainAnchors, chainReadBegins =
 * a of the chain's first anchor, chainReadEnds = e of its last, chainBeginDiagonals / chainEndDiagonals = D of the first / last:
 * the chain covers [readBegin + beginDiagonal, readEnd + endDiagonal) of the sequence.  Unused slots and slots without an anchor
 * get all zeros.  Per read: bestSlots = the slot with the largest score among those with an anchor, ties to the lowest,
 * 0xFFFFFFFF when there is none; keptHits as in the candidate call.  *numOverflowed is ADDED to.
 *
 * LIMITS.  Overflowed reads (more than AWFM_CANDIDATES_MAX_HITS kept hits) and malformed reads are reported exactly as
 * awfmReadCandidates reports them: all slots zero, bestSlots 0xFFFFFFFF, keptHits the saturated number / 0xFFFFFFFF, counted in
 * *numOverflowed.  A read is also MALFORMED when two of its slots name the same sequence and their intervals [diagonal,
 * diagonal + span] intersect: neither side then has to decide whose hit it is.  Neither side reads outside the arrays it was
 * given, whatever the offsets or the slot arrays say.
 *
 * Error codes as in the candidate call; lookback outside 1..64: AwFmIllegalPositionError; a missing slot array (or dScratch):
 * AwFmNullPtrError; numReads == 0 succeeds and touches nothing.
 *
 * awfmReadChains (csrc/awfm_chains.c): on the host over `threads` threads of the pool, a read at a time: collect, assign to
 * slots, qsort, recurrence.  awfmGpuReadChains (csrc/awfm_chains_kernel.h): the same on device arrays; asynchronous on `stream`,
 * no host wait, no allocation, none of the handle's scratch slots: two streams may run it on one image at once, each with its
 * own dScratch of awfmGpuReadChainsScratchBytes(numReads) bytes.  A wave per read for reads of up to 256 anchors, a worklist in
 * dScratch and a workgroup per read beyond; per anchor one step of one wave, a lane per predecessor.  `g` names the device and
 * takes the error text; the call reads nothing of the index. */
#define AWFM_CHAINS_MAX_LOOKBACK 64u
#define AWFM_CHAINS_NO_SLOT 0xFFFFFFFFu /* bestSlots of a read without an anchor */
struct AwFmChainOutputs {
  uint32_t *chainScores; /* the six per-slot arrays: [numReads * maxCandidates] */
  uint32_t *chainAnchors;
  uint32_t *chainReadBegins;
  uint32_t *chainReadEnds;
  int64_t *chainBeginDiagonals;
  int64_t *chainEndDiagonals;
  uint32_t *bestSlots;     /* [numReads] */
  uint32_t *keptHits;      /* [numReads] */
  uint64_t *numOverflowed; /* one counter, added to */
};
enum AwFmReturnCode awfmReadChains(const struct AwFmCandidateInputs *in, uint64_t numReads, uint32_t maxHitsPerSeed, uint32_t band,
                                   uint32_t maxCandidates, const uint32_t *sequences, const int64_t *diagonals,
                                   const uint32_t *diagonalSpans, uint32_t lookback, uint32_t gapPenalty,
                                   const struct AwFmChainOutputs *out, unsigned threads);
uint64_t awfmGpuReadChainsScratchBytes(uint64_t numReads);
enum AwFmReturnCode awfmGpuReadChains(AwFmGpuIndex *g, const struct AwFmCandidateInputs *dIn, uint64_t numReads, uint32_t maxHitsPerSeed,
                                      uint32_t band, uint32_t maxCandidates, const uint32_t *dSequences, const int64_t *dDiagonals,
                                      const uint32_t *dDiagonalSpans, uint32_t lookback, uint32_t gapPenalty,
                                      const struct AwFmChainOutputs *dOut, void *dScratch, void *stream);

/* ---- chain verification: the indexed text on the device, batched recall, and the banded edit distance of every chain ----
 * The stage after awfmGpuReadChains: a chain says where a read probably lies; this stage compares the read's characters with the
 * text there and gives the caller a number to rank or reject on.  One definition on both sides, the host twin being the
 * definition and the checker of the device calls.  (The reference keeps the text for this purpose and reads one segment per
 * call: ref src/AwFmFile.c awFmReadSequenceFromFile, one pread each.)
 *
 * THE TEXT ON THE DEVICE.  awfmGpuIndexSetText uploads the indexed text as it was given to awFmCreateIndex (host bytes, one per
 * position, unchanged; a FASTA index's text is its records concatenated with their NUL terminators).  length must equal
 * bwtLength - 1, else AwFmIllegalPositionError and the old text stays; NULL / 0 removes the text.  awfmGpuIndexTextLength
 * returns the length, 0 without a text.  The text is ONE allocation of alignUp(length, 16) + 16 bytes whose bytes from `length`
 * on are zero, so that any ALIGNED 4-, 8- or 16-byte load that holds at least one byte of [0, length) lies inside the
 * allocation: that is the only kind of load a kernel makes of it.  It belongs to the image: all handles share it, it is counted
 * in awfmGpuIndexDeviceBytes, named by awfmGpuIndexDescribe and freed by awfmGpuIndexDestroy; it is installed like the record
 * table (waits for the searches on the image; calls already enqueued finish on the text they were enqueued with).  Nothing
 * uploads it automatically: not awfmGpuCreateIndex, not an index that carries storeOriginalSequence.
 *
 * BATCHED RECALL.  Window i of positions[i] = p is out[i * (before + after) ..) = text[p - before, p + after): every byte
 * outside [0, length) is written as 0, every byte of a window with p >= length included.  before + after must be 1..4096
 * (AwFmIllegalPositionError).  awfmTextWindows: on the host over `threads` threads of the pool.  awfmGpuTextWindows: on device
 * arrays, the first n positions, n = capacity when dNumPositions is NULL and min(*dNumPositions, capacity) otherwise, the count
 * being read ON THE DEVICE as in awfmGpuLocalPositions; windows past the count stay as they were.  One launch, asynchronous on
 * `stream`, no host wait, no allocation.  AwFmUnsupportedVersionError when the image has no text.
 *
 * VERIFICATION.  The reads: read r is readChars[readOffsets[r] .. readOffsets[r + 1]) of numReadChars characters.  C =
 * maxCandidates (1..16); the per-slot arrays [numReads * C] are sequences as awfmReadCandidates wrote it and chainAnchors,
 * chainReadBegins (rb), chainReadEnds (re), chainBeginDiagonals (bD), chainEndDiagonals (eD) as awfmReadChains wrote them.
 * bandPad w and maxDrift x with x + 2 w + 1 <= AWFM_VERIFY_MAX_BAND, else AwFmIllegalPositionError.  The host twin takes text,
 * length, the records' ends (numRecords == 0: one sequence [0, length)) and the alphabet; the device call takes text, record
 * table (none: one sequence) and alphabet from the image, and gives AwFmUnsupportedVersionError without a text.
 *
 * Per slot, with s its sequence:
 *   UNUSED     sequences == AWFM_CANDIDATES_NONE or chainAnchors == 0: AWFM_VERIFY_NONE.
 *   INTERVALS  in exact arithmetic, no wrap-around (a value that does not fit is malformed): the record is [S, E[s]) with
 *              S = s ? E[s - 1] + 1 : 0;  n = re - rb, tb = rb + bD, te = re + eD, m = te - tb, delta = m - n = eD - bD.
 *   MALFORMED  s >= the number of sequences; rb > re or re > the read's length; the read's offsets inverted or beyond
 *              numReadChars; tb < 0, tb > te, te > E[s] - S; or a record that leaves the text (E[s] < S or E[s] > length, which a
 *              table that belongs to the text never has): AWFM_VERIFY_MALFORMED.  NOTHING is read through a malformed slot,
 *              neither read nor text.  Chains that awfmReadChains made from located hits are never malformed.
 *   TOO WIDE   |delta| > x: AWFM_VERIFY_TOO_WIDE.
 *   TOO LONG   n > AWFM_VERIFY_MAX_LENGTH: AWFM_VERIFY_TOO_LONG (so every value fits 32 bits).
 *   otherwise the BANDED GLOBAL EDIT DISTANCE of R = read[rb .. re) and T = text[S + tb .. S + te):
 *     band        cell (i, j), 0 <= i <= n, 0 <= j <= m, is in the band when lo <= j - i <= hi, lo = min(0, delta) - w,
 *                 hi = max(0, delta) + w;
 *     recurrence  H(0, 0) = 0; H(i, j) = the minimum over those of its three predecessors that are in the band and in the matrix
 *                 of H(i-1, j-1) + sub(R[i-1], T[j-1]), H(i-1, j) + 1, H(i, j-1) + 1;
 *     sub         0 when both characters map to the same PROPER letter index under the library's mapping (the reference's
 *                 letter tables, ref src/AwFmLetter.c:4-22 / :55-67: index < 4 of a nucleotide, < 20 of an amino index; blind to
 *                 case), 1 otherwise: an ambiguity letter matches nothing, not even itself;
 *     result      H(n, m); both corners are always in the band.
 *   The value is an UPPER BOUND of the unbanded edit distance and EQUALS it whenever that distance is <= 2 w + |delta| (a
 *   path of cost d takes a steps along T alone and b along R alone with a - b = delta and a + b <= d, and stays on the diagonals
 *   [-b, a]; min(a, b) = (a + b - |delta|) / 2 <= w then keeps it inside [lo, hi]).
 *
 * OUTPUTS (every pointer may be NULL): editDistances [numReads * C]; bestSlots [numReads]: the slot with the smallest distance
 * among those that have one, ties to the lowest slot, AWFM_CHAINS_NO_SLOT when none; *numUnverified: the slots that got
 * MALFORMED, TOO_WIDE or TOO_LONG, ADDED to (zero it first).  numReads == 0 succeeds and touches nothing; a missing input array:
 * AwFmNullPtrError; numReads >= 2^32 or maxCandidates outside 1..16: AwFmIllegalPositionError.
 *
 * awfmVerifyChains (csrc/awfm_verify.c): on the host over `threads` threads of the pool, a read at a time, two rows of at most
 * 64 cells, the plain recurrence.  awfmGpuVerifyChains (csrc/awfm_verify_kernel.h): the same on device arrays (both structs live
 * on the host and hold device addresses); one launch, asynchronous on `stream`, no host wait, no allocation, no scratch: two
 * streams may run it on one image at once.  A wave per read; a group of G lanes (16, 32 or 64: the smallest that holds the band's
 * x + 2 w + 1 diagonals) per slot, a lane per diagonal, a row per step.  $AWFM_GPU_DIAG verify_group=16|32|64 forces a larger G
 * than the band needs (tests; the result does not depend on it). */
#define AWFM_VERIFY_MAX_BAND 64u
#define AWFM_VERIFY_MAX_LENGTH (1u << 20)
#define AWFM_VERIFY_NONE 0xFFFFFFFFu
#define AWFM_VERIFY_MALFORMED 0xFFFFFFFEu
#define AWFM_VERIFY_TOO_WIDE 0xFFFFFFFDu
#define AWFM_VERIFY_TOO_LONG 0xFFFFFFFCu
struct AwFmVerifyInputs {
  const uint8_t *readChars;
  uint64_t numReadChars;
  const uint64_t *readOffsets; /* [numReads + 1] */
  const uint32_t *sequences;   /* the six per-slot arrays: [numReads * maxCandidates] */
  const uint32_t *chainAnchors;
  const uint32_t *chainReadBegins;
  const uint32_t *chainReadEnds;
  const int64_t *chainBeginDiagonals;
  const int64_t *chainEndDiagonals;
};
struct AwFmVerifyOutputs {
  uint32_t *editDistances; /* [numReads * maxCandidates] */
  uint32_t *bestSlots;     /* [numReads] */
  uint64_t *numUnverified; /* one counter, added to */
};
enum AwFmReturnCode awfmGpuIndexSetText(AwFmGpuIndex *g, const uint8_t *text, uint64_t length);
uint64_t awfmGpuIndexTextLength(const AwFmGpuIndex *g);
enum AwFmReturnCode awfmTextWindows(const uint8_t *text, uint64_t length, const uint64_t *positions, uint64_t numPositions,
                                    uint32_t before, uint32_t after, uint8_t *out, unsigned threads);
enum AwFmReturnCode awfmGpuTextWindows(AwFmGpuIndex *g, const uint64_t *dPositions, uint64_t capacity, const uint64_t *dNumPositions,
                                       uint32_t before, uint32_t after, uint8_t *dOut, void *stream);
enum AwFmReturnCode awfmVerifyChains(const struct AwFmVerifyInputs *in, uint64_t numReads, uint32_t maxCandidates, uint32_t bandPad,
                                     uint32_t maxDrift, const uint8_t *text, uint64_t length, const uint64_t *sequenceEnds,
                                     uint64_t numRecords, enum AwFmAlphabetType alphabet, const struct AwFmVerifyOutputs *out,
                                     unsigned threads);
enum AwFmReturnCode awfmGpuVerifyChains(AwFmGpuIndex *g, const struct AwFmVerifyInputs *dIn, uint64_t numReads, uint32_t maxCandidates,
                                        uint32_t bandPad, uint32_t maxDrift, const struct AwFmVerifyOutputs *dOut, void *stream);

/* ---- chain alignment: where a read lies in its record, at what distance and by which operations ----
 * The stage after verification: one slot of every read, slots[r], is ALIGNED -- the whole read, not the chain's interval, with
 * free ends in the text, with a record of each cell's direction and a walk back that emits the edit script.  slots[r] is
 * normally bestSlots of awfmGpuReadChains or awfmGpuVerifyChains as it is; a caller who wants secondary alignments calls again
 * with another array.  Inputs, C = maxCandidates (1..16), bandPad w, maxDrift x (x + 2 w + 1 <= AWFM_VERIFY_MAX_BAND, else
 * AwFmIllegalPositionError), text, record table and alphabet are verification's.  One definition on both sides, the host twin
 * (csrc/awfm_align.c) being the definition and the checker of the device call.
 *
 * Per read, in this order, with j = slots[r] and n the length of the WHOLE read:
 *   UNUSED     j == AWFM_CHAINS_NO_SLOT, or the slot's sequences == AWFM_CANDIDATES_NONE or its chainAnchors == 0:
 *              AWFM_VERIFY_NONE.  Not counted.
 *   MALFORMED  j >= C (and not the no-slot value), or the slot is malformed as in verification (record and sequence checks,
 *              rb > re, re > n, read offsets inverted or beyond numReadChars, tb < 0, tb > te, te > the record's length L,
 *              diagonals whose sums would wrap): AWFM_VERIFY_MALFORMED.  NOTHING is read through a malformed slot.
 *   TOO WIDE   |eD - bD| > x: AWFM_VERIFY_TOO_WIDE.
 *   TOO LONG   n > maxRows on the device (maxRows is 1..AWFM_ALIGN_MAX_LENGTH, else AwFmIllegalPositionError), n >
 *              AWFM_ALIGN_MAX_LENGTH on the host: AWFM_VERIFY_TOO_LONG.
 *   OVERHANG   with lo = min(bD, eD) - w and hi = max(bD, eD) + w: hi < 0 or lo + n > L -- the band around the chain's diagonals
 *              has left the record before the read's first or after its last character: AWFM_ALIGN_OVERHANG.  Such reads are
 *              reported, not clipped.
 *   A read with one of these five gets the status in editDistances and zeros in textBegins, textEnds and numOps; its row of ops
 *   is not written.  Only ALIGNED reads load text.
 *   otherwise the BANDED FITTING ALIGNMENT of R = the whole read against the record T (sequence-local coordinates), global in
 *   the read and free at both ends in the text:
 *     cells       (i, t) exists for 0 <= i <= n, 0 <= t <= L, lo <= t - i <= hi;
 *     recurrence  H(0, t) = 0; for i > 0, H(i, t) = the minimum over the existing predecessors of H(i-1, t-1) + sub(R[i-1],
 *                 T[t-1]), H(i-1, t) + 1, H(i, t-1) + 1; sub is verification's (0 only for two characters of the same proper
 *                 letter index, blind to case, an ambiguity letter matches nothing);
 *     finiteness  every existing cell with i > 0 has an existing predecessor: the diagonal one exists whenever t >= 1 (same
 *                 diagonal, 0 <= t - 1 <= L), and in column 0 the upper one does, its diagonal 1 - i <= 0 <= hi.  Row n has a
 *                 cell because n + lo <= L and n + hi >= 0.  So no infinity ever reaches an output;
 *     direction   of a cell, a function of the cell alone: DIAGONAL when the diagonal predecessor exists and attains the
 *                 minimum, else UP when the upper one does, else LEFT;
 *     end         textEnd = the smallest t that minimises H(n, t) over the existing cells of row n; editDistance that minimum;
 *     walk back   follow the directions from (n, textEnd) to row 0; the column reached there is textBegin;
 *     operations  from the read's first character on: diagonal gives '=' when sub is 0 and 'X' otherwise, up gives 'I' (a
 *                 read character without a text character), left gives 'D'; equal neighbours are merged into runs, and run k
 *                 is ops[r * maxOps + k] = run << 4 | op in BAM numbering (I = 1, D = 2, '=' = 7, X = 8); numOps is the
 *                 number of runs.  Entries of the row from numOps on are not written.
 *   The value is an UPPER BOUND of the unbanded fitting distance of the read against the record; the runs' read lengths sum to
 *   n, their text lengths to textEnd - textBegin, and the number of X, I and D characters equals the distance.  A read with
 *   n = 0 is aligned: distance 0, no run, textBegin = textEnd = max(lo, 0).
 *   maxOps is 1..AWFM_ALIGN_MAX_OPS (AwFmIllegalPositionError).  When a read's numOps > maxOps its row of ops has unspecified
 *   content, nothing outside the row is written, the read is counted in *numTruncated and every other output stays valid
 *   (numOps is the true number).
 *
 * OUTPUTS (every pointer may be NULL): see the struct; the two counters are ADDED to.  numReads == 0 succeeds and touches nothing;
 * a missing input array, slots or dScratch: AwFmNullPtrError; numReads >= 2^32, C outside 1..16: AwFmIllegalPositionError.
 *
 * awfmAlignChains (csrc/awfm_align.c): on the host over `threads` threads of the pool, a read at a time, the plain recurrence
 * with a direction byte per cell in an n x band table, then the walk.  awfmGpuAlignChains (csrc/awfm_align_kernel.h): the same on
 * device arrays; text, record table and alphabet are the image's (AwFmUnsupportedVersionError without a text); one launch,
 * asynchronous on `stream`, no host wait, no allocation.  A group of G lanes (16, 32 or 64: the smallest that holds the band)
 * per read, a lane per diagonal, a row per step; the directions of a row go to the group's trace arena in dScratch, 16 bytes
 * per row and wave of a persistent grid: awfmGpuAlignChainsScratchBytes(g, maxRows) bytes, 16-byte aligned
 * (AwFmIllegalPositionError otherwise), of this call's own until it has finished -- two streams may run the call at once with
 * a dScratch each.  $AWFM_GPU_DIAG align_group=16|32|64 forces a larger G than the band needs (tests; the result does not
 * depend on it). */
#define AWFM_ALIGN_MAX_LENGTH (1u << 16) /* read characters per aligned read */
#define AWFM_ALIGN_MAX_OPS 4096u         /* upper limit of maxOps */
#define AWFM_ALIGN_OVERHANG 0xFFFFFFFBu  /* beside AWFM_VERIFY_NONE / MALFORMED / TOO_WIDE / TOO_LONG, which are reused */
struct AwFmAlignOutputs {
  uint32_t *editDistances; /* [numReads]  a distance or one of the five status values */
  uint64_t *textBegins;    /* [numReads]  sequence-local, of the slot's sequence */
  uint64_t *textEnds;      /* [numReads] */
  uint32_t *numOps;        /* [numReads]  the true number of runs, also when it exceeds maxOps */
  uint32_t *ops;           /* [numReads * maxOps]  run << 4 | op, BAM numbering: I = 1, D = 2, '=' = 7, X = 8 */
  uint64_t *numUnaligned;  /* one counter, added to: MALFORMED, TOO_WIDE, TOO_LONG, OVERHANG */
  uint64_t *numTruncated;  /* one counter, added to: aligned reads with numOps > maxOps */
};
enum AwFmReturnCode awfmAlignChains(const struct AwFmVerifyInputs *in, const uint32_t *slots, uint64_t numReads, uint32_t maxCandidates,
                                    uint32_t bandPad, uint32_t maxDrift, uint32_t maxOps, const uint8_t *text, uint64_t length,
                                    const uint64_t *sequenceEnds, uint64_t numRecords, enum AwFmAlphabetType alphabet,
                                    const struct AwFmAlignOutputs *out, unsigned threads);
uint64_t awfmGpuAlignChainsScratchBytes(const AwFmGpuIndex *g, uint32_t maxRows);
enum AwFmReturnCode awfmGpuAlignChains(AwFmGpuIndex *g, const struct AwFmVerifyInputs *dIn, const uint32_t *dSlots, uint64_t numReads,
                                       uint32_t maxCandidates, uint32_t bandPad, uint32_t maxDrift, uint32_t maxOps, uint32_t maxRows,
                                       const struct AwFmAlignOutputs *dOut, void *dScratch, void *stream);

/* ---- affine alignment: the scored local alignment of a read against its record, with soft clipping ----
 * A stage BESIDE chain alignment, for callers that report what a read mapper reports: an alignment score under affine gap
 * costs, a script whose gaps are whole runs, and clips ('S') where the read's ends do not pay.  Inputs, slots, C = maxCandidates,
 * bandPad w, maxDrift x, maxOps, maxRows, text, record table and alphabet are chain alignment's, as are the error codes, the
 * NULL rules, "every output may be NULL" and "counters are added to".  scoring: match 1..255, mismatch 0..255, gapOpen o 0..255,
 * gapExtend e 1..255 (a value outside its range: AwFmIllegalPositionError; scoring == NULL: AwFmNullPtrError); a gap of g
 * characters costs o + g e.  One definition on both sides, the host twin (csrc/awfm_align_affine.c) being the definition and
 * the checker of the device call.
 *
 * Per read, in this order, with j = slots[r] and n the length of the WHOLE read:
 *   UNUSED, MALFORMED, TOO WIDE, TOO LONG exactly as in chain alignment; the value goes to scores, the read's other outputs are
 *   0 and its row of ops is not written.  There is NO OVERHANG: a band that leaves the record clips the read.
 *   otherwise the BANDED LOCAL ALIGNMENT of R = the whole read against the record T of length L (sequence-local coordinates),
 *   with lo = min(bD, eD) - w and hi = max(bD, eD) + w:
 *     cells       (i, t) exists for 0 <= i <= n, 0 <= t <= L, lo <= t - i <= hi; a row may have no cell.  A cell has three values
 *                 H, E, F in exact signed arithmetic; the values of a cell that does not exist are minus infinity;
 *     s(R, T)     + match when verification's sub is 0, - mismatch otherwise (an ambiguity letter matches nothing);
 *     recurrence  row 0: H(0, t) = 0, E = F = -inf.  For i >= 1:
 *                   M = H(i-1, t-1) + s(R[i-1], T[t-1]);
 *                   F(i, t) = max(H(i-1, t) - o - e, F(i-1, t) - e);
 *                   E(i, t) = max(H(i, t-1) - o - e, E(i, t-1) - e);
 *                   H(i, t) = max(0, M, F, E).
 *                 H <= 2^16 * 255 < 2^24: everything fits 32 bits, and the stand-in for -inf only has to survive one
 *                 subtraction of o + 64 e;
 *     end cell    the existing cell with i >= 1 of the largest H; ties go to the smallest i, then the smallest t (on equal
 *                 score the shorter alignment).  score is that H.  When it is 0 (also n = 0, or no existing cell with i >= 1)
 *                 NOTHING is aligned: every other output of the read is 0, numOps is 0, the read is counted nowhere;
 *     walk back   from the end cell in state H; each decision is a function of the cell alone.
 *                   state H: stop when H = 0 (readBegin = i, textBegin = t); else DIAGONAL when M = H: emit '=' or 'X' by sub,
 *                            go to (i-1, t-1); else UP when F = H: state F at the same cell; else state E at the same cell;
 *                   state F at (i, t): emit 'I'; go to (i-1, t), in state H when H(i-1, t) - o - e >= F(i-1, t) - e (the gap was
 *                            opened there), else in state F;
 *                   state E at (i, t): emit 'D'; go to (i, t-1), in state H when H(i, t-1) - o - e >= E(i, t-1) - e, else in
 *                            state E.
 *                 readEnd and textEnd are the end cell's i and t;
 *     script      from the read's first character: readBegin << 4 | 4 ('S') when readBegin > 0; the merged runs of '=', 'X', 'I',
 *                 'D' as in chain alignment; (n - readEnd) << 4 | 4 when readEnd < n.  numOps counts all of them; maxOps,
 *                 numTruncated and the unspecified row of a truncated read are chain alignment's.  editDistance is the number
 *                 of X, I and D characters.
 *   INVARIANTS: the runs' read lengths sum to n; their text lengths to textEnd - textBegin; the script re-scored with the four
 *   costs (match per '=', - mismatch per 'X', - o - g e per run of g 'I' or 'D') equals score; the script neither begins nor
 *   ends with 'I', 'D' or 'X' next to a clip or a read end (a first operation that is not '=' would start from H = 0 at no
 *   gain, and a last one would leave an earlier cell with at least the score); 0 <= textBegin <= textEnd <= L whatever the
 *   band does.  The score never exceeds the unbanded local score and equals it when an optimal unbanded path lies inside
 *   [lo, hi].
 *   Only ALIGNED reads load text, every load of text or read is an aligned dword that holds a byte the slot owns, and the record
 *   is checked against the text's length before anything is read.
 *
 * awfmAlignChainsAffine (csrc/awfm_align_affine.c): on the host over `threads` threads of the pool, a read at a time, the
 * recurrence as written with three rows of at most 64 cells and a trace byte per cell in an n x width table, then the walk.
 * awfmGpuAlignChainsAffine (csrc/awfm_align_affine_kernel.h): the same on device arrays with the image's text, record table and
 * alphabet; one launch, asynchronous on `stream`, no host wait, no allocation; a group of G lanes per read as in chain
 * alignment, E of a row by one max-prefix-scan over the group, five trace bits per cell in dScratch:
 * awfmGpuAlignChainsAffineScratchBytes(g, maxRows) bytes, 16-byte aligned, of this call's own until it has finished -- two
 * streams may run the call at once with a dScratch each.  $AWFM_GPU_DIAG affine_group=32|64 forces a larger G than the band
 * needs (tests; the result does not depend on it). */
#define AWFM_ALIGN_OP_S 4u /* the soft clip among the operations, BAM numbering */
struct AwFmAlignScoring {
  uint32_t match, mismatch, gapOpen, gapExtend;
};
struct AwFmAffineOutputs {
  uint32_t *scores;        /* [numReads]  a score (0: nothing aligned) or one of the four status values */
  uint32_t *editDistances; /* [numReads]  X + I + D characters of the script */
  uint32_t *readBegins;    /* [numReads]  the aligned part of the read: [readBegin, readEnd) */
  uint32_t *readEnds;      /* [numReads] */
  uint64_t *textBegins;    /* [numReads]  sequence-local, of the slot's sequence */
  uint64_t *textEnds;      /* [numReads] */
  uint32_t *numOps;        /* [numReads]  the true number of runs, also when it exceeds maxOps */
  uint32_t *ops;           /* [numReads * maxOps]  run << 4 | op: I = 1, D = 2, S = 4, '=' = 7, X = 8 */
  uint64_t *numUnaligned;  /* one counter, added to: MALFORMED, TOO_WIDE, TOO_LONG */
  uint64_t *numTruncated;  /* one counter, added to: aligned reads with numOps > maxOps */
};
enum AwFmReturnCode awfmAlignChainsAffine(const struct AwFmVerifyInputs *in, const uint32_t *slots, uint64_t numReads,
                                          uint32_t maxCandidates, uint32_t bandPad, uint32_t maxDrift,
                                          const struct AwFmAlignScoring *scoring, uint32_t maxOps, const uint8_t *text, uint64_t length,
                                          const uint64_t *sequenceEnds, uint64_t numRecords, enum AwFmAlphabetType alphabet,
                                          const struct AwFmAffineOutputs *out, unsigned threads);
uint64_t awfmGpuAlignChainsAffineScratchBytes(const AwFmGpuIndex *g, uint32_t maxRows);
enum AwFmReturnCode awfmGpuAlignChainsAffine(AwFmGpuIndex *g, const struct AwFmVerifyInputs *dIn, const uint32_t *dSlots, uint64_t numReads,
                                             uint32_t maxCandidates, uint32_t bandPad, uint32_t maxDrift,
                                             const struct AwFmAlignScoring *scoring, uint32_t maxOps, uint32_t maxRows,
                                             const struct AwFmAffineOutputs *dOut, void *dScratch, void *stream);

/* ---- slot scores and mapping quality: the affine score of EVERY slot, the best one, the runner-up and how far to trust it ----
 * The stage BETWEEN chains and affine alignment, for callers that report a mapping quality: the banded local affine score and
 * end cell of every slot of every read -- score only, no trace, no script --, and per read the best slot, the second and a
 * mapping quality.  bestSlots goes straight into awfmGpuAlignChainsAffine as its slots, which then produces the script of the
 * slot that wins under the scoring the caller reports (awfmGpuVerifyChains ranks by a unit-cost distance over the chain's own
 * interval, another objective); secondary alignments are a second call with secondSlots.  Inputs, C = maxCandidates, bandPad
 * w, maxDrift x, scoring, text, record table and alphabet are affine alignment's, as are the scoring ranges, the band rule, the
 * limits of C and numReads, the NULL rules, "every output may be NULL", "counters are added to" and "numReads == 0 touches
 * nothing".  One definition on both sides, the host twin (csrc/awfm_score_affine.c) being the definition and the checker.
 *
 * PER SLOT (r, j): slotScores, slotReadEnds, slotTextEnds [r * C + j] are EXACTLY what awfmAlignChainsAffine puts into scores[r],
 * readEnds[r] and textEnds[r] when slots[r] = j: the same order UNUSED, MALFORMED, TOO WIDE, TOO LONG, the same cells, the same
 * three-value recurrence, the same end cell (the largest H over existing cells with i >= 1, then the smallest i, then the
 * smallest t), and "score 0 means nothing aligned, and nothing is read" (then both ends are 0, as with a status).  One
 * difference: there is no trace, hence no maxRows: TOO LONG is n > AWFM_ALIGN_MAX_LENGTH on BOTH sides, the affine host twin's
 * rule.  The tests hold the two calls to this equivalence.
 *
 * PER READ, over its C slots:
 *   1. a slot COUNTS when it has a score (not a status) that is >= max(minScore, 1); minScore may be any value;
 *   2. the BEST slot is the counting slot with the largest score, ties to the lowest slot; without one bestSlots[r] =
 *      AWFM_CHAINS_NO_SLOT and bestScores[r] = 0;
 *   3. a counting slot other than the best is a DUPLICATE when it names the best slot's sequence and has the best slot's
 *      (readEnd, textEnd): the same alignment reached through two clusters whose bands overlap, not a competitor;
 *   4. the SECOND slot is the largest-scoring counting slot that is neither the best nor a duplicate, ties to the lowest slot;
 *      without one secondSlots[r] = AWFM_CHAINS_NO_SLOT and secondScores[r] = 0;
 *   5. mappingQualities[r] = 0 without a best slot, else floor(mapqCap * (best - second) / best) with second = 0 when there is
 *      none: exact in unsigned 32 bits, since best < 2^24 and mapqCap <= AWFM_SCORE_MAX_MAPQ = 254 (255 is SAM's "unavailable":
 *      AwFmIllegalPositionError).
 * This rule is the library's OWN, not BWA's and not minimap2's; nothing on the path is floating-point.  A caller with another
 * rule takes bestScores and secondScores.  Duplicates are told by their end cell only; mates are paired by "pair mates" below.
 * *numUnscored: the slots that got MALFORMED, TOO_WIDE or TOO_LONG; *numMapped: the reads with a best slot.
 *
 * awfmScoreChainsAffine (csrc/awfm_score_affine.c): on the host over `threads` threads of the pool, a read at a time, three rows
 * of at most 64 cells, the recurrence as written, then the rules above over the read's C results.  awfmGpuScoreChainsAffine
 * (csrc/awfm_score_affine_kernel.h): the same on device arrays with the image's text, record table and alphabet
 * (AwFmUnsupportedVersionError without a text); ONE launch, asynchronous on `stream`, no host wait, no allocation, no scratch:
 * two streams may run it on one image at once.  A wave per read, a group of G lanes (16, 32 or 64: the smallest that holds the
 * band) per slot, a lane per diagonal, a row per step; E of a row by one max-prefix-scan over the group.  $AWFM_GPU_DIAG
 * score_group=32|64 forces a larger G than the band needs (tests; the result does not depend on it). */
#define AWFM_SCORE_MAX_MAPQ 254u
struct AwFmSlotScoreOutputs {
  uint32_t *slotScores;       /* [numReads * C]  a score (0: nothing aligned) or one of the four status values */
  uint32_t *slotReadEnds;     /* [numReads * C]  the end cell's i; 0 with a status or score 0 */
  uint64_t *slotTextEnds;     /* [numReads * C]  the end cell's t, sequence-local; 0 likewise */
  uint32_t *bestSlots;        /* [numReads]  AWFM_CHAINS_NO_SLOT when no slot counts */
  uint32_t *bestScores;       /* [numReads]  0 when none */
  uint32_t *secondSlots;      /* [numReads]  AWFM_CHAINS_NO_SLOT when none */
  uint32_t *secondScores;     /* [numReads]  0 when none */
  uint8_t *mappingQualities;  /* [numReads] */
  uint64_t *numUnscored;      /* one counter, added to: slots that got MALFORMED, TOO_WIDE or TOO_LONG */
  uint64_t *numMapped;        /* one counter, added to: reads with a best slot */
};
enum AwFmReturnCode awfmScoreChainsAffine(const struct AwFmVerifyInputs *in, uint64_t numReads, uint32_t maxCandidates, uint32_t bandPad,
                                          uint32_t maxDrift, const struct AwFmAlignScoring *scoring, uint32_t minScore, uint32_t mapqCap,
                                          const uint8_t *text, uint64_t length, const uint64_t *sequenceEnds, uint64_t numRecords,
                                          enum AwFmAlphabetType alphabet, const struct AwFmSlotScoreOutputs *out, unsigned threads);
enum AwFmReturnCode awfmGpuScoreChainsAffine(AwFmGpuIndex *g, const struct AwFmVerifyInputs *dIn, uint64_t numReads, uint32_t maxCandidates,
                                             uint32_t bandPad, uint32_t maxDrift, const struct AwFmAlignScoring *scoring, uint32_t minScore,
                                             uint32_t mapqCap, const struct AwFmSlotScoreOutputs *dOut, void *stream);

/* ---- substitution matrices: slot scores and affine alignment with s(a, b) from a table ----
 * Twins of the two calls above for callers whose substitutions are not all alike: protein alignments (I/V is not W/P), or
 * nucleotide scorings that tell N from a mismatch and transitions from transversions.  NEW CALLS ONLY: nothing above changes.
 *
 * struct AwFmMatrixScoring: substitution[class(read character) * AWFM_MATRIX_CLASSES + class(text character)], any int8 anywhere,
 * not necessarily symmetric -- a positive value between two different letters, a non-positive diagonal and a positive "other x
 * other" are all legal --, and gapOpen o 0..255, gapExtend e 1..255 as in struct AwFmAlignScoring (outside: AwFmIllegalPositionError).
 *   CLASSES.  Amino: class(c) = min(awfmAminoAsciiToIndex(c), 20): 0..19 the twenty letters in index order (A C D E F G H I K L
 *   M N P Q R S T V W Y, either case), 20 every other byte, the sentinel '$' included.  Nucleotide: class(c) =
 *   min(awfmNucAsciiToIndex(c), 4): 0..3 are A C G T/U (either case), 4 every other byte, the sentinel included (whose letter index
 *   is 5).  Entries with an index >= 5 on either side are never read for nucleotides and may hold anything.
 *
 * awfmScoreChainsMatrix / awfmGpuScoreChainsMatrix are awfmScoreChainsAffine / awfmGpuScoreChainsAffine, and awfmAlignChainsMatrix /
 * awfmGpuAlignChainsMatrix are awfmAlignChainsAffine / awfmGpuAlignChainsAffine, with the matrix in place of the scoring: the same
 * inputs, outputs (struct AwFmSlotScoreOutputs, struct AwFmAffineOutputs), per-read rules, status order, counters, NULL rules
 * (scoring == NULL: AwFmNullPtrError, where the sibling reports it), order of the argument checks, maxOps, maxRows, and dScratch
 * of awfmGpuAlignChainsAffineScratchBytes(g, maxRows) bytes with the same five trace bits per cell; the score call is one launch
 * without scratch, host wait or allocation.  awfmGpuAlignmentStrings takes the alignment's outputs unchanged.  The DEFINITION is
 * "affine alignment"'s word for word, except:
 *   s(R[i-1], T[t-1]) = substitution[class(R[i-1]) * 21 + class(T[t-1])];
 *   '=' and 'X', in the trace and in the script, stay BY IDENTITY: '=' exactly when verification's sub is 0 (both characters map
 *   to the same proper letter).  An 'X' may therefore carry a positive score and an '=' a negative one; editDistance counts X +
 *   I + D characters as before;
 *   bounds: H <= 2^16 * 127 < 2^24, so the end cell's key and the 32-bit arithmetic hold as they are.  The device's stand-in for
 *   minus infinity, -2^30, is reset by its lane every row; between two resets it takes one s (at most +127 or -128), one o + e
 *   and twice 63 e, less than 2^16 in either direction, so it neither reaches the real values (>= -2^16 below 0 at most) nor
 *   wraps;
 *   INVARIANTS: the runs' read lengths sum to n, their text lengths to textEnd - textBegin; the script re-scored from the text
 *   with the matrix and the gap costs (s per '=' or 'X' column, - o - g e per run of g 'I' or 'D') equals score; the script neither
 *   begins nor ends with 'I' or 'D' next to a clip or a read end; its first and its last aligned column have s > 0 (a first
 *   column with s <= 0 would start from H = 0 at no gain, a last one would leave an earlier cell with at least the score).
 *   "Neither begins nor ends with 'X'" NO LONGER HOLDS: a substitution may score positively.  0 <= textBegin <= textEnd <= L, and the
 *   score never exceeds the unbanded local score under the same matrix.
 * Under awfmMatrixScoringUniform's matrix every output of the four calls equals the affine sibling's under that scoring.
 *
 * THE MATRIX TRAVELS IN THE LAUNCH'S ARGUMENTS: the caller may change or free its struct as soon as the call returns, two streams
 * may run different matrices on one image at once, and nothing is stored in the image or the handle.  On the device a workgroup
 * copies it once into LDS (rows 32 bytes apart); per cell the two staged characters become letters, then classes, then one
 * signed byte load.  $AWFM_GPU_DIAG score_group / affine_group force G as for the siblings.
 *
 * awfmMatrixScoringUniform(alphabet, scoring, out): + match where both classes are the same proper letter, - mismatch everywhere
 * else ("other x other" included, all 21 x 21 entries), gaps copied.  AwFmNullPtrError for a NULL; AwFmIllegalPositionError for an
 * alphabet that is none, a scoring affine alignment refuses, match > 127 or mismatch > 128.
 *
 * awfmMatrixScoringFromText(alphabet, text, bytes, gapOpen, gapExtend, out): the usual matrix text format out of memory, no I/O,
 * nothing read outside [text, text + bytes), no terminator needed.  Lines end with '\n' (a '\r' before it is blank); lines whose
 * first non-blank character is '#' and blank lines are skipped; the first remaining line is the column letters, blank-separated
 * (at most 64); every further line is a row letter followed by one integer (optional sign, decimal) per column.  Letters are
 * case-insensitive; U is T.  The "other" class takes the row and column of X (amino) or N (nucleotide) where the text has them;
 * entries of that class the text does not give take the smallest proper x proper entry.  Every other letter that is not proper
 * (B, Z, J, ... / R, Y, ...) and every other single character ('*') is skipped as a row and as a column, its values still
 * counted and checked.  Entries of classes the alphabet does not have are 0.  *out is written on success only.  Refused:
 *   AwFmNullPtrError          out == NULL, or text == NULL with bytes != 0;
 *   AwFmIllegalPositionError  an alphabet that is none, gapOpen > 255, gapExtend outside 1..255; a value outside -128..127;
 *   AwFmFileFormatError       a proper letter (or X / N) repeated as a row or as a column; a proper letter missing as a row or as
 *                             a column (also: no lines at all); a row or column name of more than one character; more than 64
 *                             columns; a value that is no integer; a row with more or fewer values than columns -- which is
 *                             also what a text that ends inside a row is. */
#define AWFM_MATRIX_CLASSES 21u
struct AwFmMatrixScoring {
  int8_t substitution[AWFM_MATRIX_CLASSES * AWFM_MATRIX_CLASSES]; /* [class(read) * 21 + class(text)] */
  uint32_t gapOpen, gapExtend;                                    /* 0..255, 1..255: affine alignment's */
};
enum AwFmReturnCode awfmMatrixScoringUniform(enum AwFmAlphabetType alphabet, const struct AwFmAlignScoring *scoring,
                                             struct AwFmMatrixScoring *out);
enum AwFmReturnCode awfmMatrixScoringFromText(enum AwFmAlphabetType alphabet, const char *text, uint64_t bytes, uint32_t gapOpen,
                                              uint32_t gapExtend, struct AwFmMatrixScoring *out);
enum AwFmReturnCode awfmScoreChainsMatrix(const struct AwFmVerifyInputs *in, uint64_t numReads, uint32_t maxCandidates, uint32_t bandPad,
                                          uint32_t maxDrift, const struct AwFmMatrixScoring *scoring, uint32_t minScore, uint32_t mapqCap,
                                          const uint8_t *text, uint64_t length, const uint64_t *sequenceEnds, uint64_t numRecords,
                                          enum AwFmAlphabetType alphabet, const struct AwFmSlotScoreOutputs *out, unsigned threads);
enum AwFmReturnCode awfmGpuScoreChainsMatrix(AwFmGpuIndex *g, const struct AwFmVerifyInputs *dIn, uint64_t numReads, uint32_t maxCandidates,
                                             uint32_t bandPad, uint32_t maxDrift, const struct AwFmMatrixScoring *scoring, uint32_t minScore,
                                             uint32_t mapqCap, const struct AwFmSlotScoreOutputs *dOut, void *stream);
enum AwFmReturnCode awfmAlignChainsMatrix(const struct AwFmVerifyInputs *in, const uint32_t *slots, uint64_t numReads,
                                          uint32_t maxCandidates, uint32_t bandPad, uint32_t maxDrift,
                                          const struct AwFmMatrixScoring *scoring, uint32_t maxOps, const uint8_t *text, uint64_t length,
                                          const uint64_t *sequenceEnds, uint64_t numRecords, enum AwFmAlphabetType alphabet,
                                          const struct AwFmAffineOutputs *out, unsigned threads);
enum AwFmReturnCode awfmGpuAlignChainsMatrix(AwFmGpuIndex *g, const struct AwFmVerifyInputs *dIn, const uint32_t *dSlots, uint64_t numReads,
                                             uint32_t maxCandidates, uint32_t bandPad, uint32_t maxDrift,
                                             const struct AwFmMatrixScoring *scoring, uint32_t maxOps, uint32_t maxRows,
                                             const struct AwFmAffineOutputs *dOut, void *dScratch, void *stream);

/* ---- end bonus: slot scores and affine alignment whose reads reach their ends ----
 * The calls above are purely local: under (1, 4, 6, 1) a substitution within four characters of a read end never pays and the end
 * is soft-clipped, so a variant at position 148 of 150 vanishes from the script, from NM and from MD:Z.  The remedy of every
 * short-read mapper (BWA-MEM's clip penalty, minimap2's end bonus): an alignment that reaches a read end earns B there.  NEW CALLS
 * ONLY: nothing above changes.
 *
 * awfmScoreChainsEndBonus / awfmGpuScoreChainsEndBonus are awfmScoreChainsMatrix / awfmGpuScoreChainsMatrix, and
 * awfmAlignChainsEndBonus / awfmGpuAlignChainsEndBonus are awfmAlignChainsMatrix / awfmGpuAlignChainsMatrix, with one more argument
 * behind the matrix, endBonus B in 0 .. AWFM_END_BONUS_MAX = 255 (more: AwFmIllegalPositionError, where the siblings check the
 * scoring): the same inputs, outputs, per-read rules, statuses and their order, counters, NULL rules, order of the argument
 * checks, maxOps, maxRows and dScratch of awfmGpuAlignChainsAffineScratchBytes(g, maxRows) bytes; one launch, no host wait, no
 * allocation; the matrix and B travel by value in the launch's arguments.  MATRIX ONLY: identity scoring is
 * awfmMatrixScoringUniform's matrix.  The host twins (csrc/awfm_score_affine.c, csrc/awfm_align_affine.c) are the definition and
 * the checkers.  The DEFINITION is "substitution matrices"' word for word, except:
 *   row 0       H(0, t) = B for every existing cell of row 0 (it was 0); cells that do not exist stay minus infinity, and E = F =
 *               -inf in row 0 as before.  Rows i >= 1 are unchanged, H = max(0, M, F, E): the floor 0 is a fresh start behind a
 *               clipped prefix and carries no bonus;
 *   value       V(i, t) = H(i, t) + B when i = n and H(i, t) > 0, else V(i, t) = H(i, t).  A cell of row n with H = 0 has V = 0:
 *               the bonus never creates an empty alignment;
 *   end cell    the existing cell with i >= 1 of the largest V; ties go to the smallest i, then the smallest t: on a tie the
 *               clipped alignment wins over the one that reaches the read's end, as in BWA-MEM.  score is that V; 0 means
 *               nothing aligned, as before;
 *   walk back   unchanged: stop at H = 0 or at row 0, the same five trace bits, the same three states.  Reaching row 0 gives
 *               readBegin = 0; an 'I' may now lead out of row 0, when B > o + e.
 * THE SCORE IS THE OBJECTIVE THAT WAS MAXIMISED AND INCLUDES THE BONUSES.  The raw alignment score is
 *   score - B * [readBegin == 0] - B * [readEnd == n],
 * which a caller forms from the alignment call's outputs.  Slot scores, bestScores / secondScores, minScore, the duplicate rule
 * and the mapping quality all work on V, and the two calls stay held to "a slot's score is what the alignment call reports for
 * that slot".
 *   bounds: H <= 2^16 * 127 + 2 * 255 < 2^24, so the end cell's key holds; the device's -2^30 is reset every row and never meets B.
 *   INVARIANTS: the runs' read lengths sum to n, their text lengths to textEnd - textBegin; the script re-scored from the text
 *   with the matrix and the gap costs, plus B per read end that is not clipped, equals score; the script neither begins nor ends
 *   with 'D'; next to a clip the first / last aligned column has s > 0 and is no 'I'; next to an unclipped read end it may be
 *   'X', a column with s <= 0, or 'I' -- also when it is the alignment's ONLY column and a clip follows it (readBegin = 0,
 *   readEnd = 1 < n: the cell before it lies in row 0, which is no end cell, so B + s > 0 or B - o - e > 0 is all it needs;
 *   minScore is the caller's guard against such an alignment); 0 <= textBegin <= textEnd <= L; the score never exceeds the unbanded value under the same
 *   B and equals it when an optimal unbanded path lies inside the band.
 * With B = 0 every output of the four calls equals the matrix sibling's.  Under a uniform matrix a substitution k characters from
 * a read end (k matching characters behind it) is kept exactly when k * match + B > mismatch.  $AWFM_GPU_DIAG score_group /
 * affine_group force G as for the siblings. */
#define AWFM_END_BONUS_MAX 255u
enum AwFmReturnCode awfmScoreChainsEndBonus(const struct AwFmVerifyInputs *in, uint64_t numReads, uint32_t maxCandidates, uint32_t bandPad,
                                            uint32_t maxDrift, const struct AwFmMatrixScoring *scoring, uint32_t endBonus, uint32_t minScore,
                                            uint32_t mapqCap, const uint8_t *text, uint64_t length, const uint64_t *sequenceEnds,
                                            uint64_t numRecords, enum AwFmAlphabetType alphabet, const struct AwFmSlotScoreOutputs *out,
                                            unsigned threads);
enum AwFmReturnCode awfmGpuScoreChainsEndBonus(AwFmGpuIndex *g, const struct AwFmVerifyInputs *dIn, uint64_t numReads, uint32_t maxCandidates,
                                               uint32_t bandPad, uint32_t maxDrift, const struct AwFmMatrixScoring *scoring, uint32_t endBonus,
                                               uint32_t minScore, uint32_t mapqCap, const struct AwFmSlotScoreOutputs *dOut, void *stream);
enum AwFmReturnCode awfmAlignChainsEndBonus(const struct AwFmVerifyInputs *in, const uint32_t *slots, uint64_t numReads,
                                            uint32_t maxCandidates, uint32_t bandPad, uint32_t maxDrift,
                                            const struct AwFmMatrixScoring *scoring, uint32_t endBonus, uint32_t maxOps, const uint8_t *text,
                                            uint64_t length, const uint64_t *sequenceEnds, uint64_t numRecords, enum AwFmAlphabetType alphabet,
                                            const struct AwFmAffineOutputs *out, unsigned threads);
enum AwFmReturnCode awfmGpuAlignChainsEndBonus(AwFmGpuIndex *g, const struct AwFmVerifyInputs *dIn, const uint32_t *dSlots, uint64_t numReads,
                                               uint32_t maxCandidates, uint32_t bandPad, uint32_t maxDrift,
                                               const struct AwFmMatrixScoring *scoring, uint32_t endBonus, uint32_t maxOps, uint32_t maxRows,
                                               const struct AwFmAffineOutputs *dOut, void *dScratch, void *stream);

/* ---- window scores:the full-width local affine alignment of a read against a text window the caller names, as a slot ----
 * The stage for reads WITHOUT a chain: a mate with a burst of errors, a read across a divergent stretch, a read shorter than a
 * seed, whose place the caller knows to within some hundred positions (from its mate, from an earlier pass).  No seeds, no
 * chain, no band: every cell of read x window.  The result is the score with its begin and end cell, and a chain slot that
 * affine alignment and slot scores take as it is.  Which window a mate gets is the caller's or "pair mates"' business: one window
 * per read and call, no second best inside a window.  Read buffer, scoring and its ranges, the letter rule (an ambiguity
 * letter matches nothing), text, record table, alphabet, the NULL rules, "every output may be NULL", "counters are added to",
 * "numReads == 0 touches nothing" and numReads < 2^32 are affine alignment's.  slotStride 1..16 and slotColumn < slotStride,
 * else AwFmIllegalPositionError.  One definition on both sides, the host twin (csrc/awfm_window_affine.c) being the definition
 * and the checker of the device call.
 *
 * Per read r, in this order, with n the read's length and L the length of the record windowSequences[r]:
 *   NOT LOOKED AT  windowSequences[r] == AWFM_CANDIDATES_NONE: scores[r] = AWFM_VERIFY_NONE, the read's other per-read outputs are 0
 *                  and ITS SLOT ELEMENT IS NOT WRITTEN: a caller fills column j of an existing slot table for the reads that need
 *                  it and keeps the chains of the others.
 *   MALFORMED      the sequence is >= the number of sequences, windowBegins[r] > windowEnds[r], the read's offsets are inverted or
 *                  beyond numReadChars, or the record leaves the text: AWFM_VERIFY_MALFORMED, nothing is read through it.
 *   clipping       b = min(begin, L), e = min(end, L), W = e - b: a window is clipped to its record, never refused for leaving it.
 *   TOO WIDE       W > AWFM_WINDOW_MAX_WIDTH.
 *   TOO LONG       n > AWFM_WINDOW_MAX_LENGTH; ON THE DEVICE ALSO n > maxLength, the read length the call's scratch was sized for
 *                  (the one place where the two sides may differ: a checker passes maxLength >= the longest read).
 *   otherwise      the LOCAL affine alignment of the whole read R against T = record[b, e): the recurrence of "affine alignment"
 *                  word for word (row 0: H = 0, E = F = -inf; M, F, E, H = max(0, M, F, E)) over ALL cells 0 <= i <= n,
 *                  0 <= t <= W, and its end cell: the largest H with i >= 1, then the smallest i, then the smallest t.  scores[r]
 *                  is that H; when it is 0 (also n = 0 or W = 0) nothing is aligned and every other output of the read is 0.
 *                  readEnds[r] = i, textEnds[r] = b + t.
 *   begin cell     where affine alignment's walk back from that end cell stops, defined FORWARD so that neither side keeps a
 *                  trace.  Every value carries an origin:
 *                    O_H(i, t) = (i, t) when H = 0; else O_H(i-1, t-1) when M = H; else O_F(i, t) when F = H; else O_E(i, t);
 *                    O_F(i, t) = O_H(i-1, t) when H(i-1, t) - o - e >= F(i-1, t) - e, else O_F(i-1, t);
 *                    O_E(i, t) = O_H(i, t-1) when H(i, t-1) - o - e >= E(i, t-1) - e, else O_E(i, t-1).
 *                  (i0, t0) = O_H(end cell): readBegins[r] = i0, textBegins[r] = b + t0.
 *   THE SLOT, element r * slotStride + slotColumn of the six arrays, is written for every read that is looked at: with a score
 *   >= max(minScore, 1): sequences = the window's sequence, chainAnchors = 1, chainReadBegins = readBegin, chainReadEnds =
 *   readEnd, chainBeginDiagonals = textBegin - readBegin, chainEndDiagonals = textEnd - readEnd; otherwise, status values
 *   included, the unused slot AWFM_CANDIDATES_NONE, 0, 0, 0, 0, 0.  A written slot is never malformed under chain verification's
 *   rules (0 <= tb <= te <= L).  Handed to awfmAlignChainsAffine with (w, x) it yields a score <= this one, and the same score,
 *   begin and end whenever the optimal path stays within [min(bD, eD) - w, max(bD, eD) + w]; |eD - bD| > x is TOO WIDE there:
 *   the caller chooses x for the gaps it expects.
 *   *numUnscored: reads that got MALFORMED, TOO_WIDE or TOO_LONG; *numFound: reads with a score >= max(minScore, 1).
 *
 * awfmScoreWindowsAffine (csrc/awfm_window_affine.c): on the host over `threads` threads of the pool, a read at a time, two rows
 * of W + 1 cells with the three values and their origins; no n x W table.  awfmGpuScoreWindowsAffine
 * (csrc/awfm_window_affine_kernel.h): the same on device arrays with the image's text, record table and alphabet
 * (AwFmUnsupportedVersionError without a text); ONE launch, asynchronous on `stream`, no host wait, no allocation.  A wave per
 * read as a systolic array: a lane owns Q consecutive columns (4, 8 or 12: the smallest with 64 Q >= W, chosen per read),
 * rows flow through the lanes a step apart; a window wider than 768 goes in blocks of 768 columns whose boundary column
 * passes through dScratch: awfmGpuScoreWindowsAffineScratchBytes(g, maxLength) bytes (maxLength 1..AWFM_WINDOW_MAX_LENGTH, else
 * 0), 16-byte aligned, this call's own until it has finished -- two streams may run the call at once with a dScratch each.
 * dScratch == NULL or maxLength outside its range: AwFmNullPtrError / AwFmIllegalPositionError.  $AWFM_GPU_DIAG
 * window_q=4|8|12 fixes Q for every read (tests: narrower blocks, so the column-block path at small widths; the result
 * does not depend on it). */
#define AWFM_WINDOW_MAX_WIDTH 4096u  /* text characters per window after clipping to the record */
#define AWFM_WINDOW_MAX_LENGTH 4096u /* read characters */
struct AwFmWindowInputs {
  const uint8_t *readChars; /* as AwFmVerifyInputs */
  uint64_t numReadChars;
  const uint64_t *readOffsets;     /* [numReads + 1] */
  const uint32_t *windowSequences; /* [numReads]  AWFM_CANDIDATES_NONE: this read is not looked at */
  const uint64_t *windowBegins;    /* [numReads]  sequence-local, [begin, end) */
  const uint64_t *windowEnds;      /* [numReads] */
};
struct AwFmWindowOutputs {
  uint32_t *scores;     /* [numReads]  a score (0: nothing aligned) or a status value */
  uint32_t *readBegins; /* [numReads]  the aligned part of the read: [readBegin, readEnd) */
  uint32_t *readEnds;   /* [numReads] */
  uint64_t *textBegins; /* [numReads]  sequence-local */
  uint64_t *textEnds;   /* [numReads] */
  /* the slot, element r * slotStride + slotColumn of each: the six per-slot arrays of AwFmVerifyInputs */
  uint32_t *sequences, *chainAnchors, *chainReadBegins, *chainReadEnds;
  int64_t *chainBeginDiagonals, *chainEndDiagonals;
  uint64_t *numUnscored; /* one counter, added to: MALFORMED, TOO_WIDE, TOO_LONG */
  uint64_t *numFound;    /* one counter, added to: reads with score >= max(minScore, 1) */
};
enum AwFmReturnCode awfmScoreWindowsAffine(const struct AwFmWindowInputs *in, uint64_t numReads, const struct AwFmAlignScoring *scoring,
                                           uint32_t minScore, uint32_t slotStride, uint32_t slotColumn, const uint8_t *text, uint64_t length,
                                           const uint64_t *sequenceEnds, uint64_t numRecords, enum AwFmAlphabetType alphabet,
                                           const struct AwFmWindowOutputs *out, unsigned threads);
uint64_t awfmGpuScoreWindowsAffineScratchBytes(const AwFmGpuIndex *g, uint32_t maxLength);
enum AwFmReturnCode awfmGpuScoreWindowsAffine(AwFmGpuIndex *g, const struct AwFmWindowInputs *dIn, uint64_t numReads,
                                              const struct AwFmAlignScoring *scoring, uint32_t minScore, uint32_t slotStride,
                                              uint32_t slotColumn, uint32_t maxLength, const struct AwFmWindowOutputs *dOut, void *dScratch,
                                              void *stream);

/* ---- pair mates: reverse complement of reads, proper pairs, pair mapping quality and rescue windows ----
 * The stage for PAIRED reads, between slot scores and affine alignment: reads 2p (mate A) and 2p + 1 (mate B) are a pair, both
 * GIVEN ON THE SAME STRAND.  For the usual inward-facing library the caller reverse-complements mate 2 where the reads lie
 * (awfmGpuReverseComplementReads, below) and a two-strand index finds fragments of either strand, each in its own record; with a
 * one-strand index "strands" below searches every read on both strands and pairs in both orientations.  This call knows no strands:
 * minInsert and maxInsert are signed, so other library geometries are a matter of sign and of which mate is complemented.  They
 * are the caller's here; a caller who does not know the library's insert distribution takes them from "insert size" below, which
 * estimates the interval from the batch's confidently placed pairs and hands it to awfmGpuPairMatesEstimated in device memory.
 * The loop runs without a host wait: chains, awfmGpuScoreChainsAffine, [awfmGpuInsertHistogram, awfmGpuInsertInterval,]
 * awfmGpuPairMates[Estimated], awfmGpuScoreWindowsAffine on the windows the pairing names, awfmGpuScoreChainsAffine and
 * awfmGpuPairMates[Estimated] again, awfmGpuAlignChainsAffine with pairSlots.  "every output may be NULL", "counters are added
 * to", "numPairs == 0 touches nothing" are slot scores'.  One definition on both sides, the host twin (csrc/awfm_pair_mates.c)
 * being the definition and the checker.
 *
 * Inputs, C = maxCandidates (1..16), numReads = 2 numPairs < 2^32: readOffsets [numReads + 1]; sequences [numReads * C], the
 * slot table's column of that name; slotScores, slotReadEnds, slotTextEnds [numReads * C] exactly as awfmGpuScoreChainsAffine
 * wrote them; mappingQualities [numReads], slot scores' (may be NULL: 0 everywhere).  params: minScore; minInsert <= maxInsert,
 * both within +-2^40; unpairedPenalty; windowPad; mapqCap 0..AWFM_SCORE_MAX_MAPQ.  C or numPairs outside their range, or params
 * outside theirs: AwFmIllegalPositionError; in, out, params or a required array NULL: AwFmNullPtrError.  All sums of positions
 * below are 64-bit two's complement (exact for whatever slot scores wrote: text ends < 2^63, read ends < 2^32), values and
 * qualities are computed in 64 bits, and pairScores / pairSecondScores keep the low 32 bits (exact: a score is < 2^24).
 *
 * Per pair p, in this order (A = 2p, B = 2p + 1, n_r the length of read r):
 *   1. a slot (r, j) COUNTS when its score is not one of the four status values and is >= max(minScore, 1) (slot scores' rule
 *      1); a read whose offsets are inverted has no counting slot.  Its START is S(r, j) = (int64) slotTextEnds - slotReadEnds,
 *      the end cell's diagonal (it may be negative).  best(r) is slot scores' rule 2: the largest score, ties to the lowest slot.
 *   2. (a, b) is CONCORDANT when both slots count, they name the same sequence and minInsert <= T <= maxInsert with
 *      T = S(B, b) + n_B - S(A, a).  Its value is the sum of the two scores.
 *   3. the DISCORDANT candidate exists when both mates have a best slot and (best(A), best(B)) is not concordant; its value is
 *      max(0, score + score - unpairedPenalty).
 *   4. the WINNER is the candidate of the largest value; at equal value a concordant one goes first, then the lowest a, then
 *      the lowest b.  properPairs[p] = 1 when the winner is concordant, else 0; pairSlots[A], pairSlots[B] = the winner's slots
 *      (with one mate placed: its best slot, and AWFM_CHAINS_NO_SLOT for the other; with none: both AWFM_CHAINS_NO_SLOT);
 *      pairSlots has the shape of bestSlots and goes into awfmGpuAlignChainsAffine as it is.  pairScores[p] = the winner's
 *      value, or the single placed mate's score, or 0.  templateLengths[p] = T for a proper pair, else 0.
 *   5. slot j' is THE SAME as slot j of a read when j' = j, or when both count, name one sequence and have one (readEnd,
 *      textEnd) (slot scores' rule 3); a candidate (a', b') DUPLICATES the winner when a' is the same as a and b' the same as b.
 *      pairSecondScores[p] = the largest value among the other candidates that do not duplicate the winner (the discordant
 *      one included unless it is the winner), 0 without one.
 *   6. pairQualities[p] = floor(mapqCap * (win - second) / win) for a proper pair, else 0.  For the reads of a proper pair the
 *      output mappingQualities[r] = max(pairQualities[p], q), q being the input mappingQualities[r] when pairSlots[r] ==
 *      best(r), else 0; otherwise the input quality passes through, or 0 when the read has no best slot.  The output array may
 *      be the input array.  This integer rule is the library's OWN, like slot scores': not BWA's and not minimap2's.
 *   7. RESCUE WINDOWS, in the shape of struct AwFmWindowInputs: read r gets a window when its pair is not proper and its mate m
 *      has a best slot: windowSequences[r] = that slot's sequence and, with S = S(m, best(m)),
 *        r = B: [S + minInsert - n_B - windowPad, S + maxInsert + windowPad);
 *        r = A: with E = S + n_B, [E - maxInsert - windowPad, E - minInsert + n_A + windowPad),
 *      each bound computed signed and then raised to 0 (clipping to the record and the width limit are the window call's).
 *      Every other read gets AWFM_CANDIDATES_NONE, 0, 0, so that the window call leaves its slot alone.
 *   8. *numProper: proper pairs; *numWindows: reads that got a window.
 * THE WINDOW CALL AND THE SLOT TABLE are the caller's business: awfmGpuScoreWindowsAffine overwrites column slotColumn of every
 * read it looks at, also with the unused slot, so the caller keeps a column free for it -- for one, chains with C - 1 slots in
 * a table of stride C.
 *
 * awfmPairMates (csrc/awfm_pair_mates.c): on the host over `threads` threads of the pool, a pair at a time, the rules as written.
 * awfmGpuPairMates (csrc/awfm_pair_mates_kernel.h): the same on device arrays; it reads no text and nothing of the image, g
 * gives the device.  ONE launch, asynchronous on `stream`, no host wait, no allocation, no scratch: two streams may run it on
 * one image at once.  A group of 16 lanes per pair for C <= 4 (a lane per (a, b)), a wave per pair up to C = 16 (four
 * candidates a lane); the winner and the second are one packed-key maximum over the group each.  $AWFM_GPU_DIAG pair_group=64
 * forces the wave per pair at small C (tests; the result does not depend on it).
 *
 * REVERSE COMPLEMENT, DNA only (no alphabet argument).  out has numReadChars bytes and the same offsets.  `which` selects the
 * reads: AWFM_COMPLEMENT_ALL, AWFM_COMPLEMENT_ODD (mate 2 of interleaved pairs) or AWFM_COMPLEMENT_EVEN, anything else
 * AwFmIllegalPositionError; a read that is not selected is copied.  Per selected read of length n, byte i of the output is the
 * complement of byte n - 1 - i: A<->T and C<->G in either letter case, the case kept, every other byte as it is (an ambiguity
 * letter matches nothing on either strand under the library's letter rule).  A read with inverted offsets or offsets beyond
 * numReadChars is neither read nor written and counts in *numMalformed (added to, may be NULL); bytes of the buffer that no
 * read owns are not written, and where two reads share bytes the output holds either's.  Input and output may not overlap as
 * pointer ranges of numReadChars bytes: AwFmIllegalPositionError.  numReads == 0 touches nothing.  awfmReverseComplementReads:
 * on the host over `threads` threads.  awfmGpuReverseComplementReads: one launch, asynchronous on `stream`, a wave per read,
 * a lane per aligned word of the output; g gives the device only. */
#define AWFM_COMPLEMENT_ALL 0u
#define AWFM_COMPLEMENT_ODD 1u
#define AWFM_COMPLEMENT_EVEN 2u
#define AWFM_PAIR_MAX_INSERT (1ll << 40) /* |minInsert|, |maxInsert| <= this */
struct AwFmPairInputs {
  const uint64_t *readOffsets;     /* [2 numPairs + 1] */
  const uint32_t *sequences;       /* [numReads * C]  the slot table's */
  const uint32_t *slotScores;      /* [numReads * C]  struct AwFmSlotScoreOutputs' */
  const uint32_t *slotReadEnds;    /* [numReads * C] */
  const uint64_t *slotTextEnds;    /* [numReads * C] */
  const uint8_t *mappingQualities; /* [numReads]  may be NULL: 0 everywhere */
};
struct AwFmPairParams {
  int64_t minInsert, maxInsert; /* minInsert <= T <= maxInsert makes a pair proper */
  uint32_t minScore, unpairedPenalty, windowPad, mapqCap;
};
struct AwFmPairOutputs {
  uint8_t *properPairs;       /* [numPairs]  1: the winner is concordant */
  uint32_t *pairSlots;        /* [numReads]  the shape of bestSlots; AWFM_CHAINS_NO_SLOT for a read that is not placed */
  uint32_t *pairScores;       /* [numPairs] */
  uint32_t *pairSecondScores; /* [numPairs] */
  int64_t *templateLengths;   /* [numPairs]  T of a proper pair, else 0 */
  uint8_t *pairQualities;     /* [numPairs] */
  uint8_t *mappingQualities;  /* [numReads]  may be the input array */
  uint32_t *windowSequences;  /* [numReads]  struct AwFmWindowInputs'; AWFM_CANDIDATES_NONE: no window */
  uint64_t *windowBegins;     /* [numReads] */
  uint64_t *windowEnds;       /* [numReads] */
  uint64_t *numProper;        /* one counter, added to: proper pairs */
  uint64_t *numWindows;       /* one counter, added to: reads with a window */
};
enum AwFmReturnCode awfmPairMates(const struct AwFmPairInputs *in, uint64_t numPairs, uint32_t maxCandidates,
                                  const struct AwFmPairParams *params, const struct AwFmPairOutputs *out, unsigned threads);
enum AwFmReturnCode awfmGpuPairMates(AwFmGpuIndex *g, const struct AwFmPairInputs *dIn, uint64_t numPairs, uint32_t maxCandidates,
                                     const struct AwFmPairParams *params, const struct AwFmPairOutputs *dOut, void *stream);
enum AwFmReturnCode awfmReverseComplementReads(const uint8_t *readChars, uint64_t numReadChars, const uint64_t *readOffsets,
                                               uint64_t numReads, uint32_t which, uint8_t *out, uint64_t *numMalformed, unsigned threads);
enum AwFmReturnCode awfmGpuReverseComplementReads(AwFmGpuIndex *g, const uint8_t *dReadChars, uint64_t numReadChars,
                                                  const uint64_t *dReadOffsets, uint64_t numReads, uint32_t which, uint8_t *dOut,
                                                  uint64_t *dNumMalformed, void *stream);

/* ---- insert size: the insert interval estimated from the confidently placed pairs, and pairing that reads it on the device ----
 * The stage that gives "pair mates" its minInsert and maxInsert without a host wait: a HISTOGRAM of the template lengths of the
 * pairs whose two best slots agree, an INTERVAL from its quartiles, and awfmGpuPairMatesEstimated, which is awfmGpuPairMates with
 * the interval read from device memory.  The loop: slot scores -> awfmGpuInsertHistogram -> awfmGpuInsertInterval ->
 * awfmGpuPairMatesEstimated -> window scores -> slot scores -> awfmGpuPairMatesEstimated -> affine alignment, all on one stream.
 * All rules are INTEGER rules -- there is no floating point on this path -- and they are the library's OWN, like the mapping
 * quality's: not BWA's and not any other mapper's.  ONE interval per call: no per-orientation estimates (the reads are on one
 * strand, see "pair mates") and no standard deviation.  The host twins (csrc/awfm_insert.c) are the definition and the checker.
 *
 * params (struct AwFmInsertParams): lowTemplate <= highTemplate, the histogram's range with both ends included, bins =
 * highTemplate - lowTemplate + 1 <= AWFM_INSERT_MAX_BINS, both within +-AWFM_PAIR_MAX_INSERT; minScore: pairing's rule 1;
 * minQuality; spread 0..AWFM_INSERT_MAX_SPREAD; minSamples; fallbackMin <= fallbackMax, both within +-AWFM_PAIR_MAX_INSERT.  All
 * four calls check all of them: anything outside is AwFmIllegalPositionError, as are maxCandidates outside 1..16 and numPairs
 * >= 2^31; a NULL image, params, `in`, required input array, histogram or estimate is AwFmNullPtrError.
 *
 * HISTOGRAM, per pair p (A = 2p, B = 2p + 1; `in` is struct AwFmPairInputs as pairing takes it).  Slots COUNT and best(r) is as
 * in pairing's rules 1 and 2, with THIS call's minScore.  The pair QUALIFIES when both mates have a best slot, the two best
 * slots name one sequence and both INPUT mapping qualities are >= minQuality (mappingQualities NULL: 0 everywhere).  Its
 * T = S(B, best(B)) + n_B - S(A, best(A)) in 64-bit two's complement, pairing's rule 2.  A qualifying pair with lowTemplate <= T
 * <= highTemplate is a SAMPLE: histogram[T - lowTemplate] += 1 and *numSamples += 1; a qualifying pair outside the range adds
 * 1 to *numOutside.  The histogram has `bins` 64-bit counters and is ADDED TO, like the two counters: the caller zeroes it
 * and may accumulate over batches.  Either counter may be NULL.  numPairs == 0 touches nothing.
 *
 * INTERVAL.  N = the sum of the histogram.  N < max(minSamples, 1): valid = 0, minInsert / maxInsert = fallbackMin /
 * fallbackMax, the quartiles and the mean 0, numSamples = N.  Otherwise rank_k = (k N + 3) / 4 for k = 1, 2, 3 (integer
 * division: the smallest rank that has at least k quarters of the samples at or below it); q_k = lowTemplate + the smallest
 * bin i whose inclusive prefix sum reaches rank_k; w = spread * max(q_3 - q_1, 1); minInsert = q_1 - w and maxInsert = q_3 + w,
 * each clamped to +-AWFM_PAIR_MAX_INSERT; mean = lowTemplate + floor(sum of i h[i] / sum of h[i]) over the bins whose T lies in
 * [minInsert, maxInsert] (they hold at least half of the samples: never empty); valid = 1; numSamples = N.  Sums are 64-bit and
 * exact for N < 2^47.  All eight fields are written every time.
 *
 * ESTIMATED PAIRING.  awfmGpuPairMatesEstimated is awfmGpuPairMates to the bit -- rule 7's windows included -- with the
 * interval read from dEstimate->minInsert / maxInsert on the device; params->minInsert and maxInsert are not looked at.  What
 * the host cannot see the kernel validates: the interval is NOT USABLE when minInsert > maxInsert, minInsert <
 * -AWFM_PAIR_MAX_INSERT or maxInsert > AWFM_PAIR_MAX_INSERT.  Then no slot pair is concordant and no read gets a window (every
 * read's window outputs are AWFM_CANDIDATES_NONE, 0, 0 and *numWindows stays); everything else follows from the rules as
 * written: the discordant candidate, bests and qualities as for improper pairs.  There is no host twin: the host reads the
 * struct and calls awfmPairMates.
 *
 * awfmInsertHistogram: over `threads` threads of the pool, atomic adds into the histogram.  awfmInsertInterval: one thread.
 * awfmGpuInsertHistogram (csrc/awfm_insert_kernel.h): ONE launch, a thread per pair over a persistent grid; up to 8192 bins a
 * workgroup counts in a private histogram in LDS and adds only its nonzero bins to the caller's, above that (or with
 * $AWFM_GPU_DIAG insert_tier=global: tests, the result is the same) it adds to the caller's directly, one atomic per wave and
 * distinct bin; the two counters take one atomic per wave.  awfmGpuInsertInterval: ONE launch of one workgroup.  Every device
 * call is asynchronous on `stream`, with no host wait, no allocation and no scratch of the image (g gives the device only):
 * two streams may run them on one image at once. */
#define AWFM_INSERT_MAX_BINS 65536u
#define AWFM_INSERT_MAX_SPREAD 16u
struct AwFmInsertParams {
  int64_t lowTemplate, highTemplate; /* histogram range, both ends included; bins = high - low + 1 <= AWFM_INSERT_MAX_BINS;
                                        both within +-AWFM_PAIR_MAX_INSERT */
  uint32_t minScore;                 /* pairing's rule 1 */
  uint32_t minQuality;               /* both mates' INPUT mapping quality >= this (qualities NULL: 0 everywhere) */
  uint32_t spread;                   /* 0..AWFM_INSERT_MAX_SPREAD */
  uint32_t minSamples;               /* fewer samples in the histogram: the fallback interval */
  int64_t fallbackMin, fallbackMax;  /* fallbackMin <= fallbackMax, within +-AWFM_PAIR_MAX_INSERT */
};
struct AwFmInsertEstimate { /* 64 bytes; minInsert, maxInsert FIRST: what pairing reads */
  int64_t minInsert, maxInsert;
  int64_t quartiles[3];
  int64_t mean;
  uint64_t numSamples;
  uint64_t valid; /* 1: estimated, 0: the fallback */
};
enum AwFmReturnCode awfmInsertHistogram(const struct AwFmPairInputs *in, uint64_t numPairs, uint32_t maxCandidates,
                                        const struct AwFmInsertParams *params, uint64_t *histogram, uint64_t *numSamples,
                                        uint64_t *numOutside, unsigned threads);
enum AwFmReturnCode awfmGpuInsertHistogram(AwFmGpuIndex *g, const struct AwFmPairInputs *dIn, uint64_t numPairs, uint32_t maxCandidates,
                                           const struct AwFmInsertParams *params, uint64_t *dHistogram, uint64_t *dNumSamples,
                                           uint64_t *dNumOutside, void *stream);
enum AwFmReturnCode awfmInsertInterval(const uint64_t *histogram, const struct AwFmInsertParams *params, struct AwFmInsertEstimate *estimate);
enum AwFmReturnCode awfmGpuInsertInterval(AwFmGpuIndex *g, const uint64_t *dHistogram, const struct AwFmInsertParams *params,
                                          struct AwFmInsertEstimate *dEstimate, void *stream);
enum AwFmReturnCode awfmGpuPairMatesEstimated(AwFmGpuIndex *g, const struct AwFmPairInputs *dIn, uint64_t numPairs, uint32_t maxCandidates,
                                              const struct AwFmPairParams *params, const struct AwFmInsertEstimate *dEstimate,
                                              const struct AwFmPairOutputs *dOut, void *stream);

/* ---- alignment strings: the CIGAR and the MD:Z string of every aligned read, packed, on host and device ----
 * The last step to a mapper's output record.  Both strings are functions of arrays that lie on the device after
 * awfmGpuAlignChains or awfmGpuAlignChainsAffine -- the scripts, where they begin in their record -- and of the text, which only
 * the library holds there (awfmGpuIndexSetText): no script and no text window is downloaded to make them.  The host twin
 * (csrc/awfm_strings.c) is the definition and the checker of the device call.
 *
 * INPUTS (struct AwFmStringInputs), as the alignment calls left them: sequences [numReads * C], the slot table's; slots
 * [numReads], the array the alignment call was given; textBegins [numReads], sequence-local; numOps [numReads]; ops [numReads *
 * maxOps].  C = maxCandidates 1..16, maxOps 1..AWFM_ALIGN_MAX_OPS, numReads < 2^32, flags: AWFM_STRINGS_CIGAR_M or 0 (anything
 * outside its range, or another bit: AwFmIllegalPositionError).  A missing input array: AwFmNullPtrError.  The read characters
 * are no input: neither string needs them.  The call TRUSTS the script: '=' and 'X' are not checked against the text.
 *
 * Per read r, in this order, with k = numOps[r], j = slots[r] and run i = (len_i, op_i) = (ops[r * maxOps + i] >> 4, & 15):
 *   NONE      k == 0: both strings are empty, the read is counted nowhere and nothing else of it is read.
 *   SKIPPED   both strings are empty, the read is counted in *numSkipped and NOTHING of the text is read through it, when any of
 *             these holds: k > maxOps (a truncated row); j >= C (AWFM_CHAINS_NO_SLOT among them); s = sequences[r * C + j] >=
 *             max(numRecords, 1) (no record table: one sequence, the text); the record's end lies beyond the text's length or
 *             before its begin; a run with len == 0 or an op outside {1 I, 2 D, 4 S, 7 =, 8 X}; the script's read length (the sum
 *             of len over I, S, =, X) exceeds AWFM_ALIGN_MAX_LENGTH; its text length Tn (the sum over =, X, D) exceeds 2 *
 *             AWFM_ALIGN_MAX_LENGTH; with L the record's length, textBegins[r] > L or Tn > L - textBegins[r].  Sums are taken in
 *             64 bits; with the two caps a string stays below 2^19 bytes.
 *   otherwise the read gets both strings:
 *     CIGAR, extended  for every run in order len in decimal without leading zeros, then its letter I D S = X;
 *     CIGAR, classic   (AWFM_STRINGS_CIGAR_M) the same, except that every maximal sequence of adjacent '=' and 'X' runs becomes
 *                      ONE run, its length their sum, its letter M;
 *     MD               p = the global text position of the record's begin + textBegins[r], m = 0; for every run in order:
 *                      '=': m += len, p += len;  'X': for each of its len characters emit m in decimal, then letter(text[p]), m =
 *                      0, p += 1;  'D': emit m in decimal, then '^', then letter of text[p .. p + len), m = 0, p += len;  I, S:
 *                      nothing.  After the last run emit m.  letter(c): a..z are raised to upper case, A..Z stay, every other
 *                      byte becomes N on a nucleotide image and X on an amino one.  The result matches
 *                      [0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*: the 0 between adjacent mismatches, and between a deletion and a
 *                      mismatch, falls out of the rule.
 *
 * OUTPUTS (struct AwFmStringOutputs; every pointer may be NULL): cigarOffsets / mdOffsets [numReads + 1] are the exclusive prefix
 * sums of the TRUE string lengths whatever the capacities are; cigarChars / mdChars are arenas of cigarCapacity / mdCapacity
 * bytes.  An arena without its offsets: AwFmNullPtrError; offsets without an arena are how a caller sizes one.  A read's string
 * is written to an arena exactly when offsets[r + 1] <= that arena's capacity; a read with a non-empty string that was not
 * written to at least one requested arena is counted once in *numOverflow.  No byte of an arena beyond min(total, capacity) is
 * written, nor any byte that belongs to a read that does not fit.  Both counters are ADDED to.  numReads == 0 succeeds and
 * touches nothing.
 *
 * awfmAlignmentStrings (csrc/awfm_strings.c): over `threads` threads of the pool, one formatter counts and writes; text, record
 * table and alphabet are parameters as with the alignment twins.  awfmGpuAlignmentStrings (csrc/awfm_strings_kernel.h): text,
 * record table and alphabet are the image's (AwFmUnsupportedVersionError without a text); asynchronous on `stream`, no host
 * wait, no allocation.  A lengths kernel (a thread per read, the rows in 16-byte loads where maxOps % 4 == 0, no text), the
 * library's on-device scan once per requested offsets array, and a write kernel: a wave owns 64 consecutive reads, hence one
 * contiguous span of each arena; it formats the span in LDS and stores it in whole dwords, the span's edges up to the next dword
 * boundary as bytes; a span beyond the LDS tile is stored read by read in bytes ($AWFM_GPU_DIAG strings_tier=direct: every
 * wave; tests, the result is the same).  Text loads are aligned dwords that hold a byte the record owns, issued only for reads
 * that passed every check.  dScratch: awfmGpuAlignmentStringsScratchBytes(g, numReads) bytes, 16-byte aligned
 * (AwFmIllegalPositionError otherwise; NULL: AwFmNullPtrError), this call's own until it has finished -- two streams may run the
 * call at once with a dScratch each.  Out of scope: hard clips, N, P, BAM bytes. */
#define AWFM_STRINGS_CIGAR_M 1u /* flags: the classic CIGAR, '=' and 'X' merged into M */
struct AwFmStringInputs {
  const uint32_t *sequences;  /* [numReads * maxCandidates]  the slot table's */
  const uint32_t *slots;      /* [numReads]  what the alignment call was given */
  const uint64_t *textBegins; /* [numReads]  sequence-local */
  const uint32_t *numOps;     /* [numReads] */
  const uint32_t *ops;        /* [numReads * maxOps]  run << 4 | op */
};
struct AwFmStringOutputs {
  uint64_t *cigarOffsets; /* [numReads + 1] */
  uint8_t *cigarChars;    /* cigarCapacity bytes */
  uint64_t cigarCapacity;
  uint64_t *mdOffsets;    /* [numReads + 1] */
  uint8_t *mdChars;       /* mdCapacity bytes */
  uint64_t mdCapacity;
  uint64_t *numSkipped;   /* one counter, added to */
  uint64_t *numOverflow;  /* one counter, added to */
};
enum AwFmReturnCode awfmAlignmentStrings(const struct AwFmStringInputs *in, uint64_t numReads, uint32_t maxCandidates, uint32_t maxOps,
                                         uint32_t flags, const uint8_t *text, uint64_t length, const uint64_t *sequenceEnds,
                                         uint64_t numRecords, enum AwFmAlphabetType alphabet, const struct AwFmStringOutputs *out,
                                         unsigned threads);
uint64_t awfmGpuAlignmentStringsScratchBytes(const AwFmGpuIndex *g, uint64_t numReads);
enum AwFmReturnCode awfmGpuAlignmentStrings(AwFmGpuIndex *g, const struct AwFmStringInputs *dIn, uint64_t numReads, uint32_t maxCandidates,
                                            uint32_t maxOps, uint32_t flags, const struct AwFmStringOutputs *dOut, void *dScratch,
                                            void *stream);

/* ---- SAM records: one SAM line per read, packed behind offsets, on host and device ----
 * The step that closes the read path: reads in, SAM text out.  Every field is a function of arrays the earlier calls leave on
 * the device -- the slot table, the alignment's scores and positions, the two string arenas, the mapping qualities and the
 * proper-pair marks -- and of the reads and names the caller holds; neither the text nor the image's record table is read.  The
 * host twin (csrc/awfm_sam.c) is the definition and the checker of the device call.
 *
 * INPUTS (struct AwFmSamInputs; C = maxCandidates 1..16).  Required: readChars, readOffsets [numReads + 1], sequences [numReads *
 * C], slots, scores, editDistances, textBegins, textEnds [numReads], cigarOffsets [numReads + 1] and cigarChars; and, when
 * numRecordNames != 0, recordNameOffsets [numRecordNames + 1] and recordNameChars (awfmRecordNames).  Pairs of offsets and
 * arena that come together or not at all (one without the other: AwFmNullPtrError): nameOffsets [numReads + 1] / nameChars,
 * mdOffsets [numReads + 1] / mdChars.  Optional, NULL allowed: qualities (numReadChars bytes parallel to readChars),
 * mappingQualities, secondScores, baseFlags [numReads], properPairs [numReads / 2].  flags: 0 or AWFM_SAM_PAIRED (reads 2p and
 * 2p + 1 are mates, the mate of r is m = r ^ 1; numReads must be even).  The call TRUSTS the strings and the names: bytes are
 * copied as they are, offsets arrays are taken to ascend, and a line is taken to stay below 2^32 bytes.
 *
 * Per read r, with n = readOffsets[r + 1] - readOffsets[r], or 0 when those two are inverted:
 *   ALIGNED    scores[r] != 0 and < AWFM_VERIFY_TOO_LONG, slots[r] < C, s = sequences[r * C + slots[r]] < numRecordNames, and the
 *              read offsets are not inverted.  Otherwise UNALIGNED, counted in *numUnaligned.
 *   The line is these fields joined by tabs and ended by '\n'; integers are decimal without leading zeros:
 *     QNAME    the bytes nameChars[nameOffsets[r] .. nameOffsets[r + 1]); without names the decimal of r, of r / 2 when paired.
 *     FLAG     baseFlags[r] (NULL: 0), | 0x4 when unaligned; paired also | 0x1, | 0x40 (even r) or | 0x80 (odd r), | 0x2 when
 *              properPairs[r / 2] != 0 and both mates are aligned, | 0x8 when the mate is unaligned, | 0x20 when baseFlags[m] has
 *              0x10.
 *     RNAME POS  aligned: record s's name (recordNameChars[recordNameOffsets[s] .. [s + 1])) and textBegins[r] + 1; unaligned
 *              with an aligned mate: the mate's two; otherwise `*` and 0.
 *     MAPQ     aligned: mappingQualities[r] (NULL: 255); unaligned: 0.
 *     CIGAR    aligned: the bytes cigarChars[cigarOffsets[r] .. cigarOffsets[r + 1]), `*` when there are none; unaligned: `*`.
 *     RNEXT PNEXT  unpaired, or the mate is unaligned: `*` and 0; otherwise `=` when this line's RNAME is the mate's record, else
 *              the mate's record's name; then textBegins[m] + 1.
 *     TLEN     both mates aligned in the same record: with b the smaller of the two textBegins and e the larger of the two
 *              textEnds, the mate with the smaller textBegins (a tie: the even read) gets e - b, the other -(e - b), in 64-bit
 *              two's complement; else 0.
 *     SEQ      the n read bytes, `*` when n == 0.   QUAL  the n parallel bytes of qualities; `*` without them or when n == 0.
 *     tags, for an aligned read only, in this order: NM:i:editDistances[r], AS:i:scores[r], XS:i:secondScores[r] when that
 *              array is given, MD:Z: and the bytes mdChars[mdOffsets[r] .. mdOffsets[r + 1]) when the pair is given and there
 *              are any.
 *
 * OUTPUTS (struct AwFmSamOutputs; every pointer may be NULL): lineOffsets [numReads + 1] are the exclusive prefix sums of the
 * TRUE line lengths whatever lineCapacity is; lineChars is an arena of lineCapacity bytes.  An arena without its offsets:
 * AwFmNullPtrError; offsets without an arena size one.  With an arena, a line is written exactly when lineOffsets[r + 1] <=
 * lineCapacity and otherwise counted in *numOverflow; no byte beyond min(total, capacity) is written, nor any byte of a line
 * that does not fit.  Both counters are ADDED to.  numReads == 0 succeeds and touches nothing.
 *
 * Refusals, in this order: a missing required array, half a pair, an arena without its offsets: AwFmNullPtrError; C outside
 * 1..16, another flag bit, odd numReads with AWFM_SAM_PAIRED, numReads >= 2^32: AwFmIllegalPositionError.
 *
 * awfmSamRecords (csrc/awfm_sam.c): over `threads` threads of the pool; ONE formatter counts and writes.
 * awfmGpuSamRecords (csrc/awfm_sam_kernel.h): every pointer is a device pointer of the caller's; asynchronous on `stream`, no
 * host wait, no allocation.  A lengths kernel (a thread per read), the library's on-device scan, and a write kernel: a WAVE
 * per read, whose lanes each own one field -- they compute the fields' places by a prefix sum over the lanes and the decimal
 * digits in registers --, while the reads, names and strings are copied by all lanes; the line is staged in LDS and stored in
 * whole dwords, bytes only at its two edges; a line beyond the LDS tile goes out in lane-consecutive bytes ($AWFM_GPU_DIAG
 * sam_tier=direct: every line; tests, the result is the same).  dScratch: awfmGpuSamRecordsScratchBytes(g, numReads) bytes,
 * 16-byte aligned (AwFmIllegalPositionError otherwise; NULL: AwFmNullPtrError), this call's own until it has finished -- two
 * streams may run the call at once with a dScratch each.
 *
 * awfmRecordNames (host only): the first whitespace-delimited token of every record's header (the whole header when it has no
 * whitespace; an index without a FASTA trailer: AwFmUnsupportedVersionError), packed behind offsets [numRecords + 1] (required);
 * chars == NULL sizes the arena, otherwise the names that fit `capacity` whole are written (offsets[i + 1] <= capacity).
 * awfmSamHeader (host only): "@HD\tVN:1.6\tSO:unknown\n" and one "@SQ\tSN:<that token>\tLN:<the record's length>\n" per
 * record; returns the header's true length; out == NULL sizes it, otherwise the lines that fit `capacity` whole are written;
 * 0 for an index without records.
 * Out of scope: BAM bytes, header lines on the device, reversing SEQ or QUAL inside this call ("strands" below: awfmGpuOrientReads
 * hands over the chosen strand's bytes with the qualities reversed, awfmGpuChooseStrands writes baseFlags), supplementary
 * records, other optional tags; how pairing defines templateLengths is untouched (TLEN here is the SAM one). */
#define AWFM_SAM_PAIRED 1u /* flags: reads 2p and 2p + 1 are mates; numReads must be even */
struct AwFmSamInputs {
  /* reads */
  const uint8_t *readChars;
  uint64_t numReadChars;
  const uint64_t *readOffsets; /* [numReads + 1] */
  const uint8_t *qualities;    /* NULL, or numReadChars bytes parallel to readChars, printed as they are */
  const uint64_t *nameOffsets; /* [numReads + 1]; with nameChars, or both NULL: QNAME is a decimal number */
  const uint8_t *nameChars;
  /* records */
  const uint64_t *recordNameOffsets; /* [numRecordNames + 1] */
  const uint8_t *recordNameChars;
  uint32_t numRecordNames;
  /* the alignment, as the alignment and string calls left it */
  const uint32_t *sequences;     /* [numReads * maxCandidates]  the slot table's */
  const uint32_t *slots;         /* [numReads] */
  const uint32_t *scores;        /* [numReads] */
  const uint32_t *editDistances; /* [numReads] */
  const uint64_t *textBegins;    /* [numReads]  sequence-local */
  const uint64_t *textEnds;      /* [numReads]  sequence-local */
  const uint64_t *cigarOffsets;  /* [numReads + 1]  awfmGpuAlignmentStrings' outputs, complete arenas */
  const uint8_t *cigarChars;
  const uint64_t *mdOffsets; /* [numReads + 1]; with mdChars, or both NULL: no MD tag */
  const uint8_t *mdChars;
  /* optional, NULL allowed */
  const uint8_t *mappingQualities; /* [numReads]; NULL: 255 */
  const uint32_t *secondScores;    /* [numReads]; NULL: no XS tag */
  const uint16_t *baseFlags;       /* [numReads]; the caller's bits (0x10 strand, 0x100 secondary, ...); NULL: 0 */
  const uint8_t *properPairs;      /* [numReads / 2]; read only with AWFM_SAM_PAIRED; NULL: no pair is proper */
};
struct AwFmSamOutputs {
  uint64_t *lineOffsets; /* [numReads + 1] */
  uint8_t *lineChars;    /* lineCapacity bytes */
  uint64_t lineCapacity;
  uint64_t *numUnaligned; /* one counter, added to */
  uint64_t *numOverflow;  /* one counter, added to */
};
enum AwFmReturnCode awfmSamRecords(const struct AwFmSamInputs *in, uint64_t numReads, uint32_t maxCandidates, uint32_t flags,
                                   const struct AwFmSamOutputs *out, unsigned threads);
uint64_t awfmGpuSamRecordsScratchBytes(const AwFmGpuIndex *g, uint64_t numReads);
enum AwFmReturnCode awfmGpuSamRecords(AwFmGpuIndex *g, const struct AwFmSamInputs *dIn, uint64_t numReads, uint32_t maxCandidates,
                                      uint32_t flags, const struct AwFmSamOutputs *dOut, void *dScratch, void *stream);
enum AwFmReturnCode awfmRecordNames(const struct AwFmIndex *index, uint64_t *offsets, uint8_t *chars, uint64_t capacity);
uint64_t awfmSamHeader(const struct AwFmIndex *index, uint8_t *out, uint64_t capacity);

/* ---- strands: both strands of the reads on a one-strand index: choose, pair and orient ----
 * The stage that lets an index of ONE strand place reads of either: the caller searches every read twice, as sequenced and
 * reverse-complemented, and these two calls choose per read (or per pair) the strand and slot, name the rescue windows on the
 * right strand, and gather the chosen strand of every read into a batch on which affine alignment, alignment strings and SAM
 * records run as they are.  The host twins (csrc/awfm_strands.c) are the definition and the checkers of the device calls.
 *
 * LAYOUT.  ONE batch of 2R rows: rows [0, R) are the reads as sequenced (row F(r) = r), rows [R, 2R) their reverse
 * complements (row V(r) = R + r), made by awfmGpuReverseComplementReads(..., AWFM_COMPLEMENT_ALL) into the second half of the
 * buffer.  Seeds, candidates, chains and slot scores (affine, matrix or end bonus) run on the 2R rows as they are.  With C =
 * maxCandidates (1..16), read r has 2C STRAND SLOTS u = sigma * C + j: slot j of row r + sigma * R, sigma = 0 as sequenced,
 * sigma = 1 the reverse strand.
 *
 * awfmChooseStrands / awfmGpuChooseStrands.  Inputs (struct AwFmStrandInputs): readOffsets [2R + 1]; sequences, slotScores,
 * slotReadEnds, slotTextEnds [2R * C] exactly as slot scores left them.  flags: 0, or AWFM_STRANDS_PAIRED: reads 2p and 2p + 1
 * are mates (R even) that come from OPPOSITE strands of one fragment -- FR and RF libraries, told apart by the sign of the
 * interval; same-strand libraries are out of scope.  params is pair mates' struct; unpaired, only minScore and mapqCap are read.
 * n_r = readOffsets[r + 1] - readOffsets[r] is the length of read r (64-bit two's complement).  A read is MALFORMED when the
 * offsets of F(r) or of V(r) are inverted or the two lengths differ: none of its strand slots counts, and it is counted in
 * *numMalformed.  All sums of positions are 64-bit two's complement, values and qualities 64-bit, as in "pair mates".
 *
 * Per read r, in both modes:
 *   1. a strand slot COUNTS by slot scores' rule 1: its score is none of the status values and is >= max(minScore, 1).
 *   2. BEST(r) is the counting strand slot of the largest score, ties to the lowest u: the forward strand first, then the lowest
 *      slot.  bestScores[r] is its score, 0 without one.
 *   3. a counting strand slot DUPLICATES another when both lie on ONE strand, name one sequence and have one (readEnd, textEnd).
 *      Strand slots on different strands are never duplicates: a palindromic read placed equally on both strands has a second
 *      as good as its best and gets quality 0.
 *   4. SECOND(r) is the largest-scoring counting strand slot that is neither the best nor its duplicate; secondScores[r] is its
 *      score, 0 without one (what XS:i wants).
 *   5. q_r = 0 without a best, else floor(mapqCap * (best - second) / best).
 * UNPAIRED: the chosen strand slot is the best; mappingQualities[r] = q_r.
 * PAIRED, per pair p (m1 = 2p, m2 = 2p + 1).  A CANDIDATE is (u1 of m1, u2 of m2), both counting.
 *   6. it is CONCORDANT when the two lie on different strands, name one sequence and minInsert <= T <= maxInsert, where A is the
 *      one on strand 0, B the one on strand 1, S = (int64) textEnd - readEnd and T = S(B) + n_B - S(A), n_B the length of B's
 *      read.  Its value is the sum of the two scores.
 *   7. the DISCORDANT candidate is (best(m1), best(m2)); it exists when both reads have a best and that pair is not concordant
 *      (two bests on one strand never are).  Its value is max(0, sum - unpairedPenalty).
 *   8. the WINNER: the largest value, then a concordant one first, then the lowest u1, then the lowest u2.  The winner's strand
 *      slots are the chosen ones.  With one read placed and no candidate that read's best is chosen and the other read gets
 *      none; with none placed neither gets one.
 *   9. properPairs, pairScores, pairSecondScores, templateLengths, pairQualities and the reads' mappingQualities are pair mates'
 *      rules 4 to 6 with "strand slot" for "slot", rule 3 above for sameness, and q_r as the given quality.
 *  10. RESCUE WINDOWS, indexed by ROW [2R] so that awfmGpuScoreWindowsAffine takes them on the 2R-row batch unchanged: read r
 *      gets a window when its pair is not proper and its mate m has a best (sigma_m, j), with S that slot's start:
 *        sigma_m = 0: row V(r) gets [S + minInsert - n_r - windowPad, S + maxInsert + windowPad);
 *        sigma_m = 1: with E = S + n_m, row F(r) gets [E - maxInsert - windowPad, E - minInsert + n_r + windowPad),
 *      each bound signed 64-bit and then raised to 0; windowSequences is that slot's sequence.  Every other row -- all rows when
 *      unpaired -- gets AWFM_CANDIDATES_NONE, 0, 0.
 * Outputs (struct AwFmStrandOutputs; every pointer may be NULL, counters are added to, R == 0 touches nothing).  Per read [R]:
 * strands (0 without a chosen slot), strandSlots (j, or AWFM_CHAINS_NO_SLOT), bestScores, secondScores, mappingQualities,
 * baseFlags (0x10 when the chosen slot is on strand 1, else 0: what awfmGpuSamRecords takes).  Per row [2R]: rowSlots (the chosen
 * j at the chosen row, AWFM_CHAINS_NO_SLOT at every other row: what the slot calls take on the 2R rows) and the windows.  Per
 * pair [R / 2], written only when paired: properPairs, pairScores, pairSecondScores, templateLengths, pairQualities.  Counters:
 * *numReverse (reads whose chosen slot is on strand 1), *numProper, *numWindows, *numMalformed.
 * Refusals, in this order: in, out, params or a required array NULL: AwFmNullPtrError; C outside 1..16, 2R >= 2^32, another
 * flag bit, odd R with AWFM_STRANDS_PAIRED, and -- paired -- minInsert > maxInsert or either beyond +-2^40, and mapqCap above
 * AWFM_SCORE_MAX_MAPQ: AwFmIllegalPositionError.
 * awfmChooseStrands: on the host over `threads` threads of the pool, the rules as written.  awfmGpuChooseStrands
 * (csrc/awfm_strands_kernel.h): ONE launch, asynchronous on `stream`; no scratch, no allocation, no host wait, nothing of the
 * image but its device: two streams may run it on one image at once.  Paired: 32 lanes a pair for C <= 4 (the orientation in
 * the lane's fifth bit), a wave a pair above; unpaired: 16 lanes a read.  $AWFM_GPU_DIAG strand_group=64 forces the wave per
 * pair or per read (tests; the result does not depend on it).
 *
 * awfmOrientReads / awfmGpuOrientReads: the gather that turns the 2R-row batch and strands [R] into an R-row batch.  Inputs
 * (struct AwFmOrientInputs): `rows`, the struct AwFmVerifyInputs of the 2R rows (readChars, readOffsets [2R + 1] required; each
 * of the six slot columns may be NULL); optionally slotScores, slotReadEnds, slotTextEnds [2R * C]; optionally qualities,
 * numReadChars bytes parallel to readChars of which only the forward rows' are read; strands [R], required.  Outputs (struct
 * AwFmOrientOutputs): readChars of `capacity` bytes and readOffsets [R + 1], required; qualities, the six slot columns and the
 * three score columns [R * C], each required exactly when its input is given (one without the other: AwFmNullPtrError);
 * *numMalformed, added to, may be NULL.
 *   readOffsets[r] (out) = readOffsets[r] - readOffsets[0] (in) for r = 0 .. R, always written: read r's output bytes are
 *   [readOffsets[r] - readOffsets[0], readOffsets[r + 1] - readOffsets[0]).
 *   Read r is WELL FORMED when the offsets of F(r) and of V(r) ascend and stay within numReadChars, the two rows are equally
 *   long, strands[r] <= 1, readOffsets[r] >= readOffsets[0] and its output bytes end within capacity.  Its characters are the
 *   bytes of row r + strands[r] * R; its qualities the forward row's, copied when strands[r] = 0 and REVERSED (not
 *   complemented) when 1; its slot and score columns that row's.
 *   A MALFORMED read: no byte of characters or qualities is written; its columns are written as unused (sequences =
 *   AWFM_CANDIDATES_NONE, slotScores = AWFM_VERIFY_NONE, everything else 0); it is counted in *numMalformed.
 * Refusals, in this order: NULL in, out or a required array, an output without its input or the reverse: AwFmNullPtrError; C
 * outside 1..16, 2R >= 2^32, input and output characters (numReadChars and capacity bytes) or input and output qualities
 * overlapping as pointer ranges: AwFmIllegalPositionError.  R == 0 touches nothing.
 * awfmOrientReads: on the host over `threads` threads.  awfmGpuOrientReads: one launch, asynchronous on `stream`, a wave per
 * read: lanes own ALIGNED words of the output, their sources are funnelled from one or two aligned words of the input, bytes
 * are stored singly only at a read's two edges; lanes 0 .. C - 1 copy the columns.
 *
 * THE LOOP, without a host wait: awfmGpuReverseComplementReads (ALL, into the second half), seeds .. slot scores on 2R rows,
 * awfmGpuChooseStrands, awfmGpuScoreWindowsAffine on the windows it names (2R rows), slot scores and awfmGpuChooseStrands
 * again, awfmGpuOrientReads, then awfmGpuAlignChainsAffine with strandSlots, awfmGpuAlignmentStrings and awfmGpuSamRecords with
 * baseFlags, properPairs and mappingQualities on R rows.  Out of scope: same-strand libraries, per-orientation insert
 * estimates (awfmGpuInsertHistogram keeps working on same-strand tables only), supplementary records. */
#define AWFM_STRANDS_PAIRED 1u /* flags: reads 2p and 2p + 1 are mates from opposite strands; numReads must be even */
struct AwFmStrandInputs {
  const uint64_t *readOffsets;  /* [2 numReads + 1] */
  const uint32_t *sequences;    /* [2 numReads * C]  the slot table's */
  const uint32_t *slotScores;   /* [2 numReads * C]  struct AwFmSlotScoreOutputs' */
  const uint32_t *slotReadEnds; /* [2 numReads * C] */
  const uint64_t *slotTextEnds; /* [2 numReads * C] */
};
struct AwFmStrandOutputs {
  /* per read */
  uint8_t *strands;          /* [numReads]  0 or 1; 0 without a chosen slot */
  uint32_t *strandSlots;     /* [numReads]  the shape of bestSlots, for the oriented batch */
  uint32_t *bestScores;      /* [numReads] */
  uint32_t *secondScores;    /* [numReads] */
  uint8_t *mappingQualities; /* [numReads] */
  uint16_t *baseFlags;       /* [numReads]  0x10 or 0: struct AwFmSamInputs' */
  /* per row */
  uint32_t *rowSlots;        /* [2 numReads]  the shape of bestSlots, for the 2R-row batch */
  uint32_t *windowSequences; /* [2 numReads]  struct AwFmWindowInputs'; AWFM_CANDIDATES_NONE: no window */
  uint64_t *windowBegins;    /* [2 numReads] */
  uint64_t *windowEnds;      /* [2 numReads] */
  /* per pair, written with AWFM_STRANDS_PAIRED only */
  uint8_t *properPairs;       /* [numReads / 2] */
  uint32_t *pairScores;       /* [numReads / 2] */
  uint32_t *pairSecondScores; /* [numReads / 2] */
  int64_t *templateLengths;   /* [numReads / 2]  T of a proper pair, else 0 */
  uint8_t *pairQualities;     /* [numReads / 2] */
  /* counters, added to */
  uint64_t *numReverse, *numProper, *numWindows, *numMalformed;
};
struct AwFmOrientInputs {
  struct AwFmVerifyInputs rows; /* the 2 numReads rows; the six slot columns may be NULL */
  const uint32_t *slotScores;   /* [2 numReads * C]  may be NULL, like the two below */
  const uint32_t *slotReadEnds;
  const uint64_t *slotTextEnds;
  const uint8_t *qualities; /* NULL, or rows.numReadChars bytes parallel to rows.readChars */
  const uint8_t *strands;   /* [numReads] */
};
struct AwFmOrientOutputs {
  uint8_t *readChars; /* capacity bytes */
  uint64_t capacity;
  uint64_t *readOffsets; /* [numReads + 1] */
  uint8_t *qualities;    /* capacity bytes */
  uint32_t *sequences;   /* the nine columns: [numReads * C] */
  uint32_t *chainAnchors;
  uint32_t *chainReadBegins;
  uint32_t *chainReadEnds;
  int64_t *chainBeginDiagonals;
  int64_t *chainEndDiagonals;
  uint32_t *slotScores;
  uint32_t *slotReadEnds;
  uint64_t *slotTextEnds;
  uint64_t *numMalformed; /* one counter, added to */
};
enum AwFmReturnCode awfmChooseStrands(const struct AwFmStrandInputs *in, uint64_t numReads, uint32_t maxCandidates, uint32_t flags,
                                      const struct AwFmPairParams *params, const struct AwFmStrandOutputs *out, unsigned threads);
enum AwFmReturnCode awfmGpuChooseStrands(AwFmGpuIndex *g, const struct AwFmStrandInputs *dIn, uint64_t numReads, uint32_t maxCandidates,
                                         uint32_t flags, const struct AwFmPairParams *params, const struct AwFmStrandOutputs *dOut,
                                         void *stream);
enum AwFmReturnCode awfmOrientReads(const struct AwFmOrientInputs *in, uint64_t numReads, uint32_t maxCandidates,
                                    const struct AwFmOrientOutputs *out, unsigned threads);
enum AwFmReturnCode awfmGpuOrientReads(AwFmGpuIndex *g, const struct AwFmOrientInputs *dIn, uint64_t numReads, uint32_t maxCandidates,
                                       const struct AwFmOrientOutputs *dOut, void *stream);

/* -1 = automatic (default), 0 = never, 1 = whenever the ordered path applies */
void awfmGpuIndexSetOrdered(AwFmGpuIndex *g, int mode);
/* 1 when awfmGpuSearchHits would search such a batch in seed order on this image (reporting, bench.py) */
int awfmGpuSearchHitsIsOrdered(const AwFmGpuIndex *g, int hasOffsets, uint32_t fixedLength, uint64_t numQueries);
/* STREAMS AND THE IMAGE'S SCRATCH.  The seed-order searches and the list's ordering share scratch memory that belongs to the
 * image, and the image orders its use across streams with events.  For a stream the caller created, the event of a use is
 * not recorded when the use is enqueued (a recorded event leaves the queue idle for ~5 us; a search followed by another on the
 * SAME stream needs none) but when a search on ANOTHER stream needs the scratch -- on the first stream, behind whatever it has
 * been given since.  The image therefore keeps the handle of the last stream that used each piece of scratch.  Rule: a stream
 * that has searched on an image must either outlive the image, or be RETIRED before it is destroyed:
 * awfmGpuStreamRetire(g, stream) records what is still owed on it and forgets the handle (cheap; no wait unless an event
 * cannot be recorded).  The null stream and hipStreamPerThread need nothing: their uses are recorded at once. */
void awfmGpuStreamRetire(AwFmGpuIndex *g, void *stream);

/* measurement hook: with $AWFM_GPU_TIME_ORDERED set, awfmGpuSearchHits brackets its dominant kernel (orderedSearchKernel,
 * or encodeLookupKernel when the batch was one for "lookup first") with HIP events on the launch stream; this returns the
 * last bracket in ms (<0: none).  Reporting calls: this one and the two below may wait for the device. */
double awfmGpuLastOrderedKernelMs(AwFmGpuIndex *g);
/* 1 when the last seed-order search on the image looked the table entries up while encoding ("lookup first": batches of
 * ASCII k-mers of which, by a sample, fewer than a quarter are still alive after the deeper table; only those are then
 * ordered and searched; $AWFM_GPU_LOOKUP_FIRST=0 / 1: never / whenever it applies) -- the timed kernel is then
 * encodeLookupKernel */
int awfmGpuLastOrderedKernelIsLookup(AwFmGpuIndex *g);
/* Which front end(s) the last SAMPLED search on the image launched (reporting): 0 both -- the sample's verdict stays on the
 * device and the kernels of the front end it does not choose return at once --, 1 the lookup kernel only, 2 the ordering
 * passes and the ordered kernel only; -1: no sampled search yet.  1 and 2 happen when the verdict of an earlier search of
 * the same k-mer length has reached the host (it is published in page-locked memory by the kernel that takes the sample;
 * nothing waits for it): a stream of like batches then pays for one front end's launches, not two ($AWFM_GPU_LOOKUP_PREDICT=0:
 * always both).  Either front end alone searches any batch correctly; a verdict that contradicts the mode its own search
 * ran in switches the prediction off for the next 8, 16, ... searches. */
int awfmGpuLastLookupFront(AwFmGpuIndex *g);
/* Whether the last awfmGpuSearch on the image (also the one behind a hits-only search that the seed-order path did not take)
 * went through exactLookupSearchKernel -- the exact ranges from one table entry per k-mer -- (1) or the general kernel (0);
 * reporting only */
int awfmGpuLastSearchWasExactLookup(AwFmGpuIndex *g);
/* with $AWFM_GPU_TIME_ORDERED: orderedSearchKernel's own bracket of the last search, whichever kernel was the dominant one
 * (after encodeLookupKernel it searched only the k-mers that kernel kept); < 0: none */
double awfmGpuLastOrderedSearchKernelMs(AwFmGpuIndex *g);
/* the brackets of EVERY timed search since the last call (at most the last 1024), oldest first: frontMs[i] =
 * encodeLookupKernel's (< 0: that search had none), kernelMs[i] = orderedSearchKernel's; returns how many and empties the
 * log.  A loop of searches is timed kernel by kernel without a host wait inside the loop (bench.py). */
int awfmGpuOrderedKernelLog(AwFmGpuIndex *g, double *frontMs, double *kernelMs, int max);
/* k-mers the last seed-order search with 8-byte records ordered and searched: the batch, or what the lookup-first pass kept
 * of it (reporting; waits for the device) */
uint64_t awfmGpuLastOrderedKept(AwFmGpuIndex *g);
/* out = {tested, dropped}: the survivors the lookup kernel of the last seed-order search put to its second table window -- the
 * entry of a k-mer's LEFTMOST characters: a k-mer that occurs in the text has every window of itself in the text -- and those
 * the window dropped before any step.  Zeros when that kernel did not run.  Reporting: waits for the device. */
void awfmGpuLastSecondWindow(AwFmGpuIndex *g, uint64_t out[2]);

/* Instrumented run of the same kernel for the roofline accounting: tallyOut =
 * {queries that used the seed table, backward steps executed, distinct blocks over those steps,
 * query characters}.  Synchronous, not for timing. */
enum AwFmReturnCode awfmGpuSearchTally(AwFmGpuIndex *g, const uint8_t *dChars, const uint64_t *dOffsets,
                                       uint32_t fixedLength, uint64_t numQueries, uint64_t tallyOut[4]);

/* What the lookup-first kernel of mixed-length batches (awfm_mixed_lookup_kernel.h: one table entry per k-mer, from the table
 * of its own length or from the deeper table, then the steps of the k-mers still alive) has to read for this batch: an
 * instrumented pass over the same k-mers with every 128-B line marked in a bitmap.  tallyOut = {lines of the length tables
 * touched, lines of the deeper table touched, distinct (search level, 128-B line) pairs of the pair image, the same of the
 * one-letter image, k-mers still alive after their table entry, k-mers with hits, k-mers left to the general kernel,
 * block lines the steps of the k-mers still alive read as executed (no line shared between two k-mers)}.  Builds the length tables when the image can have them and has none yet;
 * AwFmUnsupportedVersionError when it cannot (amino, 2^32 positions or more, no narrow deeper table).  Synchronous, not for
 * timing. */
enum AwFmReturnCode awfmGpuMixedLookupLineTally(AwFmGpuIndex *g, const uint8_t *dChars, const uint64_t *dOffsets,
                                                uint64_t numQueries, uint64_t tallyOut[8]);

/* Instrumented run of the seed-order path of awfmGpuSearchHits on the same batch (encode + sort + search with every
 * line the search kernel reads marked in per-level bitmaps): the COMPULSORY memory traffic of that kernel, i.e. what an
 * ideal cache would still have to fetch.  tallyOut = {128-B lines of the seed table touched, lines of the deeper
 * device-only table touched, distinct (search level, 128-B line) pairs of the pair image, the same of the one-letter
 * image, k-mers the seed-order kernel searched, bytes of sorted record + key it reads per k-mer, k-mers with hits,
 * k-mers left to the general kernel}.  AwFmUnsupportedVersionError when the batch would not take the seed-order path
 * (awfmGpuSearchHitsIsOrdered).  Synchronous, not for timing. */
enum AwFmReturnCode awfmGpuSearchHitsLineTally(AwFmGpuIndex *g, const uint8_t *dChars, const uint64_t *dOffsets,
                                               uint32_t fixedLength, uint64_t numQueries, uint64_t tallyOut[8]);

/* dHitOffsets[numQueries+1] = exclusive scan of the range lengths; the total is
 * also copied to *totalHits (host) -- this call synchronises `stream`.
 * dScratch must hold awfmGpuScanScratchBytes(numQueries) bytes. */
uint64_t awfmGpuScanScratchBytes(uint64_t numQueries);
enum AwFmReturnCode awfmGpuHitOffsets(AwFmGpuIndex *g, const struct AwFmSearchRange *dRanges, uint64_t numQueries,
                                      uint64_t *dHitOffsets, void *dScratch, uint64_t *totalHits, void *stream);
/* The same from the 32-bit counts awfmGpuSearch / awfmGpuSearchHits wrote (a quarter of the bytes of the
 * ranges); exact, hence allowed, only for images below 2^32 positions. */
enum AwFmReturnCode awfmGpuHitOffsetsFromCounts(AwFmGpuIndex *g, const uint32_t *dCounts, uint64_t numQueries,
                                                uint64_t *dHitOffsets, void *dScratch, uint64_t *totalHits, void *stream);

/* The scan without the read-back: dHitOffsets[numQueries] (device) holds the total, nothing waits for the host.  From
 * the 32-bit counts (images below 2^32 positions) when dCounts is given, from the ranges otherwise. */
enum AwFmReturnCode awfmGpuHitOffsetsOnDevice(AwFmGpuIndex *g, const uint32_t *dCounts, const struct AwFmSearchRange *dRanges,
                                              uint64_t numQueries, uint64_t *dHitOffsets, void *dScratch, void *stream);
/* awfmGpuLocate with the number of hits read ON THE DEVICE (dHitOffsets[numQueries]): dPositions holds capacityHits
 * entries, the first min(total, capacityHits) hits are located; the caller learns the total whenever it next reads
 * dHitOffsets[numQueries] and repeats with a larger buffer if it was too small.  Asynchronous on `stream`. */
enum AwFmReturnCode awfmGpuLocateOnDevice(AwFmGpuIndex *g, const struct AwFmSearchRange *dRanges, const uint64_t *dHitOffsets,
                                          uint64_t numQueries, uint64_t capacityHits, uint64_t *dPositions, void *stream);

/* dPositions[dHitOffsets[i] + h] = text position of hit h (BWT order) of query i.
 * Asynchronous on `stream`. */
enum AwFmReturnCode awfmGpuLocate(AwFmGpuIndex *g, const struct AwFmSearchRange *dRanges,
                                  const uint64_t *dHitOffsets, uint64_t numQueries, uint64_t totalHits,
                                  uint64_t *dPositions, void *stream);

/* The same with the final positions written to outPositions instead of over dPositions (which stays the work array of
 * the walk): outPositions may be any memory the device can store to, e.g. page-locked host memory (awfmGpuHostAlloc),
 * in which case the kernel that produces the positions also delivers them and no device-to-host copy is needed. */
enum AwFmReturnCode awfmGpuLocateTo(AwFmGpuIndex *g, const struct AwFmSearchRange *dRanges,
                                    const uint64_t *dHitOffsets, uint64_t numQueries, uint64_t totalHits,
                                    uint64_t *dPositions, uint64_t *outPositions, void *stream);

/* A window of the batch's hit list: the hits numbered hitBegin .. hitEnd-1 (in the numbering of dHitOffsets, i.e. hit h of
 * query i has number dHitOffsets[i] + h), which belong to the queries queryBegin .. queryEnd-1 (any superset of the
 * queries whose lists meet the window will do); dPositions / outPositions hold hitEnd - hitBegin entries, entry 0 is hit
 * hitBegin.  A window may begin and end inside the list of one k-mer: this is how a locate whose hit list exceeds a
 * device-memory budget is taken in pieces (the reference grows every positionList on its own, ref
 * src/AwFmParallelSearch.c:315-387; here the list is flat and the budget bounds what is resident). */
enum AwFmReturnCode awfmGpuLocateWindow(AwFmGpuIndex *g, const struct AwFmSearchRange *dRanges, const uint64_t *dHitOffsets,
                                        uint64_t queryBegin, uint64_t queryEnd, uint64_t hitBegin, uint64_t hitEnd,
                                        uint64_t *dPositions, uint64_t *outPositions, void *stream);

/* Reporting for the drop-in AoS entry points: what the process's last awFmParallelSearchCount / Locate spent where, summed over
 * its chunks -- out = {wall ms, ms waiting for the host stages' turn, ms packing, ms in the device calls, ms scattering, chunks,
 * k-mers, hits, bytes the pack stage read + wrote, bytes the scatter stage read + wrote} (the lanes overlap: the sums of the
 * stages exceed the wall time) -- and the copy rate this box gives `threads` of the same thread pool (GB/s, bytes read + bytes
 * written, over `bytes`): the pack and scatter stages move bytes and nothing else, so that rate bounds them. */
void awfmGpuAosLastStages(double out[10]);
double awfmHostCopyGBs(unsigned threads, uint64_t bytes);

/* ---- pinned staging for the drop-in AoS entry points ---- */
/* A grow-only page-locked host buffer cached in the image (slot 0..3); valid until the next call for the
 * same slot.  awfmGpuAosLock/Unlock serialise the AoS entry points that share these buffers. */
void *awfmGpuPinnedBuffer(AwFmGpuIndex *g, int slot, uint64_t bytes);
void awfmGpuAosLock(AwFmGpuIndex *g);
void awfmGpuAosUnlock(AwFmGpuIndex *g);

/* ---- flat batch API on host buffers (upload, kernels, download) ---- */
/* Synchronous for the caller; the work is issued on the calling thread's own stream (hipStreamPerThread), so
 * several host threads (or the lanes of the AoS entry points) overlap on the device.
 * ranges / counts may be NULL. */
enum AwFmReturnCode awfmGpuCountHost(AwFmGpuIndex *g, const uint8_t *chars, const uint64_t *offsets,
                                     uint32_t fixedLength, uint64_t numQueries, struct AwFmSearchRange *ranges,
                                     uint32_t *counts);
/* hitOffsets[numQueries+1] is filled; *positions is a malloc'ed array of
 * hitOffsets[numQueries] entries that the caller frees. */
enum AwFmReturnCode awfmGpuLocateHost(AwFmGpuIndex *g, const uint8_t *chars, const uint64_t *offsets,
                                      uint32_t fixedLength, uint64_t numQueries, struct AwFmSearchRange *ranges,
                                      uint64_t *hitOffsets, uint64_t **positions);

/* awfmGpuLocateHost with the hits in sequence coordinates: (*sequenceNumbers)[h], (*localPositions)[h] for hit number h of the
 * flat hit list (both malloc'ed, hitOffsets[numQueries] entries, the caller frees them), *numIllegal (may be NULL) = how many of
 * them are illegal positions (sequence 0xFFFFFFFF, global position kept).  The mapping runs on the device on every window of
 * hits before it is downloaded (12 instead of 8 bytes per hit come back; the windows are those of awfmGpuLocateHost:
 * $AWFM_GPU_HIT_BUDGET_BYTES).  AwFmUnsupportedVersionError when the image has no record table. */
enum AwFmReturnCode awfmGpuLocateHostLocal(AwFmGpuIndex *g, const uint8_t *chars, const uint64_t *offsets, uint32_t fixedLength,
                                           uint64_t numQueries, struct AwFmSearchRange *ranges, uint64_t *hitOffsets,
                                           uint32_t **sequenceNumbers, uint64_t **localPositions, uint64_t *numIllegal);

/* The same with the hit list delivered in windows, for batches whose hits exceed what may be resident on the device
 * ($AWFM_GPU_HIT_BUDGET_BYTES; default a quarter of the free device memory, at most 2^31 hits): hitOffsets[0..numQueries]
 * is complete before the first call of the sink; the sink then receives consecutive windows [hitBegin, hitEnd) of the
 * flat hit list (hit h of query i has number hitOffsets[i] + h), `positions` holding hitEnd - hitBegin entries in
 * page-locked staging that stays valid until the sink returns, and the queries queryBegin .. queryEnd-1 whose lists meet
 * the window (the first and the last may be cut).  While the sink runs, the next window is walked and downloaded.  A
 * non-zero return stops the batch.  A batch that fits the budget is one window.  This is what the drop-in AoS entry
 * points run on (hold awfmGpuAosLock: the staging is slot 3 of the image's pinned buffers). */
typedef int (*AwFmGpuHitWindowSink)(void *user, uint64_t queryBegin, uint64_t queryEnd, uint64_t hitBegin, uint64_t hitEnd,
                                    const uint64_t *positions);
enum AwFmReturnCode awfmGpuLocateHostWindows(AwFmGpuIndex *g, const uint8_t *chars, const uint64_t *offsets,
                                             uint32_t fixedLength, uint64_t numQueries, struct AwFmSearchRange *ranges,
                                             uint64_t *hitOffsets, AwFmGpuHitWindowSink sink, void *user);

/* ---- packed k-mers and the chunked host-buffer pipeline (awfm_gpu_stream.hip) ----
 * The reference's batch is an array of structs: a kmerString pointer in and a malloc'ed positionList out per
 * k-mer (ref src/AwFmParallelSearch.c:36-93, :367-387).  These entry points take the batch flat and bit-packed
 * and return it flat, cut into chunks whose upload, kernels and download overlap.
 *
 * Packed k-mer: one 64-bit word per k-mer of kmerLength characters, first character most significant, last
 * character in the lowest bits; nucleotide 2 bits per character (a 0, c 1, g 2, t/u 3; kmerLength <= 32), amino
 * 5 bits per character = the letter index of ref src/AwFmLetter.c:55-67 (a 0, c 1, d 2, ... y 19; 20..31 search
 * as the ambiguity letter x; kmerLength <= 12).  Nucleotide ambiguity characters cannot be expressed: batches
 * that contain them go through the ASCII entry points. */
/* host-side packing of n fixed-length ASCII k-mers; returns AwFmIllegalPositionError and the number of the first
 * k-mer that cannot be expressed in *firstUnpackable (may be NULL) */
enum AwFmReturnCode awfmPackKmers(enum AwFmAlphabetType alphabet, const uint8_t *chars, uint32_t kmerLength,
                                  uint64_t numKmers, uint64_t *packedOut, uint64_t *firstUnpackable);
/* the same on device buffers, and back.  K-mers that cannot be expressed are counted in *numUnpackable and become the
 * all-ones word -- itself a k-mer ('t' x 32), so the call then returns AwFmIllegalPositionError like awfmPackKmers: the
 * output of such a batch must not be searched (search it as ASCII instead) */
enum AwFmReturnCode awfmGpuPackKmers(AwFmGpuIndex *g, const uint8_t *dChars, uint32_t kmerLength, uint64_t numKmers,
                                     uint64_t *dPacked, uint64_t *numUnpackable, void *stream);
enum AwFmReturnCode awfmGpuUnpackKmers(AwFmGpuIndex *g, const uint64_t *dPacked, uint32_t kmerLength, uint64_t numKmers,
                                       uint8_t *dChars, void *stream);
/* awfmGpuSearchHits for bit-packed k-mers resident on the device.  Nucleotide batches that take the seed-order path are
 * searched straight from the packed words; other batches are unpacked into dCharsScratch (kmerLength bytes per k-mer;
 * may be NULL when the caller knows awfmGpuSearchHitsIsOrdered) and searched as ASCII.  Same outputs and contract. */
enum AwFmReturnCode awfmGpuSearchHitsPacked(AwFmGpuIndex *g, const uint64_t *dPacked, uint32_t kmerLength, uint64_t numKmers,
                                            struct AwFmSearchRange *dRanges, uint32_t *dCounts, uint8_t *dCharsScratch,
                                            void *stream);
/* page-locked host memory: batches handed over in it are read by the DMA engine directly, anything else is first
 * copied into the pipeline's own staging by hostThreads threads */
void *awfmGpuHostAlloc(uint64_t bytes);
void awfmGpuHostFree(void *p);
/* Receives the results of k-mers firstKmer .. firstKmer+numKmers-1: counts[i] hits of k-mer firstKmer+i (the
 * reference's uint32 count, ref src/AwFmIndex.h:112-118), and -- locate -- numPositions text positions, the
 * hits of k-mer firstKmer+i starting where those of firstKmer+i-1 end, each list in BWT order (what
 * awFmParallelSearchLocate puts into positionList).  The arrays are page-locked staging of the pipeline, valid until
 * the sink returns; chunks arrive in order; a non-zero return stops the batch.  The sink runs on the calling thread
 * while the image's pipeline is locked: it must not start another batch on the same image.
 * A chunk whose hits exceed the device's hit budget ($AWFM_GPU_HIT_BUDGET_BYTES; default a quarter of the free device
 * memory) arrives in several calls: consecutive groups of whole k-mers, and a k-mer whose own list exceeds a window
 * alone, in consecutive calls with the same firstKmer and numKmers == 1, each with the next slice of its list
 * (counts[0] is its full count every time).  Concatenating the positions of all calls gives the batch's flat list. */
typedef int (*AwFmGpuChunkSink)(void *user, uint64_t firstKmer, uint64_t numKmers, const uint32_t *counts,
                                const uint64_t *positions, uint64_t numPositions);
/* Counts (locate == 0) or locates numKmers packed host-resident k-mers in chunks of chunkKmers (0: 2^24) through
 * three pipeline slots: while the sink consumes chunk t-2 on the calling thread, chunk t-1 is in the kernels and
 * chunk t on its way to the device.  One batch at a time per image. */
enum AwFmReturnCode awfmGpuStreamPacked(AwFmGpuIndex *g, const uint64_t *packedKmers, uint32_t kmerLength,
                                        uint64_t numKmers, uint64_t chunkKmers, int locate, unsigned hostThreads,
                                        AwFmGpuChunkSink sink, void *user);
/* the same pipeline for fixed-length ASCII k-mers (any character the ASCII API accepts) */
enum AwFmReturnCode awfmGpuStreamChars(AwFmGpuIndex *g, const uint8_t *chars, uint32_t kmerLength, uint64_t numKmers,
                                       uint64_t chunkKmers, int locate, unsigned hostThreads, AwFmGpuChunkSink sink,
                                       void *user);
/* The same pipelines with SPARSE results: per chunk the k-mers with hits as a list -- hitKmers[j] = number of the j-th such
 * k-mer relative to firstKmer (ascending), its hits positions[hitOffsets[j] .. hitOffsets[j + 1]) in BWT order
 * (hitOffsets has numHitKmers + 1 entries; locate == 0: positions is NULL and the offsets only say how many hits each
 * has) -- instead of a count for every k-mer of the chunk: for a batch in which few k-mers occur the download shrinks
 * from 4 bytes per k-mer to 12 bytes per k-mer WITH hits, and nothing of the chunk's size is written after the search.
 * A chunk with more than numKmers / 64 k-mers with hits is searched again densely and its list made from the counts (and
 * so are the chunks after it): correct for any batch, fast for sparse ones.  A chunk whose hits exceed the device's hit
 * budget fails with AwFmAllocationFailure (the dense pipeline takes such chunks in windows). */
typedef int (*AwFmGpuSparseChunkSink)(void *user, uint64_t firstKmer, uint64_t numKmers, uint64_t numHitKmers,
                                      const uint32_t *hitKmers, const uint64_t *hitOffsets, const uint64_t *positions,
                                      uint64_t numPositions);
enum AwFmReturnCode awfmGpuStreamPackedSparse(AwFmGpuIndex *g, const uint64_t *packedKmers, uint32_t kmerLength,
                                              uint64_t numKmers, uint64_t chunkKmers, int locate, unsigned hostThreads,
                                              AwFmGpuSparseChunkSink sink, void *user);
enum AwFmReturnCode awfmGpuStreamCharsSparse(AwFmGpuIndex *g, const uint8_t *chars, uint32_t kmerLength, uint64_t numKmers,
                                             uint64_t chunkKmers, int locate, unsigned hostThreads, AwFmGpuSparseChunkSink sink,
                                             void *user);

/* whole batch into caller arrays: counts[numKmers]; *positions is malloc'ed (caller frees), *numPositions entries */
enum AwFmReturnCode awfmGpuCountPackedHost(AwFmGpuIndex *g, const uint64_t *packedKmers, uint32_t kmerLength,
                                           uint64_t numKmers, uint32_t *counts);
enum AwFmReturnCode awfmGpuLocatePackedHost(AwFmGpuIndex *g, const uint64_t *packedKmers, uint32_t kmerLength,
                                            uint64_t numKmers, uint32_t *counts, uint64_t **positions,
                                            uint64_t *numPositions);

/* ---- seeded synthetic inputs on the device (bench and full-size tests) ---- */
/* text characters start..start+count-1 of the stream `seed`; amino != 0 selects the 20-letter alphabet */
enum AwFmReturnCode awfmGpuSynthText(uint8_t *dOut, uint64_t start, uint64_t count, uint64_t seed, int amino,
                                     void *stream);
/* `count` uniform random k-mers (query ids first..first+count-1) of `length` characters, row-major */
enum AwFmReturnCode awfmGpuSynthRandomQueries(uint8_t *dOut, uint64_t first, uint64_t count, uint32_t length,
                                              uint64_t seedQ, int amino, void *stream);
/* `count` k-mers copied from the (unsanitised) device text at seeded uniform offsets */
enum AwFmReturnCode awfmGpuSynthPlantedQueries(uint8_t *dOut, uint64_t first, uint64_t count, uint32_t length,
                                               uint64_t seedQ, const uint8_t *dText, uint64_t textLength, void *stream);

/* A genome-shaped nucleotide text of `length` characters (csrc/awfm_synth.hip, synth.py genome_text): interspersed repeat
 * families (a 300-character unit in about length/3000 copies at 10 % divergence, a 6000-character one in cut copies at
 * 5 %), tandem repeats, 24 runs of 'n' of up to 10^7 characters, unique sequence in between. */
enum AwFmReturnCode awfmGpuSynthGenomeText(uint8_t *dOut, uint64_t length, uint64_t seed, void *stream);
/* awfmGpuSynthPlantedQueries with every character that is not a,c,g,t replaced by a seeded random letter */
enum AwFmReturnCode awfmGpuSynthPlantedQueriesClean(uint8_t *dOut, uint64_t first, uint64_t count, uint32_t length,
                                                    uint64_t seedQ, const uint8_t *dText, uint64_t textLength, void *stream);

/* `count` k-mers copied from the UNIQUE sequence of the genome-shaped text of awfmGpuSynthGenomeText(textSeed): the first of up
 * to 64 seeded offsets whose window lies in blocks that are no repeat's and holds only a,c,g,t; dOffsetsOut (may be NULL)
 * gets the offset each k-mer was taken from */
enum AwFmReturnCode awfmGpuSynthPlantedQueriesUnique(uint8_t *dOut, uint64_t first, uint64_t count, uint32_t length, uint64_t seedQ,
                                                     const uint8_t *dText, uint64_t textLength, uint64_t textSeed,
                                                     uint64_t *dOffsetsOut, void *stream);

/* mixed-length set: lengths lo..hi, even ids random, odd ids copied from the text.
 * Lengths first; the caller turns them into count+1 exclusive-scan offsets; then the characters. */
enum AwFmReturnCode awfmGpuSynthMixedLengths(uint64_t *dLengths, uint64_t first, uint64_t count, uint32_t lo,
                                             uint32_t hi, uint64_t seedQ, void *stream);
enum AwFmReturnCode awfmGpuSynthMixedQueries(uint8_t *dOut, const uint64_t *dOffsets, uint64_t first, uint64_t count,
                                             uint64_t seedQ, const uint8_t *dText, uint64_t textLength, int amino,
                                             void *stream);

/* ---- seed-bucket sharding of dense-hit batches over the GPUs of a node (round 6) ----
 * The reference treats the k-mers of a batch as independent (ref src/AwFmParallelSearch.c:103-129), so ANY split of a batch
 * over index replicas gives the same results.  A contiguous split of the batch hands every rank a THIN slice of the seed order
 * (one k-mer per two block lines where the whole batch has four per line): its search re-reads nothing from the L2 and an 8-way
 * split of 10^8 k-mers drawn from the text scales to 0.67.  These calls let N ranks split the ORDER instead: every rank
 * orders its own contiguous shard (awfmGpuOrderKmers: the counting and the partition pass, records {rest of the code string,
 * number in the WHOLE batch} in bucket order), the ranks exchange the records bucket range by bucket range (rank j gets the
 * buckets [j B / N, (j + 1) B / N) of everybody: contiguous slices, whose per-bucket runs the receiver puts together bucket by
 * bucket -- the caller's all-to-all; avxwindowfmindex_amd/dist.py does it over torch.distributed), and every rank searches the
 * dense N-th of the order it then holds (awfmGpuSearchOrderedRecords: results in that order, {number in the whole batch,
 * range}, hit offsets and positions by the calls that follow awfmGpuSearchHitsInOrder).  K-mers the seed-order kernel does not
 * take (ambiguity characters) stay with the rank that holds their characters (awfmGpuSearchGeneralRecords).
 * dBucketStart: awfmGpuOrderBuckets() + 3 words -- [b] = records before bucket b, [buckets] = records the seed-order kernel
 * takes, [buckets + 1] = numQueries, [buckets + 2] = the k-mers left to the general kernel (the records' tail).
 *
 * Which batches these calls take.  A record is 8 bytes: {rest of the k-mer's 2K-bit code string : 64 - indexBits, number in the
 * whole batch : indexBits}.  depth = the characters the table lookup consumes (the deeper device-only table's when the image
 * has one and K reaches it, the index's seed table's otherwise); bucketBits = min(11, 2 * depth): the bucket of a k-mer is the
 * leading bucketBits bits of its table index -- the code string of its LAST depth letters, where the backward search starts --
 * and is not stored; indexBits = bits(totalQueries - 1), between 1 and 32.  A record fits iff
 *     depth <= K <= 32,  1 <= totalQueries <= 2^32 - 2  and  2 K - bucketBits + indexBits <= 64
 * on a nucleotide image (kernel AUTO or GROUP4).  awfmGpuOrderBuckets answers 2^bucketBits then and 0 otherwise; with 0 the
 * other calls return AwFmIllegalPositionError and write nothing (32-mers on 2048 buckets: up to 2048 k-mers; 21-mers: any batch).
 * The records' bits are the library's own: between the calls they are only moved. */
uint32_t awfmGpuOrderBuckets(const AwFmGpuIndex *g, uint32_t fixedLength, uint64_t totalQueries); /* 0: not a batch for it */
enum AwFmReturnCode awfmGpuOrderKmers(AwFmGpuIndex *g, const uint8_t *dChars, uint32_t fixedLength, uint64_t numQueries,
                                      uint64_t firstNumber, uint64_t totalQueries, uint64_t *dRecords, uint32_t *dBucketStart,
                                      void *stream);
/* What a rank holds after the exchange, put in bucket order, in one launch: `dReceived` = the numSlices slices the ranks sent
 * (slice j begins at record dSliceAt[j]; each holds the sender's records of the buckets [firstBucket, endBucket), bucket by
 * bucket), dSliceStarts[j * (endBucket - firstBucket + 1) + b] = records of slice j before its bucket firstBucket + b (the
 * last one: the slice's length).  dRecords gets the runs of a bucket from all slices next to each other, slice by slice (any
 * order inside a bucket will do), dBucketStart the buckets + 3 words awfmGpuSearchOrderedRecords wants for an array that holds
 * those buckets only.  A rank that received nothing (every slice empty: its buckets hold no k-mer of the batch) makes the call
 * all the same: dReceived and dRecords are not null but neither is read or written, every word of dBucketStart becomes 0, and
 * awfmGpuSearchOrderedRecords over such an array succeeds and stores nothing. */
enum AwFmReturnCode awfmGpuMergeBucketRuns(AwFmGpuIndex *g, const uint64_t *dReceived, const uint64_t *dSliceAt, const uint32_t *dSliceStarts,
                                           uint32_t numSlices, uint32_t firstBucket, uint32_t endBucket, uint32_t buckets, uint64_t *dRecords,
                                           uint32_t *dBucketStart, void *stream);
/* the buckets [firstBucket, endBucket) of `dRecords` (bucket order, dBucketStart as above); entry e of the outputs belongs to
 * record dBucketStart[firstBucket] + e */
enum AwFmReturnCode awfmGpuSearchOrderedRecords(AwFmGpuIndex *g, const uint64_t *dRecords, const uint32_t *dBucketStart,
                                                uint32_t firstBucket, uint32_t endBucket, uint32_t fixedLength, uint64_t totalQueries,
                                                uint32_t *dOrderKmers, struct AwFmSearchRange *dOrderRanges, void *stream);
/* ... with the 32-bit counts in that order as well (dOrderCounts may be NULL), as awfmGpuSearchHitsInOrderCounts */
enum AwFmReturnCode awfmGpuSearchOrderedRecordsCounts(AwFmGpuIndex *g, const uint64_t *dRecords, const uint32_t *dBucketStart,
                                                      uint32_t firstBucket, uint32_t endBucket, uint32_t fixedLength, uint64_t totalQueries,
                                                      uint32_t *dOrderKmers, struct AwFmSearchRange *dOrderRanges, uint32_t *dOrderCounts,
                                                      void *stream);
/* the tail of a shard's own records through the general kernel: entries [dBucketStart[buckets], numQueries) of the outputs */
enum AwFmReturnCode awfmGpuSearchGeneralRecords(AwFmGpuIndex *g, const uint8_t *dChars, uint32_t fixedLength, uint64_t numQueries,
                                                uint64_t firstNumber, uint64_t totalQueries, const uint64_t *dRecords,
                                                const uint32_t *dBucketStart, uint32_t *dOrderKmers,
                                                struct AwFmSearchRange *dOrderRanges, void *stream);

#ifdef __cplusplus
}
#endif
#endif
