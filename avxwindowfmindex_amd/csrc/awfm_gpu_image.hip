/*
 * awfm_gpu_image.hip -- the device image of an index and its lifetime: upload + re-layout of the reference's arrays
 * (awfm_device.h), the registry behind awFmParallelSearch* (one image per index and device, lanes on it), the device-only
 * accelerators an image gets by its size (pair image, deeper seed table with next-step bits; the full suffix array:
 * awfm_gpu_dense_sa.hip), their setters, and what an image says of itself.  ref src/AwFmIndex.h:55-109, src/AwFmIndexStruct.c.
 */
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <system_error>
#include <vector>

#include "awfm_device.h"
#include "awfm_search_kernel.h"
#include "awfm_locate_kernel.h"

thread_local hipStream_t awfmGpuSetupStream = nullptr; /* awfm_device.h */
static thread_local std::string tlsError;
void awfmGpuSetError(const char *what) { tlsError = what; }
void awfmGpuSetHipError(const char *what, hipError_t e) { tlsError = std::string(what) + ": " + hipGetErrorString(e); }

/* ------------------------------------------------------------------ host side */

namespace {

std::mutex tableMutex;
struct ImageEntry {
  const AwFmIndex *index;
  AwFmGpuIndex *handle; /* its device, and its lane: 0 the primary, n the n-th lane on its image (a device named again in $AWFM_GPU_DEVICES) */
};
std::vector<ImageEntry> imageTable;

}  // namespace
enum AwFmReturnCode awfmGpuEnsureWork(AwFmGpuIndex *g, size_t bytes) {
  if (bytes <= g->workBytes) return AwFmSuccess;
  if (g->dWork) (void)hipFree(g->dWork);
  g->dWork = nullptr;
  g->workBytes = 0;
  const size_t want = bytes + bytes / 4 + 4096;
  AWFM_HIP_TRY(hipMalloc(&g->dWork, want), AwFmAllocationFailure);
  g->workBytes = want;
  return AwFmSuccess;
}


namespace {
void fillDevIndex(AwFmGpuIndex *g, const struct AwFmIndex *index, unsigned superShift, unsigned long long sentinelPos) {
  DevIndex &d = g->image->dev;
  d.blocks = (const uint4 *)g->image->dBlocks;
  d.super = (const unsigned long long *)g->image->dSuper;
  d.numSuper = (unsigned)awfmNumSuper(index->bwtLength, index->config.alphabetType == AwFmAlphabetAmino, superShift);
  d.nucSuperShift = superShift;
  d.seed = (const ulonglong2 *)g->image->dSeed;
  d.sa = (const unsigned long long *)g->image->dSa;
  d.bwtLength = index->bwtLength;
  d.sentinelPos = sentinelPos;
  d.seedLen = awfmKmerTableLength(index->config.alphabetType, index->config.kmerLengthInSeedTable);
  d.prefixSums = (const unsigned long long *)g->image->dPrefix;
  d.saRatio = index->config.suffixArrayCompressionRatio;
  d.saShift = 0xFFFFFFFFu;
  if ((d.saRatio & (d.saRatio - 1)) == 0) {
    d.saShift = 0;
    while ((1u << d.saShift) < d.saRatio) d.saShift++;
  }
  d.saWidth = index->suffixArray.valueBitWidth;
  d.seedK = index->config.kmerLengthInSeedTable;
  d.deepSeed = nullptr;
  d.deepK = 0;
  d.deepNarrow = 0;
  d.pairBlocks = nullptr;
  d.pairSuper = nullptr;
  d.pairSuper32 = nullptr;
  d.pairC = nullptr;
  d.numPairSuper = 0;
  d.pairSuperInLds = 0;
}
}  // namespace

/* lanes that cooperate on one query: image setting, else $AWFM_GPU_DIAG kernel=g4|g2|g1, else the default.  A device
 * block has 4 slices, so 4 lanes is the widest group (GROUP8 of the enum maps to it); amino slices are 32 B, 2 lanes
 * per query already hold 64 registers of block data */
int awfmGpuLanesPerQuery(const AwFmGpuIndex *g) {
  int lanes = 4;
  switch (g->kernel) {
    case AWFM_GPU_KERNEL_GROUP8:
    case AWFM_GPU_KERNEL_GROUP4: lanes = 4; break;
    case AWFM_GPU_KERNEL_GROUP2: lanes = 2; break;
    case AWFM_GPU_KERNEL_GROUP1: lanes = 1; break;
    default:
      /* measured on MI355X (scripts/ab_layout.sh): 10^8 random 21-mers against the GRCh38-sized index, general
       * kernel: g4 13.2-13.7 ms, g2 13.0-13.4, g1 13.9 (within the box-to-box spread: the kernel runs at the rate the
       * chip delivers random granules; g4 keeps 8 waves per SIMD without spilling); 5*10^7 amino 10-mers: g4 3.91 ms,
       * g2 3.72 */
      lanes = g->amino ? 2 : 4;
      if (const char *env = awfmGpuDiag("kernel")) { /* lanes per k-mer of the general kernel: g4 | g2 | g1 */
        if (!strcmp(env, "g8") || !strcmp(env, "g4")) lanes = 4;
        else if (!strcmp(env, "g2")) lanes = 2;
        else if (!strcmp(env, "g1")) lanes = 1;
      }
  }
  if (g->amino && lanes < 2) lanes = 2;
  return lanes;
}

constexpr unsigned kAutoDeepSeedMin = 14, kAutoDeepSeedMax = 16; /* depths of the device-only seed table large nucleotide images get by default */
extern "C" {
static enum AwFmReturnCode applyDeepSeedFromEnv(AwFmGpuIndex *g);
static enum AwFmReturnCode applyPairFromEnv(AwFmGpuIndex *g);
static bool startBuilder(AwFmGpuIndex *g);
}

/* a new image of `index` on `device` and its primary handle; nothing of it is on the device yet */
static AwFmGpuIndex *newImage(const struct AwFmIndex *index, int device) {
  AwFmGpuIndex *g = new AwFmGpuIndex();
  g->image = new AwFmGpuImage();
  g->image->handles.push_back(g);
  g->device = device;
  g->amino = index->config.alphabetType == AwFmAlphabetAmino;
  g->image->numBlocks = awfmDeviceBlocks(index->bwtLength);
  return g;
}

/* The tail of making an image, once its arrays are on the device: the kernels' view, then the optional accelerators -- the pair
 * image first (the deeper table's next-step bits are computed through it), then the deeper table and the full suffix array, or
 * (behind) a thread that builds those two behind the first searches.  deepRequired: a deeper table that was asked for and could
 * not be built fails the image; otherwise it carries on without one, as it does without the others. */
static enum AwFmReturnCode finishImage(AwFmGpuIndex *g, const struct AwFmIndex *index, unsigned superShift, unsigned long long sentinelPos,
                                       bool behind, bool deepRequired) {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, g->device) == hipSuccess && prop.multiProcessorCount > 0)
    g->numCUs = prop.multiProcessorCount;
  fillDevIndex(g, index, superShift, sentinelPos);
  if (const char *env = awfmKnob(AWFM_KNOB_FORCE_WIDE)) g->forceWide = atoi(env) != 0;
  /* the record table of a multi-record index: small and needed by the first mapping call, so it is not left to the builder thread */
  if (awfmGpuInstallRecordTableOf(g, index) != AwFmSuccess) return AwFmGeneralFailure;
  (void)applyPairFromEnv(g); /* without it (no memory left) searches simply take one step per read */
  if (behind && startBuilder(g)) return AwFmSuccess;
  if (applyDeepSeedFromEnv(g) != AwFmSuccess && deepRequired) return AwFmGeneralFailure;
  (void)awfmGpuApplyDenseSaAuto(g); /* without it (no memory left) a locate walks */
  return AwFmSuccess;
}

AwFmGpuIndex *awfmGpuIndexAdopt(const struct AwFmIndex *index, int device, void *dBlocks, void *dSuper, unsigned superShift,
                                void *dSeed, void *dSa, void *dPrefix, unsigned long long sentinelPos, uint64_t deviceBytes) {
  AwFmGpuIndex *g = newImage(index, device);
  g->image->dBlocks = dBlocks;
  g->image->dSuper = dSuper;
  g->image->dSeed = dSeed;
  g->image->dSa = dSa;
  g->image->dPrefix = dPrefix;
  g->image->deviceBytes = deviceBytes;
  (void)finishImage(g, index, superShift, sentinelPos, false, false);
  return g;
}

void awfmGpuIndexRegister(const struct AwFmIndex *index, AwFmGpuIndex *g) {
  std::lock_guard<std::mutex> lock(tableMutex);
  imageTable.push_back({index, g});
}

bool awfmGpuRelayout(const void *dRefBlocks, uint64_t bwtLength, bool amino, unsigned superShift, void *dBlocks,
                     void *dSuper, unsigned long long *sentinelPosOut) {
  const uint64_t numRef = awfmNumBlocks(bwtLength);
  const unsigned numSuper = (unsigned)awfmNumSuper(bwtLength, amino, superShift);
  unsigned long long *dSentinel = nullptr;
  hipError_t e = hipMalloc((void **)&dSentinel, 8);
  if (e == hipSuccess) e = hipMemset(dSentinel, 0, 8);
  if (e == hipSuccess) {
    const unsigned words = numSuper * (amino ? kAminoSuperStride : 4u);
    hipLaunchKernelGGL(gatherSuperKernel, dim3((words + 255) / 256), dim3(256), 0, 0, (const unsigned long long *)dRefBlocks,
                       (unsigned long long)numRef, amino ? 1 : 0, superShift, numSuper, (unsigned long long *)dSuper);
    const uint64_t threads = numRef * 2 * kSlices;
    const unsigned grid = (unsigned)((threads + 255) / 256);
    if (amino)
      hipLaunchKernelGGL(relayoutAminoKernel, dim3(grid), dim3(256), 0, 0, (const unsigned long long *)dRefBlocks,
                         (unsigned long long)numRef, (unsigned long long)bwtLength, (const unsigned long long *)dSuper,
                         (uint4 *)dBlocks, dSentinel);
    else
      hipLaunchKernelGGL(relayoutNucKernel, dim3(grid), dim3(256), 0, 0, (const unsigned long long *)dRefBlocks,
                         (unsigned long long)numRef, (unsigned long long)bwtLength, superShift,
                         (const unsigned long long *)dSuper, (uint4 *)dBlocks, dSentinel);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(sentinelPosOut, dSentinel, 8, hipMemcpyDeviceToHost);
  if (dSentinel) (void)hipFree(dSentinel);
  if (e != hipSuccess) {
    setError("awfmGpuRelayout", e);
    return false;
  }
  return true;
}

extern "C" {

int awfmGpuDeviceCount(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char *awfmGpuLastError(void) { return tlsError.c_str(); }

static enum AwFmReturnCode createImage(const struct AwFmIndex *index, int device, AwFmGpuIndex **out, bool deferAccelerators);
enum AwFmReturnCode awfmGpuIndexCreate(const struct AwFmIndex *index, int device, AwFmGpuIndex **out) {
  return createImage(index, device, out, false);
}
static void accelBuilder(AwFmGpuIndex *g);
/* images whose builder thread has not been joined yet */
static std::mutex buildingMutex;
static std::vector<AwFmGpuImage *> building;
/* the one place that joins an image's builder thread (it returns when the thread is done) */
static void joinBuilder(AwFmGpuImage *image) {
  std::lock_guard<std::mutex> lock(image->joinMutex);
  if (image->accelThread.joinable()) image->accelThread.join();
  std::lock_guard<std::mutex> listLock(buildingMutex);
  for (size_t i = 0; i < building.size(); i++)
    if (building[i] == image) {
      building[i] = building.back();
      building.pop_back();
      break;
    }
}
static void settleBuildersAtExit() {
  for (;;) {
    AwFmGpuImage *image = nullptr;
    {
      std::lock_guard<std::mutex> lock(buildingMutex);
      if (building.empty()) return;
      image = building.back();
    }
    joinBuilder(image);
  }
}
/* starts the thread that builds the image's deeper table and full suffix array behind its first searches; false: there is no
 * thread (the caller builds them itself) */
static bool startBuilder(AwFmGpuIndex *g) {
  AwFmGpuImage *image = g->image;
  image->accelState.store(1);
  try {
    image->accelThread = std::thread(accelBuilder, g);
  } catch (const std::system_error &) {
    image->accelState.store(0);
    return false;
  }
  /* a program that exits while a builder is at work (no awFmDeallocIndex) must not tear the runtime down under it */
  std::lock_guard<std::mutex> lock(buildingMutex);
  static bool hooked = false;
  if (!hooked) hooked = atexit(settleBuildersAtExit) == 0;
  building.push_back(image);
  return true;
}
static unsigned chooseDeepSeedK(const AwFmGpuIndex *g, std::string &notes);
static enum AwFmReturnCode buildDeepSeed(AwFmGpuIndex *g, unsigned deepK, AwFmGpuImage::PendingAccel *to);
static void installDeepSeed(AwFmGpuImage *image, AwFmGpuImage::PendingAccel *from);
static enum AwFmReturnCode createImage(const struct AwFmIndex *index, int device, AwFmGpuIndex **out, bool deferAccelerators) {
  if (!index || !out) {
    setError("awfmGpuIndexCreate: null argument");
    return AwFmNullPtrError;
  }
  *out = nullptr;
  if (awfmGpuDeviceCount() <= 0) {
    setError("awfmGpuIndexCreate: no HIP device available (this library has no CPU search path)");
    return AwFmGeneralFailure;
  }
  if (device < 0) {
    const char *env = awfmKnob(AWFM_KNOB_DEVICE);
    if (env && *env) {
      device = atoi(env);
    } else if (hipGetDevice(&device) != hipSuccess) {
      device = 0;
    }
  }
  DeviceGuard guard(device);
  if (!guard.ok) {
    setError("awfmGpuIndexCreate: hipSetDevice failed");
    return AwFmGeneralFailure;
  }
  const bool amino = index->config.alphabetType == AwFmAlphabetAmino;
  const unsigned superShift = awfmSuperShift(amino, index->bwtLength);
  if (!amino && awfmNumSuper(index->bwtLength, false, superShift) > kMaxNucSuper) {
    setError("awfmGpuIndexCreate: nucleotide device images hold at most 64 superblocks (2^38 positions)");
    return AwFmUnsupportedVersionError;
  }
  if (index->config.suffixArrayCompressionRatio == 0) {
    setError("awfmGpuIndexCreate: suffixArrayCompressionRatio must be >= 1");
    return AwFmGeneralFailure;
  }

  AwFmGpuIndex *g = newImage(index, device);
  const size_t refBytes = awfmNumBlocks(index->bwtLength) * awfmBlockBytes(index->config.alphabetType);
  const size_t devBlockBytes = g->image->numBlocks * awfmDeviceBlockBytes(amino);
  const size_t superBytes = awfmSuperBytes(index->bwtLength, amino, superShift);
  const uint64_t seedLen = awfmKmerTableLength(index->config.alphabetType, index->config.kmerLengthInSeedTable);
  const size_t seedBytes = seedLen * sizeof(struct AwFmSearchRange);
  const size_t saBytes = index->suffixArray.compressedByteLength;
  const size_t saAlloc = alignUp(saBytes, 16) + 256; /* the locate kernel reads a 128-byte window at a sample */

  auto fail = [&](enum AwFmReturnCode rc) {
    awfmGpuIndexDestroy(g);
    return rc;
  };
  void *dRef = nullptr;
#define TRY_OR_FAIL(call, rc)                 \
  do {                                        \
    hipError_t e__ = (call);                  \
    if (e__ != hipSuccess) {                  \
      setError(#call, e__);                   \
      if (dRef) (void)hipFree(dRef);          \
      return fail(rc);                        \
    }                                         \
  } while (0)

  TRY_OR_FAIL(hipMalloc(&g->image->dBlocks, devBlockBytes), AwFmAllocationFailure);
  TRY_OR_FAIL(hipMalloc(&g->image->dSuper, superBytes), AwFmAllocationFailure);
  TRY_OR_FAIL(hipMalloc(&g->image->dSeed, seedBytes ? seedBytes : 16), AwFmAllocationFailure);
  TRY_OR_FAIL(hipMalloc(&g->image->dSa, saAlloc), AwFmAllocationFailure);
  TRY_OR_FAIL(hipMalloc(&dRef, refBytes), AwFmAllocationFailure);
  g->image->deviceBytes = devBlockBytes + superBytes + seedBytes + saAlloc;

  TRY_OR_FAIL(hipMemcpy(dRef, index->bwtBlockList.asNucleotide, refBytes, hipMemcpyHostToDevice), AwFmGeneralFailure);
  unsigned long long sentinelPos = 0;
  if (!awfmGpuRelayout(dRef, index->bwtLength, amino, superShift, g->image->dBlocks, g->image->dSuper, &sentinelPos)) {
    (void)hipFree(dRef);
    return fail(AwFmGeneralFailure);
  }
  (void)hipFree(dRef);
  dRef = nullptr;

  TRY_OR_FAIL(hipMemcpy(g->image->dSeed, index->kmerSeedTable, seedBytes, hipMemcpyHostToDevice), AwFmGeneralFailure);
  {
    unsigned long long prefix[24] = {0};
    memcpy(prefix, index->prefixSums, awfmPrefixSumsLength(index->config.alphabetType) * sizeof(uint64_t));
    TRY_OR_FAIL(hipMalloc(&g->image->dPrefix, sizeof prefix), AwFmAllocationFailure);
    TRY_OR_FAIL(hipMemcpy(g->image->dPrefix, prefix, sizeof prefix, hipMemcpyHostToDevice), AwFmGeneralFailure);
  }

  /* sampled SA: from memory, or staged from the index file (keepSuffixArrayInMemory == false) */
  TRY_OR_FAIL(hipMemset(g->image->dSa, 0, saAlloc), AwFmGeneralFailure);
  if (index->suffixArray.values) {
    TRY_OR_FAIL(hipMemcpy(g->image->dSa, index->suffixArray.values, saBytes, hipMemcpyHostToDevice), AwFmGeneralFailure);
  } else {
    uint8_t *staged = awfmReadPackedSaFromFile(index);
    if (!staged) {
      setError("awfmGpuIndexCreate: index has no in-memory suffix array and it could not be read from its file");
      return fail(AwFmFileReadFail);
    }
    hipError_t e = hipMemcpy(g->image->dSa, staged, saBytes, hipMemcpyHostToDevice);
    free(staged);
    TRY_OR_FAIL(e, AwFmGeneralFailure);
  }
#undef TRY_OR_FAIL

  /* deferAccelerators: usable once the pair image is made (general kernel, pair steps, LF walk), the rest comes behind */
  if (finishImage(g, index, superShift, sentinelPos, deferAccelerators, true) != AwFmSuccess) return fail(AwFmGeneralFailure);
  *out = g;
  return AwFmSuccess;
}

/* the thread that builds an image's deeper table and full suffix array behind its first searches: the choices the
 * synchronous construction makes (by the image's size and the free memory), on a non-blocking stream of the thread's own */
static void accelBuilder(AwFmGpuIndex *g) {
  DeviceGuard guard(g->device);
  hipStream_t own = nullptr;
  if (hipStreamCreateWithFlags(&own, hipStreamNonBlocking) != hipSuccess) own = nullptr; /* (the null stream then: correct, not hidden) */
  awfmGpuSetupStream = own;
  AwFmGpuImage::PendingAccel &to = g->image->pendingAccel;
  const unsigned deepK = chooseDeepSeedK(g, to.notes);
  if (deepK != 0 && buildDeepSeed(g, deepK, &to) != AwFmSuccess) to.notes += "deeper table: construction failed; ";
  (void)awfmGpuBuildDenseSaAuto(g, &to.dense, &to.denseWide, &to.denseBytes, &to.denseSeconds, &to.notes);
  (void)awfmGpuSetupSync();
  awfmGpuSetupStream = nullptr;
  if (own) (void)hipStreamDestroy(own);
  (void)hipGetLastError();
  g->image->accelState.store(2);
}

}  // extern "C"
AwFmGpuExclusive::AwFmGpuExclusive(AwFmGpuImage *image, bool wait) {
  auto take = [&](std::mutex &m) {
    if (wait) m.lock();
    else if (!m.try_lock()) return false;
    locked.push_back(&m);
    return true;
  };
  if (!take(image->handlesMutex)) return;
  for (AwFmGpuIndex *h : image->handles)
    if (!take(h->aosMutex) || !take(h->workMutex) || !take(h->orderMutex)) return;
  held = true;
}
AwFmGpuExclusive::~AwFmGpuExclusive() {
  while (!locked.empty()) {
    locked.back()->unlock();
    locked.pop_back();
  }
}

void awfmGpuAdoptAccelerators(AwFmGpuImage *image, bool wait) {
  if (image->accelState.load() == 0) return;
  if (wait) joinBuilder(image);
  else if (image->accelState.load() != 2) return;
  AwFmGpuExclusive section(image, wait); /* (not waiting: now or another time) */
  if (!section.held || image->accelState.load() != 2) return;
  joinBuilder(image); /* (the thread is done) */
  AwFmGpuImage::PendingAccel &from = image->pendingAccel;
  if (from.deepTable) installDeepSeed(image, &from);
  if (from.dense) {
    image->dDenseSa = from.dense;
    image->denseWide = from.denseWide;
    image->denseSaBytes = from.denseBytes;
    image->denseSaBuildSeconds = from.denseSeconds;
    from.dense = nullptr;
  }
  image->accelNotes += from.notes;
  from.notes.clear();
  image->accelState.store(0);
}
extern "C" {

/* a lane's handle goes alone; the primary's takes the image with it (its lanes are gone by then: awfmGpuIndexRelease) */
void awfmGpuIndexDestroy(AwFmGpuIndex *g) {
  if (!g) return;
  AwFmGpuImage *image = g->image;
  if (g->lane) {
    std::lock_guard<std::mutex> lock(image->handlesMutex);
    for (size_t i = 0; i < image->handles.size(); i++)
      if (image->handles[i] == g) {
        image->handles.erase(image->handles.begin() + (long)i);
        break;
      }
  } else {
    joinBuilder(image);
  }
  {
    DeviceGuard guard(g->device);
    if (!g->lane) {
      if (image->pendingAccel.deepTable) (void)hipFree(image->pendingAccel.deepTable); /* (built, never installed) */
      if (image->pendingAccel.deepBig) (void)hipFree(image->pendingAccel.deepBig);
      if (image->pendingAccel.dense) (void)hipFree(image->pendingAccel.dense);
      awfmGpuStreamStateFree(image);
      void *owned[] = {image->dBlocks, image->dSuper, image->dSeed, image->dSa, image->dPrefix, image->dDeepSeed, image->dDeepBig,
                       image->dDenseSa, image->dLengthTable, image->dLengthBig, image->dPairBlocks, image->dPairSuper,
                       image->dPairSuper32, image->dPairC, image->dRecords, image->dText};
      for (void *p : owned)
        if (p) (void)hipFree(p);
    }
    if (g->dWork) (void)hipFree(g->dWork);
    if (g->dHits) (void)hipFree(g->dHits);
    for (auto &slot : g->orderSlot) {
      if (slot.mem) (void)hipFree(slot.mem);
      if (slot.gate.done) (void)hipEventDestroy(slot.gate.done);
    }
    if (g->dSparse) (void)hipFree(g->dSparse);
    if (g->sparseGate.done) (void)hipEventDestroy(g->sparseGate.done);
    for (auto &entry : g->orderLog)
      for (int i = 0; i < 4; i++)
        if (entry.ev[i]) (void)hipEventDestroy(entry.ev[i]);
    for (int i = 0; i < 2; i++)
      if (g->windowEvent[i]) (void)hipEventDestroy(g->windowEvent[i]);
    for (int i = 0; i < 4; i++)
      if (g->pinned[i]) (void)hipHostFree(g->pinned[i]);
    if (g->predict.verdictHost) (void)hipHostFree(g->predict.verdictHost);
  }
  if (!g->lane) delete image;
  delete g;
}

/* device ordinals the AoS entry points shard over: $AWFM_GPU_DEVICES = "all" or a comma list (a device named
 * again gets a lane on its image); unset = the default device (-1) with three lanes, so that one chunk of a
 * list is packed / scattered on the host while others are on the PCIe bus or in the kernels (awfm_batch.c) */
static int aosDevices(int *devs, int maxOut) {
  int n = 0;
  const char *env = awfmKnob(AWFM_KNOB_DEVICES);
  if (env && !strcmp(env, "all")) {
    const int count = awfmGpuDeviceCount();
    for (int d = 0; d < count && n < maxOut; d++) devs[n++] = d;
  } else if (env && *env) {
    for (const char *c = env; *c && n < maxOut;) {
      devs[n++] = atoi(c);
      while (*c && *c != ',') c++;
      if (*c == ',') c++;
    }
  }
  if (n == 0) { /* three lanes on the default device: one packs or scatters while two are in their device stage */
    devs[n++] = -1;
    for (int lane = 1; lane < 3 && n < maxOut; lane++) devs[n++] = -1;
  }
  return n;
}

/* a lane: a new handle on the image of `primary`, with the primary's selections; waits for an exclusive section in progress */
static AwFmGpuIndex *addLane(AwFmGpuIndex *primary) {
  AwFmGpuIndex *g = new AwFmGpuIndex();
  g->image = primary->image;
  g->device = primary->device;
  g->amino = primary->amino;
  g->numCUs = primary->numCUs;
  g->kernel = primary->kernel;
  g->forceWide = primary->forceWide;
  std::lock_guard<std::mutex> lock(g->image->handlesMutex);
  g->lane = (int)g->image->handles.size();
  g->image->handles.push_back(g);
  return g;
}

int awfmGpuIndexAcquireAll(const struct AwFmIndex *index, AwFmGpuIndex **out, int maxOut) {
  int devs[64];
  const int numDevs = aosDevices(devs, 64);
  /* -1 = the default device: $AWFM_GPU_DEVICE, else the calling thread's current device.  Entries are keyed by
   * the resolved ordinal, so a list that changes between calls never hands out another device's image. */
  int fallback = 0;
  if (const char *env = awfmKnob(AWFM_KNOB_DEVICE); env && *env) fallback = atoi(env);
  else if (hipGetDevice(&fallback) != hipSuccess) fallback = 0;
  for (int i = 0; i < numDevs; i++)
    if (devs[i] < 0) devs[i] = fallback;
  std::lock_guard<std::mutex> lock(tableMutex);
  auto find = [&](int device, int lane) -> AwFmGpuIndex * {
    for (auto &e : imageTable)
      if (e.index == index && e.handle->device == device && e.handle->lane == lane) return e.handle;
    return nullptr;
  };
  int n = 0;
  for (int slot = 0; slot < numDevs && n < maxOut; slot++) {
    int lane = 0; /* how often this device was named before */
    for (int earlier = 0; earlier < slot; earlier++) lane += devs[earlier] == devs[slot];
    AwFmGpuIndex *g = find(devs[slot], lane);
    if (!g) {
      if (lane > 0) { /* a device named again gets a lane on the image it already has */
        AwFmGpuIndex *primary = find(devs[slot], 0);
        if (!primary) return n;
        g = addLane(primary);
      } else if (createImage(index, devs[slot], &g, true) != AwFmSuccess) {
        return n;
      }
      imageTable.push_back({index, g});
    }
    out[n++] = g;
  }
  /* what the images' builder threads have finished since the last call is installed now, if nobody is inside a search */
  for (int i = 0; i < n; i++) awfmGpuAdoptAccelerators(out[i]->image, false);
  return n;
}

/* the explicit way to an index's image: complete -- whatever is built behind the first searches is waited for and installed */
AwFmGpuIndex *awfmGpuIndexAcquire(const struct AwFmIndex *index) {
  AwFmGpuIndex *g = nullptr;
  if (awfmGpuIndexAcquireAll(index, &g, 1) != 1) return nullptr;
  awfmGpuAdoptAccelerators(g->image, true);
  return g;
}

void awfmGpuIndexRelease(const struct AwFmIndex *index) {
  std::vector<AwFmGpuIndex *> doomed;
  {
    std::lock_guard<std::mutex> lock(tableMutex);
    for (size_t i = 0; i < imageTable.size();) {
      if (imageTable[i].index == index) {
        doomed.push_back(imageTable[i].handle);
        imageTable.erase(imageTable.begin() + (long)i);
      } else {
        i++;
      }
    }
  }
  for (AwFmGpuIndex *g : doomed)
    if (g->lane) awfmGpuIndexDestroy(g); /* lanes first: their image goes with its primary */
  for (AwFmGpuIndex *g : doomed)
    if (!g->lane) awfmGpuIndexDestroy(g);
}

void *awfmGpuPinnedBuffer(AwFmGpuIndex *g, int slot, uint64_t bytes) {
  if (!g || slot < 0 || slot > 3) return nullptr;
  if (bytes <= g->pinnedBytes[slot]) return g->pinned[slot];
  DeviceGuard guard(g->device);
  if (g->pinned[slot]) (void)hipHostFree(g->pinned[slot]);
  g->pinned[slot] = nullptr;
  g->pinnedBytes[slot] = 0;
  const size_t want = bytes + bytes / 4 + 4096;
  if (hipHostMalloc(&g->pinned[slot], want, hipHostMallocDefault) != hipSuccess) {
    setError("awfmGpuPinnedBuffer: hipHostMalloc failed");
    g->pinned[slot] = nullptr;
    return nullptr;
  }
  g->pinnedBytes[slot] = want;
  return g->pinned[slot];
}
void awfmGpuAosLock(AwFmGpuIndex *g) {
  if (g) g->aosMutex.lock();
}
void awfmGpuAosUnlock(AwFmGpuIndex *g) {
  if (g) g->aosMutex.unlock();
}

static uint64_t imageBytes(const AwFmGpuImage *image) {
  return image->deviceBytes + image->deepSeedBytes + image->denseSaBytes + image->pairBytes + image->lengthTableBytes + image->recordBytes + image->textBytes;
}
uint64_t awfmGpuIndexDeviceBytes(const AwFmGpuIndex *g) { return g && !g->lane ? imageBytes(g->image) : 0; } /* (a lane holds none of it) */

/* replaces the deeper table of an image; the caller holds whatever locks the image needs (none for an image nobody else has a
 * pointer to yet) */
static enum AwFmReturnCode applyDeepSeed(AwFmGpuIndex *g, unsigned deepK);

enum AwFmReturnCode awfmGpuIndexSetDeepSeed(AwFmGpuIndex *g, unsigned deepK) {
  if (!g) {
    setError("awfmGpuIndexSetDeepSeed: null image");
    return AwFmNullPtrError;
  }
  if (g->lane) {
    setError("awfmGpuIndexSetDeepSeed: set it on the primary image, not on a lane");
    return AwFmIllegalPositionError;
  }
  awfmGpuAdoptAccelerators(g->image, true);
  DeviceGuard guard(g->device);
  AwFmGpuExclusive section(g->image); /* nobody searches through the image while the table is replaced */
  return applyDeepSeed(g, deepK);
}

/* the deeper table of depth deepK with its next-step bits, built from the image as it is (nothing of the image is written):
 * into `to` */
static enum AwFmReturnCode buildDeepSeed(AwFmGpuIndex *g, unsigned deepK, AwFmGpuImage::PendingAccel *to) {
  void *table = nullptr, *big = nullptr;
  uint64_t bytes = 0, peak = 0;
  unsigned format = 0, numBig = 0;
  struct timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  if (!awfmGpuBuildDeepSeedTable(g, deepK, &table, &bytes, &peak, &to->deepAllocSeconds, &format, &big)) return AwFmGeneralFailure;
  /* the next-step bits: images with pair blocks (format 1: the long lengths move to `big` with them) */
  const int next = awfmGpuDeepSeedAddNext(g, table, deepK, format, &big, &numBig);
  (void)awfmGpuSetupSync();
  clock_gettime(CLOCK_MONOTONIC, &t1);
  if (next < 0) {
    (void)hipFree(table);
    if (big) (void)hipFree(big);
    return AwFmGeneralFailure;
  }
  to->deepTable = table;
  to->deepBig = big;
  to->deepBytes = bytes;
  to->deepBigBytes = !big ? 0u
                     : format == 2u ? ((g->image->dev.bwtLength >> (g->amino ? kAminoWideBigShift : kDeepWideBigShift)) + 2u) * 8u
                                    : ((g->image->dev.bwtLength >> (g->amino ? kAminoDeepBigShift : kDeepBigShift)) + 5u) * 4u;
  to->deepTransient = peak > bytes ? peak - bytes : 0;
  to->deepK = deepK;
  to->deepFormat = format;
  to->deepNext = next > 0 ? 1u : 0u;
  to->numDeepBig = numBig;
  to->deepSeconds = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
  if (awfmKnob(AWFM_KNOB_VERBOSE))
    fprintf(stderr, "[awfm deeper table] depth %u, entry format %u: %.2f GB in %.2f s; next-step bits %s; %u entries with long ranges\n", deepK, format,
            (double)bytes * 1e-9, to->deepSeconds, next > 0 ? "yes" : "no", numBig);
  return AwFmSuccess;
}
/* a built table becomes the image's; the caller holds whatever locks the image needs */
static void installDeepSeed(AwFmGpuImage *image, AwFmGpuImage::PendingAccel *from) {
  image->dDeepSeed = from->deepTable;
  image->dDeepBig = from->deepBig;
  image->deepSeedBytes = from->deepBytes + from->deepBigBytes;
  image->deepSeedBuildSeconds = from->deepSeconds;
  image->deepSeedAllocSeconds = from->deepAllocSeconds;
  image->deepSeedTransientBytes = from->deepTransient;
  image->dev.deepSeed = (const ulonglong2 *)from->deepTable;
  image->dev.deepNarrow = from->deepFormat;
  image->dev.deepNext = from->deepNext;
  image->dev.numDeepBig = from->numDeepBig;
  image->dev.deepBigBySp = (const unsigned *)from->deepBig;
  image->dev.deepK = from->deepTable ? from->deepK : 0u;
  from->deepTable = from->deepBig = nullptr;
}

static enum AwFmReturnCode applyDeepSeed(AwFmGpuIndex *g, unsigned deepK) {
  AwFmGpuImage *image = g->image;
  (void)hipDeviceSynchronize();
  if (image->dDeepSeed) (void)hipFree(image->dDeepSeed);
  if (image->dDeepBig) (void)hipFree(image->dDeepBig);
  { /* the tables of the shorter lengths go with the deeper table they complete; the next mixed-length batch builds them again */
    std::lock_guard<std::mutex> lock(image->lengthMutex);
    if (image->dLengthTable) (void)hipFree(image->dLengthTable);
    if (image->dLengthBig) (void)hipFree(image->dLengthBig);
    image->dLengthTable = nullptr;
    image->dLengthBig = nullptr;
    image->lengthDepths = 0;
    image->lengthTableBytes = 0;
    image->lengthTried = false;
  }
  AwFmGpuImage::PendingAccel built; /* (nothing: the image without a deeper table) */
  enum AwFmReturnCode rc = AwFmSuccess;
  if (deepK != 0) {
    /* (the construction reads the image's view: without the table that is being replaced) */
    image->dev.deepSeed = nullptr;
    image->dev.deepK = 0;
    rc = buildDeepSeed(g, deepK, &built);
  }
  installDeepSeed(image, &built);
  return rc;
}

/* $AWFM_GPU_DEEP_SEED_K on an image that was just created or adopted: nobody else holds it, so no lock is taken */
static unsigned chooseDeepSeedK(const AwFmGpuIndex *g, std::string &notes);
static enum AwFmReturnCode applyDeepSeedFromEnv(AwFmGpuIndex *g) {
  const unsigned deepK = chooseDeepSeedK(g, g->image->accelNotes);
  if (deepK == 0) return AwFmSuccess;
  DeviceGuard guard(g->device);
  return applyDeepSeed(g, deepK);
}
/* the depth of the device-only table an image gets by itself ($AWFM_GPU_DEEP_SEED_K / $AWFM_GPU_AMINO_DEEP_SEED_K, else by its size
 * and the memory that is free); 0: none */
static unsigned chooseDeepSeedK(const AwFmGpuIndex *g, std::string &notes) {
  int deepK = 0;
  if (const char *env = awfmKnob(g->amino ? AWFM_KNOB_AMINO_DEEP_SEED_K : AWFM_KNOB_DEEP_SEED_K)) {
    deepK = atoi(env); /* 0: none */
  } else if (g->amino) {
    /* Automatic, amino: an image of >= 2^26 positions whose own table is shallower gets the deepest table of up to 7
     * characters with at most 8 entries per text position, when three times its size is free on the device: 20^7 x 8 B =
     * 10.2 GB for a Swiss-Prot-sized text (2 * 10^8 residues), where 85 % of random 10-mers end at their entry (no such
     * 7-mer) and the rest start two steps further on.  Exact: an entry is what the stepping holds after those steps. */
    size_t freeBytes = 0, totalBytes = 0;
    DeviceGuard guard(g->device);
    if (g->image->dev.bwtLength >= (1ull << 26) && g->image->dev.bwtLength < (1ull << kDeepWideMaxBits) && g->image->dev.seedK >= 2 && hipMemGetInfo(&freeBytes, &totalBytes) == hipSuccess) {
      unsigned long long entries = 1;
      for (unsigned k = 1; k <= 7u; k++) {
        entries *= 20ull;
        if (k > g->image->dev.seedK && entries <= 8ull * g->image->dev.bwtLength && freeBytes / 3u >= entries * 8ull) deepK = (int)k;
        else if (k > g->image->dev.seedK && entries <= 8ull * g->image->dev.bwtLength && k > (unsigned)deepK) notes += "deeper table: depth " + std::to_string(k) + " not built (less than 3 x its size free); ";
      }
    } else {
      (void)hipGetLastError();
    }
  } else if (g->image->dev.bwtLength >= (1ull << 28) && g->image->dev.seedK >= 8 && g->image->dev.seedK < kAutoDeepSeedMin) {
    /* Automatic: an image far beyond the L2s gets the deepest table of 14..16 characters that has no more than two
     * entries per text position, when the device has room to spare (8 B -- 16 B from 2^32 positions -- x 4^K: 2.1 GB
     * at 14, 34 GB at 16; its construction holds the level below beside it; asked for: three times the table).  Every
     * level of the table replaces a dependent block read of EVERY k-mer by a wider spread of the one table read: 10^8
     * random 21-mers against a 3.1 Gbp image, seed-order search kernel 3.44 ms at 14, 3.21 at 15, 2.87 at 16 (the
     * index's own k = 12 table: 4.6); planted 21-mers 6.08 -> 5.13 ms.  Results are bit-identical (the table holds
     * what the stepping would compute, stop-at-first-invalid rule included). */
    size_t freeBytes = 0, totalBytes = 0;
    DeviceGuard guard(g->device);
    if (hipMemGetInfo(&freeBytes, &totalBytes) == hipSuccess) {
      const uint64_t entryBytes = g->image->dev.bwtLength < (1ull << kDeepWideMaxBits) ? 8u : 16u;
      for (unsigned k = kAutoDeepSeedMax; k >= kAutoDeepSeedMin && deepK == 0; k--)
        if ((1ull << (2u * k)) <= 2ull * g->image->dev.bwtLength && freeBytes / 3u >= (entryBytes << (2u * k))) deepK = (int)k;
      if (deepK == 0 && freeBytes / 4u >= (16ull << (2u * kAutoDeepSeedMin))) deepK = (int)kAutoDeepSeedMin;
      unsigned wanted = 0; /* the depth the image's size asks for */
      for (unsigned k = kAutoDeepSeedMax; k >= kAutoDeepSeedMin && wanted == 0; k--)
        if ((1ull << (2u * k)) <= 2ull * g->image->dev.bwtLength) wanted = k;
      if ((unsigned)deepK < wanted)
        notes += "deeper table: depth " + std::to_string(wanted) + " not built (less than 3 x its size free)" +
                         (deepK ? ", depth " + std::to_string(deepK) + " instead; " : "; ");
    } else {
      (void)hipGetLastError();
    }
  }
  return deepK <= 0 || (unsigned)deepK <= g->image->dev.seedK ? 0u : (unsigned)deepK; /* (nothing deeper than the index's own table) */
}
/* Pair image (awfm_pair.h) of a nucleotide image that was just created or adopted (nobody else holds it, no lanes, so
 * no lock): built unless $AWFM_GPU_PAIR=0.  It doubles the block bytes of the image (128 B per 128 positions beside
 * the 64 B of the one-letter blocks) and halves the dependent block reads of hits-only searches and of the LF walk. */
static enum AwFmReturnCode applyPairFromEnv(AwFmGpuIndex *g) {
  if (g->amino) return AwFmSuccess;
  if (const char *env = awfmKnob(AWFM_KNOB_PAIR))
    if (atoi(env) == 0) return AwFmSuccess;
  DeviceGuard guard(g->device);
  const enum AwFmReturnCode rc = awfmGpuApplyPairImage(g, true);
  if (rc != AwFmSuccess) {
    (void)awfmGpuApplyPairImage(g, false);
    g->image->accelNotes += "pair image: not built (no device memory for 1 byte per position); ";
  }
  return rc;
}

enum AwFmReturnCode awfmGpuIndexSetPairImage(AwFmGpuIndex *g, int enable) {
  if (!g) {
    setError("awfmGpuIndexSetPairImage: null image");
    return AwFmNullPtrError;
  }
  if (g->lane) {
    setError("awfmGpuIndexSetPairImage: set it on the primary image, not on a lane");
    return AwFmIllegalPositionError;
  }
  awfmGpuAdoptAccelerators(g->image, true);
  DeviceGuard guard(g->device);
  AwFmGpuExclusive section(g->image); /* nobody searches through the image while it changes */
  const enum AwFmReturnCode rc = awfmGpuApplyPairImage(g, enable != 0);
  if (rc != AwFmSuccess) (void)awfmGpuApplyPairImage(g, false);
  return rc;
}
int awfmGpuIndexHasPairImage(const AwFmGpuIndex *g) { return g && g->image->dev.pairBlocks ? 1 : 0; }
unsigned awfmGpuIndexDeepSeedK(const AwFmGpuIndex *g) { return g ? g->image->dev.deepK : 0u; }
double awfmGpuIndexDeepSeedAllocSeconds(const AwFmGpuIndex *g) { return g ? g->image->deepSeedAllocSeconds : 0.0; }
double awfmGpuIndexDeepSeedBuildSeconds(const AwFmGpuIndex *g) { return g ? g->image->deepSeedBuildSeconds : 0.0; }
uint64_t awfmGpuIndexDeepSeedTransientBytes(const AwFmGpuIndex *g) { return g ? g->image->deepSeedTransientBytes : 0; }

int awfmGpuIndexDevice(const AwFmGpuIndex *g) { return g ? g->device : -1; }
void awfmGpuIndexSetKernel(AwFmGpuIndex *g, enum AwFmGpuKernel kernel) {
  if (g) g->kernel = kernel;
}
int awfmGpuIndexIsWide(const AwFmGpuIndex *g) { return g && !awfmImageNarrow(g) ? 1 : 0; }
void awfmGpuIndexSetWide(AwFmGpuIndex *g, int wide) {
  if (!g) return;
  if (g->lane) {
    g->forceWide = wide != 0;
    return;
  }
  std::lock_guard<std::mutex> lock(g->image->handlesMutex); /* the primary's setting reaches its lanes */
  for (AwFmGpuIndex *h : g->image->handles) h->forceWide = wide != 0;
}


/* see include/awfm_gpu.h */
int awfmGpuIndexDescribe(const AwFmGpuIndex *g, char *out, int outBytes) {
  if (!g || !out || outBytes <= 0) return 0;
  const AwFmGpuImage *image = g->image; /* (a lane reports its image) */
  std::string text = std::string(g->amino ? "amino" : "nucleotide") + " image of " + std::to_string(image->dev.bwtLength) + " positions, " +
                     std::to_string(imageBytes(image)) + " bytes on device " + std::to_string(g->device) + ": ";
  if (!g->amino) text += image->dev.pairBlocks ? "pair image yes; " : "pair image no; ";
  text += image->dev.deepK ? "deeper table depth " + std::to_string(image->dev.deepK) + (image->dev.deepNext ? " with next-step bits; " : "; ") : "deeper table no; ";
  text += image->dDenseSa ? "full suffix array yes; " : "full suffix array no; ";
  if (!g->amino) text += image->dLengthTable ? "tables per k-mer length 1.." + std::to_string(image->lengthDepths) + "; " : "tables per k-mer length not built (the first large mixed-length batch builds them); ";
  text += awfmGpuDescribeRecordTable(image);
  text += awfmGpuDescribeText(image);
  if (!image->accelNotes.empty()) text += "notes: " + image->accelNotes;
  while (!text.empty() && (text.back() == ' ' || text.back() == ';')) text.pop_back();
  const int n = (int)text.size() < outBytes - 1 ? (int)text.size() : outBytes - 1;
  memcpy(out, text.data(), (size_t)n);
  out[n] = 0;
  return (int)text.size();
}
/* the tables per k-mer length a mixed-length batch builds on first use (awfm_gpu_ordered.hip: ensureLengthTables) */
uint64_t awfmGpuIndexLengthTableBytes(const AwFmGpuIndex *g) { return g ? g->image->lengthTableBytes : 0; }
double awfmGpuIndexLengthTableBuildSeconds(const AwFmGpuIndex *g) { return g ? g->image->lengthTableBuildSeconds : 0.0; }

}  // extern "C"
