// fsmc_capi.hip -- host side of libfastsmc_hip.so: the C ABI of include/fastsmc_hip.h.
//
// Owns device memory (model tables, packed haplotypes, work list, per-wave workspace, record
// buffer), validates every shape on the host before a launch (an out-of-bounds kernel can take
// the whole node down), picks the chunking of the beta stream, launches the decode kernel and
// orders the results the way the reference writes them.  No CPU fallback exists: if HIP is not
// usable every entry point fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "fsmc_identify.h"
#include "fsmc_instances.h"
#include "fsmc_model_tables.h"
#include "fsmc_pair_bins.h"
#include "fsmc_pair_cdf.h"
#include "fsmc_pair_layout.h"
#include "fsmc_pair_tail.h"
#include "fsmc_pair_minima.h"
#include "fsmc_pair_posteriors.h"
#include "fsmc_plan.h"

namespace fsmc
{
hipError_t idSortCandidates(hipStream_t stream, const fsmc_candidate* in, fsmc_candidate* sorted, unsigned n,
                            unsigned nHaps, unsigned nWords); // fsmc_identify_sort.hip
hipError_t idSeedDepths(hipStream_t stream, const unsigned long long* words, unsigned nHaps, unsigned nWords,
                        unsigned maxSeeds, unsigned readAhead, unsigned char* depthOut,
                        unsigned hapStride); // fsmc_identify_seeds.hip
}

using namespace fsmc;

namespace fsmc
{
// acc[i] = (((acc[i] + plane_0[i]) + plane_1[i]) + ...): the per-batch sums of one launch are added to the running
// accumulator one batch after the other, the order of sumOverPairs(pos, k) += sum in HMM::augmentSumOverPairs
// (HMM.cpp:1054-1073) -- the same fp32 additions in the same order, hence the same bits.
__global__ void add_planes_in_order_kernel(const float* __restrict__ planes, float* __restrict__ acc, size_t n,
                                           int nPlanes, size_t planeStride)
{
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float s = acc[i];
    for (int sl = 0; sl < nPlanes; ++sl) {
      s = s + planes[(size_t)sl * planeStride + i];
    }
    acc[i] = s;
  }
}
} // namespace fsmc

namespace
{
thread_local std::string g_createError;

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

// The pool of chunk buffers (fsmc_ctx_set_chunk_pool): the shipped defaults, chosen by measurement
constexpr int kChunkPoolDefault = -1;
constexpr uint32_t kChunkPoolPhiDefault = 200;

// The entry points that send the work list through the device in slices of groups (planSlices): each has its own
// slice setting and its own count of the last call's slices.
enum PairSlicing {
  kSlicePosteriors,
  kSliceMinima,
  kSliceBins,
  kSliceCdf,
  kSliceTail,
  kSliceLoglik,
  kSliceViterbi,
  kSliceSamples,
  kSliceTransitions,
  kPairSlicings
};
} // namespace

struct fsmc_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool ownStream = false;
  int nCU = 0;
  uint64_t hbmBytes = 0;
  uint64_t wsLimit = 0;
  plan::Credit credit; // what the launches and the announced job have earned for the workspace
  std::string err;

  unsigned long long* dHaps = nullptr;
  uint32_t nHaps = 0, nSites = 0, W = 0;

  fsmc_pair* dPairs = nullptr;
  fsmc_group* dGroups = nullptr;
  size_t nPairs = 0, nGroups = 0;
  std::vector<fsmc_pair> hPairs;
  std::vector<fsmc_group> hGroups;

  unsigned* dCounters = nullptr;
  unsigned long long* dPhase = nullptr;
  DevBuf ws;
  DevBuf recs;
  size_t recCap = 0;
  DevBuf aux;  // dump offsets
  DevBuf out;  // device-side result staging (dump / per-pair / sums)

  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;
  int lastSlots = 0;
  int lastChunk = 0, lastMaxChunks = 0, lastResident = 0;
  int residentChunks = -1; // chunks of a window that skip the rebuild: -1 = as many as the workspace limit allows, 0 = none
  // The resident chunk buffers of a launch as one pool the waves claim from (decode_kernel_pool, KParamsPool)
  int chunkPool = kChunkPoolDefault; // -1 = IBD launches of more than two rounds, 0 = never, 1 = wherever it is built
  uint32_t chunkPoolPhi = kChunkPoolPhiDefault; // per cent of its share of the pool that a window may ask for
  DevBuf poolState;        // the pool's cursor, counters and claim words: zeroed on the stream before every launch
  uint32_t lastPoolBuffers = 0; // ... of the last launch (0: it kept the static layout)
  uint32_t chunkSites = 0; // 0 = automatic
  uint32_t betaStride = 0; // 0 = automatic (2 where the kernel exists), 1 = store every beta row
  int lastStride = 1;
  bool lastSpsLds = false; // the last IBD launch kept the segments' per-state sums in LDS
  int lastMember = 0; // member of the last launch: KT of the lane-per-pair kernel; wave-group kernel: 1000 + KH (four waves of KH states), 1000 * NW + KH (NW = 5 ... 8 waves)

  // The queues an IBD decode's waves pull from (fsmc_decode_ibd_launch): built from the uploaded groups once per
  // work list and pairing, longest window first.
  struct IbdQueues {
    uint64_t serial = 0;  // work list they were built from
    bool pairing = false; // half-full groups were paired where they pair up (the setting, and a model it is built for)
    bool valid = false;
    bool dual = false;    // items/unions in use: two half-groups per wave
    bool reordered = false; // rest is in use (a reordered copy or subset of the uploaded groups)
    bool alone = false;     // every group rides in the paired kernel: it has the whole workspace
    std::vector<fsmc_group> items, unions, rest;
  } q;
  uint64_t worklistSerial = 0;
  fsmc_group* dItems = nullptr; // two half-groups per wave: {A, B} per item
  fsmc_group* dRest = nullptr;  // the groups that run one per wave, longest window first
  uint32_t pairing = 1;         // 0 = never pair half-full groups, 1 = automatic
  int lastItems = 0;            // items of the last IBD launch (0: it ran on the groups as uploaded)
  unsigned twoWaves = 0;        // two waves per window (fsmc_kernels_bidir.h): 0 automatic, 1 never
  int lastWavesPerWindow = 1;   // ... of the last dump / per-pair / sums launch
  hipStream_t side = nullptr;   // the one-group-per-wave kernel of a paired decode runs here, beside the paired kernel
  hipEvent_t evFork = nullptr, evJoin = nullptr;
  DevBuf wsSide;

  // The fsmc_decode_pair_* entry points: the work list goes through the device in slices of groups (planSlices)
  struct {
    uint32_t groups = 0; // groups a slice, 0 = automatic
    int last = 0;        // slices of the last call
  } pairSlices[kPairSlicings];
  DevBuf ppStage;           // a slice's decode: the dump, [group][site][k][lane], or its mean / MAP rows, [pair][S]
  DevBuf ppRows;            // the rows a slice's reduction leaves: [pair][K][S] (posteriors), [output][pair][S] (cdf, tail)
  DevBuf ppAcc;             // posteriors: [expCoal K floats][sum K * S floats]
  hipStream_t copyStream = nullptr; // the rows leave on this one, through the two pinned buffers (drainRows)
  void* ppPinned[2] = {nullptr, nullptr};
  size_t ppPinnedBytes = 0; // size of each
  hipEvent_t evRows = nullptr, evCopied[2] = {nullptr, nullptr};
  DevBuf pmAcc;             // minima: [expCoal KP floats][the carried state, 4 x S][the ranges' partials, 4 x nRanges x S]
  DevBuf pbAcc;             // bins: [expCoal KP floats][edges, B + 1][a slice's outputs, up to 5 x pairs x B]
  DevBuf pcSpec;            // cdf, tail summaries: the call's outputs, PairCdfSpec each
  DevBuf plAcc;             // log-likelihoods: a slice's [mant][bin mant][expo][bin expo], then the edges, B + 1
  DevBuf pvAcc;             // Viterbi paths: a slice's [mant][expo]; its state rows, [pair][S] bytes, are in ppRows
  DevBuf pxAcc;             // change probabilities: [edges, B + 1][weights, S ones][a slice's bin outputs, 2 x pairs x B]
  DevBuf ptAcc;             // tail summaries: [sum, n_tail x S doubles][edges, B + 1][weights, S][a slice's outputs, up to 2 x n_tail x pairs x B]

  uint64_t scratchFilled = 0; // bytes FSMC_DIAG_SCRATCH_FILL has filled on this context (fsmc_ctx_scratch_filled)

  DevBuf idStash;       // fsmc_identify on overflow: the complete, ordered candidate list, kept for fsmc_identify_fetch
  size_t idStashCount = 0;

  const fsmc_model* ibdModel = nullptr;
  uint32_t ibdFlags = 0;
  bool ibdPending = false;
};

struct fsmc_model {
  fsmc_ctx* ctx = nullptr;
  int K = 0, KP = 0, S = 0, nRows = 0;
  int w2NW = 0; // wave-group kernel: waves per group (each holds KP / w2NW states); 0 for every other model
  float *pi = nullptr, *cR = nullptr, *expT = nullptr;
  float *D = nullptr, *B = nullptr, *U = nullptr, *RR = nullptr;
  float* rowSets = nullptr; // [rows][5][KP]: D | B | U | Ush | RR per key, Ush[k] = U[k-1] (kernels' RowSet)
  float* ghostMask = nullptr; // [KP]: 1.0f for the K real states, 0.0f for the padding states
  int* stepRow = nullptr;
  bool sequence = false;
  int *rowGapF = nullptr, *rowSiteB = nullptr, *rowGapB = nullptr; // sequence mode (stepRow = forward site step)
  float4* emis3 = nullptr; // [S][3 or 4][KP]: emission per observation class (+ the gap row in sequence mode)
  unsigned stateThr = 0, ageThr = 0;
  float probThr = 0.f;
};

namespace
{

// Two copies of the HIP runtime in one process (e.g. this library linked against /opt/rocm and a PyTorch wheel that
// bundles its own libamdhip64, loaded in that order) share the device but not their state: kernels built for one
// wave per SIMD then fail to launch with an opaque "unknown error" from the occupancy query.  When that query fails,
// fsmc_ctx_create looks at the mapped files and says so.  Returns the paths of the distinct runtimes found.
std::vector<std::string> mappedHipRuntimes()
{
  std::vector<std::string> found;
  if (FILE* f = std::fopen("/proc/self/maps", "r")) {
    char line[4096];
    while (std::fgets(line, sizeof(line), f)) {
      const char* slash = std::strchr(line, '/');
      if (!slash || !std::strstr(slash, "libamdhip64.so")) {
        continue;
      }
      std::string path(slash);
      while (!path.empty() && (path.back() == '\n' || path.back() == ' ')) {
        path.pop_back();
      }
      if (std::find(found.begin(), found.end(), path) == found.end()) {
        found.push_back(path);
      }
    }
    std::fclose(f);
  }
  return found;
}

int fail(fsmc_ctx* ctx, int code, const std::string& msg)
{
  if (ctx) {
    ctx->err = msg;
  } else {
    g_createError = msg;
  }
  return code;
}

#define FSMC_HIP(ctx, call)                                                                                            \
  do {                                                                                                                 \
    hipError_t e_ = (call);                                                                                            \
    if (e_ != hipSuccess) {                                                                                            \
      return fail((ctx), FSMC_EHIP, std::string(#call) + ": " + hipGetErrorString(e_));                                \
    }                                                                                                                  \
  } while (0)

// `call` gives FSMC_OK or the caller returns what it gave (the error text is set where it failed).
#define FSMC_TRY(call)                                                                                                 \
  do {                                                                                                                 \
    const int rc_ = (call);                                                                                            \
    if (rc_ != FSMC_OK) {                                                                                              \
      return rc_;                                                                                                      \
    }                                                                                                                  \
  } while (0)

// FSMC_DIAG_SCRATCH_FILL=<0..255> (tests: every kernel on scratch memory an earlier launch left dirty): the byte every
// scratch buffer holds, over its whole allocation, when an entry point takes it -- `fill`, -1 where the variable is not
// set.  Read at every use, never cached: the tests set and unset it inside one process.  A value that is no integer in
// 0..255 is an error, not "unset": a typo must not turn those tests into no-ops.
int scratchFill(fsmc_ctx* ctx, int& fill)
{
  fill = -1;
  const char* s = std::getenv("FSMC_DIAG_SCRATCH_FILL");
  if (!s) {
    return FSMC_OK;
  }
  char* end = nullptr;
  const long v = std::strtol(s, &end, 10);
  if (end == s || *end != '\0' || v < 0 || v > 255 || !(*s >= '0' && *s <= '9')) {
    return fail(ctx, FSMC_EINVAL, std::string("FSMC_DIAG_SCRATCH_FILL must be an integer in 0..255, not \"") + s + "\"");
  }
  fill = (int)v;
  return FSMC_OK;
}

int allocate(fsmc_ctx* ctx, DevBuf& b, size_t bytes); // `b` freed, then `bytes` (16 at least) from hipMalloc

// `b` holds at least `bytes` afterwards.  Every entry point calls this for each of its scratch buffers before its first
// upload into them, so this is where FSMC_DIAG_SCRATCH_FILL dirties them: the whole allocation, new or held, on the
// context's stream in front of everything the entry point writes there (the call sites, and why no live
// data precedes any of them).  Unset, the variable adds no call.
int ensure(fsmc_ctx* ctx, DevBuf& b, size_t bytes)
{
  int fill = -1;
  FSMC_TRY(scratchFill(ctx, fill));
  if (!(b.bytes >= bytes && b.p)) {
    FSMC_TRY(allocate(ctx, b, bytes));
  }
  if (fill >= 0) {
    FSMC_HIP(ctx, hipMemsetAsync(b.p, fill, b.bytes, ctx->stream));
    ctx->scratchFilled += b.bytes;
  }
  return FSMC_OK;
}

int allocate(fsmc_ctx* ctx, DevBuf& b, size_t bytes)
{
  if (b.p) {
    (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
  }
  if (bytes == 0) {
    bytes = 16;
  }
  const bool timing = bytes >= (256u << 20) && std::getenv("FSMC_HOST_TIMING") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  hipError_t e = hipMalloc(&b.p, bytes);
  if (e != hipSuccess) {
    b.p = nullptr;
    return fail(ctx, FSMC_ENOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes failed: " + hipGetErrorString(e));
  }
  if (timing) { // (FSMC_HOST_TIMING: where a job's wall time goes -- allocations of 256 MiB and more)
    std::fprintf(stderr, "[fsmc] hipMalloc of %.2f GB took %.3f s\n", (double)bytes / 1e9,
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  }
  b.bytes = bytes;
  return FSMC_OK;
}

template <typename T> int upload(fsmc_ctx* ctx, T** dst, const T* src, size_t n)
{
  if (*dst) {
    (void)hipFree(*dst);
    *dst = nullptr;
  }
  hipError_t e = hipMalloc((void**)dst, std::max<size_t>(n, 1) * sizeof(T));
  if (e != hipSuccess) {
    *dst = nullptr;
    return fail(ctx, FSMC_ENOMEM, std::string("hipMalloc failed: ") + hipGetErrorString(e));
  }
  if (n) {
    FSMC_HIP(ctx, hipMemcpyAsync(*dst, src, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return FSMC_OK;
}

// A host table on its way to the device.
template <typename T> int upload(fsmc_ctx* ctx, T** dst, const std::vector<T>& table)
{
  return upload(ctx, dst, table.data(), table.size());
}

using KernelFn = void (*)(const KParams);
using PoolKernelFn = void (*)(const KParamsPool); // decode_kernel_pool: the same sweeps with the chunk pool

// Which member of the lane-per-pair family decodes a model (fsmc_instances.h): 69 for the reference's 69-state
// models and K itself where the library has an exact member of K states, the padded row length for every other model
// of at most 128 states, 0 beyond.
int familyMember(const fsmc_model* m)
{
  if (exactMember(m->K)) {
    return m->K;
  }
  return (m->K <= 128 && m->KP % kKPad == 0 && m->KP <= 128) ? m->KP : 0;
}

// The member's kernel with the chunk pool (array mode, one group per wave: IBD decode and sums), nullptr where none is built.
template <int KT> PoolKernelFn pickPoolMember(int mode, bool track, bool half)
{
  if constexpr (poolBuilt(KT)) {
    if (mode == kModeIbd) {
      return half ? (track ? decode_kernel_pool<KT, kModeIbd, true, true> : decode_kernel_pool<KT, kModeIbd, false, true>)
                  : (track ? decode_kernel_pool<KT, kModeIbd, true, false> : decode_kernel_pool<KT, kModeIbd, false, false>);
    }
    if (mode == kModeSums) {
      return half ? decode_kernel_pool<KT, kModeSums, false, true> : decode_kernel_pool<KT, kModeSums, false, false>;
    }
  }
  return nullptr;
}

template <int KT> KernelFn pickMember(int mode, bool track, bool seq, bool half, bool dual = false)
{
  if constexpr (KT > 0 && halfBuilt(KT)) {
    if (dual && half && mode == kModeIbd && !seq) {
      return track ? decode_kernel<KT, kModeIbd, true, false, true, true>
                   : decode_kernel<KT, kModeIbd, false, false, true, true>;
    }
  }
  if constexpr (KT > 0) {
    if (dual && mode == kModeIbd && !seq) {
      return track ? decode_kernel<KT, kModeIbd, true, false, false, true>
                   : decode_kernel<KT, kModeIbd, false, false, false, true>;
    }
  }
  switch (mode) {
  case kModeIbd:
    if constexpr (halfBuilt(KT)) {
      if (half && !seq) {
        return track ? decode_kernel<KT, kModeIbd, true, false, true> : decode_kernel<KT, kModeIbd, false, false, true>;
      }
    }
    if (seq) {
      return track ? decode_kernel<KT, kModeIbd, true, true, false> : decode_kernel<KT, kModeIbd, false, true, false>;
    }
    return track ? decode_kernel<KT, kModeIbd, true, false, false> : decode_kernel<KT, kModeIbd, false, false, false>;
  case kModeDump:
    return seq ? decode_kernel<KT, kModeDump, false, true, false> : decode_kernel<KT, kModeDump, false, false, false>;
  case kModePerPair:
    return seq ? decode_kernel<KT, kModePerPair, false, true, false>
               : decode_kernel<KT, kModePerPair, false, false, false>;
  case kModeSums:
    if constexpr (halfSumsBuilt(KT)) {
      if (half && !seq) {
        return decode_kernel<KT, kModeSums, false, false, true>;
      }
    }
    return seq ? decode_kernel<KT, kModeSums, false, true, false> : decode_kernel<KT, kModeSums, false, false, false>;
  default:
    return nullptr;
  }
}

// The wide-model kernel with lane = pair and several waves per group (fsmc_kernels_w2.h): 128 < K <= 1024, every
// consumer, array and sequence mode.  fsmc_model_create picks the member (w2Member) and pads such a model's rows to
// KP = waves x states per wave: four waves of 48 or 64 (two workgroups per CU) or 80 states, six to eight waves of 64,
// eight waves of 80 / 96 / 128 beyond 512 states.
bool waveGroups(int mode, const fsmc_model* m)
{
  return m->w2NW > 0 && (mode == kModeIbd || mode == kModeDump || mode == kModeSums || mode == kModePerPair);
}

// The members of the wave-group kernel the library is built with: {waves per group, states per wave}.  plan::w2Member
// picks a model's; the diagnostic override may name any of these.
const std::vector<plan::W2Member>& builtW2Members()
{
#define FSMC_LIST_W2(KHX, NWX) {NWX, KHX},
  static const std::vector<plan::W2Member> built = {FSMC_ALL_W2(FSMC_LIST_W2)};
#undef FSMC_LIST_W2
  return built;
}

template <int KH, int NW, bool SEQ> KernelFn pickWaveGroupKernelOf(int mode, bool track)
{
  if (mode == kModeIbd) {
    return track ? decode_kernel_w2<KH, kModeIbd, true, SEQ, NW> : decode_kernel_w2<KH, kModeIbd, false, SEQ, NW>;
  }
  if (mode == kModeSums) {
    return decode_kernel_w2<KH, kModeSums, false, SEQ, NW>;
  }
  if (mode == kModePerPair) {
    return decode_kernel_w2<KH, kModePerPair, false, SEQ, NW>;
  }
  return decode_kernel_w2<KH, kModeDump, false, SEQ, NW>;
}
template <int KH, int NW> KernelFn pickWaveGroupKernel(int mode, bool track, bool seq)
{
  return seq ? pickWaveGroupKernelOf<KH, NW, true>(mode, track) : pickWaveGroupKernelOf<KH, NW, false>(mode, track);
}

// more than 1024 states: the any-K kernel (fsmc_kernels_any.h)
bool anyStates(const fsmc_model* m)
{
  return m->K > kMaxStatesW2;
}

template <bool SEQ> KernelFn pickAnyKernel(int mode, bool track)
{
  switch (mode) {
  case kModeIbd:
    return track ? decode_kernel_any<kModeIbd, true, SEQ> : decode_kernel_any<kModeIbd, false, SEQ>;
  case kModeDump:
    return decode_kernel_any<kModeDump, false, SEQ>;
  case kModePerPair:
    return decode_kernel_any<kModePerPair, false, SEQ>;
  case kModeSums:
    return decode_kernel_any<kModeSums, false, SEQ>;
  default:
    return nullptr;
  }
}

// What a launch needs to know of its kernel.  `member`: as fsmc_ctx::lastMember.  `stride`: the beta stride the kernel
// is built for -- the plan lays the chunk buffer out for it, so everything downstream reads it from here.
struct KernelChoice {
  KernelFn fn = nullptr; // nullptr: no such kernel is built
  unsigned threads = kWave;
  int member = 0;
  int stride = 1;
  PoolKernelFn poolFn = nullptr; // the same kernel with the chunk pool, launched when the plan has one (planOneWave)
};

// The one-wave kernel of a model and mode.  `wantStride`: as fsmc_ctx::betaStride (the context's setting or the
// caller's own decision).  `dual`: two half-groups per wave.  Writes nothing.
// Beta stride 2 (every second beta row stored, the others recomputed in the alpha sweep): array-mode IBD decode and
// array-mode sums over pairs (round 5: at size the sums moved 8K bytes a pair-site at the rate the CUs' path to memory
// delivers -- the IBD decode's situation before stride 2) of the family members it is built for.
KernelChoice chooseKernel(const fsmc_model* m, int mode, bool track, bool dual, uint32_t wantStride)
{
  KernelChoice k;
  if (anyStates(m)) {
    k.fn = m->sequence ? pickAnyKernel<true>(mode, track) : pickAnyKernel<false>(mode, track);
    return k;
  }
  if (waveGroups(mode, m)) { // a workgroup of NW waves takes a group
    const int NW = m->w2NW, KH = m->KP / NW;
    k.threads = (unsigned)(NW * kWave);
    // 1048 ... 1112: four waves per group of 48 ... 112 states; 5064 ... 8064: five ... eight waves of 64
    k.member = NW == kW2NW ? 1000 + KH : 1000 * NW + KH; // (2128: two waves of 128)
#define FSMC_PICK_W2(KHX, NWX)                                                                                          \
  if (KH == KHX && NW == NWX) {                                                                                        \
    k.fn = pickWaveGroupKernel<KHX, NWX>(mode, track, m->sequence != 0);                                               \
  }
    FSMC_ALL_W2(FSMC_PICK_W2)
#undef FSMC_PICK_W2
    return k;
  }
  k.member = familyMember(m);
  const bool half = wantStride != 1 && !m->sequence && // (also with two half-groups per wave)
                    ((mode == kModeIbd && halfBuilt(k.member)) || (mode == kModeSums && halfSumsBuilt(k.member)));
  k.stride = half ? 2 : 1;
  switch (k.member) {
#define FSMC_PICK_CASE(KTX)                                                                                             \
  case KTX:                                                                                                            \
    k.fn = pickMember<KTX>(mode, track, m->sequence, half, dual);                                                      \
    k.poolFn = (dual || m->sequence) ? nullptr : pickPoolMember<KTX>(mode, track, half);                               \
    break;
    FSMC_ALL_KT(FSMC_PICK_CASE)
    FSMC_EXACT_KT(FSMC_PICK_CASE)
#undef FSMC_PICK_CASE
  default:
    break; // (no such model passes fsmc_model_create: K <= 128 has a member, 128 < K <= 256 the wave-group kernel)
  }
  return k;
}

// Two waves per window (fsmc_kernels_bidir.h): the dump / per-pair / sums consumers of the lane-per-pair family in
// array mode.  nullptr where the kernel is not built (wave-group and any-K models, sequence mode, the IBD decode).
template <int KT> KernelFn pickBidirMember(int mode)
{
  switch (mode) {
  case kModeDump:
    return decode_kernel_bidir<KT, kModeDump>;
  case kModePerPair:
    return decode_kernel_bidir<KT, kModePerPair>;
  case kModeSums:
    return decode_kernel_bidir<KT, kModeSums>;
  default:
    return nullptr;
  }
}
KernelChoice chooseTwoWaveKernel(const fsmc_model* m, int mode)
{
  KernelChoice k{nullptr, 2 * kWave, familyMember(m), 1};
  if (m->sequence || anyStates(m) || waveGroups(mode, m)) {
    return k;
  }
  switch (k.member) {
#define FSMC_PICK_BIDIR(KTX)                                                                                            \
  case KTX:                                                                                                            \
    k.fn = pickBidirMember<KTX>(mode);                                                                                 \
    break;
    FSMC_ALL_KT(FSMC_PICK_BIDIR)
    FSMC_EXACT_KT(FSMC_PICK_BIDIR)
#undef FSMC_PICK_BIDIR
  default:
    break;
  }
  return k;
}

// The sweep kernel of a model (fsmc_pair_sweep.h): forward_kernel or viterbi_kernel of its lane-per-pair member, nullptr
// beyond 128 states.  `fn` is the kernel under its own type, for the launch; `k` carries it as a KernelChoice -- the
// occupancy query and the launch record take one -- with the pointer under the decode kernels' type.
template <typename Params> struct SweepKernel {
  KernelChoice k;                     // (k.fn is fn, cast: chooseSweepKernel sets the two together)
  void (*fn)(const Params) = nullptr;
};
// `pick(std::integral_constant<int, KT>)` names the instantiation of member KT.
template <typename Params, typename Pick> SweepKernel<Params> chooseSweepKernel(const fsmc_model* m, Pick pick)
{
  SweepKernel<Params> s;
  s.k = KernelChoice{nullptr, kWave, m->K <= 128 ? familyMember(m) : 0, 1};
  switch (s.k.member) {
#define FSMC_PICK_SWEEP(KTX)                                                                                            \
  case KTX:                                                                                                            \
    s.fn = pick(std::integral_constant<int, KTX>{});                                                                   \
    break;
    FSMC_ALL_KT(FSMC_PICK_SWEEP)
    FSMC_EXACT_KT(FSMC_PICK_SWEEP)
#undef FSMC_PICK_SWEEP
  default:
    break;
  }
  s.k.fn = reinterpret_cast<KernelFn>(s.fn);
  return s;
}

// An environment variable as a count, 0 where it is not set.
long envCount(const char* name)
{
  const char* s = std::getenv(name);
  return s ? std::atol(s) : 0;
}

// A diagnostic switch that lowers a count: NAME=<n> gives n where that is at least 1 and below `value`.
size_t loweredByEnv(const char* name, size_t value)
{
  return plan::lowered(value, envCount(name));
}

// The planner's inputs (fsmc_plan.h decides, this file does): the diagnostic switches as the environment has them at
// this call -- the tests change them between contexts --, the context's settings, and what the card has free.
plan::Diag readDiag()
{
  plan::Diag d;
  d.maxSlots = envCount("FSMC_DIAG_MAX_SLOTS");
  d.wavesPerCU = envCount("FSMC_DIAG_WAVES_PER_CU");
  d.sumsSlots = envCount("FSMC_DIAG_SUMS_SLOTS");
  d.minimaRange = envCount("FSMC_DIAG_MINIMA_RANGE");
  if (const char* v = std::getenv("FSMC_DIAG_WS_FREE")) {
    d.wsFree = std::strtoull(v, nullptr, 10);
  }
  if (const char* v = std::getenv("FSMC_DIAG_WS_EARN_SCALE")) {
    d.earnScale = std::atof(v);
  }
  if (const char* v = std::getenv("FSMC_DIAG_TWO_WAVE_WINDOWS")) {
    d.twoWavesNever = std::strcmp(v, "never") == 0;
  }
  if (const char* v = std::getenv("FSMC_DIAG_W2_MEMBER")) {
    int nw = 0, kh = 0;
    if (std::sscanf(v, "%dx%d", &nw, &kh) == 2) {
      d.w2NW = nw;
      d.w2KH = kh;
    }
  }
  return d;
}

plan::Settings settingsOf(const fsmc_ctx* ctx)
{
  plan::Settings s;
  s.nCU = ctx->nCU;
  s.hbmBytes = ctx->hbmBytes;
  s.wsLimit = ctx->wsLimit;
  s.chunkSites = ctx->chunkSites;
  s.residentChunks = ctx->residentChunks;
  s.chunkPool = ctx->chunkPool;
  s.chunkPoolPhi = ctx->chunkPoolPhi;
  return s;
}

plan::MemInfo memInfo()
{
  size_t freeB = 0, totalB = 0;
  plan::MemInfo mem;
  mem.known = hipMemGetInfo(&freeB, &totalB) == hipSuccess;
  mem.freeBytes = (uint64_t)freeB;
  return mem;
}

// Workgroups of a kernel that a CU holds at once, as the runtime counts them, `most` at the most.  `capDivisor` > 0:
// and no more than FSMC_DIAG_WAVES_PER_CU / capDivisor (occupancy experiments only).  The one occupancy query of the
// launch path; 0 comes back for a kernel that cannot run at all.
hipError_t workgroupsPerCU(const KernelChoice& k, int most, int capDivisor, int& perCU)
{
  perCU = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, k.fn, (int)k.threads, 0);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return e;
  }
  perCU = plan::capWorkgroups(perCU, most, capDivisor, readDiag());
  return hipSuccess;
}

static_assert(plan::kWave == kWave && plan::kFloat4Bytes == sizeof(float4), "fsmc_plan.h lays rows out for the kernels' wave");
static_assert(layout::kSpecBytes == sizeof(PairCdfSpec), "fsmc_pair_layout.h sizes pcSpec for the kernels' PairCdfSpec");

// A launch: its plan (fsmc_plan.h) and the kernel it was planned for.
struct LaunchPlan : plan::LaunchPlan {
  KernelChoice k;
};

// What a plan reads of kernel `k` of a model and mode; `perCU`: its workgroups a CU (workgroupsPerCU).
plan::KernelTraits traitsOf(const fsmc_model* m, int mode, const KernelChoice& k, int perCU)
{
  const bool w2 = waveGroups(mode, m); // a workgroup of four waves takes a group, lane = pair
  const bool any = anyStates(m);
  plan::KernelTraits t;
  t.member = k.member;
  t.stride = k.stride;
  t.rowFloat4 = w2 ? (size_t)m->KP / 4 : (size_t)((k.member > 0 ? k.member : m->K) + 3) / 4 + (any ? 1 : 0);
  t.sideRows = any ? (size_t)kAnyExtraRows + 2 : 4;
  t.chunkFloor = w2 ? 2048 : 512;
  t.resident = (mode == kModeIbd || mode == kModeSums) && !m->sequence && !any && (!w2 || w2ResidentBuilt(m->w2NW, false));
  t.pool = !w2 && k.poolFn != nullptr;
  t.perCU = perCU;
  return t;
}

// plan::workspaceBudget of the context as it is now.  `cur`: the buffer about to be re-used.
plan::WsBudget workspaceBudget(const fsmc_ctx* ctx, const DevBuf& cur)
{
  return plan::workspaceBudget(settingsOf(ctx), ctx->credit, memInfo(), cur.bytes, readDiag());
}

// A launch over the uploaded work list earns workspace for this and the following launches.
void earnWorkspace(fsmc_ctx* ctx, const fsmc_model* m, int mode)
{
  plan::earnWorkspace(ctx->credit, ctx->hGroups, mode == kModeIbd, m->K, readDiag());
}

// plan::planOneWave for kernel `k` over `list`.  Computes only: allocates nothing, leaves the context as it is
// (holdWorkspace, recordLaunch).  `why`: the message of a status other than FSMC_OK.
int planOneWave(const fsmc_ctx* ctx, const fsmc_model* m, int mode, const KernelChoice& k,
                const std::vector<fsmc_group>& list, bool paired, const plan::WsBudget& budget, unsigned share,
                LaunchPlan& plan, std::string& why)
{
  if (!k.fn) {
    why = "no kernel for this model";
    return FSMC_EUNSUPPORTED;
  }
  // the any-K kernel streams its K-vectors through the caches: with four waves per CU more of them stay there
  // (600 x 3000 list, K = 300: 1 / 2 / 4 / 8 waves per CU run 10.3 / 6.9 / 5.0 / 6.5 s)
  int perCU = 0;
  const hipError_t e = workgroupsPerCU(k, anyStates(m) ? 4 : 8, 1, perCU);
  if (e != hipSuccess) {
    why = std::string("occupancy query of the decode kernel: ") + hipGetErrorString(e);
    return FSMC_EHIP;
  }
  plan.k = k;
  return plan::planOneWave(settingsOf(ctx), traitsOf(m, mode, k, perCU), mode == kModeIbd, list, paired, budget, share,
                           readDiag(), plan, why);
}

// Two waves per window (plan::planTwoWaves).  twoWavesWanted: what can be said before the budget is read.
bool twoWavesWanted(const fsmc_ctx* ctx, const KernelChoice& k2, size_t nItems)
{
  if (ctx->twoWaves == 1 || nItems == 0 || !k2.fn || readDiag().twoWavesNever) {
    return false;
  }
  int perCU = 0;
  return workgroupsPerCU(k2, 4, 2, perCU) == hipSuccess && plan::allResident(settingsOf(ctx), perCU, nItems);
}

bool planTwoWaves(const fsmc_ctx* ctx, const KernelChoice& k2, size_t nItems, const plan::WsBudget& budget, LaunchPlan& plan)
{
  plan.k = k2;
  return plan::planTwoWaves(ctx->hGroups, k2.member, nItems, budget, plan);
}

// The one place the decode's workspace is allocated: `buf` holds at least `bytes` afterwards, or nothing.  A buffer
// that grows is freed first (it may be 80 % of the card: the two do not fit side by side) and debited from the credit.
// (diagnostic: FSMC_DIAG_WS_ALLOC_MAX=<bytes>: a request above it goes the way of a hipMalloc that failed after the
//  buffer held was released -- tests of what a launch does then)
int holdWorkspace(fsmc_ctx* ctx, DevBuf& buf, size_t bytes)
{
  const char* most = std::getenv("FSMC_DIAG_WS_ALLOC_MAX");
  if (most && bytes > std::strtoull(most, nullptr, 10) && !(buf.p && buf.bytes >= bytes)) {
    if (buf.p) {
      (void)hipFree(buf.p);
    }
    buf = DevBuf();
    return fail(ctx, FSMC_ENOMEM, "workspace of " + std::to_string(bytes) + " bytes refused (FSMC_DIAG_WS_ALLOC_MAX)");
  }
  const size_t held = buf.bytes;
  const int rc = ensure(ctx, buf, bytes);
  if (rc != FSMC_OK) {
    (void)hipGetLastError(); // (the failed hipMalloc's: a later launch's check must not find it)
  } else if (buf.bytes != held) {
    plan::payForWorkspace(settingsOf(ctx), ctx->credit, buf.bytes, readDiag());
  }
  return rc;
}

// One one-wave launch planned for `buf` and its workspace held.
int planAndHold(fsmc_ctx* ctx, const fsmc_model* m, int mode, const KernelChoice& k, const std::vector<fsmc_group>& list,
                bool paired, unsigned share, DevBuf& buf, LaunchPlan& plan)
{
  std::string why;
  const int rc = planOneWave(ctx, m, mode, k, list, paired, workspaceBudget(ctx, buf), share, plan, why);
  if (rc != FSMC_OK) {
    return fail(ctx, rc, why);
  }
  if (plan.poolBuffers) { // the pool's cursor, counters and claim words
    FSMC_TRY(ensure(ctx, ctx->poolState, (kPoolClaims + (size_t)plan.poolBuffers) * sizeof(unsigned)));
  }
  return holdWorkspace(ctx, buf, plan.bytes);
}

// The launch of sweep kernel `k` (the `name` kernel, in the occupancy message) planned into the decode's workspace and
// that workspace held: the credit the launch earns, then `planFn(perCU, budget, plan, why)` -- plan::planViterbi or
// plan::planSamples with what the entry point knows -- over the kernel's workgroups a CU.
template <typename PlanFn>
int planSweepAndHold(fsmc_ctx* ctx, const fsmc_model* m, const KernelChoice& k, const char* name, PlanFn planFn,
                     LaunchPlan& plan)
{
  earnWorkspace(ctx, m, kModePerPair);
  const plan::WsBudget budget = workspaceBudget(ctx, ctx->ws);
  int perCU = 0;
  const hipError_t e = workgroupsPerCU(k, 8, 1, perCU);
  if (e != hipSuccess) {
    return fail(ctx, FSMC_EHIP, std::string("occupancy query of the ") + name + " kernel: " + hipGetErrorString(e));
  }
  plan.k = k;
  std::string why;
  const int rc = planFn(perCU, budget, plan, why);
  if (rc != FSMC_OK) {
    return fail(ctx, rc, why);
  }
  return holdWorkspace(ctx, ctx->ws, plan.bytes);
}

// planSweepAndHold with the sampling kernel's plan (fsmc_decode_pair_transitions' kernel takes the same workspace and
// reports its occupancy as the sampling kernel's).
int planSamplingSweep(fsmc_ctx* ctx, const fsmc_model* m, const KernelChoice& k, size_t nGroups, LaunchPlan& plan)
{
  return planSweepAndHold(
      ctx, m, k, "sampling",
      [&](int perCU, const plan::WsBudget& budget, LaunchPlan& pl, std::string& why) {
        return plan::planSamples(settingsOf(ctx), m->S, k.member, perCU, nGroups, budget, pl, why);
      },
      plan);
}

// The launch the getters describe (fsmc_ctx_last_kernel, _last_beta_stride, _last_plan, _last_resident_chunks,
// _last_waves_per_window, fsmc_ctx_info's n_slots): written here, where a launch is committed, and nowhere else.
// `slotsBeside`: the workgroups of a second kernel that runs beside this one.
void recordLaunch(fsmc_ctx* ctx, const KernelChoice& k, const LaunchPlan& plan, int slotsBeside = 0)
{
  ctx->lastMember = k.member;
  ctx->lastStride = k.stride;
  ctx->lastChunk = plan.chunk;
  ctx->lastMaxChunks = plan.maxChunks;
  ctx->lastResident = plan.residentChunks;
  ctx->lastPoolBuffers = plan.poolBuffers;
  ctx->lastWavesPerWindow = plan.wavesPerWindow;
  ctx->lastSlots = plan.slots + slotsBeside;
}

int checkReady(fsmc_ctx* ctx, const fsmc_model* m)
{
  if (!ctx || !m) {
    return fail(ctx, FSMC_EINVAL, "null context or model");
  }
  if (m->ctx != ctx) {
    return fail(ctx, FSMC_EINVAL, "model belongs to another context");
  }
  if (!ctx->dHaps) {
    return fail(ctx, FSMC_ESTATE, "no haplotypes uploaded (fsmc_haps_upload)");
  }
  if (!ctx->dPairs || !ctx->dGroups || ctx->nGroups == 0) {
    return fail(ctx, FSMC_ESTATE, "no work list uploaded (fsmc_worklist_upload)");
  }
  if ((uint32_t)m->S != ctx->nSites) {
    return fail(ctx, FSMC_EINVAL, "model has " + std::to_string(m->S) + " sites but haplotypes have " +
                                      std::to_string(ctx->nSites));
  }
  for (const fsmc_pair& pr : ctx->hPairs) {
    if (pr.hap_a >= ctx->nHaps || pr.hap_b >= ctx->nHaps) {
      return fail(ctx, FSMC_EINVAL, "pair refers to a haplotype row outside the uploaded matrix");
    }
  }
  for (const fsmc_group& g : ctx->hGroups) {
    if (g.to > (uint32_t)m->S) {
      return fail(ctx, FSMC_EINVAL, "group window exceeds the number of sites");
    }
  }
  if (m->K > kMaxStatesAny) {
    return fail(ctx, FSMC_EUNSUPPORTED, "more than " + std::to_string(kMaxStatesAny) + " states");
  }
  return FSMC_OK;
}

void fillParams(const fsmc_ctx* ctx, const fsmc_model* m, const LaunchPlan& plan, uint32_t flags, KParams& p)
{
  std::memset(&p, 0, sizeof(p));
  p.K = m->K;
  p.KP = m->KP;
  p.S = m->S;
  p.W = (int)ctx->W;
  p.nGroups = (int)ctx->nGroups;
  p.chunk = plan.chunk;
  p.chunkRows = plan.chunkRows;
  p.maxChunks = plan.maxChunks;
  p.residentChunks = plan.residentChunks;
  p.flags = flags;
  p.pi = m->pi;
  p.cR = m->cR;
  p.expT = m->expT;
  p.D = m->D;
  p.B = m->B;
  p.U = m->U;
  p.rowSets = m->rowSets;
  p.RR = m->RR;
  p.ghostMask = m->ghostMask;
  p.stepRow = m->stepRow;
  p.rowGapF = m->rowGapF;
  p.rowSiteB = m->rowSiteB;
  p.rowGapB = m->rowGapB;
  p.emis3 = m->emis3;
  p.haps = ctx->dHaps;
  p.pairs = ctx->dPairs;
  p.groups = ctx->dGroups;
  p.counters = ctx->dCounters;
  p.phaseCycles = ctx->dPhase;
  p.ws = (float4*)ctx->ws.p;
  p.wsSlot = plan.wsSlot;
  p.stateThr = m->stateThr;
  p.ageThr = m->ageThr;
  p.spsLds = 0u;
  // int * float, evaluated in fp32 like HMM.cpp:1226,1254,1281,1308
  p.thr[0] = 1000 * m->probThr;
  p.thr[1] = 100 * m->probThr;
  p.thr[2] = 10 * m->probThr;
  p.thr[3] = m->probThr;
  p.recs = (fsmc_ibd_record*)ctx->recs.p;
  p.recCap = (unsigned)ctx->recCap;
}

// The one shape the kernels cannot check: every workgroup of the grid indexes its own wsSlot float4 of the workspace.
int checkWorkspace(fsmc_ctx* ctx, const KParams& p, int slots)
{
  const DevBuf& buf = p.ws == (float4*)ctx->wsSide.p ? ctx->wsSide : ctx->ws;
  if (!p.ws || p.ws != (float4*)buf.p || slots < 1 || buf.bytes / sizeof(float4) / (size_t)slots < p.wsSlot) {
    return fail(ctx, FSMC_ESTATE, "the workspace does not hold the launch planned for it");
  }
  return FSMC_OK;
}

// The parameters of decode_kernel_pool for a plan with a pool: `p` and the pool's place.  Checked like the slots: every
// buffer lies behind them, inside the workspace, and has its claim word.
int poolParams(fsmc_ctx* ctx, const KernelChoice& k, const KParams& p, const LaunchPlan& plan, int slots, KParamsPool& pp)
{
  static_cast<KParams&>(pp) = p;
  pp.poolOff = plan.poolOff;
  pp.poolBuffers = plan.poolBuffers;
  pp.poolCap = plan.poolCap;
  pp.poolState = (unsigned*)ctx->poolState.p;
  const DevBuf& buf = p.ws == (float4*)ctx->wsSide.p ? ctx->wsSide : ctx->ws;
  const size_t rowF4 = (size_t)((p.K + 3) / 4) * kWave; // (at most the member's: a lower bound is checked)
  const size_t poolF4 = (size_t)pp.poolBuffers * (size_t)p.chunkRows * rowF4;
  if (!k.poolFn || pp.poolOff < p.wsSlot * (size_t)slots || buf.bytes / sizeof(float4) < pp.poolOff ||
      buf.bytes / sizeof(float4) - pp.poolOff < poolF4 || !pp.poolState ||
      ctx->poolState.bytes / sizeof(unsigned) < kPoolClaims + (size_t)pp.poolBuffers || pp.poolCap < 1 ||
      pp.poolCap > p.maxChunks) {
    return fail(ctx, FSMC_ESTATE, "the workspace does not hold the chunk pool planned for it");
  }
  return FSMC_OK;
}

// The pool's state starts every launch from zero: cursor, counters, every buffer free.
int resetPool(fsmc_ctx* ctx, const KParamsPool& pp)
{
  FSMC_HIP(ctx, hipMemsetAsync(pp.poolState, 0, (kPoolClaims + (size_t)pp.poolBuffers) * sizeof(unsigned), ctx->stream));
  return FSMC_OK;
}

// `continues`: a later launch of one call's sequence (the sums' batches, `slots` a launch): the timed span started with
// the first one and ends behind the last (fsmc_last_kernel_ms: the whole sequence, its plane additions included).
// `plan`: the launch's plan where it may hold a chunk pool -- decode_kernel_pool then runs in decode_kernel's place.
int launch(fsmc_ctx* ctx, const KernelChoice& k, const KParams& p, int slots, size_t dynLds = 0, bool continues = false,
           const LaunchPlan* plan = nullptr)
{
  if (checkWorkspace(ctx, p, slots) != FSMC_OK) {
    return FSMC_ESTATE;
  }
  const bool pool = plan && plan->poolBuffers != 0;
  KParamsPool pp;
  if (pool) {
    FSMC_TRY(poolParams(ctx, k, p, *plan, slots, pp));
  }
  FSMC_HIP(ctx, hipMemsetAsync(ctx->dCounters, 0, 4 * sizeof(unsigned), ctx->stream));
  if (pool) {
    FSMC_TRY(resetPool(ctx, pp));
  }
  if (!continues) {
    FSMC_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  }
  if (pool) {
    hipLaunchKernelGGL(k.poolFn, dim3((unsigned)slots), dim3(k.threads), dynLds, ctx->stream, pp);
  } else {
    hipLaunchKernelGGL(k.fn, dim3((unsigned)slots), dim3(k.threads), dynLds, ctx->stream, p);
  }
  FSMC_HIP(ctx, hipGetLastError());
  FSMC_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  ctx->timed = true;
  return FSMC_OK;
}

// One decode as two kernels side by side: `pSide` (one group per wave; the long windows, so it starts first) on the
// side stream and `pMain` (two half-groups per wave) on the context's stream.  They share the record buffer and its
// counter and have a queue head each; the timed span covers both.
// `planSide`: the side kernel's plan, which may hold a chunk pool (the paired kernel keeps no resident chunks).
int launchBeside(fsmc_ctx* ctx, const KernelChoice& kSide, KParams& pSide, int slotsSide, const LaunchPlan& planSide,
                 const KernelChoice& kMain, KParams& pMain, int slotsMain)
{
  if (checkWorkspace(ctx, pSide, slotsSide) != FSMC_OK || checkWorkspace(ctx, pMain, slotsMain) != FSMC_OK) {
    return FSMC_ESTATE;
  }
  pMain.groupBase = 0;
  pSide.groupBase = 2;
  const bool pool = planSide.poolBuffers != 0;
  KParamsPool ppSide;
  if (pool) {
    FSMC_TRY(poolParams(ctx, kSide, pSide, planSide, slotsSide, ppSide));
  }
  FSMC_HIP(ctx, hipMemsetAsync(ctx->dCounters, 0, 4 * sizeof(unsigned), ctx->stream));
  if (pool) {
    FSMC_TRY(resetPool(ctx, ppSide));
  }
  FSMC_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  FSMC_HIP(ctx, hipEventRecord(ctx->evFork, ctx->stream));
  FSMC_HIP(ctx, hipStreamWaitEvent(ctx->side, ctx->evFork, 0));
  if (pool) {
    hipLaunchKernelGGL(kSide.poolFn, dim3((unsigned)slotsSide), dim3(kSide.threads), 0, ctx->side, ppSide);
  } else {
    hipLaunchKernelGGL(kSide.fn, dim3((unsigned)slotsSide), dim3(kSide.threads), 0, ctx->side, pSide);
  }
  FSMC_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(kMain.fn, dim3((unsigned)slotsMain), dim3(kMain.threads), 0, ctx->stream, pMain);
  FSMC_HIP(ctx, hipGetLastError());
  FSMC_HIP(ctx, hipEventRecord(ctx->evJoin, ctx->side));
  FSMC_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->evJoin, 0));
  FSMC_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  ctx->timed = true;
  return FSMC_OK;
}

// plan::stagingLimit of what the card has free right now.
uint64_t stagingLimit(const fsmc_ctx* ctx, uint64_t held, unsigned parts)
{
  return plan::stagingLimit(settingsOf(ctx), memInfo(), held, parts);
}

// The way out for rows a slice leaves on the device (the posterior tables, the tail / quantile rows): two pinned buffers
// of `need` bytes each at least, the copy stream and its events.
int ensureRowCopies(fsmc_ctx* ctx, size_t need)
{
  int fill = -1;
  FSMC_TRY(scratchFill(ctx, fill));
  if (ctx->ppPinnedBytes < need) {
    for (int i = 0; i < 2; ++i) {
      if (ctx->ppPinned[i]) {
        (void)hipHostFree(ctx->ppPinned[i]);
        ctx->ppPinned[i] = nullptr;
      }
    }
    ctx->ppPinnedBytes = 0;
    for (int i = 0; i < 2; ++i) {
      const hipError_t e = hipHostMalloc(&ctx->ppPinned[i], need, hipHostMallocDefault);
      if (e != hipSuccess) {
        ctx->ppPinned[i] = nullptr;
        return fail(ctx, FSMC_ENOMEM, std::string("hipHostMalloc of the row buffers failed: ") + hipGetErrorString(e));
      }
    }
    ctx->ppPinnedBytes = need;
  }
  if (fill >= 0) { // (no copy is in flight: every entry point has emptied both buffers when it returns)
    for (int i = 0; i < 2; ++i) {
      std::memset(ctx->ppPinned[i], fill, ctx->ppPinnedBytes);
      ctx->scratchFilled += ctx->ppPinnedBytes;
    }
  }
  if (!ctx->copyStream) {
    FSMC_HIP(ctx, hipStreamCreateWithFlags(&ctx->copyStream, hipStreamNonBlocking));
    FSMC_HIP(ctx, hipEventCreateWithFlags(&ctx->evRows, hipEventDisableTiming));
    FSMC_HIP(ctx, hipEventCreateWithFlags(&ctx->evCopied[0], hipEventDisableTiming));
    FSMC_HIP(ctx, hipEventCreateWithFlags(&ctx->evCopied[1], hipEventDisableTiming));
  }
  return FSMC_OK;
}

// What the dump / per-pair / pair-posterior / sums entry points share: the kernel, the credit the launch earns, the
// one-wave plan over `list` and its workspace; then, if a launch of `nItems` workgroups qualifies for two waves per
// window, that plan and its workspace; the record of what was committed.  The one-wave workspace is held first: the
// two-wave budget and the sums' plane limit count what is held, and a buffer only grows (a whole-window one-wave plan
// needs no less than the two-wave plan: one allocation).  If the two-wave buffer cannot be had, the one-wave buffer is
// taken again and the launch runs on that plan; FSMC_ENOMEM if that fails too.
// `stagingPerItem` (the sums): bytes of output staging a workgroup needs beside the workspace; the slots are cut to the
// items whose staging fits stagingLimit (and FSMC_DIAG_SUMS_SLOTS -- tests: many launches on a small problem), and two
// waves, whose items are all resident at once, are taken only if that leaves all of them.
int prepareDecode(fsmc_ctx* ctx, const fsmc_model* m, int mode, uint32_t wantStride,
                  const std::vector<fsmc_group>& list, size_t nItems, size_t stagingPerItem, LaunchPlan& plan)
{
  const KernelChoice k = chooseKernel(m, mode, false, false, wantStride);
  earnWorkspace(ctx, m, mode);
  FSMC_TRY(planAndHold(ctx, m, mode, k, list, false, 1, ctx->ws, plan));
  size_t staged = nItems;
  if (stagingPerItem) {
    staged = plan::stagedItems(stagingLimit(ctx, ctx->out.bytes, 1), stagingPerItem, readDiag());
    plan.slots = (int)std::min({(size_t)plan.slots, nItems, staged});
  }
  const KernelChoice k2 = chooseTwoWaveKernel(m, mode);
  LaunchPlan plan2;
  if (staged >= nItems && twoWavesWanted(ctx, k2, nItems) &&
      planTwoWaves(ctx, k2, nItems, workspaceBudget(ctx, ctx->ws), plan2)) {
    if (holdWorkspace(ctx, ctx->ws, plan2.bytes) == FSMC_OK) {
      plan = plan2;
    } else {
      ctx->err.clear();
      FSMC_TRY(holdWorkspace(ctx, ctx->ws, plan.bytes));
    }
  }
  recordLaunch(ctx, plan.k, plan);
  return FSMC_OK;
}

int setPairSlice(fsmc_ctx* ctx, PairSlicing kind, uint32_t groups)
{
  if (!ctx) {
    return FSMC_EINVAL;
  }
  ctx->pairSlices[kind].groups = groups;
  return FSMC_OK;
}

int lastPairSlices(const fsmc_ctx* ctx, PairSlicing kind, int32_t* slices)
{
  if (!ctx || !slices) {
    return FSMC_EINVAL;
  }
  *slices = ctx->pairSlices[kind].last;
  return FSMC_OK;
}

// The work list in slices of groups (plan::Slices), as the fsmc_decode_pair_* entry points send it through the device:
// the launch of a slice sees the slice as its whole group list (p.groups points at the slice's first group of the
// resident list).
struct WorkSlices : plan::Slices {
  LaunchPlan plan;
  // per-pair mode (perPairSetup): the slice's mean / MAP rows in ppStage
  float* stageMean = nullptr;
  int* stageMap = nullptr;
  // what the setups upload from: alive until the entry point synchronises the stream
  std::vector<size_t> hOffsets;
  std::vector<float> hCoal;
};

// The sliced entry points decode whole sequences only.  (A check of its own: each entry point keeps it where it
// always fired among its argument checks.)
int checkWholeSequence(fsmc_ctx* ctx, const fsmc_model* m, const char* what)
{
  for (const fsmc_group& g : ctx->hGroups) {
    if (g.from != 0 || g.to != (uint32_t)m->S) {
      return fail(ctx, FSMC_EINVAL, std::string(what) + " need whole-sequence groups (HMM.cpp:1378)");
    }
  }
  return FSMC_OK;
}

// The slices of a call and its decode plan, `mode` kModeDump or kModePerPair -- or kNoDecode: the slices alone, for an
// entry point that launches a sweep kernel of its own: fsmc_decode_pair_loglik, which needs no workspace, and
// fsmc_decode_pair_viterbi, _samples and _transitions, which plan their own (planSweepAndHold).  The slice is the
// caller's setting, or what stagingLimit holds of `groupBytes` a group, of half the room the card has free with the
// `held` bytes this entry point's buffers hold already counted as free -- the decode's workspace is allocated after
// this -- and `sliceMost` groups at the most.  One wave per window: planned from the first slice's groups; two waves: a
// workgroup for each group of a slice.
constexpr int kNoDecode = -1;
int planSlices(fsmc_ctx* ctx, const fsmc_model* m, int mode, PairSlicing kind, uint64_t held, size_t groupBytes,
               WorkSlices& ws, size_t sliceMost = SIZE_MAX)
{
  FSMC_HIP(ctx, hipSetDevice(ctx->device));
  const size_t setting = ctx->pairSlices[kind].groups;
  plan::planSlices(ctx->hGroups, setting, setting ? 0 : stagingLimit(ctx, held, 2), groupBytes, sliceMost, ws);
  if (mode != kNoDecode) {
    const std::vector<fsmc_group> first(ctx->hGroups.begin(), ctx->hGroups.begin() + (ptrdiff_t)ws.slice);
    FSMC_TRY(prepareDecode(ctx, m, mode, ctx->betaStride, first, ws.slice, 0, ws.plan));
  }
  return FSMC_OK;
}

// Dump mode: a slice's groups land in ppStage one after the other, [group][site][k][lane]; the offsets (which count
// from the slice's start) go to aux.  Both buffers are the entry point's to `ensure` before this.
int dumpSetup(fsmc_ctx* ctx, const fsmc_model* m, WorkSlices& ws, KParams& p)
{
  ws.hOffsets.resize(ws.slice);
  for (size_t i = 0; i < ws.slice; ++i) {
    ws.hOffsets[i] = i * (size_t)kWave * (size_t)m->K * (size_t)m->S;
  }
  FSMC_HIP(ctx, hipMemcpyAsync(ctx->aux.p, ws.hOffsets.data(), ws.slice * sizeof(size_t), hipMemcpyHostToDevice,
                               ctx->stream));
  fillParams(ctx, m, ws.plan, 0, p);
  p.dumpOut = (float*)ctx->ppStage.p;
  p.dumpOffsets = (const size_t*)ctx->aux.p;
  return FSMC_OK;
}

// The expected coalescence times as the per-pair consumers read them: a row padded to KP floats, to `dst` on the device.
// `keep` holds the padded row until the caller synchronises the stream.
int uploadExpCoal(fsmc_ctx* ctx, const fsmc_model* m, const float* exp_coal_times, void* dst, std::vector<float>& keep)
{
  keep.assign((size_t)m->KP, 0.f);
  std::memcpy(keep.data(), exp_coal_times, sizeof(float) * (size_t)m->K);
  FSMC_HIP(ctx, hipMemcpyAsync(dst, keep.data(), keep.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  return FSMC_OK;
}

// Per-pair mode: the expected coalescence times go to `dCoal`, and a slice's mean rows, then its MAP rows, [pair][S]
// each, take ppStage from its start (the entry point's to `ensure` before this).
int perPairSetup(fsmc_ctx* ctx, const fsmc_model* m, const float* exp_coal_times, void* dCoal, bool wantMean,
                 bool wantMap, WorkSlices& ws, KParams& p)
{
  FSMC_TRY(uploadExpCoal(ctx, m, exp_coal_times, dCoal, ws.hCoal));
  ws.stageMean = wantMean ? (float*)ctx->ppStage.p : nullptr;
  ws.stageMap = wantMap ? (int*)ctx->ppStage.p + (wantMean ? ws.slicePairsMax * (size_t)m->S : 0) : nullptr;
  fillParams(ctx, m, ws.plan, 0, p);
  p.expCoal = (const float*)dCoal;
  return FSMC_OK;
}

// The decode of slice `sl`.  The per-pair consumers index rows by pair of the work list, so the launch gets the staging
// pointers moved back by the slice's first pair: row `pair` of the work list is row `pair - firstPair` of the buffer.
int launchSlice(fsmc_ctx* ctx, const WorkSlices& ws, size_t sl, KParams& p)
{
  const size_t nG = ws.groups(sl), back = ws.firstPair(sl) * (size_t)p.S;
  p.groups = ctx->dGroups + ws.firstGroup(sl);
  p.nGroups = (int)nG;
  p.ppMean = ws.stageMean ? ws.stageMean - back : nullptr;
  p.ppMap = ws.stageMap ? ws.stageMap - back : nullptr;
  return launch(ctx, ws.plan.k, p, (int)std::min<size_t>((size_t)ws.plan.slots, nG), 0, sl != 0);
}

// The fields every sweep kernel's argument carries (FwdParams, VitParams: SweepParams of fsmc_pair_sweep.h, flat); the
// slice's own are launchSweepSlice's.
template <typename Params> void fillSweepParams(const fsmc_ctx* ctx, const fsmc_model* m, Params& p)
{
  p.S = m->S;
  p.W = (int)ctx->W;
  p.pi = m->pi;
  p.cR = m->cR;
  p.rowSets = m->rowSets;
  p.stepRow = m->stepRow;
  p.emis3 = m->emis3;
  p.haps = ctx->dHaps;
  p.pairs = ctx->dPairs;
  p.counter = ctx->dCounters;
}

// The sweep kernel of an entry point (`what`, as its messages begin) for a model: chooseSweepKernel's, or the refusal.
// A kernel without a sequence mode (`sequenceMode` false) refuses more than 128 states, then a sequence-mode model, and
// reports a member that was not built as FSMC_EUNSUPPORTED; the forward kernel, which has both modes, has one refusal.
// `name`: the kernel, as the refusals call it.
template <typename Params, typename Pick>
int sweepKernelFor(fsmc_ctx* ctx, const fsmc_model* m, const char* what, const char* name, bool sequenceMode, Pick pick,
                   SweepKernel<Params>& kern)
{
  const std::string noKernel = std::string(what) + ": no " + name + " kernel for a ";
  const std::string tooManyStates = noKernel + "model of more than 128 states (" + std::to_string(m->K) + ")";
  if (!sequenceMode && m->K > 128) {
    return fail(ctx, FSMC_EINVAL, tooManyStates);
  }
  if (!sequenceMode && m->sequence) {
    return fail(ctx, FSMC_EINVAL, noKernel + "sequence-mode model");
  }
  kern = chooseSweepKernel<Params>(m, pick);
  if (!kern.fn) {
    return sequenceMode ? fail(ctx, FSMC_EINVAL, tooManyStates)
                        : fail(ctx, FSMC_EUNSUPPORTED, std::string(what) + ": no kernel for this model");
  }
  return FSMC_OK;
}

// The argument of a sweep kernel whose launch planSweepAndHold planned: zero but for fillSweepParams' fields and the
// plan's -- the entry point adds its own --, and the record of the launch.
template <typename Params> void plannedSweepParams(fsmc_ctx* ctx, const fsmc_model* m, const LaunchPlan& plan, Params& p)
{
  std::memset(&p, 0, sizeof(p));
  fillSweepParams(ctx, m, p);
  p.K = m->K;
  p.chunk = plan.chunk;
  p.nChunks = plan.maxChunks;
  p.ws = (char*)ctx->ws.p;
  p.slotBytes = plan.wsSlot * sizeof(float4);
  recordLaunch(ctx, plan.k, plan);
}

// The sweep of slice `sl`: min(slots, groups) workgroups pull the slice's groups from the queue.  The call's timed span
// runs from the first slice's launch to the last one's end.
template <typename Params>
int launchSweepSlice(fsmc_ctx* ctx, const WorkSlices& ws, size_t sl, const SweepKernel<Params>& kern, int slots, Params& p)
{
  const size_t nG = ws.groups(sl);
  p.groups = ctx->dGroups + ws.firstGroup(sl);
  p.nGroups = (int)nG;
  p.pairBase = (unsigned)ws.firstPair(sl);
  FSMC_HIP(ctx, hipMemsetAsync(ctx->dCounters, 0, 4 * sizeof(unsigned), ctx->stream));
  if (sl == 0) {
    FSMC_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  }
  hipLaunchKernelGGL(kern.fn, dim3((unsigned)std::min<size_t>((size_t)slots, nG)), dim3(kern.k.threads), 0, ctx->stream,
                     p);
  FSMC_HIP(ctx, hipGetLastError());
  FSMC_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  ctx->timed = true;
  return FSMC_OK;
}

// A slice's per-pair values, `pairBytes` a pair from the start of `dev`, go to the caller's array at the slice's first
// pair: a blocking copy, before the next slice overwrites them.  A null `host` is an output that was not asked for.
int sliceToCaller(fsmc_ctx* ctx, const WorkSlices& ws, size_t sl, void* host, const void* dev, size_t pairBytes)
{
  if (host) {
    FSMC_HIP(ctx, hipMemcpy((char*)host + ws.firstPair(sl) * pairBytes, dev, ws.pairs(sl) * pairBytes,
                            hipMemcpyDeviceToHost));
  }
  return FSMC_OK;
}

// The pinned buffers' size, each: 128 MiB, FSMC_DIAG_ROW_COPY_BYTES=<bytes> for less -- tests: several copies a slice
// on a small problem.
size_t rowCopyBytes()
{
  return loweredByEnv("FSMC_DIAG_ROW_COPY_BYTES", (size_t)128 << 20);
}

// Spans of device memory leave through the two pinned buffers on the copy stream (ensureRowCopies), once the work
// stream has passed evRows: `chunk(c)` names span c of `nChunks`, none larger than a pinned buffer, and `sink(c, host)`
// receives it -- the next copy in flight while the host empties the one before.
struct RowChunk {
  const void* src;
  size_t bytes;
};
template <typename Chunk, typename Sink> int drainRows(fsmc_ctx* ctx, size_t nChunks, Chunk chunk, Sink sink)
{
  FSMC_HIP(ctx, hipStreamWaitEvent(ctx->copyStream, ctx->evRows, 0));
  auto issue = [&](size_t c, int b) -> int {
    const RowChunk ch = chunk(c);
    FSMC_HIP(ctx, hipMemcpyAsync(ctx->ppPinned[b], ch.src, ch.bytes, hipMemcpyDeviceToHost, ctx->copyStream));
    FSMC_HIP(ctx, hipEventRecord(ctx->evCopied[b], ctx->copyStream));
    return FSMC_OK;
  };
  FSMC_TRY(issue(0, 0));
  for (size_t c = 0, b = 0; c < nChunks; ++c, b ^= 1) {
    if (c + 1 < nChunks) {
      FSMC_TRY(issue(c + 1, (int)b ^ 1));
    }
    FSMC_HIP(ctx, hipEventSynchronize(ctx->evCopied[b]));
    sink(c, (const char*)ctx->ppPinned[b]);
  }
  return FSMC_OK;
}

// A slice whose rows are one span on the device and one span of the caller's array: `bytes` from `src` leave for `dst`
// through drainRows in copies of `copyBytes` -- spanCopyBytes' -- that need not end with a row.  (evRows is the entry
// point's to record: once a slice, however many spans leave.)
size_t spanCopyBytes(size_t slicePairsMax, size_t bytesPerPair)
{
  return std::max<size_t>(1, std::min(rowCopyBytes(), slicePairsMax * bytesPerPair));
}
int drainSpan(fsmc_ctx* ctx, const void* src, void* dst, size_t bytes, size_t copyBytes)
{
  auto span = [&](size_t c) { return std::min(copyBytes, bytes - c * copyBytes); };
  return drainRows(
      ctx, (bytes + copyBytes - 1) / copyBytes,
      [&](size_t c) { return RowChunk{(const char*)src + c * copyBytes, span(c)}; },
      [&](size_t c, const char* host) { std::memcpy((char*)dst + c * copyBytes, host, span(c)); });
}

// The slice loop of the entry points whose rows leave through drainRows: slice by slice the decode, `reduce(sl)` -- the
// launches that turn the slice's dump into rows -- and the end of the call's timed span (every decode and every
// reduction).  `wantRows`: `drain(sl)` takes the rows of a slice to the caller while the next slice decodes, and
// returns before that one's reduction overwrites them; the last slice's rows leave after the loop.
template <typename Reduce, typename Drain>
int decodeSlicesDrained(fsmc_ctx* ctx, const WorkSlices& ws, KParams& p, bool wantRows, Reduce reduce, Drain drain)
{
  bool pending = false; // the rows of slice sl - 1 are still on the device
  for (size_t sl = 0; sl < ws.nSlices; ++sl) {
    FSMC_TRY(launchSlice(ctx, ws, sl, p));
    if (pending) { // (while this slice decodes; ppRows is free again when it returns)
      FSMC_TRY(drain(sl - 1));
    }
    FSMC_TRY(reduce(sl));
    FSMC_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    if (wantRows) {
      FSMC_HIP(ctx, hipEventRecord(ctx->evRows, ctx->stream));
    }
    pending = wantRows && ws.pairs(sl) > 0;
  }
  return pending ? drain(ws.nSlices - 1) : FSMC_OK;
}

int checkBinEdges(fsmc_ctx* ctx, const fsmc_model* m, const int32_t* edges, size_t n_bins)
{
  if (n_bins == 0) {
    return fail(ctx, FSMC_EINVAL, "need one bin at least (n_bins + 1 edges)");
  }
  if (n_bins > (size_t)m->S) {
    return fail(ctx, FSMC_EINVAL, "bin edges must be strictly ascending: more bins than sites");
  }
  if (edges[0] < 0 || edges[n_bins] > m->S) {
    return fail(ctx, FSMC_EINVAL, "bin edges must lie in [0, sites]");
  }
  for (size_t b = 0; b < n_bins; ++b) {
    if (edges[b] >= edges[b + 1]) {
      return fail(ctx, FSMC_EINVAL, "bin edges must be strictly ascending");
    }
  }
  return FSMC_OK;
}

// The tail states of a call, each in [1, K], as outputs of pair_cdf_kernel appended to `spec`.  `rows` (may be null):
// the caller's matrix of each, checked first.
constexpr size_t kMaxOfAKind = 8; // tail states, quantiles a call
constexpr const char* kTooManyTailStates = "at most 8 tail states a call";
int tailSpecs(fsmc_ctx* ctx, const fsmc_model* m, const int32_t* tail_states, size_t n_tail, float* const* rows,
              std::vector<PairCdfSpec>& spec)
{
  for (size_t j = 0; j < n_tail; ++j) {
    if (rows && !rows[j]) {
      return fail(ctx, FSMC_EINVAL, "tail_rows[" + std::to_string(j) + "] is null");
    }
    if (tail_states[j] < 1 || tail_states[j] > m->K) {
      return fail(ctx, FSMC_EINVAL, "tail state " + std::to_string(tail_states[j]) + " outside [1, K]");
    }
    spec.push_back(PairCdfSpec{tail_states[j], 0.f});
  }
  return FSMC_OK;
}

// The B + 1 edges of B bins of sites, to `dst` on the device; the caller's array is the source until the entry point
// synchronises the stream.
int uploadBinEdges(fsmc_ctx* ctx, void* dst, const int32_t* bin_edges, size_t B)
{
  FSMC_HIP(ctx, hipMemcpyAsync(dst, bin_edges, (B + 1) * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  return FSMC_OK;
}

// Workgroups of pair_bins_kernel / pair_tail_bins_kernel over `cells` cells (pair x bin): a wave per cell, no more than
// fill the chip `wavesDeep` deep over the `cuts` the grid's y dimension repeats them for.
unsigned binBlocks(const fsmc_ctx* ctx, size_t wavesDeep, size_t cuts, size_t cells)
{
  const size_t wavesPerBlock = kPairBinsThreads / kWave;
  const size_t blocksMax = std::max<size_t>(1, wavesDeep * (size_t)std::max(ctx->nCU, 1) / cuts);
  return (unsigned)std::min(blocksMax, (cells + wavesPerBlock - 1) / wavesPerBlock);
}

// pair_cdf_kernel reduces a slice's dump in ppStage into ppRows, [output][pair of slice][S], the `nOut` outputs pcSpec
// names: the argument but for the slice's fields, and the launch of slice `sl` -- a workgroup per group and site block.
PairCdfParams cdfParams(const fsmc_ctx* ctx, const fsmc_model* m, const WorkSlices& ws, size_t nOut)
{
  PairCdfParams q;
  q.stage = (const float*)ctx->ppStage.p;
  q.K = m->K;
  q.S = m->S;
  q.spec = (const PairCdfSpec*)ctx->pcSpec.p;
  q.nOut = (int)nOut;
  q.rows = (int*)ctx->ppRows.p;
  q.rowsPerOut = ws.slicePairsMax;
  return q;
}
int launchCdf(fsmc_ctx* ctx, const WorkSlices& ws, size_t sl, PairCdfParams& q)
{
  q.groups = ctx->dGroups + ws.firstGroup(sl);
  q.nGroups = (int)ws.groups(sl);
  q.firstPair = (unsigned)ws.firstPair(sl);
  hipLaunchKernelGGL(pair_cdf_kernel, dim3((unsigned)(ws.groups(sl) * layout::siteBlocks((size_t)q.S))),
                     dim3(kPairCdfThreads), 0, ctx->stream, q);
  FSMC_HIP(ctx, hipGetLastError());
  return FSMC_OK;
}

} // namespace

extern "C" {

const char* fsmc_last_error(const fsmc_ctx* ctx)
{
  return ctx ? ctx->err.c_str() : g_createError.c_str();
}

int fsmc_ctx_create(int device_id, void* stream, fsmc_ctx** out)
{
  if (!out) {
    return fail(nullptr, FSMC_EINVAL, "out is null");
  }
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    return fail(nullptr, FSMC_ENODEVICE,
                std::string("no HIP device available (") + (e == hipSuccess ? "count = 0" : hipGetErrorString(e)) +
                    "); this library has no CPU fallback");
  }
  if (device_id < 0 || device_id >= n) {
    return fail(nullptr, FSMC_EINVAL, "device_id out of range");
  }
  fsmc_ctx* ctx = new (std::nothrow) fsmc_ctx();
  if (!ctx) {
    return fail(nullptr, FSMC_ENOMEM, "host allocation failed");
  }
  ctx->device = device_id;
  e = hipSetDevice(device_id);
  hipDeviceProp_t prop;
  if (e == hipSuccess) {
    e = hipGetDeviceProperties(&prop, device_id);
  }
  if (e != hipSuccess) {
    delete ctx;
    return fail(nullptr, FSMC_ENODEVICE, std::string("hipSetDevice/hipGetDeviceProperties: ") + hipGetErrorString(e));
  }
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    std::string arch = prop.gcnArchName;
    delete ctx;
    return fail(nullptr, FSMC_ENODEVICE, "device is " + arch + "; this library is built for gfx950 (MI355X) only");
  }
  ctx->nCU = prop.multiProcessorCount;
  ctx->hbmBytes = (uint64_t)prop.totalGlobalMem;
  if (stream) {
    ctx->stream = (hipStream_t)stream;
  } else {
    e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    ctx->ownStream = (e == hipSuccess);
  }
  if (e == hipSuccess) e = hipEventCreate(&ctx->ev0);
  if (e == hipSuccess) e = hipEventCreate(&ctx->ev1);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->evFork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->evJoin, hipEventDisableTiming);
  if (e == hipSuccess) e = hipMalloc((void**)&ctx->dCounters, 4 * sizeof(unsigned));
  if (e == hipSuccess) e = hipMalloc((void**)&ctx->dPhase, kPhaseSlots * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemset(ctx->dPhase, 0, kPhaseSlots * sizeof(unsigned long long));
  if (e != hipSuccess) {
    std::string msg = std::string("context set-up failed: ") + hipGetErrorString(e);
    fsmc_ctx_destroy(ctx);
    return fail(nullptr, FSMC_EHIP, msg);
  }
  // Two copies of the HIP runtime in the process (mappedHipRuntimes) are a DIAGNOSIS, not a gate: an embedding process
  // may map a second copy and still launch fine.  So try what breaks in that case -- the occupancy query of a kernel
  // built for one wave per SIMD -- and name the cause only if it does.
  {
    int blocks = 0;
    const hipError_t pe = hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &blocks, decode_kernel<128, kModeIbd, true, false, false>, kWave, 0);
    if (pe != hipSuccess) {
      (void)hipGetLastError();
      const std::vector<std::string> rts = mappedHipRuntimes();
      std::string msg = std::string("kernels of this library cannot be launched (") + hipGetErrorString(pe) + ")";
      int code = FSMC_EHIP;
      if (rts.size() > 1) {
        code = FSMC_ERUNTIME;
        msg += ": two HIP runtimes are loaded in this process (";
        for (size_t i = 0; i < rts.size(); ++i) {
          msg += (i ? ", " : "") + rts[i];
        }
        msg += "): load one libamdhip64 only -- e.g. import torch before this library so that both resolve to the "
               "copy torch bundles, or link both against the same ROCm";
      }
      fsmc_ctx_destroy(ctx);
      return fail(nullptr, code, msg);
    }
  }
  *out = ctx;
  return FSMC_OK;
}

void fsmc_ctx_destroy(fsmc_ctx* ctx)
{
  if (!ctx) {
    return;
  }
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) {
    (void)hipStreamSynchronize(ctx->stream);
  }
  if (ctx->dHaps) (void)hipFree(ctx->dHaps);
  if (ctx->dPairs) (void)hipFree(ctx->dPairs);
  if (ctx->dGroups) (void)hipFree(ctx->dGroups);
  if (ctx->dItems) (void)hipFree(ctx->dItems);
  if (ctx->dRest) (void)hipFree(ctx->dRest);
  if (ctx->dCounters) (void)hipFree(ctx->dCounters);
  if (ctx->poolState.p) (void)hipFree(ctx->poolState.p);
  if (ctx->dPhase) (void)hipFree(ctx->dPhase);
  if (ctx->idStash.p) (void)hipFree(ctx->idStash.p);
  if (ctx->ws.p) (void)hipFree(ctx->ws.p);
  if (ctx->recs.p) (void)hipFree(ctx->recs.p);
  if (ctx->aux.p) (void)hipFree(ctx->aux.p);
  if (ctx->out.p) (void)hipFree(ctx->out.p);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  if (ctx->evFork) (void)hipEventDestroy(ctx->evFork);
  if (ctx->evJoin) (void)hipEventDestroy(ctx->evJoin);
  if (ctx->side) (void)hipStreamDestroy(ctx->side);
  if (ctx->wsSide.p) (void)hipFree(ctx->wsSide.p);
  if (ctx->copyStream) (void)hipStreamSynchronize(ctx->copyStream);
  if (ctx->ppStage.p) (void)hipFree(ctx->ppStage.p);
  if (ctx->ppRows.p) (void)hipFree(ctx->ppRows.p);
  if (ctx->pcSpec.p) (void)hipFree(ctx->pcSpec.p);
  if (ctx->ptAcc.p) (void)hipFree(ctx->ptAcc.p);
  if (ctx->ppAcc.p) (void)hipFree(ctx->ppAcc.p);
  if (ctx->pmAcc.p) (void)hipFree(ctx->pmAcc.p);
  if (ctx->pbAcc.p) (void)hipFree(ctx->pbAcc.p);
  if (ctx->plAcc.p) (void)hipFree(ctx->plAcc.p);
  if (ctx->pxAcc.p) (void)hipFree(ctx->pxAcc.p);
  if (ctx->pvAcc.p) (void)hipFree(ctx->pvAcc.p);
  for (int i = 0; i < 2; ++i) {
    if (ctx->ppPinned[i]) (void)hipHostFree(ctx->ppPinned[i]);
    if (ctx->evCopied[i]) (void)hipEventDestroy(ctx->evCopied[i]);
  }
  if (ctx->evRows) (void)hipEventDestroy(ctx->evRows);
  if (ctx->copyStream) (void)hipStreamDestroy(ctx->copyStream);
  if (ctx->ownStream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

int fsmc_ctx_info(const fsmc_ctx* ctx, int32_t* n_cu, int32_t* n_slots, uint64_t* hbm_bytes)
{
  if (!ctx) {
    return FSMC_EINVAL;
  }
  if (n_cu) *n_cu = ctx->nCU;
  if (n_slots) *n_slots = ctx->lastSlots;
  if (hbm_bytes) *hbm_bytes = ctx->hbmBytes;
  return FSMC_OK;
}

uint64_t fsmc_ctx_scratch_filled(const fsmc_ctx* ctx)
{
  return ctx ? ctx->scratchFilled : 0;
}

int fsmc_ctx_set_workspace_limit(fsmc_ctx* ctx, uint64_t bytes)
{
  if (!ctx) {
    return FSMC_EINVAL;
  }
  ctx->wsLimit = bytes;
  return FSMC_OK;
}

int fsmc_ctx_expect_work(fsmc_ctx* ctx, double pair_sites, int32_t states)
{
  if (!ctx) {
    return fail(nullptr, FSMC_EINVAL, "null context");
  }
  if (!(pair_sites >= 0) || states < 1) {
    return fail(ctx, FSMC_EINVAL, "expected work: pair-sites >= 0 and states >= 1");
  }
  plan::expectWork(settingsOf(ctx), ctx->credit, pair_sites, states, readDiag());
  return FSMC_OK;
}

int fsmc_ctx_set_chunk_sites(fsmc_ctx* ctx, uint32_t sites)
{
  if (!ctx) {
    return FSMC_EINVAL;
  }
  ctx->chunkSites = sites;
  return FSMC_OK;
}

int fsmc_ctx_set_beta_stride(fsmc_ctx* ctx, uint32_t stride)
{
  if (!ctx || stride > 2) {
    return fail(ctx, FSMC_EINVAL, "beta stride must be 0 (automatic), 1 or 2");
  }
  ctx->betaStride = stride;
  return FSMC_OK;
}

int fsmc_ctx_last_beta_stride(const fsmc_ctx* ctx, int32_t* stride)
{
  if (!ctx || !stride) {
    return FSMC_EINVAL;
  }
  *stride = ctx->lastStride;
  return FSMC_OK;
}

int fsmc_ctx_last_plan(const fsmc_ctx* ctx, int32_t* chunk_sites, int32_t* max_chunks, int32_t* n_slots)
{
  if (!ctx) {
    return FSMC_EINVAL;
  }
  if (chunk_sites) *chunk_sites = ctx->lastChunk;
  if (max_chunks) *max_chunks = ctx->lastMaxChunks;
  if (n_slots) *n_slots = ctx->lastSlots;
  return FSMC_OK;
}

int fsmc_ctx_set_resident_chunks(fsmc_ctx* ctx, int32_t chunks)
{
  if (!ctx || chunks < -1) {
    return fail(ctx, FSMC_EINVAL, "resident chunks: -1 (automatic), 0 (none) or a count");
  }
  ctx->residentChunks = chunks;
  return FSMC_OK;
}

int fsmc_ctx_last_resident_chunks(const fsmc_ctx* ctx, int32_t* chunks)
{
  if (!ctx || !chunks) {
    return FSMC_EINVAL;
  }
  *chunks = ctx->lastResident;
  return FSMC_OK;
}

int fsmc_ctx_set_chunk_pool(fsmc_ctx* ctx, int32_t mode, uint32_t phi_percent)
{
  if (!ctx || mode < -1 || mode > 1) {
    return fail(ctx, FSMC_EINVAL, "chunk pool: -1 (automatic), 0 (never) or 1 (also in launches of one or two rounds and the sums)");
  }
  if (phi_percent != 0 && (phi_percent < 100 || phi_percent > 100000)) {
    return fail(ctx, FSMC_EINVAL, "chunk pool: phi is 100 ... 100000 per cent of a wave's share (0: the default)");
  }
  ctx->chunkPool = mode;
  ctx->chunkPoolPhi = phi_percent ? phi_percent : kChunkPoolPhiDefault;
  return FSMC_OK;
}

int fsmc_ctx_last_chunk_pool(fsmc_ctx* ctx, uint32_t* buffers, uint32_t* kept, uint32_t* rebuilt, uint32_t* outstanding)
{
  if (!ctx) {
    return FSMC_EINVAL;
  }
  uint32_t k = 0, r = 0, o = 0;
  if (ctx->lastPoolBuffers) {
    FSMC_HIP(ctx, hipSetDevice(ctx->device));
    FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<unsigned> st(kPoolClaims + (size_t)ctx->lastPoolBuffers);
    if (!ctx->poolState.p || ctx->poolState.bytes < st.size() * sizeof(unsigned)) {
      return fail(ctx, FSMC_ESTATE, "the chunk pool's state is gone");
    }
    FSMC_HIP(ctx, hipMemcpy(st.data(), ctx->poolState.p, st.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    k = st[kPoolKept];
    r = st[kPoolRebuilt];
    for (size_t i = kPoolClaims; i < st.size(); ++i) {
      o += st[i] != 0u;
    }
  }
  if (buffers) *buffers = ctx->lastPoolBuffers;
  if (kept) *kept = k;
  if (rebuilt) *rebuilt = r;
  if (outstanding) *outstanding = o;
  return FSMC_OK;
}

int fsmc_ctx_set_pair_posterior_slice(fsmc_ctx* ctx, uint32_t groups) { return setPairSlice(ctx, kSlicePosteriors, groups); }
int fsmc_ctx_last_pair_posterior_slices(const fsmc_ctx* ctx, int32_t* slices) { return lastPairSlices(ctx, kSlicePosteriors, slices); }
int fsmc_ctx_set_pair_minima_slice(fsmc_ctx* ctx, uint32_t groups) { return setPairSlice(ctx, kSliceMinima, groups); }
int fsmc_ctx_last_pair_minima_slices(const fsmc_ctx* ctx, int32_t* slices) { return lastPairSlices(ctx, kSliceMinima, slices); }
int fsmc_ctx_set_pair_bins_slice(fsmc_ctx* ctx, uint32_t groups) { return setPairSlice(ctx, kSliceBins, groups); }
int fsmc_ctx_last_pair_bins_slices(const fsmc_ctx* ctx, int32_t* slices) { return lastPairSlices(ctx, kSliceBins, slices); }
int fsmc_ctx_set_pair_cdf_slice(fsmc_ctx* ctx, uint32_t groups) { return setPairSlice(ctx, kSliceCdf, groups); }
int fsmc_ctx_last_pair_cdf_slices(const fsmc_ctx* ctx, int32_t* slices) { return lastPairSlices(ctx, kSliceCdf, slices); }
int fsmc_ctx_set_pair_tail_slice(fsmc_ctx* ctx, uint32_t groups) { return setPairSlice(ctx, kSliceTail, groups); }
int fsmc_ctx_last_pair_tail_slices(const fsmc_ctx* ctx, int32_t* slices) { return lastPairSlices(ctx, kSliceTail, slices); }
int fsmc_ctx_set_pair_loglik_slice(fsmc_ctx* ctx, uint32_t groups) { return setPairSlice(ctx, kSliceLoglik, groups); }
int fsmc_ctx_last_pair_loglik_slices(const fsmc_ctx* ctx, int32_t* slices) { return lastPairSlices(ctx, kSliceLoglik, slices); }
int fsmc_ctx_set_pair_viterbi_slice(fsmc_ctx* ctx, uint32_t groups) { return setPairSlice(ctx, kSliceViterbi, groups); }
int fsmc_ctx_last_pair_viterbi_slices(const fsmc_ctx* ctx, int32_t* slices) { return lastPairSlices(ctx, kSliceViterbi, slices); }
int fsmc_ctx_set_pair_samples_slice(fsmc_ctx* ctx, uint32_t groups) { return setPairSlice(ctx, kSliceSamples, groups); }
int fsmc_ctx_last_pair_samples_slices(const fsmc_ctx* ctx, int32_t* slices) { return lastPairSlices(ctx, kSliceSamples, slices); }
int fsmc_ctx_set_pair_transitions_slice(fsmc_ctx* ctx, uint32_t groups) { return setPairSlice(ctx, kSliceTransitions, groups); }
int fsmc_ctx_last_pair_transitions_slices(const fsmc_ctx* ctx, int32_t* slices) { return lastPairSlices(ctx, kSliceTransitions, slices); }

int fsmc_ctx_last_kernel(const fsmc_ctx* ctx, int32_t* member)
{
  if (!ctx || !member) {
    return FSMC_EINVAL;
  }
  *member = ctx->lastMember;
  return FSMC_OK;
}

int fsmc_model_create(fsmc_ctx* ctx, const fsmc_model_desc* d, fsmc_model** out)
{
  if (!ctx || !d || !out) {
    return fail(ctx, FSMC_EINVAL, "null argument");
  }
  *out = nullptr;
  std::string why;
  const int checked = model::checkDesc(*d, why);
  if (checked != FSMC_OK) {
    return fail(ctx, checked, why);
  }
  FSMC_HIP(ctx, hipSetDevice(ctx->device));
  fsmc_model* m = new (std::nothrow) fsmc_model();
  if (!m) {
    return fail(ctx, FSMC_ENOMEM, "host allocation failed");
  }
  const model::Shape shape = model::shapeOf(d->K, readDiag(), builtW2Members());
  m->ctx = ctx;
  m->K = d->K;
  m->KP = shape.KP;
  m->w2NW = shape.w2NW;
  m->S = d->S;
  m->nRows = d->n_rows;
  m->stateThr = d->state_threshold;
  m->ageThr = d->age_threshold;
  m->probThr = d->probability_threshold;
  m->sequence = d->sequence != 0;
  // fsmc_model_tables.h builds, this uploads: one table at a time, each gone from the host before the next is built
  auto uploadTables = [&]() -> int {
    const int K = m->K, KP = m->KP;
    const size_t rows = (size_t)d->n_rows;
    FSMC_TRY(upload(ctx, &m->pi, model::padRows(d->pi, 1, K, KP)));
    FSMC_TRY(upload(ctx, &m->cR, model::padRows(d->col_ratios, 1, K, KP)));
    FSMC_TRY(upload(ctx, &m->expT, model::padRows(d->exp_times, 1, K, KP)));
    FSMC_TRY(upload(ctx, &m->D, model::padRows(d->D, rows, K, KP)));
    FSMC_TRY(upload(ctx, &m->B, model::padRows(d->B, rows, K, KP)));
    FSMC_TRY(upload(ctx, &m->U, model::padRows(d->U, rows, K, KP)));
    FSMC_TRY(upload(ctx, &m->RR, model::padRows(d->RR, rows, K, KP)));
    FSMC_TRY(upload(ctx, &m->rowSets, model::rowSets(d->D, d->B, d->U, d->RR, rows, K, KP)));
    FSMC_TRY(upload(ctx, &m->ghostMask, model::ghostMask(K, KP)));
    // the kernel's "stepRow" is the (forward) site step: step_row in array mode, site_row_f in sequence mode
    FSMC_TRY(upload(ctx, &m->stepRow, model::stepRows(m->sequence ? d->site_row_f : d->step_row, d->S)));
    if (m->sequence) {
      FSMC_TRY(upload(ctx, &m->rowGapF, model::stepRows(d->gap_row_f, d->S)));
      FSMC_TRY(upload(ctx, &m->rowSiteB, model::stepRows(d->site_row_b, d->S)));
      FSMC_TRY(upload(ctx, &m->rowGapB, model::stepRows(d->gap_row_b, d->S)));
    }
    return upload(ctx, (float**)&m->emis3, model::emissions(*d, KP));
  };
  const int rc = uploadTables();
  if (rc != FSMC_OK) {
    fsmc_model_destroy(m);
    return rc;
  }
  *out = m;
  return FSMC_OK;
}

void fsmc_model_destroy(fsmc_model* m)
{
  if (!m) {
    return;
  }
  if (m->ctx) {
    (void)hipSetDevice(m->ctx->device);
    if (m->ctx->ibdModel == m) {
      m->ctx->ibdModel = nullptr;
    }
  }
  float* ptrs[] = {m->pi, m->cR, m->expT, m->D, m->B, m->U, m->rowSets, m->ghostMask, m->RR, (float*)m->emis3};
  for (float* q : ptrs) {
    if (q) (void)hipFree(q);
  }
  int* rowPtrs[] = {m->stepRow, m->rowGapF, m->rowSiteB, m->rowGapB};
  for (int* q : rowPtrs) {
    if (q) (void)hipFree(q);
  }
  delete m;
}

int fsmc_haps_upload(fsmc_ctx* ctx, const uint64_t* bits, uint32_t n_haps, uint32_t n_sites)
{
  if (!ctx || !bits || n_haps == 0 || n_sites == 0) {
    return fail(ctx, FSMC_EINVAL, "null or empty haplotype matrix");
  }
  FSMC_HIP(ctx, hipSetDevice(ctx->device));
  const uint32_t W = (n_sites + 63u) / 64u;
  FSMC_TRY(upload(ctx, &ctx->dHaps, (const unsigned long long*)bits, (size_t)n_haps * W));
  ctx->nHaps = n_haps;
  ctx->nSites = n_sites;
  ctx->W = W;
  return FSMC_OK;
}

int fsmc_worklist_upload(fsmc_ctx* ctx, const fsmc_pair* pairs, size_t n_pairs, const fsmc_group* groups,
                         size_t n_groups)
{
  if (!ctx || !pairs || !groups || n_pairs == 0 || n_groups == 0) {
    return fail(ctx, FSMC_EINVAL, "null or empty work list");
  }
  std::string why;
  const int checked = model::checkWorklist(n_pairs, groups, n_groups, why);
  if (checked != FSMC_OK) {
    return fail(ctx, checked, why);
  }
  FSMC_HIP(ctx, hipSetDevice(ctx->device));
  FSMC_TRY(upload(ctx, &ctx->dPairs, pairs, n_pairs));
  FSMC_TRY(upload(ctx, &ctx->dGroups, groups, n_groups));
  ctx->nPairs = n_pairs;
  ctx->nGroups = n_groups;
  ctx->hPairs.assign(pairs, pairs + n_pairs);
  ctx->hGroups.assign(groups, groups + n_groups);
  ctx->worklistSerial += 1;
  ctx->ibdPending = false;
  return FSMC_OK;
}

int fsmc_ctx_set_pairing(fsmc_ctx* ctx, uint32_t mode)
{
  if (!ctx || mode > 1) {
    return fail(ctx, FSMC_EINVAL, "pairing must be 0 (off) or 1 (automatic)");
  }
  ctx->pairing = mode;
  return FSMC_OK;
}

int fsmc_ctx_set_two_wave_windows(fsmc_ctx* ctx, uint32_t mode)
{
  if (!ctx || mode > 1) {
    return fail(ctx, FSMC_EINVAL, "two-wave windows: 0 (automatic) or 1 (never)");
  }
  ctx->twoWaves = mode;
  return FSMC_OK;
}

int fsmc_ctx_last_waves_per_window(const fsmc_ctx* ctx, int32_t* waves)
{
  if (!ctx || !waves) {
    return FSMC_EINVAL;
  }
  *waves = ctx->lastWavesPerWindow;
  return FSMC_OK;
}

int fsmc_ctx_last_items(const fsmc_ctx* ctx, int32_t* n_items)
{
  if (!ctx || !n_items) {
    return FSMC_EINVAL;
  }
  *n_items = ctx->lastItems;
  return FSMC_OK;
}

int fsmc_ctx_last_segment_sums_in_lds(const fsmc_ctx* ctx, int32_t* in_lds)
{
  if (!ctx || !in_lds) {
    return FSMC_EINVAL;
  }
  *in_lds = ctx->lastSpsLds ? 1 : 0;
  return FSMC_OK;
}

int fsmc_decode_ibd_launch(fsmc_ctx* ctx, const fsmc_model* m, uint32_t flags)
{
  FSMC_TRY(checkReady(ctx, m));
  FSMC_HIP(ctx, hipSetDevice(ctx->device));
  const bool track = (flags & (FSMC_WANT_MEAN | FSMC_WANT_MAP)) != 0;
  earnWorkspace(ctx, m, kModeIbd);
  // The queues.  Two half-groups per wave for the half-full groups that pair up
  // (decode_kernel<..., DUAL>, with beta stride 2 where that is built); the other groups one per wave, in a kernel that
  // runs beside it.
  KernelChoice kDual;
  const bool pairing = ctx->pairing != 0 && !m->sequence && familyMember(m) > 0;
  if (pairing) {
    kDual = chooseKernel(m, kModeIbd, track, true, ctx->betaStride);
  }
  fsmc_ctx::IbdQueues& q = ctx->q;
  if (!q.valid || q.serial != ctx->worklistSerial || q.pairing != pairing) {
    q.valid = false;
    q.items.clear();
    q.unions.clear();
    q.rest.clear();
    q.dual = pairing && plan::buildDualItems(ctx->hGroups, q.items, q.unions, q.rest);
    // (if every group rides in the paired kernel there is no second kernel to share the workspace with)
    q.alone = q.dual && q.rest.empty();
    if (!q.dual) {
      q.items.clear();
      q.unions.clear();
      q.rest = ctx->hGroups;
    }
    q.reordered = plan::longestFirst(q.rest) || q.dual;
    if (q.dual) {
      FSMC_TRY(upload(ctx, &ctx->dItems, q.items.data(), q.items.size()));
    }
    if (q.reordered && !q.rest.empty()) {
      FSMC_TRY(upload(ctx, &ctx->dRest, q.rest.data(), q.rest.size()));
    }
    q.serial = ctx->worklistSerial;
    q.pairing = pairing;
    q.valid = true;
  }
  const bool haveRest = !q.rest.empty();
  const bool beside = q.dual && haveRest;
  LaunchPlan planDual, plan;
  if (q.dual) {
    FSMC_TRY(planAndHold(ctx, m, kModeIbd, kDual, q.unions, true, q.alone ? 1 : 2, ctx->ws, planDual));
  }
  const KernelChoice k = chooseKernel(m, kModeIbd, track, false, ctx->betaStride);
  if (haveRest) {
    FSMC_TRY(planAndHold(ctx, m, kModeIbd, k, q.reordered ? q.rest : ctx->hGroups, false, beside ? 2 : 1,
                         beside ? ctx->wsSide : ctx->ws, plan));
  }
  // The getters describe the one-group-per-wave kernel (member, stride; also when every group rides in the paired
  // kernel) and its plan -- the paired kernel's plan where there is no other -- with the workgroups of both kernels.
  recordLaunch(ctx, k, haveRest ? plan : planDual, beside ? planDual.slots : 0);
  ctx->lastItems = q.dual ? (int)q.unions.size() : 0;
  if (ctx->recCap == 0) {
    ctx->recCap = std::max<size_t>(1u << 16, 8 * ctx->nPairs);
  }
  FSMC_TRY(ensure(ctx, ctx->recs, ctx->recCap * sizeof(fsmc_ibd_record)));
  KParams pDual, p;
  if (q.dual) {
    fillParams(ctx, m, planDual, flags, pDual);
    pDual.groups = ctx->dItems;
    pDual.nGroups = (int)q.unions.size();
  }
  if (haveRest) {
    fillParams(ctx, m, plan, flags, p);
    if (q.reordered) {
      p.groups = ctx->dRest;
      p.nGroups = (int)q.rest.size();
    }
    if (beside) {
      p.ws = (float4*)ctx->wsSide.p;
    }
  }
  // A launch smaller than the chip (one group per wave, segment ages wanted): where every wave of it still finds room, the
  // open segments' per-state sums live in LDS instead of the workspace (fsmc_kernels.h, KParams::spsLds) -- K4 KiB of
  // dynamic LDS a wave.  (A wave alone on its SIMD waits out every round trip of those sums to L2: C1 shape 40.6 -> 3x ms.)
  size_t spsLdsBytes = 0;
  if (!beside && !q.dual && track && !waveGroups(kModeIbd, m) && !anyStates(m) && !m->sequence) {
    const size_t dyn = (size_t)(k.member + 3) / 4 * kWave * sizeof(float4);
    hipFuncAttributes fa;
    FSMC_HIP(ctx, hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(k.fn)));
    const size_t perWave = fa.sharedSizeBytes + dyn;
    constexpr size_t kLdsPerCU = 160u << 10, kLdsPerWorkgroup = 64u << 10;
    if (perWave <= kLdsPerWorkgroup && (size_t)plan.slots * perWave <= (size_t)ctx->nCU * kLdsPerCU &&
        (size_t)plan.slots <= (size_t)ctx->nCU * (kLdsPerCU / perWave) && !std::getenv("FSMC_DIAG_NO_SPS_LDS")) {
      spsLdsBytes = dyn;
      p.spsLds = 1u;
    }
  }
  ctx->lastSpsLds = spsLdsBytes != 0;
  FSMC_TRY(beside ? launchBeside(ctx, k, p, plan.slots, plan, kDual, pDual, planDual.slots)
                  : q.dual ? launch(ctx, kDual, pDual, planDual.slots)
                           : launch(ctx, k, p, plan.slots, spsLdsBytes, false, &plan));
  ctx->ibdModel = m;
  ctx->ibdFlags = flags;
  ctx->ibdPending = true;
  return FSMC_OK;
}

int fsmc_identify(fsmc_ctx* ctx, const uint64_t* words, uint32_t n_haps, uint32_t n_words, const uint32_t* global_ids,
                  const fsmc_job_window* job, const float* gen_pos, uint32_t n_sites, int32_t gap, float skip,
                  float min_m, fsmc_candidate* out, size_t cap, size_t* n_out)
{
  const fsmc_identify_opts defaults = {64u, 1u, 0, 10u}; // DecodingParams.hpp: hashingWordSize, haploid, max_seeds,
                                                         // constReadAhead
  return fsmc_identify_ex(ctx, words, n_haps, n_words, global_ids, job, gen_pos, n_sites, gap, skip, min_m, &defaults,
                          out, cap, n_out);
}

int fsmc_identify_ex(fsmc_ctx* ctx, const uint64_t* words, uint32_t n_haps, uint32_t n_words,
                     const uint32_t* global_ids, const fsmc_job_window* job, const float* gen_pos, uint32_t n_sites,
                     int32_t gap, float skip, float min_m, const fsmc_identify_opts* opts, fsmc_candidate* out,
                     size_t cap, size_t* n_out)
{
  if (!ctx) {
    return FSMC_EINVAL;
  }
  if (!opts) {
    return fail(ctx, FSMC_EINVAL, "fsmc_identify: opts is null");
  }
  if (opts->word_size < 1 || opts->word_size > 64) {
    return fail(ctx, FSMC_EINVAL, "fsmc_identify: word_size must be 1..64 (a word is one 64-bit integer)");
  }
  const bool splitSeeds = opts->max_seeds > 0; // (SeedHash.hpp:75 compares as unsigned long: a negative one never splits)
  if (splitSeeds && (opts->read_ahead < 1 || opts->read_ahead > 32)) {
    return fail(ctx, FSMC_EINVAL, "fsmc_identify: read_ahead must be 1..32 when max_seeds is set");
  }
  if (!opts->haploid && (n_haps & 1u)) {
    return fail(ctx, FSMC_EINVAL, "fsmc_identify: haploid = 0 pairs rows 2k, 2k+1 -- n_haps must be even");
  }
  if (!n_out) {
    return fail(ctx, FSMC_EINVAL, "fsmc_identify: n_out is null");
  }
  *n_out = 0;
  if (n_haps < 2 || n_words == 0) {
    return FSMC_OK; // no pair, or no complete word (FastSMC.cpp:186-195 hashes complete words only)
  }
  if (!words || !global_ids || !job || !gen_pos || (cap && !out)) {
    return fail(ctx, FSMC_EINVAL, "fsmc_identify: null argument");
  }
  if ((uint64_t)n_words * opts->word_size > n_sites) {
    return fail(ctx, FSMC_EINVAL, "fsmc_identify: n_words * word_size exceeds n_sites");
  }
  if (gap < 0 || cap > 0xFFFFFFFFull) {
    return fail(ctx, FSMC_EINVAL, "fsmc_identify: gap < 0 or cap beyond 2^32");
  }
  int fill = -1;
  FSMC_TRY(scratchFill(ctx, fill));
  FSMC_HIP(ctx, hipSetDevice(ctx->device));
  const unsigned tiles = (n_haps + kIdTile - 1) / kIdTile;
  const unsigned chunks = (n_words + kIdChunk - 1) / kIdChunk;
  // device buffers of this call (one call per job: no caching)
  struct Bufs {
    void* p[8] = {};
    ~Bufs()
    {
      for (void* q : p) {
        if (q) {
          (void)hipFree(q);
        }
      }
    }
  } b;
  const size_t bytes[8] = {(size_t)n_haps * n_words * sizeof(uint64_t),
                           (size_t)n_haps * sizeof(uint32_t),
                           (size_t)n_sites * sizeof(float),
                           (size_t)chunks * tiles * kIdTile * sizeof(unsigned),
                           (size_t)chunks * sizeof(unsigned),
                           std::max<size_t>(cap, 1) * sizeof(fsmc_candidate),
                           sizeof(unsigned),
                           splitSeeds ? (size_t)chunks * kIdChunk * tiles * kIdTile : 16};
  for (int i = 0; i < 8; ++i) {
    const hipError_t e = hipMalloc(&b.p[i], bytes[i]);
    if (e != hipSuccess) {
      b.p[i] = nullptr;
      return fail(ctx, FSMC_ENOMEM, std::string("fsmc_identify: hipMalloc failed: ") + hipGetErrorString(e));
    }
  }
  // (FSMC_DIAG_SCRATCH_FILL: buffers 3 to 7 are scratch, 0 to 2 the call's inputs)
  for (int i = 3; fill >= 0 && i < 8; ++i) {
    FSMC_HIP(ctx, hipMemsetAsync(b.p[i], fill, bytes[i], ctx->stream));
    ctx->scratchFilled += bytes[i];
  }
  FSMC_HIP(ctx, hipMemcpyAsync(b.p[0], words, bytes[0], hipMemcpyHostToDevice, ctx->stream));
  FSMC_HIP(ctx, hipMemcpyAsync(b.p[1], global_ids, bytes[1], hipMemcpyHostToDevice, ctx->stream));
  FSMC_HIP(ctx, hipMemcpyAsync(b.p[2], gen_pos, bytes[2], hipMemcpyHostToDevice, ctx->stream));
  FSMC_HIP(ctx, hipMemsetAsync(b.p[3], 0, bytes[3], ctx->stream));
  FSMC_HIP(ctx, hipMemsetAsync(b.p[6], 0, bytes[6], ctx->stream));
  IdParams p;
  p.words = (const unsigned long long*)b.p[0];
  p.nHaps = n_haps;
  p.nWords = n_words;
  p.globalId = (const unsigned*)b.p[1];
  p.job = *job;
  p.gen = (const float*)b.p[2];
  p.nSites = n_sites;
  // An interval is reported before the end only when end < cur - gap with 0 <= end and cur < n_words: never for
  // gap >= n_words, so every such gap is the same as gap = n_words.  Clamped, end + gap + 1 (the word at which an
  // interval runs out, id_match_kernel) stays far from INT_MAX and flush_word never exceeds n_words, the bound
  // idSortCandidates sizes its keys by.
  p.gap = (int)std::min<uint32_t>((uint32_t)gap, n_words);
  p.skip = skip;
  p.minM = min_m;
  p.dupBits = (unsigned*)b.p[3];
  p.hapStride = tiles * kIdTile;
  p.usedBits = (unsigned*)b.p[4];
  p.out = (fsmc_candidate*)b.p[5];
  p.cap = (unsigned)cap;
  p.count = (unsigned*)b.p[6];
  p.wordSize = opts->word_size;
  p.depth = splitSeeds ? (const unsigned char*)b.p[7] : nullptr;
  // id_match_kernel is the default case (haplotype pairs, whole seeds); the other settings take the general kernel
  const bool general = splitSeeds || !opts->haploid;
  const bool haploid = opts->haploid != 0;
  auto launchMatch = [&]() {
    if (!general) {
      hipLaunchKernelGGL(id_match_kernel, dim3(tiles, tiles), dim3(kIdThreads), 0, ctx->stream, p);
    } else if (haploid) {
      hipLaunchKernelGGL(id_match_general_kernel<true>, dim3(tiles, tiles), dim3(kIdThreads), 0, ctx->stream, p);
    } else {
      hipLaunchKernelGGL(id_match_general_kernel<false>, dim3(tiles, tiles), dim3(kIdThreads), 0, ctx->stream, p);
    }
    return hipGetLastError();
  };
  FSMC_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  if (splitSeeds) {
    FSMC_HIP(ctx, hipMemsetAsync(b.p[7], 0, bytes[7], ctx->stream));
    const hipError_t e = idSeedDepths(ctx->stream, p.words, n_haps, n_words, (unsigned)opts->max_seeds, opts->read_ahead,
                                      (unsigned char*)b.p[7], p.hapStride);
    if (e != hipSuccess) {
      return fail(ctx, e == hipErrorOutOfMemory ? FSMC_ENOMEM : FSMC_EHIP,
                  std::string("fsmc_identify: splitting the seeds failed: ") + hipGetErrorString(e));
    }
  }
  hipLaunchKernelGGL(id_dup_kernel, dim3(tiles, tiles), dim3(kIdThreads), 0, ctx->stream, p);
  FSMC_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(id_complexity_kernel, dim3(chunks), dim3(kIdThreads), 0, ctx->stream, p);
  FSMC_HIP(ctx, hipGetLastError());
  FSMC_HIP(ctx, launchMatch());
  FSMC_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  ctx->timed = true;
  unsigned count = 0;
  FSMC_HIP(ctx, hipMemcpyAsync(&count, b.p[6], sizeof(count), hipMemcpyDeviceToHost, ctx->stream));
  FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *n_out = count;
  ctx->idStashCount = 0;
  if (count > cap) {
    // The caller's buffer is too small -- the normal case of a first call, nobody knows the count beforehand.  Only the
    // last pass depends on the buffer: run it again into one of the right size (the duplicate and complexity bits are
    // still there), order the records and keep them on the device for fsmc_identify_fetch, so that the caller does not
    // pay the uploads and the two other passes twice.
    void* full = nullptr;
    hipError_t e = hipMalloc(&full, (size_t)count * sizeof(fsmc_candidate));
    if (e == hipSuccess) {
      p.out = (fsmc_candidate*)full;
      p.cap = count;
      e = hipMemsetAsync(b.p[6], 0, bytes[6], ctx->stream);
      if (e == hipSuccess) {
        e = launchMatch();
      }
      if (e == hipSuccess && ensure(ctx, ctx->idStash, (size_t)count * sizeof(fsmc_candidate)) == FSMC_OK) {
        e = idSortCandidates(ctx->stream, (const fsmc_candidate*)full, (fsmc_candidate*)ctx->idStash.p, count, n_haps,
                             n_words);
        if (e == hipSuccess) {
          e = hipStreamSynchronize(ctx->stream);
        }
        if (e == hipSuccess) {
          ctx->idStashCount = count;
        }
      }
      (void)hipFree(full);
    }
    if (ctx->idStashCount == 0) {
      // the second run did not go through (e.g. no memory for the full list): nothing is kept, the caller calls again
      // with a buffer of *n_out records -- and must not find this failure's error state in front of that call's checks
      (void)hipGetLastError();
    }
    return fail(ctx, FSMC_EOVERFLOW, "fsmc_identify: candidate buffer too small");
  }
  if (count) {
    // the emission order: by the word at which the reference's ExtendHash reports a match, then by pair key (the
    // appends of the workgroups arrive in no particular order) -- sorted on the device, fsmc_identify_sort.hip
    void* sorted = nullptr;
    hipError_t e = hipMalloc(&sorted, (size_t)count * sizeof(fsmc_candidate));
    if (e != hipSuccess) {
      return fail(ctx, FSMC_ENOMEM, std::string("fsmc_identify: hipMalloc failed: ") + hipGetErrorString(e));
    }
    e = idSortCandidates(ctx->stream, (const fsmc_candidate*)b.p[5], (fsmc_candidate*)sorted, count, n_haps, n_words);
    if (e == hipSuccess) {
      e = hipMemcpy(out, sorted, (size_t)count * sizeof(fsmc_candidate), hipMemcpyDeviceToHost);
    }
    (void)hipFree(sorted);
    if (e != hipSuccess) {
      return fail(ctx, FSMC_EHIP, std::string("fsmc_identify: ordering the candidates failed: ") + hipGetErrorString(e));
    }
  }
  return FSMC_OK;
}

int fsmc_identify_fetch(fsmc_ctx* ctx, fsmc_candidate* out, size_t cap, size_t* n_out)
{
  if (!ctx || !n_out) {
    return fail(ctx, FSMC_EINVAL, "fsmc_identify_fetch: null argument");
  }
  *n_out = ctx->idStashCount;
  if (ctx->idStashCount == 0) {
    return fail(ctx, FSMC_ESTATE, "fsmc_identify_fetch: no candidate list is kept (it follows an fsmc_identify that "
                                  "returned FSMC_EOVERFLOW)");
  }
  if (cap < ctx->idStashCount || !out) {
    return fail(ctx, FSMC_EOVERFLOW, "fsmc_identify_fetch: candidate buffer too small");
  }
  FSMC_HIP(ctx, hipSetDevice(ctx->device));
  FSMC_HIP(ctx, hipMemcpy(out, ctx->idStash.p, ctx->idStashCount * sizeof(fsmc_candidate), hipMemcpyDeviceToHost));
  ctx->idStashCount = 0;
  (void)hipFree(ctx->idStash.p);
  ctx->idStash = DevBuf{};
  return FSMC_OK;
}

int fsmc_sync(fsmc_ctx* ctx)
{
  if (!ctx) {
    return FSMC_EINVAL;
  }
  FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return FSMC_OK;
}

int fsmc_last_kernel_ms(fsmc_ctx* ctx, float* ms)
{
  if (!ctx || !ms) {
    return FSMC_EINVAL;
  }
  if (!ctx->timed) {
    return fail(ctx, FSMC_ESTATE, "no launch has been timed yet");
  }
  FSMC_HIP(ctx, hipEventSynchronize(ctx->ev1));
  FSMC_HIP(ctx, hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
  return FSMC_OK;
}

int fsmc_phase_cycles(fsmc_ctx* ctx, uint64_t* out, size_t n)
{
  if (!ctx || !out || n > (size_t)kPhaseSlots) {
    return fail(ctx, FSMC_EINVAL, "bad argument");
  }
  FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  FSMC_HIP(ctx, hipMemcpy(out, ctx->dPhase, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  FSMC_HIP(ctx, hipMemset(ctx->dPhase, 0, kPhaseSlots * sizeof(unsigned long long)));
  return FSMC_OK;
}

int fsmc_decode_ibd_fetch(fsmc_ctx* ctx, fsmc_ibd_record* out, size_t cap, size_t* n_out)
{
  if (!ctx || !n_out) {
    return fail(ctx, FSMC_EINVAL, "null argument");
  }
  if (!ctx->ibdPending || !ctx->ibdModel) {
    return fail(ctx, FSMC_ESTATE, "no IBD decode in flight");
  }
  FSMC_HIP(ctx, hipSetDevice(ctx->device));
  unsigned counters[4] = {0, 0, 0, 0};
  for (int attempt = 0; attempt < 3; ++attempt) {
    FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    FSMC_HIP(ctx, hipMemcpy(counters, ctx->dCounters, sizeof(counters), hipMemcpyDeviceToHost));
    if (counters[1] <= ctx->recCap) {
      break;
    }
    // the device buffer was too small: grow it and decode again (results are deterministic)
    ctx->recCap = (size_t)counters[1] + (size_t)counters[1] / 8 + 1024;
    FSMC_TRY(fsmc_decode_ibd_launch(ctx, ctx->ibdModel, ctx->ibdFlags));
  }
  const size_t n = counters[1];
  if (n > ctx->recCap) {
    return fail(ctx, FSMC_EHIP, "record buffer still too small after regrowing");
  }
  *n_out = n;
  if (n > cap || (n && !out)) {
    return fail(ctx, FSMC_EOVERFLOW, "output buffer holds " + std::to_string(cap) + " records, need " +
                                         std::to_string(n));
  }
  if (n) {
    FSMC_HIP(ctx, hipMemcpy(out, ctx->recs.p, n * sizeof(fsmc_ibd_record), hipMemcpyDeviceToHost));
    // the reference writes batch by batch, pair by pair, site by site (HMM.cpp:1181,1206)
    std::sort(out, out + n, [](const fsmc_ibd_record& x, const fsmc_ibd_record& y) {
      return x.pair != y.pair ? x.pair < y.pair : x.start < y.start;
    });
  }
  return FSMC_OK;
}

int fsmc_decode_ibd(fsmc_ctx* ctx, const fsmc_model* m, const fsmc_pair* pairs, size_t n_pairs,
                    const fsmc_group* groups, size_t n_groups, uint32_t flags, fsmc_ibd_record* out, size_t cap,
                    size_t* n_out)
{
  int rc = fsmc_worklist_upload(ctx, pairs, n_pairs, groups, n_groups);
  if (rc == FSMC_OK) {
    rc = fsmc_decode_ibd_launch(ctx, m, flags);
  }
  if (rc == FSMC_OK) {
    rc = fsmc_decode_ibd_fetch(ctx, out, cap, n_out);
  }
  return rc;
}

int fsmc_decode_posteriors(fsmc_ctx* ctx, const fsmc_model* m, float* out, size_t out_floats)
{
  FSMC_TRY(checkReady(ctx, m));
  if (!out) {
    return fail(ctx, FSMC_EINVAL, "out is null");
  }
  FSMC_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<size_t> offsets(ctx->nGroups);
  size_t total = 0;
  for (size_t g = 0; g < ctx->nGroups; ++g) {
    offsets[g] = total;
    total += (size_t)kWave * m->K * (ctx->hGroups[g].to - ctx->hGroups[g].from);
  }
  if (total > out_floats) {
    return fail(ctx, FSMC_EOVERFLOW, "posterior dump needs " + std::to_string(total) + " floats");
  }
  LaunchPlan plan;
  FSMC_TRY(prepareDecode(ctx, m, kModeDump, ctx->betaStride, ctx->hGroups, ctx->nGroups, 0, plan));
  FSMC_TRY(ensure(ctx, ctx->aux, offsets.size() * sizeof(size_t)));
  FSMC_TRY(ensure(ctx, ctx->out, total * sizeof(float)));
  FSMC_HIP(ctx, hipMemcpyAsync(ctx->aux.p, offsets.data(), offsets.size() * sizeof(size_t), hipMemcpyHostToDevice,
                               ctx->stream));
  KParams p;
  fillParams(ctx, m, plan, 0, p);
  p.dumpOut = (float*)ctx->out.p;
  p.dumpOffsets = (const size_t*)ctx->aux.p;
  FSMC_TRY(launch(ctx, plan.k, p, plan.slots));
  FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  FSMC_HIP(ctx, hipMemcpy(out, ctx->out.p, total * sizeof(float), hipMemcpyDeviceToHost));
  return FSMC_OK;
}

int fsmc_decode_per_pair(fsmc_ctx* ctx, const fsmc_model* m, const float* exp_coal_times, float* mean, int32_t* map)
{
  FSMC_TRY(checkReady(ctx, m));
  if (!exp_coal_times || (!mean && !map)) {
    return fail(ctx, FSMC_EINVAL, "need expected coalescence times and at least one output");
  }
  FSMC_HIP(ctx, hipSetDevice(ctx->device));
  LaunchPlan plan;
  FSMC_TRY(prepareDecode(ctx, m, kModePerPair, ctx->betaStride, ctx->hGroups, ctx->nGroups, 0, plan));
  const size_t n = ctx->nPairs * (size_t)m->S;
  const size_t coalBytes = (size_t)m->KP * sizeof(float);
  // layout of the staging buffer: [expCoal KP floats][mean n floats][map n ints]
  FSMC_TRY(ensure(ctx, ctx->out, coalBytes + n * (sizeof(float) + sizeof(int32_t))));
  char* base = (char*)ctx->out.p;
  std::vector<float> coal;
  FSMC_TRY(uploadExpCoal(ctx, m, exp_coal_times, base, coal));
  FSMC_HIP(ctx, hipMemsetAsync(base + coalBytes, 0, n * (sizeof(float) + sizeof(int32_t)), ctx->stream));
  KParams p;
  fillParams(ctx, m, plan, 0, p);
  p.expCoal = (const float*)base;
  p.ppMean = mean ? (float*)(base + coalBytes) : nullptr;
  p.ppMap = map ? (int*)(base + coalBytes + n * sizeof(float)) : nullptr;
  FSMC_TRY(launch(ctx, plan.k, p, plan.slots));
  FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (mean) {
    FSMC_HIP(ctx, hipMemcpy(mean, p.ppMean, n * sizeof(float), hipMemcpyDeviceToHost));
  }
  if (map) {
    FSMC_HIP(ctx, hipMemcpy(map, p.ppMap, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  return FSMC_OK;
}

// The fsmc_decode_pair_* entry points below share one flow.  The work list goes through the device in slices of groups
// (planSlices): the consumers of the decode kernel write a slice into ppStage -- the dump (dumpSetup) or the mean / MAP
// rows (perPairSetup) -- the entry point's own kernels reduce it, and what is left of the slice goes to the caller before
// the next slice overwrites it.  Rows leave through drainRows while the next slice decodes (decodeSlicesDrained); small
// outputs by a blocking copy (sliceToCaller).  The entry points that launch a sweep kernel instead of the decode
// (kNoDecode) take the kernel from sweepKernelFor; the three that need a workspace plan it with planSweepAndHold, fill the
// kernel's argument with plannedSweepParams, launch a slice with launchSweepSlice and send its rows, one span of the
// caller's array, through drainSpan before the next launch.  What several entry points reduce a slice with is set up
// once: the bin edges (uploadBinEdges), the grid of the bin kernels (binBlocks), pair_cdf_kernel (cdfParams, launchCdf).
// The stream is synchronised after the small uploads, whose sources are locals or the caller's arrays, and at the end;
// the slice count of the call is recorded only then, on success.

// writePerPairOutput's posterior tables (HMM.cpp:1378-1392): pair_posteriors_kernel turns a slice's dump into rows,
// [pair][K][S], and continues the sum over pairs.
int fsmc_decode_pair_posteriors(fsmc_ctx* ctx, const fsmc_model* m, const float* exp_coal_times,
                                float* const* post_rows, float* sum)
{
  FSMC_TRY(checkReady(ctx, m));
  if (!exp_coal_times || (!post_rows && !sum)) {
    return fail(ctx, FSMC_EINVAL, "need expected coalescence times and at least one output (rows or sum)");
  }
  FSMC_TRY(checkWholeSequence(ctx, m, "per-pair posteriors"));
  if (post_rows) {
    for (size_t i = 0; i < ctx->nPairs; ++i) {
      if (!post_rows[i]) {
        return fail(ctx, FSMC_EINVAL, "post_rows[" + std::to_string(i) + "] is null");
      }
    }
  }
  const size_t K = (size_t)m->K, S = (size_t)m->S;
  const size_t plane = K * S;                      // floats of one pair's table, and of the sum
  const bool wantRows = post_rows != nullptr;
  WorkSlices ws;
  FSMC_TRY(planSlices(ctx, m, kModeDump, kSlicePosteriors, ctx->ppStage.bytes + ctx->ppRows.bytes,
                      layout::posteriorsGroupBytes(K, S, wantRows), ws));
  const layout::Posteriors L = layout::posteriors(K, S, wantRows, ws.slice, ws.slicePairsMax);
  FSMC_TRY(ensure(ctx, ctx->aux, ws.slice * sizeof(size_t)));
  FSMC_TRY(ensure(ctx, ctx->ppStage, L.stageBytes));
  FSMC_TRY(ensure(ctx, ctx->ppAcc, L.accBytes));
  if (wantRows) {
    FSMC_TRY(ensure(ctx, ctx->ppRows, L.rowsBytes));
  }
  // The way out for the rows: whole pairs a copy -- what a pinned buffer holds, one pair's table at least.
  const size_t rowBytes = L.rowBytes;
  const size_t pairsPerCopy = std::max<size_t>(1, std::min<size_t>(rowCopyBytes() / rowBytes, ws.slicePairsMax));
  if (wantRows) {
    FSMC_TRY(ensureRowCopies(ctx, pairsPerCopy * rowBytes));
  }

  char* const acc = (char*)ctx->ppAcc.p;
  float* const dCoal = (float*)(acc + L.offCoal);
  float* const dSum = (float*)(acc + L.offSum);
  KParams p;
  FSMC_TRY(dumpSetup(ctx, m, ws, p));
  FSMC_HIP(ctx, hipMemcpyAsync(dCoal, exp_coal_times, K * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if (sum) {
    FSMC_HIP(ctx, hipMemcpyAsync(dSum, sum, rowBytes, hipMemcpyHostToDevice, ctx->stream)); // (the sum is one table)
  }
  FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));

  PairPostParams q;
  q.stage = (const float*)ctx->ppStage.p;
  q.K = m->K;
  q.S = m->S;
  q.expCoal = dCoal;
  q.rows = wantRows ? (float*)ctx->ppRows.p : nullptr;
  q.sum = sum ? dSum : nullptr;
  const dim3 grid((unsigned)((S + kWave - 1) / kWave), (unsigned)K);
  auto reduce = [&](size_t sl) -> int {
    q.groups = ctx->dGroups + ws.firstGroup(sl);
    q.nGroups = (int)ws.groups(sl);
    q.firstPair = (unsigned)ws.firstPair(sl);
    hipLaunchKernelGGL(pair_posteriors_kernel, grid, dim3(kWave), 0, ctx->stream, q);
    FSMC_HIP(ctx, hipGetLastError());
    return FSMC_OK;
  };
  // the slice's pairs are the rows of ppRows from its start on: runs of whole pairs, scattered to the caller's rows
  auto drain = [&](size_t sl) -> int {
    const size_t lo = ws.firstPair(sl), n = ws.pairs(sl);
    auto run = [&](size_t c) { return std::min(pairsPerCopy, n - c * pairsPerCopy); };
    return drainRows(
        ctx, (n + pairsPerCopy - 1) / pairsPerCopy,
        [&](size_t c) { return RowChunk{(const float*)ctx->ppRows.p + c * pairsPerCopy * plane, run(c) * rowBytes}; },
        [&](size_t c, const char* host) {
          for (size_t i = 0; i < run(c); ++i) {
            std::memcpy(post_rows[lo + c * pairsPerCopy + i], host + i * rowBytes, rowBytes);
          }
        });
  };
  FSMC_TRY(decodeSlicesDrained(ctx, ws, p, wantRows, reduce, drain));
  FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (sum) {
    FSMC_HIP(ctx, hipMemcpy(sum, dSum, rowBytes, hipMemcpyDeviceToHost));
  }
  ctx->pairSlices[kSlicePosteriors].last = (int)ws.nSlices;
  return FSMC_OK;
}

// finaliseCalculations' column-wise min / first argmin of the per-pair means and MAPs (hmm.cpp:151-184) without the
// rows: pair_minima_kernel reduces a slice's rows range by range, pair_minima_combine_kernel continues the chain in the
// device copy of the state (fsmc_pair_minima.h).
int fsmc_decode_pair_minima(fsmc_ctx* ctx, const fsmc_model* m, const float* exp_coal_times, uint64_t pair_base,
                            float* min_mean, int32_t* argmin_mean, int32_t* min_map, int32_t* argmin_map)
{
  FSMC_TRY(checkReady(ctx, m));
  const bool wantMean = min_mean || argmin_mean, wantMap = min_map || argmin_map;
  if (!exp_coal_times || (!wantMean && !wantMap)) {
    return fail(ctx, FSMC_EINVAL, "need expected coalescence times and at least one output (mean or MAP minima)");
  }
  if ((wantMean && !(min_mean && argmin_mean)) || (wantMap && !(min_map && argmin_map))) {
    return fail(ctx, FSMC_EINVAL, "a minimum and its argmin come together");
  }
  FSMC_TRY(checkWholeSequence(ctx, m, "per-pair minima"));
  if (pair_base > (uint64_t)INT32_MAX || pair_base + (uint64_t)ctx->nPairs > (uint64_t)INT32_MAX) {
    return fail(ctx, FSMC_EINVAL, "pair_base + pairs of the work list exceeds the range of the int32 argmin");
  }
  const size_t S = (size_t)m->S;
  const int nOut = (wantMean ? 1 : 0) + (wantMap ? 1 : 0);
  WorkSlices ws;
  FSMC_TRY(planSlices(ctx, m, kModePerPair, kSliceMinima, ctx->ppStage.bytes, layout::minimaGroupBytes(S, (size_t)nOut),
                      ws));
  // the buffers and the ranges a slice is reduced in (a wave owns 64 sites of one range)
  const layout::Minima L = layout::minima(ctx->nCU, S, (size_t)m->KP, (size_t)nOut, ws.slicePairsMax, readDiag());
  if (L.tooManyRanges) {
    return fail(ctx, FSMC_EINVAL, "too many ranges for one launch (FSMC_DIAG_MINIMA_RANGE)");
  }
  const size_t siteBlocks = L.siteBlocks, rangeLen = L.rangeLen, vec = L.vec;

  FSMC_TRY(ensure(ctx, ctx->ppStage, L.stageBytes));
  FSMC_TRY(ensure(ctx, ctx->pmAcc, L.accBytes));
  char* const acc = (char*)ctx->pmAcc.p;
  KParams p;
  FSMC_TRY(perPairSetup(ctx, m, exp_coal_times, acc + L.offCoal, wantMean, wantMap, ws, p));
  void* const dState[4] = {acc + L.offState[0], acc + L.offState[1], acc + L.offState[2], acc + L.offState[3]};
  void* const hState[4] = {min_mean, argmin_mean, min_map, argmin_map};
  if (pair_base > 0) { // the chain continues: the caller's arrays are its state
    for (int i = 0; i < 4; ++i) {
      if (hState[i]) {
        FSMC_HIP(ctx, hipMemcpyAsync(dState[i], hState[i], vec, hipMemcpyHostToDevice, ctx->stream));
      }
    }
  }
  FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));

  PairMinimaParams q;
  q.mean = ws.stageMean;
  q.map = ws.stageMap;
  q.S = m->S;
  q.rangeLen = (int)rangeLen;
  q.partMinMean = (float*)(acc + L.offParts[0]);
  q.partArgMean = (int*)(acc + L.offParts[1]);
  q.partMinMap = (int*)(acc + L.offParts[2]);
  q.partArgMap = (int*)(acc + L.offParts[3]);
  q.minMean = (float*)dState[0];
  q.argMean = (int*)dState[1];
  q.minMap = (int*)dState[2];
  q.argMap = (int*)dState[3];

  for (size_t sl = 0; sl < ws.nSlices; ++sl) {
    FSMC_TRY(launchSlice(ctx, ws, sl, p));
    const size_t n = ws.pairs(sl);
    q.n = (int)n;
    q.nRanges = (int)((n + rangeLen - 1) / rangeLen);
    q.seeded = (pair_base == 0 && sl == 0) ? 1 : 0;
    q.firstIndex = (int)(pair_base + ws.firstPair(sl));
    hipLaunchKernelGGL(pair_minima_kernel, dim3((unsigned)((size_t)q.nRanges * siteBlocks)), dim3(kWave), 0, ctx->stream,
                       q);
    FSMC_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(pair_minima_combine_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, ctx->stream, q);
    FSMC_HIP(ctx, hipGetLastError());
    FSMC_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream)); // (the call's timed span: every decode and every reduction)
  }
  FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < 4; ++i) {
    if (hState[i]) {
      FSMC_HIP(ctx, hipMemcpy(hState[i], dState[i], vec, hipMemcpyDeviceToHost));
    }
  }
  ctx->pairSlices[kSliceMinima].last = (int)ws.nSlices;
  return FSMC_OK;
}

// Per pair, the mean / min / argmin of the posterior-mean row and the min / argmin of the MAP row over bins of sites,
// without the rows leaving the device: pair_bins_kernel reduces a slice's rows cell by cell (fsmc_pair_bins.h), and the
// slice's [pairs][B] outputs are copied to the caller's arrays at the slice's first pair.  Slices are independent:
// nothing is carried.
int fsmc_decode_pair_bins(fsmc_ctx* ctx, const fsmc_model* m, const float* exp_coal_times, const int32_t* bin_edges,
                          size_t n_bins, float* bin_mean, float* bin_min_mean, int32_t* bin_argmin_mean,
                          int32_t* bin_min_map, int32_t* bin_argmin_map)
{
  FSMC_TRY(checkReady(ctx, m));
  const bool wantMean = bin_mean || bin_min_mean || bin_argmin_mean, wantMap = bin_min_map || bin_argmin_map;
  if (!exp_coal_times || !bin_edges || (!wantMean && !wantMap)) {
    return fail(ctx, FSMC_EINVAL, "need expected coalescence times, bin edges and at least one output");
  }
  if ((bin_min_mean != nullptr) != (bin_argmin_mean != nullptr) || (bin_min_map != nullptr) != (bin_argmin_map != nullptr)) {
    return fail(ctx, FSMC_EINVAL, "a minimum and its argmin come together");
  }
  FSMC_TRY(checkBinEdges(ctx, m, bin_edges, n_bins));
  FSMC_TRY(checkWholeSequence(ctx, m, "per-pair bins"));
  const size_t S = (size_t)m->S, B = n_bins;
  const int nRows = (wantMean ? 1 : 0) + (wantMap ? 1 : 0);
  void* const hOut[5] = {bin_mean, bin_min_mean, bin_argmin_mean, bin_min_map, bin_argmin_map};
  bool want[5];
  size_t nOut = 0;
  for (int i = 0; i < 5; ++i) {
    want[i] = hOut[i] != nullptr;
    nOut += want[i] ? 1 : 0;
  }
  WorkSlices ws;
  FSMC_TRY(planSlices(ctx, m, kModePerPair, kSliceBins, ctx->ppStage.bytes + ctx->pbAcc.bytes,
                      layout::binsGroupBytes(S, B, (size_t)nRows, nOut), ws));
  if (ws.slicePairsMax > (size_t)INT32_MAX) {
    return fail(ctx, FSMC_EINVAL, "too many pairs in one slice (fsmc_ctx_set_pair_bins_slice)");
  }

  const layout::Bins L = layout::bins(S, (size_t)m->KP, B, (size_t)nRows, want, ws.slicePairsMax);
  FSMC_TRY(ensure(ctx, ctx->ppStage, L.stageBytes));
  FSMC_TRY(ensure(ctx, ctx->pbAcc, L.accBytes));
  char* const acc = (char*)ctx->pbAcc.p;
  KParams p;
  FSMC_TRY(perPairSetup(ctx, m, exp_coal_times, acc + L.offCoal, wantMean, wantMap, ws, p));
  FSMC_TRY(uploadBinEdges(ctx, acc + L.offEdges, bin_edges, B));
  FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));

  void* dOut[5];
  for (int i = 0; i < 5; ++i) {
    dOut[i] = want[i] ? acc + L.offOut[i] : nullptr;
  }
  PairBinsParams q;
  q.mean = ws.stageMean;
  q.map = ws.stageMap;
  q.edges = (const int*)(acc + L.offEdges);
  q.S = m->S;
  q.B = (int)B;
  q.binMean = (float*)dOut[0];
  q.binMinMean = (float*)dOut[1];
  q.binArgMean = (int*)dOut[2];
  q.binMinMap = (int*)dOut[3];
  q.binArgMap = (int*)dOut[4];

  for (size_t sl = 0; sl < ws.nSlices; ++sl) {
    FSMC_TRY(launchSlice(ctx, ws, sl, p));
    const size_t n = ws.pairs(sl);
    q.n = (int)n;
    // (waves of the reduction: eight deep)
    hipLaunchKernelGGL(pair_bins_kernel, dim3(binBlocks(ctx, 8, 1, n * B)), dim3(kPairBinsThreads), 0, ctx->stream, q);
    FSMC_HIP(ctx, hipGetLastError());
    FSMC_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream)); // (the call's timed span: every decode and every reduction)
    // the slice's outputs go to the caller before the next slice overwrites them (20 bytes a cell at most against the
    // 552 bytes a pair-site of the decode: no second buffer, no overlap)
    FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 5; ++i) {
      FSMC_TRY(sliceToCaller(ctx, ws, sl, hOut[i], dOut[i], B * sizeof(float)));
    }
  }
  ctx->pairSlices[kSliceBins].last = (int)ws.nSlices;
  return FSMC_OK;
}

// Per pair, the likelihood of its observations as a mantissa / exponent pair, over the whole sequence and over bins of
// sites (fsmc_pair_loglik.h): the forward sweep alone, one launch of forward_kernel a slice -- no decode plan, no
// workspace.  The slice's values are copied to the caller's arrays at the slice's first pair; slices are independent.
int fsmc_decode_pair_loglik(fsmc_ctx* ctx, const fsmc_model* m, const int32_t* bin_edges, size_t n_bins, double* mant,
                            int32_t* expo, double* bin_mant, int32_t* bin_expo)
{
  FSMC_TRY(checkReady(ctx, m));
  if ((mant != nullptr) != (expo != nullptr) || (bin_mant != nullptr) != (bin_expo != nullptr)) {
    return fail(ctx, FSMC_EINVAL, "a mantissa and its exponent come together");
  }
  if (!mant && !bin_mant) {
    return fail(ctx, FSMC_EINVAL, "need at least one pair of outputs (mant / expo, bin_mant / bin_expo)");
  }
  if (bin_mant) {
    if (!bin_edges) {
      return fail(ctx, FSMC_EINVAL, "the bin outputs need bin edges");
    }
    FSMC_TRY(checkBinEdges(ctx, m, bin_edges, n_bins));
  }
  FSMC_TRY(checkWholeSequence(ctx, m, "per-pair log-likelihoods"));
  SweepKernel<FwdParams> kern;
  FSMC_TRY(sweepKernelFor(ctx, m, "per-pair log-likelihoods", "forward", true,
                          [&](auto kt) {
                            return m->sequence ? forward_kernel<decltype(kt)::value, true>
                                               : forward_kernel<decltype(kt)::value, false>;
                          },
                          kern));
  const size_t B = bin_mant ? n_bins : 0;
  WorkSlices ws;
  FSMC_TRY(planSlices(ctx, m, kNoDecode, kSliceLoglik, ctx->plAcc.bytes, layout::loglikGroupBytes(B), ws));
  int perCU = 0;
  const hipError_t eo = workgroupsPerCU(kern.k, 8, 1, perCU);
  if (eo != hipSuccess) {
    return fail(ctx, FSMC_EHIP, std::string("occupancy query of the forward kernel: ") + hipGetErrorString(eo));
  }
  LaunchPlan plan;
  plan.k = kern.k;
  plan.slots = (int)std::max<size_t>(1, std::min((size_t)ctx->nCU * (size_t)std::max(perCU, 1), ws.slice));

  // [mant][bin mant] doubles, [expo][bin expo] ints of the largest slice, then the edges
  const layout::Loglik L = layout::loglik(B, ws.slicePairsMax);
  FSMC_TRY(ensure(ctx, ctx->plAcc, L.accBytes));
  char* const acc = (char*)ctx->plAcc.p;
  if (B) {
    FSMC_TRY(uploadBinEdges(ctx, acc + L.offEdges, bin_edges, B));
    FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  FwdParams p;
  std::memset(&p, 0, sizeof(p));
  fillSweepParams(ctx, m, p);
  p.B = (int)B;
  p.rowGapF = m->rowGapF;
  p.edges = B ? (const int*)(acc + L.offEdges) : nullptr;
  p.mant = mant ? (double*)(acc + L.offMant) : nullptr;
  p.expo = mant ? (int*)(acc + L.offExpo) : nullptr;
  p.binMant = B ? (double*)(acc + L.offBinMant) : nullptr;
  p.binExpo = B ? (int*)(acc + L.offBinExpo) : nullptr;
  recordLaunch(ctx, kern.k, plan);

  for (size_t sl = 0; sl < ws.nSlices; ++sl) {
    FSMC_TRY(launchSweepSlice(ctx, ws, sl, kern, plan.slots, p));
    // the slice's values go to the caller before the next slice overwrites them (12 bytes a pair and output)
    FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    FSMC_TRY(sliceToCaller(ctx, ws, sl, mant, acc + L.offMant, sizeof(double)));
    FSMC_TRY(sliceToCaller(ctx, ws, sl, expo, acc + L.offExpo, sizeof(int32_t)));
    FSMC_TRY(sliceToCaller(ctx, ws, sl, bin_mant, acc + L.offBinMant, B * sizeof(double)));
    FSMC_TRY(sliceToCaller(ctx, ws, sl, bin_expo, acc + L.offBinExpo, B * sizeof(int32_t)));
  }
  ctx->pairSlices[kSliceLoglik].last = (int)ws.nSlices;
  return FSMC_OK;
}

// Per pair, the most probable joint state sequence and its probability (fsmc_pair_viterbi.h): one launch of
// viterbi_kernel a slice, planned by plan::planViterbi into the decode's workspace (planSweepAndHold).  A slice's state
// rows, [pair][S] bytes in ppRows, are one span of the caller's array: they leave through drainSpan; the mantissas and
// exponents by a blocking copy.  Slices are independent; a slice's rows have left before the next launch.
int fsmc_decode_pair_viterbi(fsmc_ctx* ctx, const fsmc_model* m, uint8_t* states, double* mant, int32_t* expo)
{
  FSMC_TRY(checkReady(ctx, m));
  if ((mant != nullptr) != (expo != nullptr)) {
    return fail(ctx, FSMC_EINVAL, "a mantissa and its exponent come together");
  }
  if (!states && !mant) {
    return fail(ctx, FSMC_EINVAL, "need at least one output (states, or mant and expo)");
  }
  FSMC_TRY(checkWholeSequence(ctx, m, "per-pair Viterbi paths"));
  SweepKernel<VitParams> kern;
  FSMC_TRY(sweepKernelFor(ctx, m, "per-pair Viterbi paths", "Viterbi", false,
                          [](auto kt) { return viterbi_kernel<decltype(kt)::value>; }, kern));
  const size_t S = (size_t)m->S;
  WorkSlices ws;
  FSMC_TRY(planSlices(ctx, m, kNoDecode, kSliceViterbi, ctx->ppRows.bytes + ctx->pvAcc.bytes,
                      layout::viterbiGroupBytes(S, states != nullptr, mant != nullptr), ws));
  const size_t n = ws.slicePairsMax;
  const layout::Viterbi L = layout::viterbi(S, states != nullptr, mant != nullptr, n);
  if (states) {
    FSMC_TRY(ensure(ctx, ctx->ppRows, L.rowsBytes));
  }
  if (mant) {
    FSMC_TRY(ensure(ctx, ctx->pvAcc, L.accBytes));
  }
  const size_t copyBytes = spanCopyBytes(n, S);
  if (states) {
    FSMC_TRY(ensureRowCopies(ctx, copyBytes));
  }
  LaunchPlan plan;
  FSMC_TRY(planSweepAndHold(
      ctx, m, kern.k, "Viterbi",
      [&](int perCU, const plan::WsBudget& budget, LaunchPlan& pl, std::string& why) {
        return plan::planViterbi(settingsOf(ctx), m->S, kern.k.member, perCU, ws.slice, states != nullptr, budget, pl,
                                 why);
      },
      plan));

  char* const acc = (char*)ctx->pvAcc.p;
  VitParams p;
  plannedSweepParams(ctx, m, plan, p);
  p.states = states ? (unsigned char*)ctx->ppRows.p : nullptr;
  p.mant = mant ? (double*)(acc + L.offMant) : nullptr;
  p.expo = mant ? (int*)(acc + L.offExpo) : nullptr;

  for (size_t sl = 0; sl < ws.nSlices; ++sl) {
    const size_t first = ws.firstPair(sl), nP = ws.pairs(sl);
    FSMC_TRY(launchSweepSlice(ctx, ws, sl, kern, plan.slots, p));
    if (states && nP > 0) {
      FSMC_HIP(ctx, hipEventRecord(ctx->evRows, ctx->stream));
      FSMC_TRY(drainSpan(ctx, ctx->ppRows.p, states + first * S, nP * S, copyBytes));
    }
    // the slice's values go to the caller before the next slice overwrites them
    FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    FSMC_TRY(sliceToCaller(ctx, ws, sl, mant, acc + L.offMant, sizeof(double)));
    FSMC_TRY(sliceToCaller(ctx, ws, sl, expo, acc + L.offExpo, sizeof(int32_t)));
  }
  ctx->pairSlices[kSliceViterbi].last = (int)ws.nSlices;
  return FSMC_OK;
}

// Per pair, n_samples state sequences drawn from the joint posterior (fsmc_pair_samples.h): one launch of sample_kernel
// a slice, planned by plan::planSamples into the decode's workspace (planSamplingSweep).  A slice's state rows,
// [pair][sample][S] bytes in ppRows, are one span of the caller's array and leave through drainSpan.  Slices are
// independent; a slice's rows have left before the next launch.
int fsmc_decode_pair_samples(fsmc_ctx* ctx, const fsmc_model* m, int32_t n_samples, uint64_t seed, uint8_t* states)
{
  FSMC_TRY(checkReady(ctx, m));
  if (n_samples < 1 || n_samples > kMaxSamples) {
    return fail(ctx, FSMC_EINVAL, "sampled paths: n_samples must be 1 ... 64 (" + std::to_string(n_samples) + ")");
  }
  if (!states) {
    return fail(ctx, FSMC_EINVAL, "sampled paths: states is null");
  }
  FSMC_TRY(checkWholeSequence(ctx, m, "sampled paths"));
  SweepKernel<SmpParams> kern;
  FSMC_TRY(sweepKernelFor(ctx, m, "sampled paths", "sampling", false,
                          [](auto kt) { return sample_kernel<decltype(kt)::value>; }, kern));
  const size_t S = (size_t)m->S, nS = (size_t)n_samples;
  WorkSlices ws;
  FSMC_TRY(planSlices(ctx, m, kNoDecode, kSliceSamples, ctx->ppRows.bytes, layout::samplesGroupBytes(S, nS), ws));
  const layout::Samples L = layout::samples(S, nS, ws.slicePairsMax);
  FSMC_TRY(ensure(ctx, ctx->ppRows, L.rowsBytes));
  const size_t copyBytes = spanCopyBytes(ws.slicePairsMax, L.pairBytes);
  FSMC_TRY(ensureRowCopies(ctx, copyBytes));
  LaunchPlan plan;
  FSMC_TRY(planSamplingSweep(ctx, m, kern.k, ws.slice, plan));

  SmpParams p;
  plannedSweepParams(ctx, m, plan, p);
  p.nSamples = n_samples;
  p.seedLo = (unsigned)(seed & 0xffffffffull);
  p.seedHi = (unsigned)(seed >> 32);
  p.states = (unsigned char*)ctx->ppRows.p;

  for (size_t sl = 0; sl < ws.nSlices; ++sl) {
    const size_t first = ws.firstPair(sl), nP = ws.pairs(sl);
    FSMC_TRY(launchSweepSlice(ctx, ws, sl, kern, plan.slots, p));
    if (nP > 0) {
      FSMC_HIP(ctx, hipEventRecord(ctx->evRows, ctx->stream));
      FSMC_TRY(drainSpan(ctx, ctx->ppRows.p, states + first * L.pairBytes, nP * L.pairBytes, copyBytes));
    }
    // the slice's rows have left before the next slice overwrites them
    FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  ctx->pairSlices[kSliceSamples].last = (int)ws.nSlices;
  return FSMC_OK;
}

// Per pair and site, the posterior probability that the state is lower / higher than at the site before
// (fsmc_pair_transitions.h): one launch of transition_kernel a slice, planned by planSamplingSweep into the decode's
// workspace (the workspace is the sampling kernel's).  A slice's rows, [down | up][pair][S] floats in ppRows, are two spans
// of the caller's arrays and leave through drainSpan, one after the other behind one record of evRows; its bin sums are
// pair_tail_bins_kernel's bin_tail_length (binBlocks, four deep for each of the two outputs) over weights of
// 1.f -- (double)p * 1.0 is p -- and leave by a blocking copy.  Slices are independent; a slice's rows have left before
// the next launch.
int fsmc_decode_pair_transitions(fsmc_ctx* ctx, const fsmc_model* m, float* down_rows, float* up_rows,
                                 const int32_t* bin_edges, int32_t n_bins, float* bin_down, float* bin_up)
{
  FSMC_TRY(checkReady(ctx, m));
  if (!down_rows && !up_rows && !bin_down && !bin_up) {
    return fail(ctx, FSMC_EINVAL, "change probabilities: need at least one output (down_rows, up_rows, bin_down, bin_up)");
  }
  const bool wantBins = bin_down || bin_up;
  if (wantBins) {
    if (!bin_edges) {
      return fail(ctx, FSMC_EINVAL, "change probabilities: the bin outputs need bin edges");
    }
    if (n_bins < 0) {
      return fail(ctx, FSMC_EINVAL, "change probabilities: n_bins is negative");
    }
    FSMC_TRY(checkBinEdges(ctx, m, bin_edges, (size_t)n_bins));
  }
  FSMC_TRY(checkWholeSequence(ctx, m, "change probabilities"));
  SweepKernel<TrnParams> kern;
  FSMC_TRY(sweepKernelFor(ctx, m, "change probabilities", "transition", false,
                          [](auto kt) { return transition_kernel<decltype(kt)::value>; }, kern));
  const size_t S = (size_t)m->S, B = wantBins ? (size_t)n_bins : 0;
  WorkSlices ws;
  FSMC_TRY(planSlices(ctx, m, kNoDecode, kSliceTransitions, ctx->ppRows.bytes + ctx->pxAcc.bytes,
                      layout::transitionsGroupBytes(S, B), ws));
  if (ws.slicePairsMax > (size_t)INT32_MAX) {
    return fail(ctx, FSMC_EINVAL, "too many pairs in one slice (fsmc_ctx_set_pair_transitions_slice)");
  }
  const layout::Transitions L = layout::transitions(S, B, ws.slicePairsMax);
  FSMC_TRY(ensure(ctx, ctx->ppRows, L.rowsBytes));
  if (wantBins) {
    FSMC_TRY(ensure(ctx, ctx->pxAcc, L.accBytes));
  }
  const bool wantRows = down_rows || up_rows;
  const size_t copyBytes = spanCopyBytes(ws.slicePairsMax, S * sizeof(float));
  if (wantRows) {
    FSMC_TRY(ensureRowCopies(ctx, copyBytes));
  }
  LaunchPlan plan;
  FSMC_TRY(planSamplingSweep(ctx, m, kern.k, ws.slice, plan));

  float* const dRows[2] = {(float*)ctx->ppRows.p, (float*)ctx->ppRows.p + L.rowsPerOut * S};
  char* const acc = (char*)ctx->pxAcc.p;
  std::vector<float> ones;
  if (wantBins) {
    ones.assign(S, 1.f);
    FSMC_TRY(uploadBinEdges(ctx, acc + L.offEdges, bin_edges, B));
    FSMC_HIP(ctx, hipMemcpyAsync(acc + L.offWeights, ones.data(), S * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  TrnParams p;
  plannedSweepParams(ctx, m, plan, p);
  p.ghostMask = m->ghostMask;
  p.down = dRows[0];
  p.up = dRows[1];

  PairTailParams r;
  std::memset(&r, 0, sizeof(r));
  float* const dBins = wantBins ? (float*)(acc + L.offBins) : nullptr;
  r.rows = dRows[0];
  r.rowsPerOut = L.rowsPerOut;
  r.S = m->S;
  r.nTail = 2;
  r.edges = wantBins ? (const int*)(acc + L.offEdges) : nullptr;
  r.weights = wantBins ? (const float*)(acc + L.offWeights) : nullptr;
  r.B = (int)B;
  r.binLength = dBins;
  float* const hRows[2] = {down_rows, up_rows};
  float* const hBins[2] = {bin_down, bin_up};

  for (size_t sl = 0; sl < ws.nSlices; ++sl) {
    const size_t first = ws.firstPair(sl), nP = ws.pairs(sl);
    FSMC_TRY(launchSweepSlice(ctx, ws, sl, kern, plan.slots, p));
    if (wantBins && nP > 0) {
      r.n = (int)nP;
      // (waves of the reduction: four deep for each of the two outputs)
      hipLaunchKernelGGL(pair_tail_bins_kernel, dim3(binBlocks(ctx, 4, 1, nP * B), 2u), dim3(kPairBinsThreads), 0,
                         ctx->stream, r);
      FSMC_HIP(ctx, hipGetLastError());
      FSMC_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream)); // (the call's timed span: every sweep and every reduction)
    }
    if (wantRows && nP > 0) {
      FSMC_HIP(ctx, hipEventRecord(ctx->evRows, ctx->stream));
      for (int o = 0; o < 2; ++o) {
        if (hRows[o]) {
          FSMC_TRY(drainSpan(ctx, dRows[o], hRows[o] + first * S, nP * S * sizeof(float), copyBytes));
        }
      }
    }
    // the slice's rows and cells have left before the next slice overwrites them
    FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int o = 0; o < 2; ++o) {
      FSMC_TRY(sliceToCaller(ctx, ws, sl, hBins[o], dBins ? dBins + (size_t)o * L.rowsPerOut * B : nullptr,
                             B * sizeof(float)));
    }
  }
  ctx->pairSlices[kSliceTransitions].last = (int)ws.nSlices;
  return FSMC_OK;
}

// Per pair and site, tail probabilities at state cuts and quantile states of the posterior (fsmc_pair_cdf.h), without the
// [K][S] tables leaving the device: pair_cdf_kernel reduces a slice's dump into ppRows, [output][pair of slice][S], one
// launch of a workgroup per group and site block (cdfParams, launchCdf).  Slices are independent.
int fsmc_decode_pair_cdf(fsmc_ctx* ctx, const fsmc_model* m, const int32_t* tail_states, size_t n_tail,
                         float* const* tail_rows, const float* quantiles, size_t n_quantiles,
                         int32_t* const* quantile_rows)
{
  FSMC_TRY(checkReady(ctx, m));
  if (n_tail == 0 && n_quantiles == 0) {
    return fail(ctx, FSMC_EINVAL, "need at least one output (a tail state or a quantile)");
  }
  if (n_tail > kMaxOfAKind) {
    return fail(ctx, FSMC_EINVAL, kTooManyTailStates);
  }
  if (n_quantiles > kMaxOfAKind) {
    return fail(ctx, FSMC_EINVAL, "at most 8 quantiles a call");
  }
  if (n_tail && (!tail_states || !tail_rows)) {
    return fail(ctx, FSMC_EINVAL, "tail_states or tail_rows is null");
  }
  if (n_quantiles && (!quantiles || !quantile_rows)) {
    return fail(ctx, FSMC_EINVAL, "quantiles or quantile_rows is null");
  }
  std::vector<PairCdfSpec> spec;
  FSMC_TRY(tailSpecs(ctx, m, tail_states, n_tail, tail_rows, spec));
  std::vector<char*> hRows; // the caller's matrices, in the order of spec
  for (size_t j = 0; j < n_tail; ++j) {
    hRows.push_back((char*)tail_rows[j]);
  }
  for (size_t j = 0; j < n_quantiles; ++j) {
    if (!quantile_rows[j]) {
      return fail(ctx, FSMC_EINVAL, "quantile_rows[" + std::to_string(j) + "] is null");
    }
    if (!std::isfinite(quantiles[j]) || !(quantiles[j] > 0.f) || quantiles[j] > 1.f) {
      return fail(ctx, FSMC_EINVAL, "quantile " + std::to_string(quantiles[j]) + " not finite or outside (0, 1]");
    }
    spec.push_back(PairCdfSpec{0, quantiles[j]});
    hRows.push_back((char*)quantile_rows[j]);
  }
  FSMC_TRY(checkWholeSequence(ctx, m, "per-pair tails and quantiles"));
  const size_t K = (size_t)m->K, S = (size_t)m->S, nOut = spec.size();
  WorkSlices ws;
  FSMC_TRY(planSlices(ctx, m, kModeDump, kSliceCdf, ctx->ppStage.bytes + ctx->ppRows.bytes,
                      layout::cdfGroupBytes(K, S, nOut), ws, layout::sliceMostBySiteBlocks(S)));
  const layout::Cdf L = layout::cdf(K, S, nOut, ws.slice, ws.slicePairsMax);
  const size_t outCells = L.outCells; // cells of one output of the largest slice
  FSMC_TRY(ensure(ctx, ctx->aux, ws.slice * sizeof(size_t)));
  FSMC_TRY(ensure(ctx, ctx->ppStage, L.stageBytes));
  FSMC_TRY(ensure(ctx, ctx->ppRows, L.rowsBytes));
  FSMC_TRY(ensure(ctx, ctx->pcSpec, L.specBytes));
  // the way out: cells a copy -- what a pinned buffer holds, or one output of the largest slice if that is smaller
  const size_t cellsPerCopy = std::min(std::max<size_t>(1, rowCopyBytes() / sizeof(float)), outCells);
  FSMC_TRY(ensureRowCopies(ctx, cellsPerCopy * sizeof(float)));

  KParams p;
  FSMC_TRY(dumpSetup(ctx, m, ws, p));
  FSMC_HIP(ctx, hipMemcpyAsync(ctx->pcSpec.p, spec.data(), L.specBytes, hipMemcpyHostToDevice, ctx->stream));
  FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));

  PairCdfParams q = cdfParams(ctx, m, ws, nOut);
  auto reduce = [&](size_t sl) -> int { return launchCdf(ctx, ws, sl, q); };
  // the slice's pairs are rows 0 ... of every output on the device, `outCells` apart: output by output, runs of cells
  // into the caller's matrix
  auto drain = [&](size_t sl) -> int {
    const size_t cells = ws.pairs(sl) * S, copiesPerOut = (cells + cellsPerCopy - 1) / cellsPerCopy;
    const float* const dRows = (const float*)ctx->ppRows.p;
    auto first = [&](size_t c) { return (c % copiesPerOut) * cellsPerCopy; };
    auto bytes = [&](size_t c) { return std::min(cellsPerCopy, cells - first(c)) * sizeof(float); };
    return drainRows(
        ctx, copiesPerOut * nOut,
        [&](size_t c) { return RowChunk{dRows + c / copiesPerOut * outCells + first(c), bytes(c)}; },
        [&](size_t c, const char* host) {
          std::memcpy(hRows[c / copiesPerOut] + (ws.firstPair(sl) * S + first(c)) * sizeof(float), host, bytes(c));
        });
  };
  FSMC_TRY(decodeSlicesDrained(ctx, ws, p, true, reduce, drain));
  FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->pairSlices[kSliceCdf].last = (int)ws.nSlices;
  return FSMC_OK;
}

// The tail probabilities of fsmc_decode_pair_cdf reduced over pairs per site and over bins of sites per pair
// (fsmc_pair_tail.h), without the tail rows leaving the device: pair_cdf_kernel -- as it is, through the cdfParams and
// launchCdf of fsmc_decode_pair_cdf -- reduces a slice's dump into ppRows, [cut][pair of slice][S]; then
// pair_tail_sum_kernel continues the fp64 chain of every site in the device copy of the accumulator and
// pair_tail_bins_kernel (binBlocks, eight deep over the cuts) reduces the rows cell by cell, and the slice's
// [cut][pairs][B] outputs are copied to the caller's arrays at the slice's first pair.  Only the sum is carried from
// slice to slice.
int fsmc_decode_pair_tail_summaries(fsmc_ctx* ctx, const fsmc_model* m, const int32_t* tail_states, size_t n_tail,
                                    double* tail_sum, const int32_t* bin_edges, size_t n_bins, float* bin_tail_mean,
                                    const float* site_weights, float* bin_tail_length)
{
  FSMC_TRY(checkReady(ctx, m));
  const bool wantBins = bin_tail_mean || bin_tail_length;
  if (!tail_sum && !wantBins) {
    return fail(ctx, FSMC_EINVAL, "need at least one output (tail_sum, bin_tail_mean or bin_tail_length)");
  }
  if (n_tail == 0 || !tail_states) {
    return fail(ctx, FSMC_EINVAL, "need one tail state at least");
  }
  if (n_tail > kMaxOfAKind) {
    return fail(ctx, FSMC_EINVAL, kTooManyTailStates);
  }
  std::vector<PairCdfSpec> spec;
  FSMC_TRY(tailSpecs(ctx, m, tail_states, n_tail, nullptr, spec));
  if (wantBins) {
    if (!bin_edges) {
      return fail(ctx, FSMC_EINVAL, "bin outputs need bin edges");
    }
    FSMC_TRY(checkBinEdges(ctx, m, bin_edges, n_bins));
  }
  if (bin_tail_length) {
    if (!site_weights) {
      return fail(ctx, FSMC_EINVAL, "bin_tail_length needs site weights");
    }
    for (int t = 0; t < m->S; ++t) {
      if (!std::isfinite(site_weights[t])) {
        return fail(ctx, FSMC_EINVAL, "site weight " + std::to_string(t) + " is not finite");
      }
    }
  }
  FSMC_TRY(checkWholeSequence(ctx, m, "tail summaries"));
  const size_t K = (size_t)m->K, S = (size_t)m->S, nT = n_tail, B = wantBins ? n_bins : 0;
  const bool wantMean = bin_tail_mean != nullptr, wantLength = bin_tail_length != nullptr;
  const size_t siteBlocks = layout::siteBlocks(S);
  WorkSlices ws;
  FSMC_TRY(planSlices(ctx, m, kModeDump, kSliceTail, ctx->ppStage.bytes + ctx->ppRows.bytes + ctx->ptAcc.bytes,
                      layout::tailGroupBytes(K, S, nT, B, wantMean, wantLength), ws, layout::sliceMostBySiteBlocks(S)));
  if (ws.slicePairsMax > (size_t)INT32_MAX) {
    return fail(ctx, FSMC_EINVAL, "too many pairs in one slice (fsmc_ctx_set_pair_tail_slice)");
  }
  const layout::Tail L = layout::tail(K, S, nT, B, wantMean, wantLength, ws.slice, ws.slicePairsMax);
  FSMC_TRY(ensure(ctx, ctx->aux, ws.slice * sizeof(size_t)));
  FSMC_TRY(ensure(ctx, ctx->ppStage, L.stageBytes));
  FSMC_TRY(ensure(ctx, ctx->ppRows, L.rowsBytes));
  FSMC_TRY(ensure(ctx, ctx->pcSpec, L.specBytes));
  FSMC_TRY(ensure(ctx, ctx->ptAcc, L.accBytes));

  char* const acc = (char*)ctx->ptAcc.p;
  double* const dSum = (double*)(acc + L.offSum);
  char* const dEdges = acc + L.offEdges;
  char* const dWeights = acc + L.offWeights;
  float* const dMean = wantMean ? (float*)(acc + L.offMean) : nullptr;
  float* const dLength = wantLength ? (float*)(acc + L.offLength) : nullptr;
  const size_t sumBytes = L.sumBytes;
  KParams p;
  FSMC_TRY(dumpSetup(ctx, m, ws, p));
  FSMC_HIP(ctx, hipMemcpyAsync(ctx->pcSpec.p, spec.data(), L.specBytes, hipMemcpyHostToDevice, ctx->stream));
  if (tail_sum) { // the chain continues what the caller passes in
    FSMC_HIP(ctx, hipMemcpyAsync(dSum, tail_sum, sumBytes, hipMemcpyHostToDevice, ctx->stream));
  }
  if (wantBins) {
    FSMC_TRY(uploadBinEdges(ctx, dEdges, bin_edges, B));
  }
  if (bin_tail_length) {
    FSMC_HIP(ctx, hipMemcpyAsync(dWeights, site_weights, S * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  }
  FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));

  PairCdfParams q = cdfParams(ctx, m, ws, nT);
  PairTailParams r;
  r.rows = (const float*)ctx->ppRows.p;
  r.rowsPerOut = ws.slicePairsMax;
  r.S = m->S;
  r.nTail = (int)nT;
  r.sum = tail_sum ? dSum : nullptr;
  r.edges = wantBins ? (const int*)dEdges : nullptr;
  r.weights = bin_tail_length ? (const float*)dWeights : nullptr;
  r.B = (int)B;
  r.binMean = dMean;
  r.binLength = dLength;
  float* const hOut[2] = {bin_tail_mean, bin_tail_length};
  const float* const dOut[2] = {dMean, dLength};

  for (size_t sl = 0; sl < ws.nSlices; ++sl) {
    FSMC_TRY(launchSlice(ctx, ws, sl, p));
    const size_t n = ws.pairs(sl);
    FSMC_TRY(launchCdf(ctx, ws, sl, q));
    r.n = (int)n;
    if (tail_sum) {
      hipLaunchKernelGGL(pair_tail_sum_kernel, dim3((unsigned)siteBlocks, (unsigned)nT), dim3(kWave), 0, ctx->stream, r);
      FSMC_HIP(ctx, hipGetLastError());
    }
    if (wantBins) {
      // (waves of the bin reduction: eight deep over the cuts)
      hipLaunchKernelGGL(pair_tail_bins_kernel, dim3(binBlocks(ctx, 8, nT, n * B), (unsigned)nT), dim3(kPairBinsThreads), 0,
                         ctx->stream, r);
      FSMC_HIP(ctx, hipGetLastError());
    }
    FSMC_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream)); // (the call's timed span: every decode and every reduction)
    if (wantBins) {
      // the slice's cells go to the caller before the next slice overwrites them, cut by cut (no second buffer, no
      // overlap: 8 bytes a cell at most against the 4 K bytes a pair-site of the dump)
      FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
      for (int o = 0; o < 2; ++o) {
        for (size_t j = 0; hOut[o] && j < nT; ++j) { // (cut j: [pairs][B] of the caller's, [pairs of the slice][B] here)
          FSMC_TRY(sliceToCaller(ctx, ws, sl, hOut[o] + j * ctx->nPairs * B, dOut[o] + j * ws.slicePairsMax * B,
                                 B * sizeof(float)));
        }
      }
    }
  }
  FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (tail_sum) {
    FSMC_HIP(ctx, hipMemcpy(tail_sum, dSum, sumBytes, hipMemcpyDeviceToHost));
  }
  ctx->pairSlices[kSliceTail].last = (int)ws.nSlices;
  return FSMC_OK;
}

int fsmc_decode_sums(fsmc_ctx* ctx, const fsmc_model* m, float* sums, float* sums00, float* sums01, float* sums11)
{
  return fsmc_decode_sums_batches(ctx, m, nullptr, 0, sums, sums00, sums01, sums11);
}

int fsmc_decode_sums_batches(fsmc_ctx* ctx, const fsmc_model* m, const uint32_t* batch_first_group, size_t n_batches,
                             float* sums, float* sums00, float* sums01, float* sums11)
{
  FSMC_TRY(checkReady(ctx, m));
  if (batch_first_group) {
    // batch b = groups batch_first_group[b] .. batch_first_group[b + 1] - 1: a partition of the group list, in order
    if (n_batches == 0 || batch_first_group[0] != 0 || batch_first_group[n_batches] != ctx->nGroups) {
      return fail(ctx, FSMC_EINVAL, "batches must partition the group list");
    }
    for (size_t bI = 0; bI < n_batches; ++bI) {
      if (batch_first_group[bI + 1] <= batch_first_group[bI]) {
        return fail(ctx, FSMC_EINVAL, "a batch holds at least one group and batches are in group order");
      }
    }
  } else {
    n_batches = ctx->nGroups; // every group is a batch of its own
  }
  const bool mm = sums00 || sums01 || sums11;
  if (!sums && !mm) {
    return fail(ctx, FSMC_EINVAL, "no output requested");
  }
  if (mm && !(sums00 && sums01 && sums11)) {
    return fail(ctx, FSMC_EINVAL, "the 00/01/11 sums come together");
  }
  for (const fsmc_group& g : ctx->hGroups) {
    if (g.from != 0 || g.to != (uint32_t)m->S) {
      return fail(ctx, FSMC_EINVAL, "posterior sums need whole-sequence groups (HMM.cpp:1052)");
    }
  }
  FSMC_HIP(ctx, hipSetDevice(ctx->device));
  uint32_t wantStride = ctx->betaStride;
  if (wantStride == 0) { // left to the library: plan::sumsKeepStrideOne
    const KernelChoice k2 = chooseKernel(m, kModeSums, false, false, 0);
    int perCU = 0;
    if (k2.fn && k2.stride == 2 && workgroupsPerCU(k2, 8, 0, perCU) == hipSuccess &&
        plan::sumsKeepStrideOne(settingsOf(ctx), perCU, n_batches)) {
      wantStride = 1;
    }
  }
  // One launch decodes up to `slots` batches (one per wave; slots = resident waves, fewer if the planes would not fit)
  // and leaves each batch's sums in its own plane (the groups of a batch of more than 64 pairs in turn, each continuing
  // the running sums of the one before); add_planes_in_order_kernel then adds the planes to the accumulator in batch
  // order.  The accumulator starts from the caller's arrays, so that several calls (flushes)
  // continue the same sequential sum.
  // A launch of few batches (at most half the chip's waves) whose planes all fit: two waves per window, a workgroup per
  // batch (prepareDecode).
  const size_t plane = (size_t)m->S * m->K;
  const int nP = mm ? 4 : 1; // planes per group: the sum, or the sum and its 00 / 01 / 11 split
  const size_t slotFloats = (size_t)nP * plane; // a slot holds the planes the launch was asked for
  LaunchPlan plan;
  FSMC_TRY(prepareDecode(ctx, m, kModeSums, wantStride, ctx->hGroups, n_batches, slotFloats * sizeof(float), plan));
  const size_t slots = (size_t)plan.slots;
  FSMC_TRY(ensure(ctx, ctx->out, (slots + 1) * slotFloats * sizeof(float)));
  float* const acc = (float*)ctx->out.p + slots * slotFloats;
  float* dst[4] = {sums, sums00, sums01, sums11};
  for (int q = 0; q < 4; ++q) {
    if (dst[q]) {
      FSMC_HIP(ctx, hipMemcpyAsync(acc + (size_t)q * plane, dst[q], plane * sizeof(float), hipMemcpyHostToDevice,
                                   ctx->stream));
    }
  }
  KParams p;
  fillParams(ctx, m, plan, (sums ? FSMC_WANT_SUMS : 0u) | (mm ? FSMC_WANT_MAJOR_MINOR_SUMS : 0u), p);
  p.sums = (float*)ctx->out.p;
  p.sumsPlane = plane;
  p.sumsSlot = slotFloats;
  if (batch_first_group) {
    FSMC_TRY(ensure(ctx, ctx->aux, (n_batches + 1) * sizeof(uint32_t)));
    FSMC_HIP(ctx, hipMemcpyAsync(ctx->aux.p, batch_first_group, (n_batches + 1) * sizeof(uint32_t), hipMemcpyHostToDevice,
                                 ctx->stream));
    p.batchFirst = (const unsigned*)ctx->aux.p;
  }
  for (size_t base = 0; base < n_batches; base += slots) {
    const size_t n = std::min(slots, n_batches - base);
    p.groupBase = (int)base;
    FSMC_TRY(launch(ctx, plan.k, p, (int)n, 0, base != 0, &plan));
    // (planes the launch did not ask for hold stale values: they are added to accumulator planes nobody reads)
    hipLaunchKernelGGL(add_planes_in_order_kernel, dim3(1024), dim3(256), 0, ctx->stream, (const float*)ctx->out.p, acc,
                       slotFloats, (int)n, slotFloats);
    FSMC_HIP(ctx, hipGetLastError());
    FSMC_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream)); // (the call's timed span: decode launches + plane additions)
  }
  FSMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int q = 0; q < 4; ++q) {
    if (dst[q]) {
      FSMC_HIP(ctx, hipMemcpy(dst[q], acc + (size_t)q * plane, plane * sizeof(float), hipMemcpyDeviceToHost));
    }
  }
  return FSMC_OK;
}

} // extern "C"
