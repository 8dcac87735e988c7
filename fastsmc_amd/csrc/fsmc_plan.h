// fsmc_plan.h -- what every decode launch looks like, decided: chunk length, checkpoints, resident chunks, the chunk
// pool, slots and workspace bytes; what the context may spend and what it has earned; how half-full groups are paired;
// how the work list is cut into slices.
//
// Deciding, not doing: pure arithmetic on plain inputs.  Nothing here knows the device's runtime, a kernel, the context
// or the environment -- the library's host side reads those at each call, hands the numbers in and does what the plan says
// (allocations, launches, the getters' record).  tests/plan_driver.cpp runs these functions on a CPU.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/fastsmc_hip.h"

namespace fsmc
{
namespace plan
{
// The kernels' constants the plans are laid out for (the library's host side asserts that they are the kernel headers').
constexpr int kWave = 64;           // lanes of a wave: a stored row holds a float4 per lane and four states
constexpr size_t kFloat4Bytes = 16;   // sizeof(float4)

// What a plan reads of the context: the device and the caller's settings (the set_* entry points).
struct Settings {
  int nCU = 0;
  uint64_t hbmBytes = 0;
  uint64_t wsLimit = 0;      // set_workspace_limit, 0 = none
  uint32_t chunkSites = 0;   // 0 = automatic
  int residentChunks = -1;   // -1 = as many as the workspace limit allows, 0 = none
  int chunkPool = -1;        // -1 = IBD launches of more than two rounds, 0 = never, 1 = wherever it is built
  uint32_t chunkPoolPhi = 200; // per cent of its share of the pool that a window may ask for
};

// What the device says it has free right now (`known` false: it did not say).
struct MemInfo {
  bool known = false;
  uint64_t freeBytes = 0;
};

// What a plan reads of its kernel.
struct KernelTraits {
  int member = 0;        // as the last_kernel getter reports it
  int stride = 1;        // the beta stride the kernel is built for: the plan lays the chunk buffer out for it
  // float4 per lane of a stored K-vector: a padded family member (and the wave-group kernel) stores its ghosts too
  // (the any-K kernel, member 0, stores K states; its rows carry their scale in one more float4)
  size_t rowFloat4 = 0;
  // rows beside the chunk buffer and the checkpoints: parking / segment sums; the any-K kernel keeps every vector there
  size_t sideRows = 4;
  size_t chunkFloor = 512; // sites of a default chunk at the least (the wave-group kernel pays more per restart: 2048)
  // resident chunks are built for it: array-mode IBD decode and sums of the lane-per-pair family and of the wave-group
  // kernel's four-wave members
  bool resident = false;
  bool pool = false;     // the same kernel with the chunk pool exists (lane-per-pair family, one group per wave)
  int perCU = 0;         // workgroups of it that a CU holds at once, as queried (capWorkgroups)
};

// A launch, self-describing: a slot's layout, slots, bytes (chunkRows is computed for its kernel's beta stride).
struct LaunchPlan {
  int chunk = 0;
  int chunkRows = 0; // rows of the chunk buffer (chunk, or half of it with beta stride 2)
  int maxChunks = 0;
  int residentChunks = 0; // chunk buffers beyond the first: chunks whose rows pass B keeps (no rebuild)
  size_t wsSlot = 0; // float4 per slot
  int slots = 0;
  int wavesPerWindow = 1; // 2: the two-waves-per-window kernel, a workgroup per slot
  size_t bytes = 0;       // of workspace: wsSlot float4 for every slot, and the pool behind them
  // The resident chunk buffers as a pool behind the slots (poolBuffers == 0: each slot holds its own, the static layout)
  size_t poolOff = 0;       // float4 from the workspace's start to the pool: wsSlot x the slots planned
  uint32_t poolBuffers = 0; // slots x residentChunks buffers of chunkRows rows
  int poolCap = 0;          // the chunks of a window below this index ask for a buffer
};

// What a decode may spend on its workspace.
// The most it can have (`hard`): the caller's limit if one is set (set_workspace_limit); otherwise 80 % of the
// card where that much is free (the card has 288 GB; the model, the haplotypes and the records are small), at least 40 %.
// What its plan may be UPGRADED with (`soft`) -- a window kept whole instead of chunked, resident chunks, longer windows
// in the paired kernel: the same when the caller set a limit (the caller knows the job).  Otherwise memory has to be
// earned: an allocation costs ~40 ms per GB on this driver (230 GB: 4.4-9 s; tools/malloc_cost.py), a rebuilt chunk costs a
// few per cent of a launch, so a run of a few seconds must not start by allocating the card.  Every launch adds what
// it is expected to save -- kEarnFraction of its estimated kernel time -- at the allocation rate; the buffer is kept
// between launches, so a long job reaches the full card and a short one stays small.
// A bigger buffer is a NEW allocation of its whole size (free + allocate), so growth is amortised and every byte is
// paid for once: an upgrade is considered only when the credit covers twice the buffer held (or the whole hard
// budget), and an allocation is debited from the credit.  Creeping up a resident chunk per flush -- 16 allocations of
// 27 ... 230 GB, 80 s of allocating on a 390-s job -- is what this replaces.  A caller that knows its job announces it
// (expect_work: HMM::decodeAll knows its pair count, HMM.cpp:310-321): the credit of the whole job is there
// at the first launch, and a job long enough to pay for the card allocates it once, at the start.
// `curBytes`: the buffer about to be re-used (what it holds is paid for).
constexpr double kAllocBytesPerSecond = 25e9; // measured: allocating 64 / 128 GB takes 2.4 / 5.2 s
constexpr double kEarnFraction = 0.06;        // what resident chunks save of a chunked launch (C2: 1974 -> 1854 ms)
constexpr uint64_t kFreeWorkspace = 24ull << 30; // never argued about (at most a second; only what a plan uses is allocated)

// The diagnostic switches, as the caller read them from the environment at this call (the defaults: not set).
struct Diag {
  long maxSlots = 0;    // FSMC_DIAG_MAX_SLOTS=<n> caps the resident waves -- tests: a short list that runs several rounds
  long wavesPerCU = 0;  // FSMC_DIAG_WAVES_PER_CU (occupancy experiments only)
  long sumsSlots = 0;   // FSMC_DIAG_SUMS_SLOTS -- tests: many launches on a small problem
  uint64_t wsFree = kFreeWorkspace; // FSMC_DIAG_WS_FREE -- tests: make the policy visible on a small problem
  double earnScale = 1.0; // FSMC_DIAG_WS_EARN_SCALE -- tests: a small problem that earns like a long job
  bool twoWavesNever = false; // FSMC_DIAG_TWO_WAVE_WINDOWS=never -- tests: the whole suite on the one-wave kernels
  int w2NW = 0, w2KH = 0;     // FSMC_DIAG_W2_MEMBER="<waves>x<states per wave>", parsed (0 x 0: not set or not a pair)
  long minimaRange = 0; // FSMC_DIAG_MINIMA_RANGE=<pairs> (fsmc_pair_layout.h) -- tests: several ranges on a small problem
};

// A diagnostic switch that lowers a count: n / divisor where that is at least 1 and below `value`.
inline size_t lowered(size_t value, long n, int divisor = 1)
{
  const long v = n / divisor;
  return v >= 1 && (size_t)v < value ? (size_t)v : value;
}

// Workgroups of a kernel that a CU holds at once: what the runtime counted, `most` at the most.  `capDivisor` > 0: and
// no more than FSMC_DIAG_WAVES_PER_CU / capDivisor.
inline int capWorkgroups(int counted, int most, int capDivisor, const Diag& diag)
{
  int perCU = std::min(counted, most);
  if (capDivisor > 0) {
    perCU = (int)lowered((size_t)std::max(perCU, 0), diag.wavesPerCU, capDivisor);
  }
  return perCU;
}

struct WsBudget {
  uint64_t hard, soft;
};

// The credit of a context.
struct Credit {
  double earned = 0; // bytes of workspace the launches so far (and the announced job) have paid for and not yet
                     // spent on an allocation (earnWorkspace, expectWork, payForWorkspace)
  double announced = 0; // estimated kernel seconds of announced work not launched yet (it has earned already)
  double announcedCredit = 0; // ... and the bytes of credit that part of the announcement was given
};

inline WsBudget workspaceBudget(const Settings& set, const Credit& credit, const MemInfo& mem, uint64_t curBytes,
                                const Diag& diag)
{
  const uint64_t reachable = mem.freeBytes + curBytes;
  const uint64_t margin = (uint64_t)(0.04 * (double)set.hbmBytes);
  if (set.wsLimit) {
    // (a limit above what the card has free right now -- another process on it -- is cut to that, if it is at least
    //  a quarter of the limit: below, the caller is told by the allocation failing)
    uint64_t lim = set.wsLimit;
    if (mem.known && reachable > margin && reachable - margin < lim && reachable - margin >= lim / 4) {
      lim = reachable - margin;
    }
    return {lim, lim};
  }
  const uint64_t floor40 = (uint64_t)(0.40 * (double)set.hbmBytes);
  uint64_t hard = floor40;
  if (mem.known) {
    const uint64_t want = (uint64_t)(0.80 * (double)set.hbmBytes);
    hard = std::max<uint64_t>(floor40, std::min<uint64_t>(want, reachable > margin ? reachable - margin : 0));
  }
  uint64_t earned = (uint64_t)std::min(std::max(credit.earned, 0.0), 1e15);
  if (earned < hard && earned < 2 * curBytes) {
    earned = 0; // (not yet worth a re-allocation: growth is geometric)
  }
  const uint64_t freeBytes = diag.wsFree;
  const uint64_t soft = std::min<uint64_t>(hard, std::max<uint64_t>({curBytes, earned, freeBytes}));
  return {hard, soft};
}

// An allocation of the workspace under the earned policy is debited from the credit (beyond the free allowance).
inline void payForWorkspace(const Settings& set, Credit& credit, uint64_t allocatedBytes, const Diag& diag)
{
  if (set.wsLimit) {
    return;
  }
  const uint64_t freeBytes = diag.wsFree;
  if (allocatedBytes > freeBytes) {
    credit.earned = std::max(0.0, credit.earned - (double)(allocatedBytes - freeBytes));
  }
}

// Where a group's sweeps end: the IBD decode walks to the end of the scan window.
inline uint32_t windowEnd(const fsmc_group& g, bool ibd)
{
  return ibd ? g.scan_to : g.to;
}

// Estimated kernel time of `pairSites` pair-sites of a model of `states` states: algorithmic bytes at 80 % of the roofline.
inline double kernelSeconds(double pairSites, int states)
{
  return pairSites * (8.0 * states + 0.25) / (0.8 * 8e12);
}

// A launch over the work list `groups` earns workspace for this and the following launches.
inline void earnWorkspace(Credit& credit, const std::vector<fsmc_group>& groups, bool ibd, int states, const Diag& diag)
{
  double pairSites = 0;
  for (const fsmc_group& g : groups) {
    const uint32_t aEnd = windowEnd(g, ibd);
    pairSites += (double)g.n_pairs * (double)(aEnd > g.from ? aEnd - g.from : 0);
  }
  double seconds = kernelSeconds(pairSites, states);
  // (work that was announced has earned already: expectWork)
  const double announced = std::min(credit.announced, seconds);
  if (credit.announced > 0) {
    credit.announcedCredit *= (credit.announced - announced) / credit.announced; // (that part is spent: it was launched)
  }
  credit.announced -= announced;
  seconds -= announced;
  credit.earned += diag.earnScale * kEarnFraction * seconds * kAllocBytesPerSecond;
}

// expect_work: a job of `pairSites` pair-sites is announced, or (0) the announced job is over.
inline void expectWork(const Settings& set, Credit& credit, double pairSites, int states, const Diag& diag)
{
  if (pairSites == 0) {
    // the announced job is over (HMM::finishDecoding / finishFromHashing): what is left of the announcement -- an
    // estimate that was too high, pairs that were filtered, a job that threw -- is forgotten and its unspent credit
    // taken back, so that a later job on this context earns from its own launches again
    credit.earned = std::max(0.0, credit.earned - credit.announcedCredit);
    credit.announced = 0;
    credit.announcedCredit = 0;
    return;
  }
  // the job's launches will save what workspace upgrades save of its estimated kernel time: its credit is there at the
  // first launch (workspaceBudget); the launches themselves then earn nothing until the announced work is used up.
  // No announcement is worth more than the card: the credit is capped at the device's memory.
  const double seconds = kernelSeconds(pairSites, states);
  const double given = std::min(diag.earnScale * kEarnFraction * seconds * kAllocBytesPerSecond,
                                std::max(0.0, (double)set.hbmBytes - credit.announcedCredit));
  credit.announced += seconds;
  credit.announcedCredit += given;
  credit.earned += given;
}

// Decide chunking of the beta stream and the number of resident waves of kernel `k` over `list`, the
// groups its waves pull from.  `ibd`: an IBD decode (its windows end with the scan).  `paired`: two half-groups per
// wave, `list` holding the union of each pair's windows.  `share`: the launch runs beside another one and may take
// 1/share of the budget.  `why`: the message of a status other than FSMC_OK.
inline int planOneWave(const Settings& set, const KernelTraits& k, bool ibd, const std::vector<fsmc_group>& list,
                       bool paired, const WsBudget& budget, unsigned share, const Diag& diag, LaunchPlan& plan,
                       std::string& why)
{
  const size_t slots =
      lowered(std::max<size_t>(1, std::min((size_t)set.nCU * std::max(k.perCU, 1), list.size())), diag.maxSlots);
  size_t L = 1;
  for (const fsmc_group& g : list) {
    const size_t aEnd = windowEnd(g, ibd);
    L = std::max<size_t>(L, aEnd - g.from);
  }
  const size_t K4 = k.rowFloat4;
  const size_t vecBytes = K4 * kWave * kFloat4Bytes;
  const uint64_t limit = budget.hard / share;
  // Rows a chunk of C sites needs in the chunk buffer: with beta stride 2 only every second site's row is stored.
  const bool half = k.stride == 2;
  auto chunkRows = [&](size_t c) { return half ? (c + 1) / 2 : c; };
  const size_t rowsAvail = (size_t)(limit / (vecBytes * slots)); // rows one resident wave may hold
  const size_t rowsSoft = (size_t)(budget.soft / share / (vecBytes * slots)); // ... and may have earned so far
  const size_t sideRows = k.sideRows;
  const size_t defaultChunk = std::max<size_t>((size_t)std::ceil(std::sqrt((double)L)), k.chunkFloor);
  size_t C, maxChunks;
  // A window stays whole if that fits what the launches have earned (or is no longer than a chunk would be anyway).
  // An explicit chunk length (set_chunk_sites) is kept -- by the paired kernel too, which has the chunked
  // layout since round 3.
  if (chunkRows(L) + sideRows + 1 <= rowsAvail && (chunkRows(L) + sideRows + 1 <= rowsSoft || L <= defaultChunk) &&
      !(set.chunkSites && set.chunkSites < L)) {
    C = L;
    maxChunks = 1;
  } else {
    // The chunk length of a window that does not fit the workspace whole: 512 sites, or sqrt(window) if that is larger
    // (memory is chunk + window / chunk rows), shrunk to what the workspace limit allows.  Short chunks cost a
    // checkpoint row and a pipeline restart each and let the resident chunks (below) fill the memory that is left to
    // the last row: C2 at 2048 / 1024 / 512 sites a chunk runs 1886 / 1881 / 1870 ms.
    C = set.chunkSites ? (size_t)set.chunkSites : defaultChunk;
    // (the wave-group kernel pays more per restart: 2048)
    C = std::min((C + 15) / 16 * 16, (L + 15) / 16 * 16);
    auto fits = [&](size_t c) { return chunkRows(c) + (L + c - 1) / c + sideRows + 1 <= rowsAvail; };
    if (!set.chunkSites) {
      while (C > 16 && !fits(C)) {
        C = std::max<size_t>(16, (C / 2 + 15) / 16 * 16);
      }
    }
    maxChunks = (L + C - 1) / C;
    if (!fits(C)) {
      why = "workspace limit too small for the decode window";
      return FSMC_ENOMEM;
    }
  }
  // Resident chunks (fsmc_kernels.h): a chunked window rebuilds every chunk's rows from a checkpoint -- one of its 3.5
  // sweeps -- except for the chunks whose rows pass B can leave in the workspace.  Whatever the limit leaves after the
  // one chunk buffer, the checkpoints and the parking rows goes to such chunks (array-mode IBD decode and sums of the
  // lane-per-pair family, one group per wave -- the paired kernel is not built with them -- and of the wave-group kernel's
  // four-wave members).
  size_t resident = 0;
  const size_t rowsBudget = rowsSoft;
  // (exactly the rows of plan.wsSlot below: a plan must qualify again for the buffer it was given -- with a row of
  //  slack here a context whose soft budget is the buffer it holds lost one resident chunk at its next launch)
  const size_t fixed = chunkRows(C) + maxChunks + sideRows;
  const bool residentBuilt = maxChunks > 1 && k.resident && !paired;
  if (residentBuilt && set.residentChunks != 0 && rowsBudget > fixed) {
    resident = std::min<size_t>((rowsBudget - fixed) / chunkRows(C), maxChunks);
    if (set.residentChunks > 0) {
      resident = std::min<size_t>(resident, (size_t)set.residentChunks);
    }
  }
  // The pool (the kernels built with it: KernelTraits::pool): the same buffers, slots x resident of them, behind
  // the slots instead of inside them, claimed by whichever wave has rows to keep.  A wave holds rows from the end of its pass B to the start of its
  // pass A only, so a launch whose waves are spread over their groups -- one that runs several rounds -- keeps more
  // chunks in the same memory.  Taken when the count is left to the library and is neither nothing nor everything, and
  // the launch is an IBD decode of more than two rounds of groups -- what was measured (C2: 3.8 rounds).  One round has
  // nobody to share with (a sums launch is always one: its batches run side by side, whatever the list holds), and in a
  // launch of two rounds every wave's first group runs in phase with all the others; both keep the static layout, and
  // so do the sums, until a measurement says otherwise.  A slot gains one row, the table of its window's chunks (a
  // 32-bit entry each): where that row costs the last buffer, the plan has one buffer less a wave; it never exceeds the
  // budget the static plan was given.  A window asks for a buffer for its first poolCap chunks: phi x its share.
  size_t poolResident = 0;
  if (residentBuilt && k.pool && set.chunkPool != 0 && set.residentChunks < 0 && resident > 0 && resident < maxChunks &&
      (set.chunkPool == 1 || (ibd && list.size() > 2 * slots)) && maxChunks * sizeof(int32_t) <= vecBytes &&
      rowsBudget > fixed + 1) {
    poolResident = std::min((rowsBudget - fixed - 1) / chunkRows(C), resident);
  }
  plan.chunk = (int)C;
  plan.chunkRows = (int)chunkRows(C);
  plan.maxChunks = (int)maxChunks;
  plan.slots = (int)slots;
  plan.wavesPerWindow = 1;
  if (poolResident > 0 && slots * poolResident < (1u << 30)) {
    const size_t want = ((size_t)set.chunkPoolPhi * poolResident + 99) / 100;
    plan.residentChunks = (int)poolResident;
    plan.wsSlot = (chunkRows(C) + maxChunks + 2 + (sideRows - 2) + 1) * K4 * kWave;
    plan.poolOff = plan.wsSlot * slots;
    plan.poolBuffers = (uint32_t)(slots * poolResident);
    plan.poolCap = (int)std::min(maxChunks, std::max<size_t>(want, 1));
    plan.bytes = (plan.poolOff + (size_t)plan.poolBuffers * chunkRows(C) * K4 * kWave) * kFloat4Bytes;
    return FSMC_OK;
  }
  plan.residentChunks = (int)resident;
  plan.wsSlot = (chunkRows(C) * (1 + resident) + maxChunks + 2 + (sideRows - 2)) * K4 * kWave;
  plan.poolOff = 0;
  plan.poolBuffers = 0;
  plan.poolCap = 0;
  plan.bytes = plan.wsSlot * kFloat4Bytes * slots;
  return FSMC_OK;
}

// The launch of a checkpointed pair sweep (the Viterbi, sampling and transition kernels) over slices of at most `nGroups`
// whole-sequence groups of `S` sites.  A wave's workspace is `chunk` rows of `rowBytes` and a checkpoint of `ckptBytes` a
// chunk; without rows (`keepRows` false) one row that nobody reads.  The waves: what is resident, the groups, and what
// the hard budget holds of the smallest slot any chunk length gives (about `cMinFactor` x sqrt(S) sites a chunk).  The
// chunk: the caller's (set_chunk_sites), otherwise the whole sequence -- one sweep instead of two -- halved until the
// waves' slots fit what the context may spend (the soft budget; the hard one for sequences of at most 512 sites, as
// planOneWave keeps short windows whole).  `perCU`: the kernel's workgroups a CU, as queried; `refusal`: what `why`
// says when the hard budget does not hold one wave's smallest slot.
inline int planReplay(const Settings& set, int S, int perCU, size_t nGroups, size_t rowBytes, size_t ckptBytes,
                      double cMinFactor, bool keepRows, const char* refusal, const WsBudget& budget, LaunchPlan& plan,
                      std::string& why)
{
  size_t slots = std::max<size_t>(1, std::min((size_t)set.nCU * (size_t)std::max(perCU, 1), nGroups));
  const size_t L = (size_t)S;
  auto slotBytes = [&](size_t c) { return c * rowBytes + (L + c - 1) / c * ckptBytes; };
  size_t C = L, bytes = rowBytes;
  if (keepRows) {
    size_t cMin = std::min(L, std::max<size_t>(1, (size_t)std::ceil(cMinFactor * std::sqrt((double)L))));
    if (set.chunkSites) {
      cMin = std::min<size_t>(set.chunkSites, L);
    }
    slots = std::min<size_t>(slots, (size_t)(budget.hard / slotBytes(cMin)));
    if (slots == 0) {
      why = refusal;
      return FSMC_ENOMEM;
    }
    if (set.chunkSites) {
      C = cMin;
    } else {
      const uint64_t room = L <= 512 ? budget.hard : budget.soft;
      while (C > cMin && (uint64_t)slots * slotBytes(C) > room) {
        C = std::max(cMin, (C + 1) / 2);
      }
    }
    bytes = slotBytes(C);
  }
  plan = LaunchPlan();
  plan.chunk = (int)C;
  plan.chunkRows = (int)C;
  plan.maxChunks = (int)((L + C - 1) / C);
  plan.wsSlot = bytes / kFloat4Bytes;
  plan.slots = (int)slots;
  plan.wavesPerWindow = 1;
  plan.bytes = bytes * slots;
  return FSMC_OK;
}

// The Viterbi kernel (fsmc_pair_viterbi.h): rows of back-pointers (KT4 x 64 dwords a site) and a checkpoint (KT4 x 64
// float4) a chunk, so memory is chunk + 4 x S / chunk rows and the smallest slot has about 2 sqrt(S) sites a chunk;
// without state rows (`wantStates` false) one row.  `member`: the kernel's family member.
inline int planViterbi(const Settings& set, int S, int member, int perCU, size_t nGroups, bool wantStates,
                       const WsBudget& budget, LaunchPlan& plan, std::string& why)
{
  const size_t K4 = (size_t)(member + 3) / 4;
  return planReplay(set, S, perCU, nGroups, K4 * kWave * sizeof(uint32_t), K4 * kWave * kFloat4Bytes, 2.0, wantStates,
                    "workspace limit too small for the back-pointers of one wave", budget, plan, why);
}

// The sampling kernel (fsmc_pair_samples.h) and the transition kernel (fsmc_pair_transitions.h): rows of forward vectors
// (KT4 x 64 float4 a site) and a checkpoint of the same size a chunk, so memory is chunk + S / chunk rows and the
// smallest slot has about sqrt(S) sites a chunk.
inline int planSamples(const Settings& set, int S, int member, int perCU, size_t nGroups, const WsBudget& budget,
                       LaunchPlan& plan, std::string& why)
{
  const size_t row = (size_t)(member + 3) / 4 * kWave * kFloat4Bytes;
  return planReplay(set, S, perCU, nGroups, row, row, 1.0, true,
                    "workspace limit too small for the forward rows of one wave", budget, plan, why);
}

// A launch of the two-waves-per-window kernel, if this one qualifies: `nItems` workgroups (groups; batches of the sums)
// that are ALL resident at once -- so the launch has at most half as many items as the chip holds waves of this member,
// the case in which the one-wave kernel leaves every wave alone on a SIMD (or SIMDs idle) -- and whose whole windows fit
// the workspace (to - from rows a workgroup; the same rule as planOneWave's whole windows: inside the hard budget, and
// inside what the context has earned unless the window is no longer than a chunk would be).
// allResident: the first half, `perCU` the kernel's workgroups a CU (capWorkgroups); planTwoWaves: the plan of kernel
// member `member` over the work list `groups`, false if it does not fit.
inline bool allResident(const Settings& set, int perCU, size_t nItems)
{
  return perCU >= 1 && nItems <= (size_t)set.nCU * perCU;
}

inline bool planTwoWaves(const std::vector<fsmc_group>& groups, int member, size_t nItems, const WsBudget& budget,
                         LaunchPlan& plan)
{
  size_t L = 1;
  for (const fsmc_group& g : groups) {
    L = std::max<size_t>(L, g.to - g.from);
  }
  const size_t K4 = (size_t)(member + 3) / 4;
  plan = LaunchPlan();
  plan.chunk = (int)L;
  plan.chunkRows = (int)L;
  plan.maxChunks = 1;
  plan.wsSlot = L * K4 * kWave;
  plan.slots = (int)nItems;
  plan.wavesPerWindow = 2;
  plan.bytes = plan.wsSlot * kFloat4Bytes * nItems;
  return plan.bytes <= budget.hard && (plan.bytes <= budget.soft || L <= 512);
}

// What output staging beside the workspace may take (the sums' planes, the pair posteriors' slices): the caller's
// workspace limit or a quarter of the card, and no more than 1/`parts` of what the card has free -- `held`, the staging
// this context holds already, counted as free -- beside a reserve of 2 GiB.
inline uint64_t stagingLimit(const Settings& set, const MemInfo& mem, uint64_t held, unsigned parts)
{
  uint64_t limit = set.wsLimit ? set.wsLimit : (uint64_t)(0.25 * (double)set.hbmBytes);
  if (mem.known) {
    const uint64_t room = mem.freeBytes + held;
    const uint64_t reserve = 2ull << 30;
    limit = std::min<uint64_t>(limit, room > reserve ? (room - reserve) / parts : 0);
  }
  return limit;
}

// The sums: the batches a launch may stage, `stagingPerItem` bytes of output each beside the workspace -- what `limit`
// (stagingLimit) holds, one at the least, and FSMC_DIAG_SUMS_SLOTS.
inline size_t stagedItems(uint64_t limit, size_t stagingPerItem, const Diag& diag)
{
  return lowered(std::max<size_t>(1, (size_t)(limit / stagingPerItem)), diag.sumsSlots);
}

// The sums' beta stride, left to the library: stride 2 pays where the launch fills the chip (C2: 2762 -> 2454 ms: the
// rows' traffic was the bound); a wave alone on its SIMD only gets the recomputed half sweep on top (C1 shape: 41.2 ->
// 43.3 ms).  A launch of fewer batches than the chip holds waves (`perCU` a CU, of the stride-2 kernel) keeps stride 1.
inline bool sumsKeepStrideOne(const Settings& set, int perCU, size_t nBatches)
{
  return perCU >= 1 && nBatches < (size_t)set.nCU * (size_t)perCU;
}

// The work list in slices of groups, as the fsmc_decode_pair_* entry points send it through the device.
struct Slices {
  const std::vector<fsmc_group>* list = nullptr; // the work list: it outlives the slices
  size_t slice = 0;         // groups a slice (the last one may have fewer)
  size_t nSlices = 0;
  size_t slicePairsMax = 0; // pairs of the largest slice

  size_t firstGroup(size_t sl) const { return sl * slice; }
  size_t groups(size_t sl) const { return std::min(slice, list->size() - sl * slice); }
  size_t firstPair(size_t sl) const { return (*list)[firstGroup(sl)].first_pair; }
  size_t pairs(size_t sl) const
  {
    const fsmc_group& last = (*list)[firstGroup(sl) + groups(sl) - 1];
    return (size_t)last.first_pair + last.n_pairs - firstPair(sl);
  }
};

// The slices of a call over `list` (not empty).  The slice is the caller's setting (`setting` groups, 0 = automatic), or
// what `staging` bytes -- stagingLimit of half the room the card has free, read only when the slice is automatic -- hold
// of `groupBytes` a group, and `sliceMost` groups at the most.
inline void planSlices(const std::vector<fsmc_group>& list, size_t setting, uint64_t staging, size_t groupBytes,
                       size_t sliceMost, Slices& s)
{
  size_t slice = setting;
  if (slice == 0) {
    slice = (size_t)(staging / groupBytes);
  }
  s.list = &list;
  s.slice = std::max<size_t>(1, std::min({slice, list.size(), sliceMost}));
  s.nSlices = (list.size() + s.slice - 1) / s.slice;
  s.slicePairsMax = 0;
  for (size_t sl = 0; sl < s.nSlices; ++sl) {
    s.slicePairsMax = std::max(s.slicePairsMax, s.pairs(sl));
  }
}

// Two half-groups per wavefront.  A group of at most 32 pairs (a hashing-mode batch) fills half a wave; two of them can
// share one if the wave walks the union of their windows (decode_kernel<..., DUAL>).  Worth it when the union is not
// much longer than the longer window: groups are sorted by (window length, from) and neighbours are paired while the
// union stays within 1.25 x the longer one.  Returns false when the
// list does not call for it (no half-full groups, or all of them were packed by the caller already).
inline bool buildDualItems(const std::vector<fsmc_group>& groups, std::vector<fsmc_group>& items,
                           std::vector<fsmc_group>& unions, std::vector<fsmc_group>& rest)
{
  // half-full groups whose window (and so the union with a neighbour of the same length class) is within `maxLen`
  // are candidates (the paired kernel decodes in chunks too, so this is no real bound any more: how long a window may
  // be is no longer a question of memory); everything else -- full groups -- runs as uploaded, in a second kernel
  constexpr uint32_t maxLen = 1u << 30;
  std::vector<uint32_t> small;
  for (size_t g = 0; g < groups.size(); ++g) {
    if (groups[g].n_pairs <= 32 && (uint64_t)(groups[g].to - groups[g].from) * 5 <= (uint64_t)maxLen * 4) {
      small.push_back((uint32_t)g);
    }
  }
  if (small.size() < 2) {
    return false;
  }
  // neighbours after this sort have windows of (nearly) the same length that start close to each other: the union a
  // pair walks is then little longer than either window (lengths are compared in 64-site steps, the hashing word)
  std::sort(small.begin(), small.end(), [&](uint32_t x, uint32_t y) {
    const fsmc_group &a = groups[x], &b = groups[y];
    const uint32_t la = (a.to - a.from + 63) / 64, lb = (b.to - b.from + 63) / 64;
    return la != lb ? la < lb : a.from != b.from ? a.from < b.from : x < y;
  });
  items.clear();
  unions.clear();
  rest.clear();
  std::vector<char> taken(groups.size(), 0);
  for (size_t i = 0; i + 1 < small.size();) {
    const fsmc_group &a = groups[small[i]], &b = groups[small[i + 1]];
    const uint32_t lenA = a.to - a.from, lenB = b.to - b.from;
    const uint32_t lenU = std::max(a.to, b.to) - std::min(a.from, b.from);
    if ((uint64_t)lenU * 4 <= (uint64_t)std::max(lenA, lenB) * 5 && lenU <= maxLen) {
      items.push_back(a);
      items.push_back(b);
      fsmc_group u = a;
      u.from = std::min(a.from, b.from);
      u.to = std::max(a.to, b.to);
      u.scan_from = std::min(a.scan_from, b.scan_from);
      u.scan_to = std::max(a.scan_to, b.scan_to);
      unions.push_back(u);
      taken[small[i]] = taken[small[i + 1]] = 1;
      i += 2;
    } else {
      i += 1;
    }
  }
  if (unions.empty()) {
    return false;
  }
  // A half-full group that found no partner but fits the layout rides in the same kernel as an item of its own (B
  // empty): one queue, longest window first, instead of a second kernel whose long windows finish whenever the
  // hardware got round to starting them.  What does not fit (more than 32 pairs, a window beyond the budget) is `rest`.
  for (size_t g = 0; g < groups.size(); ++g) {
    if (taken[g]) {
      continue;
    }
    const fsmc_group& a = groups[g];
    if (a.n_pairs <= 32 && a.to - a.from <= maxLen) {
      fsmc_group none = a;
      none.n_pairs = 0;
      items.push_back(a);
      items.push_back(none);
      unions.push_back(a);
    } else {
      rest.push_back(a);
    }
  }
  // the waves pull the items longest first
  std::vector<uint32_t> order(unions.size());
  for (size_t i = 0; i < order.size(); ++i) {
    order[i] = (uint32_t)i;
  }
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
    return unions[x].scan_to - unions[x].from > unions[y].scan_to - unions[y].from;
  });
  std::vector<fsmc_group> items2(items.size()), unions2(unions.size());
  for (size_t i = 0; i < order.size(); ++i) {
    unions2[i] = unions[order[i]];
    items2[2 * i] = items[2 * order[i]];
    items2[2 * i + 1] = items[2 * order[i] + 1];
  }
  items.swap(items2);
  unions.swap(unions2);
  return true;
}

// Longest window first: the decode ends when the last wave does, and a wave that pulls a long window late in the
// queue runs on alone.  (The order of the queue is free: records are keyed by pair and sorted at fetch.)
// Returns false when the list already is in that order (every window the same length, as in the all-pairs modes).
inline bool longestFirst(std::vector<fsmc_group>& list)
{
  auto len = [](const fsmc_group& g) { return g.scan_to - g.from; };
  bool ordered = true;
  for (size_t i = 1; i < list.size() && ordered; ++i) {
    ordered = len(list[i]) <= len(list[i - 1]);
  }
  if (ordered) {
    return false;
  }
  std::stable_sort(list.begin(), list.end(), [&](const fsmc_group& a, const fsmc_group& b) { return len(a) > len(b); });
  return true;
}

// Member of the wave-group kernel for a model of K states: {waves per group, states per wave}.  Up to 320 states four
// waves (48, 64: two workgroups per CU; 80: one, with the whole register file); beyond, six to eight waves of 64 states;
// beyond 512 states eight waves of 80 / 96 / 128 states, which have no landing zones for the beta row (they would not
// fit the CU's LDS) and hold part of their vectors in scratch memory (round 5: K = 600 0.03 -> 0.28 of the roofline).
// (Three / four waves of 128 states for 321 ... 512 states were measured too: 1.5 x slower than six / eight of 64,
// profiles/r05_w2_wide_members_of_128.txt.)
// (Measured on the 600 x 3000 list, profiles/r04_wide_members_ab.txt: five waves of 64 are 6 % slower than four of 80
// at 300 / 320 states; four waves of 96 / 112 states -- round 4's first members for 321 ... 448 states, which keep part
// of their vectors in scratch memory -- 10 - 13 % slower than six / seven waves of 64.)
// `built`: the members the library is built with (FSMC_ALL_W2), which the diagnostic override picks from.
struct W2Member {
  int NW, KH;
};
inline W2Member w2Member(int K, const Diag& diag, const std::vector<W2Member>& built)
{
  // (diagnostic: FSMC_DIAG_W2_MEMBER="<waves>x<states per wave>" picks another member that holds the model -- A/B runs)
  const int nw = diag.w2NW, kh = diag.w2KH;
  // (a member whose waves the model fills all but the last of, or the 48-state one: where the kernel masks ghosts)
  if ((nw != 0 || kh != 0) && nw * kh >= K &&
      ((nw - 1) * kh < K || (kh == 48 && 2 * kh < K) || (nw * kh > 512 && (nw - 2) * kh < K))) {
    for (const W2Member& b : built) {
      if (kh == b.KH && nw == b.NW) {
        return {nw, kh};
      }
    }
  }
  if (K <= 192) return {4, 48};
  if (K <= 256) return {4, 64};
  if (K <= 320) return {4, 80};
  if (K <= 384) return {6, 64};
  if (K <= 448) return {7, 64};
  if (K <= 512) return {8, 64};
  // beyond 512 states: eight waves without landing zones (fsmc_kernels_w2.h, LAND)
  if (K <= 640) return {8, 80};
  if (K <= 768) return {8, 96};
  return {8, 128};
}
} // namespace plan
} // namespace fsmc
