// fsmc_kernels.h -- device side of libfastsmc_hip.so: the pairwise-HMM decode kernel for gfx950.
//
// Mapping: lane = haplotype pair, one wavefront = one reference batch of <= 64 pairs
// that share a decode window; the K states are walked sequentially by every lane, so every sum and
// recurrence is evaluated in the reference's order (NO_SSE variant) and results are
// bit-identical to the CPU path.  No FMA contraction (-ffp-contract=off), IEEE division.
//
// Per wave, per group:
//   pass B : beta sweep, site to-1 down to from; keeps only checkpoints every `chunk` sites
//            (or every beta when the whole window fits the workspace: single-chunk mode)
//   pass A : for each chunk, ascending: recompute the chunk's betas from the checkpoint into the
//            wave's private chunk buffer (HBM), then the alpha sweep through the chunk, fusing
//            combine/normalise and the posterior consumer (IBD scan / dump / per-pair / sums).
// Algorithmic HBM traffic: one 4*K-byte beta row written and read once per pair-site (8K + 0.25 B).
//
// Reference statements this follows (ASMC_SRC/SRC): HMM.cpp:725-784 + 787-830 (forward),
// 882-940 + 943-1016 (backward), 669-692 (combine), HmmUtils.cpp:102-151 (scaling),
// HMM.cpp:1179-1357 (IBD scan), 1087-1107 (segment age estimates).
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/fastsmc_hip.h"
#include "fsmc_constants.h"

namespace fsmc
{

constexpr int kWave = 64;

// Read-only, wave-uniform model data is addressed through the constant address space: the compiler
// may then use scalar (SMEM) loads into SGPRs instead of per-lane vector loads + v_readfirstlane.
// Valid because nothing in a launch ever writes these buffers.
typedef const float __attribute__((address_space(4))) * cfloat_p;
typedef const int __attribute__((address_space(4))) * cint_p;
typedef const unsigned __attribute__((address_space(4))) * cuint_p;
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
// (kMaxStates, kMaxStatesW2, kMaxStatesAny -- how wide a model each kernel family takes: fsmc_constants.h)

enum Mode : int { kModeIbd = 0, kModeDump = 1, kModePerPair = 2, kModeSums = 3 };

struct KParams {
  int K;       // states
  int KP;      // padded row stride of the tables (multiple of 4)
  int S;       // sites
  int W;       // 64-bit words per haplotype row
  int nGroups;
  int groupBase; // kModeSums: this launch decodes batches groupBase .. groupBase + gridDim.x - 1, one per wave;
                 // other modes: which of `counters` is this launch's queue head
  int chunk;   // sites per chunk (C)
  int chunkRows; // rows of the chunk buffer: C, or (C+1)/2 with beta stride 2
  int maxChunks;
  unsigned flags;
  const float* pi;    // [KP]
  const float* cR;    // [KP]
  const float* expT;  // [KP]
  const float* D;     // [rows][KP]
  const float* B;
  const float* U;
  const float* rowSets; // [rows][5][KP]: D | B | U | Ush | RR of one key side by side, Ush[k] = U[k-1] (packed steps)
  const float* RR;
  const float* ghostMask; // [KP] 1.0f for the K real states, 0.0f for the padding states (padded family members)
  const int* stepRow; // [S] row of the step into site q (array mode); sequence mode: the site step, forward
  const int* rowGapF; // sequence mode only: rows of the half-step across the gap (q-1, q), forward
  const int* rowSiteB; //                     site step, backward (out of site q)
  const int* rowGapB;  //                     gap half-step, backward
  const float4* emis3; // [S][3][KP/4]: emission rows for obs class het / hom-major / hom-minor
  const unsigned long long* haps; // [nHaps][W]
  const fsmc_pair* pairs;
  const fsmc_group* groups;
  unsigned* counters; // [groupBase] head of the group queue the launch pulls from (0, or 2 beside another launch), [1] IBD record count
  float4* ws;         // workspace, wsSlot float4 per resident wave
  size_t wsSlot;
  unsigned stateThr, ageThr;
  unsigned spsLds; // decode_kernel, TRACK: the launch carries dynamic LDS for the open segments' per-state sums
  float thr[4];       // {1000,100,10,1} * probabilityThreshold, evaluated in fp32 (HMM.cpp:1226...)
  fsmc_ibd_record* recs;
  unsigned recCap;
  float* dumpOut;             // kModeDump
  const size_t* dumpOffsets;  // [nGroups] float offsets
  float* ppMean;              // kModePerPair: [nPairs][S]
  int* ppMap;                 // kModePerPair: [nPairs][S]
  const float* expCoal;       // kModePerPair: [KP]
  unsigned long long* phaseCycles; // diagnostic builds (-DFSMC_PHASE_STAMPS): [0] pass B, [1] rebuild, [2] alpha sweep, [3] groups
  float* sums;                // kModeSums: one plane [S][K] (x4 with the 00/01/11 sums) per wave of the launch
  size_t sumsPlane;           // floats per plane
  size_t sumsSlot;            // floats per slot (wave / workgroup of the launch): one plane, or four with the 00/01/11 sums
  const unsigned* batchFirst; // kModeSums: [nBatches + 1] first group of every batch (null: every group is a batch)
  int residentChunks;         // chunked windows, array mode: the first this-many chunks of a window keep the rows pass B
                              // computes for them (a chunk buffer each) and skip the rebuild pass
};
// decode_kernel_pool: the resident chunk buffers of all waves of the launch as one pool behind the slots of the workspace
// (residentChunks is then the pool's buffers per wave).  A wave claims a buffer for a chunk in pass B and gives it back
// when pass A has swept the chunk.
struct KParamsPool : KParams {
  size_t poolOff;             // float4 from `ws` to the pool's first buffer (a buffer: chunkRows rows)
  unsigned poolBuffers;       // buffers in the pool
  int poolCap;                // only the chunks below this index of a window ask for a buffer
  unsigned* poolState;        // [kPoolCursor, kPoolKept, kPoolRebuilt, unused][poolBuffers claim words], zero at launch
};
enum { kPoolCursor = 0, kPoolKept = 1, kPoolRebuilt = 2, kPoolClaims = 4 };
constexpr int kPoolProbes = 4; // claim words a wave tries for one chunk before it settles for the rebuild

// ---------------------------------------------------------------------------------------------
// Scalar operand streaming.  The k-loops of a step are walked in blocks; each block needs a few
// wave-uniform table values, fetched with hand-placed scalar loads into SGPRs, and this lane's emission
// values (float4 reads from the LDS ring).  The loads of block i+1 are issued right after the wait for
// block i, so that scalar-cache / LDS latency hides under the arithmetic of block i.  Scalar loads are
// inline asm because the compiler otherwise merges and hoists them to the top of the sweep (hundreds
// of spilled SGPRs) -- it cannot see these loads, so each result is only read after an explicit
// s_waitcnt that names it as an in/out operand.  (Waits the compiler inserts for its own LDS reads stay
// correct: extra outstanding scalar loads only make a counted lgkmcnt wait stricter.)
// None of this changes the per-lane order of floating-point operations.
// (hipcc also parses kernel bodies in its host pass, where gfx950 asm constraints do not exist)
#if defined(__HIP_DEVICE_COMPILE__)
#define FSMC_GCN_ASM(...) asm volatile(__VA_ARGS__)
#else
#define FSMC_GCN_ASM(...) ((void)0)
#endif

// The same loads with the block's byte offset as an instruction immediate (compile-time K: the unrolled block
// index is a constant by the time the instruction is selected) -- no scalar address arithmetic per load.
__device__ __forceinline__ f32x4 sload4(cfloat_p p, const int byteOff)
{
  f32x4 v = {};
  FSMC_GCN_ASM("s_load_dwordx4 %0, %1, %2" : "=s"(v) : "s"(p), "i"(byteOff));
  return v;
}
__device__ __forceinline__ f32x8 sload8(cfloat_p p, const int byteOff)
{
  f32x8 v = {};
#if defined(FSMC_DIAG_NOSMEM)
  FSMC_GCN_ASM("; no load %0 %1 %2" : "=s"(v) : "s"(p), "i"(byteOff));
#else
  FSMC_GCN_ASM("s_load_dwordx8 %0, %1, %2" : "=s"(v) : "s"(p), "i"(byteOff));
#endif
  return v;
}
// Scalar-cache warm-up.  A table row spans five 64-byte lines; most of them miss the 16-KB scalar cache (16 waves
// share it, each at its own site), and because scalar loads return out of order the operand stream can only wait
// for everything at once -- every block would pay a miss.  touchLines requests one dword of each remaining line of
// a row together with the pass's first operand block: the pass's first wait then covers all the misses in
// parallel and the later blocks hit.  The destination registers are only reserved: they are handed to the next
// wait (swaitTouched) as operands so that nothing else lives in them while the loads are in flight.
#if defined(FSMC_NO_TOUCH)
constexpr bool kTouch = false;
#else
constexpr bool kTouch = true;
#endif
struct Touched {
  float r[4];
};
template <int FIRST, int STEP = 16>
__device__ __forceinline__ void touchLines(Touched& t, cfloat_p p, const int firstState)
{
  // lines FIRST, FIRST+1, ... (up to four) of the row that starts at state firstState; STEP = floats per line
  FSMC_GCN_ASM("s_load_dword %0, %4, %5\n\ts_load_dword %1, %4, %6\n\ts_load_dword %2, %4, %7\n\ts_load_dword %3, %4, %8"
               : "=&s"(t.r[0]), "=&s"(t.r[1]), "=&s"(t.r[2]), "=&s"(t.r[3]) // early clobber: never the address pair
               : "s"(p), "i"((firstState + FIRST * STEP) * 4), "i"((firstState + (FIRST + 1) * STEP) * 4),
                 "i"((firstState + (FIRST + 2) * STEP) * 4), "i"((firstState + (FIRST + 3) * STEP) * 4));
}
__device__ __forceinline__ void holdTouched(Touched& a)
{
  FSMC_GCN_ASM("" : "+s"(a.r[0]), "+s"(a.r[1]), "+s"(a.r[2]), "+s"(a.r[3]));
}
#define FSMC_SWAIT_INSN "s_waitcnt lgkmcnt(0)"
__device__ __forceinline__ void swait(f32x8& a, f32x8& b)
{
  FSMC_GCN_ASM(FSMC_SWAIT_INSN : "+s"(a), "+s"(b));
}
__device__ __forceinline__ void swait(f32x16& a, f32x16& b)
{
  FSMC_GCN_ASM(FSMC_SWAIT_INSN : "+s"(a), "+s"(b));
}
__device__ __forceinline__ void swait(f32x8& a, f32x8& b, f32x8& c, f32x8& d)
{
  FSMC_GCN_ASM(FSMC_SWAIT_INSN : "+s"(a), "+s"(b), "+s"(c), "+s"(d));
}
// block-width dispatch so the block sizes below are tunable
template <int N> struct SV;
template <> struct SV<4> {
  typedef f32x4 T;
  static __device__ __forceinline__ T loadAt(cfloat_p p, const int firstState) { return sload4(p, firstState * 4); }
};
template <> struct SV<8> {
  typedef f32x8 T;
  static __device__ __forceinline__ T loadAt(cfloat_p p, const int firstState) { return sload8(p, firstState * 4); }
};
template <> struct SV<16> {
  typedef f32x16 T;
  static __device__ __forceinline__ T loadAt(cfloat_p p, const int firstState)
  {
    f32x16 v = {};
#if defined(FSMC_DIAG_NOSMEM) // timing experiment only (results are wrong): operands are whatever the registers hold
    FSMC_GCN_ASM("; no load %0 %1 %2" : "=s"(v) : "s"(p), "i"(firstState * 4));
#else
    FSMC_GCN_ASM("s_load_dwordx16 %0, %1, %2" : "=s"(v) : "s"(p), "i"(firstState * 4));
#endif
    return v;
  }
};
__device__ __forceinline__ void swait(f32x4& a, f32x4& b, f32x4& c, f32x4& d)
{
  FSMC_GCN_ASM(FSMC_SWAIT_INSN : "+s"(a), "+s"(b), "+s"(c), "+s"(d));
}

#if defined(FSMC_WAIT_STAMPS)
#define FSMC_SWAIT(acc, ...)                                                                                           \
  do {                                                                                                                 \
    const long long t0_ = (long long)clock64();                                                                        \
    swait(__VA_ARGS__);                                                                                                \
    (acc) += (long long)clock64() - t0_;                                                                               \
  } while (0)
#else
#define FSMC_SWAIT(acc, ...) swait(__VA_ARGS__)
#endif

#ifndef FSMC_KB
#define FSMC_KB 16
#endif
#ifndef FSMC_KBF
#define FSMC_KBF 8
#endif
constexpr int kKB = FSMC_KB;   // states per operand block of the beta passes (two tables at a time)
constexpr int kKBF = FSMC_KBF; // states per operand block of the alpha pass (four tables at a time)
// (kKPad, the padding of table / emission rows, and RowSetPart, the parts of a RowSet [key][5][KP]: fsmc_constants.h)

__device__ __forceinline__ float pick(const float4& e0, const float4& e1, const int i)
{
  return i == 0 ? e0.x : i == 1 ? e0.y : i == 2 ? e0.z : i == 3 ? e0.w : i == 4 ? e1.x : i == 5 ? e1.y : i == 6 ? e1.z : e1.w;
}

template <int N> struct EmisBlk { // this lane's emission values of one operand block (N/4 float4 from LDS)
  float4 v[N / 4];
  __device__ __forceinline__ float at(const int i) const
  {
    const float4& q = v[i >> 2];
    return (i & 3) == 0 ? q.x : (i & 3) == 1 ? q.y : (i & 3) == 2 ? q.z : q.w;
  }
  __device__ __forceinline__ f32x2 pair(const int i) const // values i, i+1 (i even): one 64-bit register pair
  {
    const float4& q = v[i >> 2];
    const f32x2 lo = {q.x, q.y}, hi = {q.z, q.w};
    return (i & 2) == 0 ? lo : hi;
  }
};
// Two-state products and sums: one packed instruction each, or (-DFSMC_UNPACK, an experiment switch) two plain ones.
// Same IEEE operations either way.
__device__ __forceinline__ f32x2 pmul(const f32x2 a, const f32x2 b)
{
#if defined(FSMC_UNPACK)
  const f32x2 r = {a.x * b.x, a.y * b.y};
  return r;
#else
  return a * b;
#endif
}
__device__ __forceinline__ f32x2 padd(const f32x2 a, const f32x2 b)
{
#if defined(FSMC_UNPACK)
  const f32x2 r = {a.x + b.x, a.y + b.y};
  return r;
#else
  return a + b;
#endif
}
// values i, i+1 (i even) of a scalar operand block: an aligned SGPR pair
template <typename V> __device__ __forceinline__ f32x2 pairOf(const V& v, const int i)
{
  const f32x2 r = {v[i], v[i + 1]};
  return r;
}
template <int N> __device__ __forceinline__ EmisBlk<N> readEmis(const float4* e, const int blk)
{
  EmisBlk<N> r;
#pragma unroll
  for (int j = 0; j < N / 4; ++j) {
#if defined(FSMC_DIAG_NOEMIS) // timing experiment only (results are wrong): no LDS read, the values are undefined
    FSMC_GCN_ASM("; no read" : "=v"(r.v[j].x), "=v"(r.v[j].y), "=v"(r.v[j].z), "=v"(r.v[j].w) : "v"(e));
#else
    r.v[j] = e[blk * (N / 4) + j];
#endif
  }
  return r;
}

// Diagnostic builds only (never in the shipped library): where a wave's cycles go.
//   -DFSMC_WAIT_STAMPS    cycles parked in the operand waits of the step functions
//   -DFSMC_REGION_STAMPS  cycles per code region: FSMC_END(dg, id) charges the time since the previous stamp to region
//                         id (s_memtime, low 32 bits; the accumulators are flushed once per group)
constexpr int kDiagRegions = 30; // (the wave-group kernel stamps 30 regions per wave role: fsmc_kernels_w2.h)
constexpr int kPhaseSlots = 8 + 4 * kDiagRegions; // entries of KParams::phaseCycles
struct Diag {
  long long waitCycles = 0;
#if defined(FSMC_REGION_STAMPS)
  unsigned acc[kDiagRegions] = {};
  unsigned last = 0;
#endif
};
#if defined(FSMC_REGION_STAMPS)
#define FSMC_END(dg, id)                                                                                               \
  do {                                                                                                                 \
    const unsigned now_ = (unsigned)__builtin_readcyclecounter();                                                      \
    (dg).acc[id] += now_ - (dg).last;                                                                                  \
    (dg).last = now_;                                                                                                  \
  } while (0)
#else
#define FSMC_END(dg, id) ((void)0)
#endif

// ---------------------------------------------------------------------------------------------
// The two steps, K a compile-time parameter (the kernel family, fsmc_instances.h).  One step of the backward recursion
// for one pair is HMM.cpp:957-1016 (NO_SSE association), of the forward recursion HMM.cpp:799-830 followed by the
// per-site scaling (HmmUtils.cpp:102-151).  gfx950 multiplies / adds two fp32 values per lane in one
// VALU instruction (v_pk_mul_f32, v_pk_add_f32) when both sit in an aligned register pair.  Every operation of a
// step that is not part of a first-order recurrence is done for states (k, k+1) at once; the recurrences (BU, BL,
// AU, the suffix sum, the scaling sum) stay scalar and sequential.  Each value is produced by the same IEEE
// operation on the same operands as in the scalar step (no FMA, no re-association), so the results are
// bit-identical; only ~7.5 instead of 11 VALU instructions are issued per state.
//
// Operand delivery.  One operand block = kKB (beta) / kKBF (alpha) states: the block's table values
// (scalar loads into SGPRs, inline asm) AND this lane's emission values of the same states (LDS reads) are
// requested together, a whole block ahead, right after the single wait that opens the block before.  That wait is the
// s_waitcnt BUILTIN, not inline asm: the compiler's wait-count pass sees it, marks its own LDS reads complete and
// inserts no counted lgkmcnt wait of its own inside a step.  (It cannot see the asm scalar loads, which share the
// counter and return out of order: a counted wait it placed for an LDS value right behind a freshly issued prefetch
// waited for that prefetch as well -- every block paid a full scalar-load latency.)
//
// Ghost states (GHOST = true: K < KT, KT a multiple of kKPad).  States K..KT-1 have zero table, emission and prior
// entries; their values stay exactly +0 through every operation and a sum that adds +0 in state order is the same
// sum.  The one exception, beta'[k] = (BL + D*vec) + BU = BL for a ghost, is multiplied by a 1/0 mask row (states of
// the last operand block only) before the scaling sum -- x * 1.0f is exact.  The reference's boundary cases
// (BU[K-1] = 0, no B term for the last state) come out of the same arithmetic: U*0 + RR*0 and B*0.
//
// Backward: the term U[k]*vec[k+1] of BU[k] is taken from T[m] = Ush[m]*vec[m] with Ush[m] = U[m-1]
// (a second copy of the U table shifted by one state), so that both factors share a state index.
__device__ __forceinline__ void waitLgkm0()
{
  __builtin_amdgcn_s_waitcnt(0xC07F); // lgkmcnt(0), vmcnt / expcnt left alone (gfx9 encoding)
}
__device__ __forceinline__ void waitVm0()
{
  __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0)
}
// After a wait: the registers of the scalar loads it covered are final.  Input-only on purpose -- an in/out ("+s")
// operand is a new value to the register allocator, which may then copy the load's destination into another
// register IN FRONT of the wait (observed: s_mov_b64 of sixteen in-flight SGPRs).  What keeps the uses behind the
// wait is the __builtin_amdgcn_sched_barrier(0) that follows every wait + prefetch group.
template <typename V> __device__ __forceinline__ void landed(const V& a, const V& b)
{
  FSMC_GCN_ASM("" ::"s"(a), "s"(b));
}
template <typename V> __device__ __forceinline__ void landed(const V& a, const V& b, const V& c, const V& d)
{
  FSMC_GCN_ASM("" ::"s"(a), "s"(b), "s"(c), "s"(d));
}
template <typename V> __device__ __forceinline__ void landed(const V& a)
{
  FSMC_GCN_ASM("" ::"s"(a));
}
// The wait that opens an operand block.  The scheduling barrier right behind it keeps register copies the allocator
// makes for the code below (post-RA scheduling included) from being hoisted in front of the wait.
#if defined(FSMC_WAIT_STAMPS) // (costs more than the waits it measures: its own switch, next to FSMC_PHASE_STAMPS)
#define FSMC_WAIT_OPERANDS(acc)                                                                                        \
  do {                                                                                                                 \
    const long long t0_ = (long long)clock64();                                                                        \
    waitLgkm0();                                                                                                       \
    (acc) += (long long)clock64() - t0_;                                                                               \
    __builtin_amdgcn_sched_barrier(0);                                                                                 \
  } while (0)
#else
#define FSMC_WAIT_OPERANDS(acc)                                                                                        \
  do {                                                                                                                 \
    waitLgkm0();                                                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                                                 \
  } while (0)
#endif

// Line warm-up generalised: COUNT (0..4) dwords, one per 64-byte line FIRST, FIRST+1, ... of the row at firstState.
template <int FIRST, int COUNT> __device__ __forceinline__ void touchRow(Touched& t, cfloat_p p, const int firstState)
{
  constexpr int STEP = 16;
  if constexpr (COUNT >= 4) {
    touchLines<FIRST, STEP>(t, p, firstState);
  } else if constexpr (COUNT == 3) {
    FSMC_GCN_ASM("s_load_dword %0, %3, %4\n\ts_load_dword %1, %3, %5\n\ts_load_dword %2, %3, %6"
                 : "=&s"(t.r[0]), "=&s"(t.r[1]), "=&s"(t.r[2])
                 : "s"(p), "i"((firstState + FIRST * STEP) * 4), "i"((firstState + (FIRST + 1) * STEP) * 4),
                   "i"((firstState + (FIRST + 2) * STEP) * 4));
  } else if constexpr (COUNT == 2) {
    FSMC_GCN_ASM("s_load_dword %0, %2, %3\n\ts_load_dword %1, %2, %4"
                 : "=&s"(t.r[0]), "=&s"(t.r[1])
                 : "s"(p), "i"((firstState + FIRST * STEP) * 4), "i"((firstState + (FIRST + 1) * STEP) * 4));
  } else if constexpr (COUNT == 1) {
    FSMC_GCN_ASM("s_load_dword %0, %1, %2" : "=&s"(t.r[0]) : "s"(p), "i"((firstState + FIRST * STEP) * 4));
  }
}
template <int COUNT> __device__ __forceinline__ void heldRow(const Touched& t)
{
  if constexpr (COUNT >= 4) {
    FSMC_GCN_ASM("" ::"s"(t.r[0]), "s"(t.r[1]), "s"(t.r[2]), "s"(t.r[3]));
  } else if constexpr (COUNT == 3) {
    FSMC_GCN_ASM("" ::"s"(t.r[0]), "s"(t.r[1]), "s"(t.r[2]));
  } else if constexpr (COUNT == 2) {
    FSMC_GCN_ASM("" ::"s"(t.r[0]), "s"(t.r[1]));
  } else if constexpr (COUNT == 1) {
    FSMC_GCN_ASM("" ::"s"(t.r[0]));
  }
}

// What a backward step has in flight when it opens: its first operand block (the top states of Ush and RR), the
// warm-up of those rows' other lines and the emission values of the same states.  Requested by beta_issue_pk ahead of
// operand-free work (the scaling multiply and the row store of the step before), consumed by beta_core_pk.
// Operand loads of the packed steps.  SY = false: asynchronous (the value is final behind the next operand wait; the
// compiled code is checked for instructions that touch the destination earlier, tools/check_inflight_sgprs.py).
// SY = true: load and wait in ONE asm statement -- nothing can come between, at the price of the latency at every
// block.  The sequence-mode kernels use it: their extra live scalars made the register allocator spill operand
// blocks right behind their loads (v_writelane of registers still in flight) in some instantiations.
template <int N, bool SY> struct LD {
  typedef typename SV<N>::T T;
  static __device__ __forceinline__ T loadAt(cfloat_p p, const int firstState)
  {
    if constexpr (!SY) {
      return SV<N>::loadAt(p, firstState);
    } else {
      T v = {};
      if constexpr (N == 16) {
        FSMC_GCN_ASM("s_load_dwordx16 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p), "i"(firstState * 4));
      } else if constexpr (N == 8) {
        FSMC_GCN_ASM("s_load_dwordx8 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p), "i"(firstState * 4));
      } else {
        FSMC_GCN_ASM("s_load_dwordx4 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p), "i"(firstState * 4));
      }
      return v;
    }
  }
};

template <int KT> struct BetaOps {
  typename SV<kKB>::T u, rr;
  Touched tu, trr;
  EmisBlk<kKB> em;
};

template <int KT, bool SY = false>
__device__ __forceinline__ void beta_issue_pk(BetaOps<KT>& o, cfloat_p rowSet, const float4* e)
{
  constexpr int KPc = ((KT + kKPad - 1) / kKPad) * kKPad;
  constexpr int NB = (KT + kKB - 1) / kKB;
  constexpr int NLINES = KPc / 16;
  o.u = LD<kKB, SY>::loadAt(rowSet, kRowUsh * KPc + (NB - 1) * kKB);
  o.rr = LD<kKB, SY>::loadAt(rowSet, kRowRR * KPc + (NB - 1) * kKB);
  if constexpr (kTouch && !SY) {
    touchRow<0, NLINES - 1>(o.tu, rowSet, kRowUsh * KPc);
    touchRow<0, NLINES - 1>(o.trr, rowSet, kRowRR * KPc);
  }
  o.em = readEmis<kKB>(e, NB - 1);
}

// The recurrences of one backward step: on entry b = beta of site pos+1 (scaled), on exit w = the un-normalised
// beta of site pos and the return value its sum over the states (k ascending from 0.f); b is used up.
// SUM = false: the caller has the reciprocal of that sum already (a recomputed row of beta stride 2 whose neighbour
// carries it, fsmc_decode_kernel_body.h: kCarryScale) -- the same w, no sum, the return value is 0.f.
template <int KT, int KA, bool GHOST, bool SY = false, bool SUM = true>
__device__ __forceinline__ float beta_core_pk(float (&b)[KA], float (&w)[KA], BetaOps<KT>& ops, cfloat_p rowSet,
                                              const float4* e, cfloat_p ghostMask, Diag& dg)
{
  constexpr int K = KT;
  // the five table rows of one key sit side by side (RowSet): one base register, block offsets as immediates
  constexpr int KPc = ((KT + kKPad - 1) / kKPad) * kKPad;
  typedef typename SV<kKB>::T SVec;
  constexpr int NB = (K + kKB - 1) / kKB; // operand blocks (scalar loads + emission values, one block ahead)
  constexpr int R = kKB / 8;              // sub-blocks of 8 states per operand block
  constexpr int NLINES = KPc / 16;
  static_assert(kKB == 16, "line warm-up and ghost masking are laid out for operand blocks of one 64-byte line");
  static_assert(!GHOST || K % kKB == 0, "ghost padding fills whole operand blocks");
  // (no initialisers: a copy of a register whose scalar load is still in flight would read garbage; every one of
  //  these is assigned behind a wait before it is read -- the block loops are fully unrolled)
  SVec u, rr, nu, nrr;
  EmisBlk<kKB> em, nem;
  SVec d, bt, nd, nbt, mk;
  Touched td, tbt;
  float tcarry = 0.f; // T of the first state of the sub-block above
#pragma unroll
  for (int blk = NB - 1; blk >= 0; --blk) {
    FSMC_WAIT_OPERANDS(dg.waitCycles);
    if (blk == NB - 1) {
      landed(ops.u, ops.rr);
      if constexpr (kTouch && !SY) {
        heldRow<NLINES - 1>(ops.tu);
        heldRow<NLINES - 1>(ops.trr);
      }
      u = ops.u;
      rr = ops.rr;
      em = ops.em;
    } else {
      landed(nu, nrr);
      u = nu;
      rr = nrr;
      em = nem;
    }
    if (blk > 0) {
      nu = LD<kKB, SY>::loadAt(rowSet, kRowUsh * KPc + (blk - 1) * kKB);
      nrr = LD<kKB, SY>::loadAt(rowSet, kRowRR * KPc + (blk - 1) * kKB);
      nem = readEmis<kKB>(e, blk - 1);
    } else {
      d = LD<kKB, SY>::loadAt(rowSet, kRowD * KPc);
      bt = LD<kKB, SY>::loadAt(rowSet, kRowB * KPc);
      if constexpr (kTouch && !SY) {
        touchRow<1, NLINES - 1>(td, rowSet, kRowD * KPc);
        touchRow<1, NLINES - 1>(tbt, rowSet, kRowB * KPc);
      }
      if constexpr (GHOST && NB == 1) {
        mk = LD<kKB, SY>::loadAt(ghostMask, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int sbi = R - 1; sbi >= 0; --sbi) {
      const int sb = blk * R + sbi;
      const int o = sbi * 8; // offset of this sub-block inside the operand block
      if (sb * 8 >= K) {
        continue;
      }
      float T[9];
      T[8] = tcarry;
      // vec[k] = beta[k]*e[k] (kept in b), T[k] = U[k-1]*vec[k]
#pragma unroll
      for (int i = 0; i < 8; i += 2) {
        const int k = sb * 8 + i;
        if (k + 1 < K) {
          f32x2 v = {b[k], b[k + 1]};
          v = pmul(v, em.pair(o + i));
          const f32x2 t = pmul(pairOf(u, o + i), v);
          b[k] = v.x;
          b[k + 1] = v.y;
          T[i] = t.x;
          T[i + 1] = t.y;
        } else if (k < K) {
          b[k] = b[k] * em.at(o + i);
          T[i] = u[o + i] * b[k];
        }
      }
      // BU[k] = U[k]*vec[k+1] + RR[k]*BU[k+1], BU[K-1] = 0 (HMM.cpp:986-1005)
#pragma unroll
      for (int i = 7; i >= 0; --i) {
        const int k = sb * 8 + i;
        if (k < K) {
          if (k == K - 1) {
            w[k] = 0.f;
          } else {
            w[k] = T[i + 1] + rr[o + i] * w[k + 1];
          }
        }
      }
      tcarry = T[0];
    }
  }
  FSMC_END(dg, 2);
  // ascending: BL[k] = BL[k-1] + B[k-1]*vec[k-1];  beta'[k] = (BL[k] + D[k]*vec[k]) + BU[k]
  float BL = 0.f;
  float sum = 0.f;
#pragma unroll
  for (int blk = 0; blk < NB; ++blk) {
    FSMC_WAIT_OPERANDS(dg.waitCycles);
    if (blk > 0) {
      landed(nd, nbt);
      d = nd;
      bt = nbt;
    } else {
      landed(d, bt);
      if constexpr (kTouch && !SY) {
        heldRow<NLINES - 1>(td);
        heldRow<NLINES - 1>(tbt);
      }
    }
    if constexpr (GHOST) {
      if (blk == NB - 1) {
        landed(mk);
      }
    }
    if (blk + 1 < NB) {
      nd = LD<kKB, SY>::loadAt(rowSet, kRowD * KPc + (blk + 1) * kKB);
      nbt = LD<kKB, SY>::loadAt(rowSet, kRowB * KPc + (blk + 1) * kKB);
      if constexpr (GHOST) {
        if (blk + 1 == NB - 1) {
          mk = LD<kKB, SY>::loadAt(ghostMask, (NB - 1) * kKB);
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < kKB; i += 2) {
      const int k = blk * kKB + i;
      if (k + 1 < K) {
        const f32x2 v = {b[k], b[k + 1]};
        const f32x2 dv = pmul(pairOf(d, i), v);
        const f32x2 bv = pmul(pairOf(bt, i), v);
        f32x2 bl;
        bl.x = BL;
        bl.y = BL + bv.x;
        f32x2 x = padd(bl, dv);
        const f32x2 bu = {w[k], w[k + 1]};
        x = padd(x, bu);
        if constexpr (GHOST) {
          if (blk == NB - 1) {
            x = pmul(x, pairOf(mk, i));
          }
        }
        w[k] = x.x;
        w[k + 1] = x.y;
        if constexpr (SUM) {
          sum = sum + x.x;
          sum = sum + x.y;
        } else {
          // No instruction: the pair is final HERE.  The sum chain is what kept every state's adds in the block of their
          // operands; without it instruction selection parks the first states' adds behind the last block and the
          // operand registers they read (two blocks of sixteen SGPRs) are spilled and reloaded at every step.
          FSMC_GCN_ASM("" ::"v"(x.x), "v"(x.y));
        }
        BL =(k + 1 < K - 1) ? bl.y + bv.y : bl.y;
      } else if (k < K) {
        w[k] = (BL + d[i] * b[k]) + w[k];
        if constexpr (SUM) {
          sum = sum + w[k];
        }
        if (k < K - 1) {
          BL = BL + bt[i] * b[k];
        }
      }
    }
  }
  FSMC_END(dg, 3);
  return sum;
}

// The operand-free tail of a step (HmmUtils.cpp:102-151: scal = 1.0f/sum, vec *= scal): v = w * (1.0f / sum).
// With sum = 1.0f it is an exact copy (a loaded checkpoint, the un-normalised half-steps of sequence mode).
// Two forms: scale_by_pk takes the reciprocal c itself, scale_pk the sum -- and returns the reciprocal it used, for a
// caller that hands it on (kCarryScale, fsmc_decode_kernel_body.h).
template <int KT, int KA> __device__ __forceinline__ void scale_by_pk(float (&v)[KA], const float (&w)[KA], const float c)
{
  constexpr int K = KT;
  const f32x2 cc = {c, c};
#pragma unroll
  for (int k = 0; k < K; k += 2) {
    if (k + 1 < K) {
      const f32x2 x = {w[k], w[k + 1]};
      const f32x2 y = pmul(x, cc);
      v[k] = y.x;
      v[k + 1] = y.y;
    } else {
      v[k] = w[k] * c;
    }
  }
}
template <int KT, int KA> __device__ __forceinline__ float scale_pk(float (&v)[KA], const float (&w)[KA], const float sum)
{
  const float c = 1.0f / sum;
  scale_by_pk<KT, KA>(v, w, c);
  return c;
}

// A whole backward step in one piece (the sequence-mode passes and the recomputed rows of beta stride 2).
template <int KT, int KA, bool SCALE, bool GHOST, bool SY = false>
__device__ __forceinline__ void beta_step_pk(float (&b)[KA], float (&w)[KA], cfloat_p rowSet, const float4* e,
                                             cfloat_p ghostMask, Diag& dg)
{
  BetaOps<KT> ops;
  beta_issue_pk<KT, SY>(ops, rowSet, e);
  const float sum = beta_core_pk<KT, KA, GHOST, SY>(b, w, ops, rowSet, e, ghostMask, dg);
  if constexpr (SCALE) {
    scale_pk<KT, KA>(b, w, sum);
  } else {
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      b[k] = w[k];
    }
  }
}

// Forward.  The suffix sums are kept one slot down (w[k] = alphaC[k+1]) so that B[k]*alphaC[k+1] pairs up with the
// other products of state k; alphaC[0] is never used (HMM.cpp:799-830).
template <int KT, int KA, bool SCALE = true, bool SY = false>
__device__ __forceinline__ void alpha_step_pk(float (&a)[KA], float (&w)[KA], cfloat_p rowSet, cfloat_p cR,
                                              const float4* e, Diag& dg)
{
  constexpr int K = KT;
  constexpr int KPc = ((KT + kKPad - 1) / kKPad) * kKPad;
  static_assert(K >= 2, "packed step needs at least two states");
  typedef typename SV<kKBF>::T SVec;
  constexpr int NB = (K + kKBF - 1) / kKBF; // operand blocks (scalar loads + emission values, one block ahead)
  constexpr int NLINES = KPc / 16;
  SVec d = LD<kKBF, SY>::loadAt(rowSet, kRowD * KPc), bt = LD<kKBF, SY>::loadAt(rowSet, kRowB * KPc),
       u = LD<kKBF, SY>::loadAt(rowSet, kRowU * KPc), c4 = LD<kKBF, SY>::loadAt(cR, 0);
  Touched td, tbt, tu;
  if constexpr (kTouch && !SY) {
    touchRow<1, NLINES - 1>(td, rowSet, kRowD * KPc);
    touchRow<1, NLINES - 1>(tbt, rowSet, kRowB * KPc);
    touchRow<1, NLINES - 1>(tu, rowSet, kRowU * KPc);
  }
  SVec nd, nbt, nu, nc; // (assigned behind a wait before they are read; see beta_core_pk)
  EmisBlk<kKBF> em = readEmis<kKBF>(e, 0), nem;
  __builtin_amdgcn_sched_barrier(0);
  // operand-free: alphaC[k+1] = sum_{i>k} alpha[i], accumulated from the top (HMM.cpp:799-814)
  w[K - 2] = a[K - 1];
#pragma unroll
  for (int k = K - 2; k >= 1; --k) {
    w[k - 1] = w[k] + a[k];
  }
  float AU = 0.f;
  float sum = 0.f;
  FSMC_END(dg, 5);
#pragma unroll
  for (int blk = 0; blk < NB; ++blk) {
    FSMC_WAIT_OPERANDS(dg.waitCycles);
    if (blk > 0) {
      landed(nd, nbt, nu, nc);
      d = nd;
      bt = nbt;
      u = nu;
      c4 = nc;
      em = nem;
    } else {
      landed(d, bt, u, c4);
      if constexpr (kTouch && !SY) {
        heldRow<NLINES - 1>(td);
        heldRow<NLINES - 1>(tbt);
        heldRow<NLINES - 1>(tu);
      }
    }
    if (blk + 1 < NB) {
      nd = LD<kKBF, SY>::loadAt(rowSet, kRowD * KPc + (blk + 1) * kKBF);
      nbt = LD<kKBF, SY>::loadAt(rowSet, kRowB * KPc + (blk + 1) * kKBF);
      nu = LD<kKBF, SY>::loadAt(rowSet, kRowU * KPc + (blk + 1) * kKBF);
      nc = LD<kKBF, SY>::loadAt(cR, (blk + 1) * kKBF);
      nem = readEmis<kKBF>(e, blk + 1);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < kKBF; i += 2) {
      const int k = blk * kKBF + i;
      if (k + 1 < K - 1) {
        const f32x2 av = {a[k], a[k + 1]};
        const f32x2 da = pmul(pairOf(d, i), av);
        const f32x2 ua = pmul(pairOf(u, i), av);
        const f32x2 ac = {w[k], w[k + 1]};
        const f32x2 bw = pmul(pairOf(bt, i), ac);
        f32x2 au;
        au.x = AU;
        au.y = ua.x + c4[i] * AU; // AU of state k+1
        f32x2 term = padd(au, da);
        term = padd(term, bw);
        const f32x2 ov = pmul(em.pair(i), term);
        w[k] = ov.x;
        w[k + 1] = ov.y;
        sum = sum + ov.x;
        sum = sum + ov.y;
        AU = ua.y + c4[i + 1] * au.y; // AU of state k+2
      } else {
#pragma unroll
        for (int ii = i; ii < i + 2; ++ii) {
          const int kk = blk * kKBF + ii;
          if (kk < K) {
            float term = AU + d[ii] * a[kk];
            if (kk < K - 1) {
              term = term + bt[ii] * w[kk];
            }
            w[kk] = em.at(ii) * term;
            sum = sum + w[kk];
            if (kk < K - 1) {
              AU = u[ii] * a[kk] + c4[ii] * AU;
            }
          }
        }
      }
    }
  }
  FSMC_END(dg, 6);
  if constexpr (SCALE) {
    scale_pk<KT, KA>(a, w, sum);
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      a[k] = w[k];
    }
  }
  FSMC_END(dg, 7);
}



// The tables as the kernel addresses them: `row` selects the key of the RowSet copy.
struct Tables {
  cfloat_p rowSets, cR, ghostMask;
};

// compile-time K that is a whole number of operand blocks = a padded family member (K <= KT real states)
template <int KT> constexpr bool kGhost = KT % kKPad == 0;

template <int KT> __device__ __forceinline__ cfloat_p rowSetOf(const Tables& t, const int row)
{
  constexpr int KPc = ((KT + kKPad - 1) / kKPad) * kKPad;
  return t.rowSets + (size_t)row * (kRowSetParts * KPc);
}

// Sequence mode loaded its operands synchronously in rounds 2-3 (see LD: its extra live scalars made the allocator
// spill operand blocks right behind their loads in SOME instantiations).  The in-flight check of every compiled
// member (tools/check_inflight_sgprs.py, tests/test_isa_hazards.py) shows which: the 16- and 32-state members; all the
// others -- among them the 69-state member of the reference's own files -- are clean with the asynchronous loads of
// array mode, one operand block ahead, and use them -- in the IBD decode, the product's path; the three other consumers
// of sequence mode (posterior dump, per-pair rows, sums over pairs) keep the synchronous loads: which of their
// instantiations are clean moved with an unrelated change to the sums consumer (64-state member), and they are not
// worth a list of their own.  (-DFSMC_SEQ_SYNC_LOADS: synchronous everywhere, as before.)
// The LDS home of the segments' per-state sums (KParams::spsLds) is built into the array-mode IBD decode with one group
// per wave -- the kernel of launches that can be smaller than the chip.
template <int MODE, bool SEQ, bool DUAL> constexpr bool kSpsLdsBuilt = MODE == kModeIbd && !SEQ && !DUAL;
#if defined(FSMC_SEQ_SYNC_LOADS)
template <bool SEQ, int KT, int MODE> constexpr bool kSeqSyncLoads = SEQ;
#else
template <bool SEQ, int KT, int MODE> constexpr bool kSeqSyncLoads = SEQ && (KT <= 32 || MODE != kModeIbd);
#endif
template <int KT, int KA, bool SCALE = true, bool SY = false>
__device__ __forceinline__ void beta_step(const int K, float (&b)[KA], float (&w)[KA], const Tables& t, const int row,
                                          const float4* e, Diag& dg)
{
  (void)K;
  beta_step_pk<KT, KA, SCALE, kGhost<KT>, SY>(b, w, rowSetOf<KT>(t, row), e, t.ghostMask, dg);
}

template <int KT, int KA, bool SCALE = true, bool SY = false>
__device__ __forceinline__ void alpha_step(const int K, float (&a)[KA], float (&w)[KA], const Tables& t, const int row,
                                           const float4* e, Diag& dg)
{
  (void)K;
  alpha_step_pk<KT, KA, SCALE, SY>(a, w, rowSetOf<KT>(t, row), t.cR, e, dg);
}

// alpha at the first site of the window: pi * emission, scaled (HMM.cpp:736-747).
template <int KT, int KA>
__device__ __forceinline__ void alpha_init(const int K, float (&a)[KA], cfloat_p pi, const float4* e)
{
  float sum = 0.f;
  float4 ev = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if ((k & 3) == 0) {
      ev = e[k >> 2];
    }
    const float em = (k & 3) == 0 ? ev.x : (k & 3) == 1 ? ev.y : (k & 3) == 2 ? ev.z : ev.w;
    a[k] = pi[k] * em;
    sum = sum + a[k];
  }
  const float c = 1.0f / sum;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    a[k] = a[k] * c;
  }
}

// beta at the last site of the window: all ones, scaled (HMM.cpp:887-897).
// (Kreal < K for a padded family member: the ghost states start at +0 and add +0 to the sum)
template <int KT, int KA> __device__ __forceinline__ void beta_init(const int K, const int Kreal, float (&b)[KA])
{
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    b[k] = (!kGhost<KT> || k < Kreal) ? 1.0f : 0.f;
    sum = sum + b[k];
  }
  const float c = 1.0f / sum;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    b[k] = b[k] * c;
  }
}

// A K-vector of one wave lives in HBM as [K/4][64 lanes] float4: one coalesced 1-KiB row per
// group of four states (global_store/load_dwordx4).
// Addressing: `row` is the WAVE-UNIFORM address of the vector (lane 0, states 0..3) and laneOff = 16 * lane.  Each
// access is then "scalar base + 32-bit lane offset + immediate" (the saddr form of the global instructions): no
// per-row 64-bit address vectors.  (Kept as per-lane pointers the compiler hoisted eighteen of them out of the site
// loops, spilled them, and reloaded each in front of its store behind an s_waitcnt vmcnt(0) -- every row went out
// as fifteen serialised memory round trips, which was 50 % of the kernel's time.)
// (the result is typed as a GLOBAL pointer: rebuilt from integers the address space cannot be inferred, and a
//  generic pointer makes these flat_* instructions, which count in lgkmcnt as well and complete out of order)
typedef char __attribute__((address_space(1))) * gchar_p;
typedef f32x4 __attribute__((address_space(1))) * gf32x4_p;
__device__ __forceinline__ gchar_p uniformPtr(const void* p)
{
  const unsigned long long v = reinterpret_cast<unsigned long long>(p);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return (gchar_p)(((unsigned long long)hi << 32) | lo);
}
// address of float4 group k4 of this lane inside the 1-KiB-per-group row at `base`
__device__ __forceinline__ gf32x4_p rowSlot(const gchar_p base, const int k4, const unsigned laneOff)
{
  return (gf32x4_p)(base + (size_t)k4 * (kWave * sizeof(float4)) + laneOff);
}
// LDS-DMA of 16 bytes per lane (lane i lands at lds + 16*i) as inline asm, for the two-slot rings.  Through the
// builtin the compiler knows that LDS is being written and -- the two slots of a ring being one array -- guards the
// reads of the OTHER slot with a vmcnt(0), i.e. waits for the request that was just issued for the next site.  As
// asm the request is opaque (a "memory" clobber keeps LDS accesses from moving across it) and is covered by the
// explicit vmcnt waits of the callers.  M0 carries the LDS address; the compiler re-initialises M0 before every use
// of its own, and the clobber tells it that this statement changes it.
#if defined(__clang__)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
#endif
__device__ __forceinline__ void dmaToLds(const gf32x4_p src, const void* ldsDst)
{
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned lds = (unsigned)(unsigned long long)(const char __attribute__((address_space(3)))*)ldsDst;
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(lds) : "memory", "m0");
#endif
}
#if defined(__clang__)
#pragma clang diagnostic pop
#endif

// `pad`: the value of float K of the row, the first spare float of the last float4 when K is no multiple of four (the
// other spare floats are 0.f) -- a row of beta stride 2 carries a scaling reciprocal there (kCarryScale,
// fsmc_decode_kernel_body.h).
template <int KT, int KA>
__device__ __forceinline__ void store_vec(const int K, float4* row, const unsigned laneOff, const float (&v)[KA],
                                          const float pad = 0.f)
{
  const gchar_p base = uniformPtr(row);
  const int K4 = (K + 3) >> 2;
#pragma unroll
  for (int k4 = 0; k4 < K4; ++k4) {
    float4 o;
    o.x = v[4 * k4];
    o.y = (4 * k4 + 1 < K) ? v[4 * k4 + 1] : (4 * k4 + 1 == K) ? pad : 0.f;
    o.z = (4 * k4 + 2 < K) ? v[4 * k4 + 2] : (4 * k4 + 2 == K) ? pad : 0.f;
    o.w = (4 * k4 + 3 < K) ? v[4 * k4 + 3] : (4 * k4 + 3 == K) ? pad : 0.f;
    // streamed once, read back once: keep it from evicting the model tables out of L2
    const f32x4 ov = {o.x, o.y, o.z, o.w};
    __builtin_nontemporal_store(ov, rowSlot(base, k4, laneOff));
  }
}

template <int KT, int KA>
__device__ __forceinline__ void load_vec(const int K, const float4* row, const unsigned laneOff, float (&v)[KA])
{
  const gchar_p base = uniformPtr(row);
  const int K4 = (K + 3) >> 2;
#pragma unroll
  for (int k4 = 0; k4 < K4; ++k4) {
    const f32x4 ov = __builtin_nontemporal_load(rowSlot(base, k4, laneOff));
    const float4 o = make_float4(ov.x, ov.y, ov.z, ov.w);
    v[4 * k4] = o.x;
    if (4 * k4 + 1 < K) v[4 * k4 + 1] = o.y;
    if (4 * k4 + 2 < K) v[4 * k4 + 2] = o.z;
    if (4 * k4 + 3 < K) v[4 * k4 + 3] = o.w;
  }
}

// Float KT of this lane's column of a stored row: what store_vec wrote as `pad` (KT no multiple of four).
template <int KT> __device__ __forceinline__ float load_pad(const float4* row, const unsigned laneOff)
{
  static_assert(KT % 4 != 0, "a row of 4n states has no spare float");
  const f32x4 ov = __builtin_nontemporal_load(rowSlot(uniformPtr(row), KT >> 2, laneOff));
  return ov[KT & 3];
}

// Segment age estimates from the per-state posterior sums of a segment
// (HMM::getPosteriorMean, HMM.cpp:1087-1097; HMM::getMAP, 1099-1107).  The sums live in the wave's workspace
// as [K/4][64 lanes] float4 (sps points at this lane's column); this runs once per IBD record, so it walks
// memory with real loops instead of holding a K-vector in registers.
__device__ __forceinline__ float spsAt(const float4* sps, const int k)
{
  return reinterpret_cast<const float*>(sps + (size_t)(k >> 2) * kWave)[k & 3];
}
__device__ __forceinline__ void segment_ages(const int K, const unsigned nAge, const float4* sps, cfloat_p pi,
                                             cfloat_p expT, const bool wantMean, const bool wantMap, float& mean,
                                             float& mapv)
{
  mean = 0.f;
  mapv = 0.f;
  const int n = (unsigned)K < nAge ? K : (int)nAge;
  if (wantMean) {
    float acc = 0.f;
#pragma nounroll
    for (int k = 0; k < n; ++k) {
      acc = acc + spsAt(sps, k);
    }
    const float norm = 1.f / acc;
#pragma nounroll
    for (int k = 0; k < n; ++k) {
      mean = mean + (norm * spsAt(sps, k)) * expT[k];
    }
  }
  if (wantMap) {
    float best = 0.f;
    float bestT = 0.f;
#pragma nounroll
    for (int k = 0; k < n; ++k) {
      const float r = spsAt(sps, k) / pi[k];
      if (k == 0 || best < r) {
        best = r;
        bestT = expT[k];
      }
    }
    mapv = bestT;
  }
}

// The IBD scan's sum over the states below the threshold, k ascending from 0.f (HMM.cpp:1207-1224), over a K-vector in
// registers; the states it covers are scaled in place on the way.  The walk leaves at the first block of four states
// beyond the threshold -- one taken branch per site -- and inside the block that holds the threshold the states beyond it
// add +0.f, which leaves the non-negative sum unchanged.  `nPost` must be a value the compiler cannot prove
// loop-invariant (launderScalar): the compare of every state was otherwise hoisted out of the site loop as a lane mask in
// an SGPR pair, all of them spilled -- two v_readlane per state and site in front of every v_cndmask.
__device__ __forceinline__ unsigned launderScalar(unsigned v)
{
  FSMC_GCN_ASM("" : "+s"(v));
  return v;
}
template <int KA, int K, int K4>
__device__ __forceinline__ void scanBlocks(float (&w)[KA], float& s, const float cq, const unsigned nPost)
{
#pragma unroll
  for (int k4 = 0; k4 < K4; ++k4) {
    if ((unsigned)(4 * k4) >= nPost) {
      break;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (4 * k4 + i < K) {
        w[4 * k4 + i] = w[4 * k4 + i] * cq;
        s = s + ((unsigned)(4 * k4 + i) < nPost ? w[4 * k4 + i] : 0.f);
      }
    }
  }
}

} // namespace fsmc

// the lane-per-pair scaffold and the site consumers, built on the helpers above
#include "fsmc_lane_scaffold.h"
#include "fsmc_site_consumers.h"

namespace fsmc
{

// SEQ: sequence mode (DecodingParams::decodingSequence) -- every site step is preceded by an un-normalised
// half-step across the homozygous stretch since the neighbouring site, and the vectors the posterior is built
// from are the ones the reference's buffers end up holding (HMM.cpp:767, 922; oracle/hmm_oracle.h):
//   stored beta of site p  = beta after the half-step towards p-1 (p > from),
//   stored alpha of site p = alpha after the half-step towards p+1 (p < to-1).
// The emission ring then carries a fourth row per site: the homozygous emission of the gap before it.
//
// HALF: beta stride 2.  Within a chunk [lo, hi) only the beta rows of the sites at odd offsets
// (and of the chunk's last site) are written to HBM; the alpha sweep recomputes the row of an even-offset site
// from its successor's row (already landed in LDS) with one more beta step.  Half the HBM traffic of the beta
// stream for half a sweep of extra arithmetic; the floating-point operations of every row are unchanged.
// Waves per SIMD the register allocation leaves room for: two 256-register waves up to 80 states; the members for 96,
// 112 and 128 states keep their two or three K-vectors in registers only with the whole 512-entry file (one wave).
constexpr int minWavesPerSimd(const int KT)
{
  return KT >= 70 ? 1 : 2; // (the exact members between 69 and 80 states: three K-vectors no longer fit 256 registers)
}
//
// DUAL: two half-groups per wavefront (hashing mode: a batch is 32 pairs, half a wave).  Lanes 0..31 decode half A, lanes
// 32..63 half B, each over ITS OWN decode and scan window; the wave walks the union of the two windows and a lane is
// (re)initialised where its own window opens -- beta at site to-1 of its window, alpha at site from -- so within its
// window every value is produced by exactly the operations of a stand-alone decode (what a lane computes outside its
// window is overwritten before it is used and never reaches an output).  Single-chunk layout, beta stride 1 or 2 (with
// stride 2 a window may end at a site whose row is recomputed in the alpha sweep: the re-initialisation is repeated
// there); the work list is an array of item = {group A, group B} (B may be empty) prepared by the host library.
#define FSMC_DECODE_POOL 0
#include "fsmc_decode_kernel_body.h"
#undef FSMC_DECODE_POOL
#define FSMC_DECODE_POOL 1
#include "fsmc_decode_kernel_body.h"
#undef FSMC_DECODE_POOL


} // namespace fsmc
