// The lane-per-pair decode kernel's definition.  fsmc_kernels.h includes this file twice: with FSMC_DECODE_POOL 0 it
// defines decode_kernel<KT, MODE, TRACK, SEQ, HALF, DUAL>, with FSMC_DECODE_POOL 1 decode_kernel_pool<KT, MODE, TRACK,
// HALF>, the same sweeps with the resident chunk buffers claimed from a pool shared by the launch's waves (KParamsPool).
// Two definitions from one text, not one template with a switch: the pool's bookkeeping must cost the other kernel
// nothing -- not a register, not a kernel argument -- and text the preprocessor drops cannot.
#if FSMC_DECODE_POOL
template <int KT, int MODE, bool TRACK, bool HALF>
__global__ __launch_bounds__(kWave, minWavesPerSimd(KT)) void decode_kernel_pool(const KParamsPool p)
#else
template <int KT, int MODE, bool TRACK, bool SEQ, bool HALF, bool DUAL = false>
__global__ __launch_bounds__(kWave, minWavesPerSimd(KT)) void decode_kernel(const KParams p)
#endif
{
#if FSMC_DECODE_POOL
  constexpr bool SEQ = false, DUAL = false; // (array mode, one group per wave: where resident chunks are built)
#endif
  static_assert(!HALF || (!SEQ && (MODE == kModeIbd || MODE == kModeSums)),
                "beta stride 2 is built for the array-mode IBD decode and the array-mode sums over pairs");
  static_assert(KT > 0 && KT <= kMaxStates, "a member of the kernel family (fsmc_instances.h)");
  static_assert(!DUAL || (MODE == kModeIbd && !SEQ), "two half-groups per wave: array-mode IBD");
  // array mode: the backward loops are rotated (operand-free step tails overlap the next step's first operand requests)
  constexpr bool kRotate = !SEQ;
  // Beta stride 2, a row with a spare float (K no multiple of four): a stored row carries, in float K, the scaling
  // reciprocal of the row ABOVE it -- the row the alpha sweep recomputes, which then needs neither its sum nor a division.
  // Every other instantiation passes 0.f pads and keeps its sums.
  constexpr bool kCarryScale = HALF && !SEQ && !DUAL && (KT % 4 != 0);
  constexpr int KA = KT;
  constexpr int K4A = (KA + 3) / 4;
  constexpr int E4A = ((KA + kKPad - 1) / kKPad) * (kKPad / 4); // float4 per emission row (rows padded to kKPad)
  constexpr int NC = SEQ ? 4 : 3;                         // emission rows per site: 3 observation classes (+ gap)
  constexpr int NL = (NC * E4A + kWave - 1) / kWave;      // float4 per lane to stage one site's rows
  constexpr int K = KT;
  // states of the model: < K for a padded family member (the states Kreal..K-1 are ghosts), otherwise K
  const int Kreal = kGhost<KT> ? p.K : K;
  constexpr int K4 = (K + 3) >> 2;
  const int KP = p.KP; // (a compile-time KP for fixed K measured 6 % slower on C2: keep the runtime value)
  const int E4 = KP >> 2;

  __shared__ float4 emisLds[2][NC * E4A]; // ring of two sites x three observation classes (+ the gap row)
  // landing zone of the next site's beta row (LDS-DMA); the sums consumer also transposes the K x 64 posterior tile
  // through it with a row stride of 65 floats
  constexpr int kLandF4 = (MODE == kModeSums && (KA * 65 + 3) / 4 > K4A * kWave) ? (KA * 65 + 3) / 4 : K4A * kWave;
  __shared__ float4 betaLds[kLandF4];
  // kModePerPair: the expected coalescence times (read in the consumer's loop over the states; as scalar loads they
  // were K values live at once -- fsmc_kernels_bidir.h, same place)
  __shared__ float coalLds[MODE == kModePerPair ? KA : 1];

  const int lane = threadIdx.x;
  const cfloat_p tPi = (cfloat_p)p.pi, tCR = (cfloat_p)p.cR, tExpT = (cfloat_p)p.expT;
  const Tables tabs = {(cfloat_p)p.rowSets, tCR, (cfloat_p)p.ghostMask};
  const cint_p tStepRow = (cint_p)p.stepRow;
  const cint_p tRowGapF = (cint_p)p.rowGapF, tRowSiteB = (cint_p)(SEQ ? p.rowSiteB : p.stepRow),
               tRowGapB = (cint_p)p.rowGapB;
  const size_t vecF4 = (size_t)K4 * kWave; // float4 per stored K-vector of a wave
  float4* const chunkbuf = p.ws + (size_t)blockIdx.x * p.wsSlot;
  float4* const ckpt = chunkbuf + (size_t)p.chunkRows * vecF4;
  float4* const saveA = ckpt + (size_t)(p.maxChunks + 2) * vecF4;
  float4* const saveS = saveA + vecF4;
  // Resident chunks (multi-chunk windows, array mode): pass B walks down to the window's first site, so the rows of the
  // window's FIRST chunks are the last it computes -- where the workspace has room (288 GB of HBM: the host plans up to
  // p.residentChunks extra chunk buffers per wave) pass B keeps them and pass A sweeps those chunks without rebuilding
  // them: the same rows, bit for bit (the rebuild repeats pass B's operations on the same operands).
  float4* const resBase = saveS + vecF4;
  // (array-mode IBD decode and sums over pairs, one group per wave: the paired kernel is chunked too, but keeps no
  //  resident chunks)
  constexpr bool kResidentBuilt = !SEQ && !DUAL && (MODE == kModeIbd || MODE == kModeSums);
  const int nResident = kResidentBuilt ? p.residentChunks : 0;
#if FSMC_DECODE_POOL
  // The pool (KParamsPool::poolBuffers != 0): the resident buffers of all waves lie behind the slots and belong to whoever
  // claims them.  A wave holds rows only from the end of its pass B to the start of its pass A, and the waves of a launch
  // that runs several rounds are not there together: a wave that finds a free buffer keeps a chunk its own share would
  // not have held.  Which chunks a window keeps is then decided while the kernel runs -- a kept row and a rebuilt row
  // are the same bits.  In place of its own buffers a slot has one row with a 32-bit entry per chunk: the buffer that
  // holds the chunk's rows, or -1.  Pass B writes the entry of every chunk below poolCap, pass A reads it.
  // This is the kernel's instantiation WITH the pool (decode_kernel_pool; fsmc_instances.h names the members built with
  // it); decode_kernel, the other expansion of this file, has none of it.  A launch without pool buffers would run the
  // static layout here too (the host never asks for that: it launches decode_kernel).
  const bool pooled = p.poolBuffers != 0;
  int* const poolTable = reinterpret_cast<int*>(resBase);
  float4* const poolBase = p.ws + p.poolOff;
#endif
  const int C = p.chunk;
  // per-state posterior sums of the open segments (TRACK), one column per lane.  They live in the wave's workspace --
  // or, when the launch leaves LDS for them (fewer waves a CU than LDS could hold: the host passes K4 x 1 KiB of dynamic
  // LDS and sets p.spsLds), in LDS: a lane inside a segment reads and rewrites them at every site, a round trip to L2 per
  // sixteen states that a wave alone on its SIMD waits out in full (C1 shape: 27 % of the kernel).
  extern __shared__ float4 spsDyn[]; // [K4][64 lanes]
  const bool spsInLds = TRACK && kSpsLdsBuilt<MODE, SEQ, DUAL> && p.spsLds != 0;
  const float4* const spsMem = spsInLds ? (const float4*)(spsDyn + threadIdx.x) : (const float4*)(saveS + threadIdx.x);
  const unsigned laneOff = threadIdx.x * (unsigned)sizeof(float4); // this lane's byte offset inside a 1-KiB row
  // chunk-buffer slot of the row stored for the site at offset rel of its chunk
#if defined(FSMC_DIAG_SAMEROW)
  // timing experiment only (results are wrong): every stored row lands on the chunk buffer's first slot, so the
  // instruction stream is unchanged but the beta stream stays in the caches instead of going through HBM
  auto slotOf = [](const int rel) -> size_t { return (size_t)(rel & 0); };
#else
  auto slotOf = [](const int rel) -> size_t { return (size_t)(HALF ? (rel >> 1) : rel); };
#endif

  struct EmisRegs {
    float4 v[NL];
  };
  if (MODE == kModePerPair) {
    for (int k = lane; k < K; k += kWave) {
      coalLds[k] = (k < Kreal) ? p.expCoal[k] : 0.f;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }

  for (unsigned round = 0;; ++round) {
#if defined(FSMC_DIAG_GROUP_TIMES)
    const unsigned long long diagT0 = __builtin_amdgcn_s_memrealtime();
#endif
    unsigned g = 0;
    if (MODE == kModeSums) {
      g = sumsGroupOf(p, round); // one BATCH per wave and launch, its groups in turn
    } else {
      if (lane == 0) {
        g = atomicAdd(&p.counters[p.groupBase], 1u);
      }
      g = __builtin_amdgcn_readfirstlane(g);
    }
    if (g >= (unsigned)p.nGroups) {
      break;
    }
    const cuint_p gw = (cuint_p)(p.groups + (DUAL ? 2 * (size_t)g : (size_t)g));
    const unsigned firstPair = gw[0];
    const int nPairsInGroup = (int)gw[1];
    int from = (int)gw[2];
    int to = (int)gw[3];
    int scanFrom = (int)gw[4];
    int aEnd = (MODE == kModeIbd) ? (int)gw[5] : to; // the alpha sweep stops here
    const LanePair me = laneInGroup(firstPair, nPairsInGroup, lane);
    bool valid = me.valid;
    unsigned pairIdx = me.pairIdx;
    // DUAL: this lane's own windows, and the wave-uniform windows of the two halves
    int myFrom = from, myTo = to, mySF = scanFrom, myST = aEnd;
    int toA = to, toB = to, fromA = from, fromB = from, stA = aEnd, stB = aEnd;
    if constexpr (DUAL) {
      const int nB = (int)gw[7];
      if (nB > 0) {
        fromB = (int)gw[8];
        toB = (int)gw[9];
        stB = (int)gw[11];
        const bool half = lane >= 32;
        valid = half ? (lane - 32 < nB) : (lane < nPairsInGroup);
        pairIdx = half ? gw[6] + (valid ? (unsigned)(lane - 32) : 0u) : firstPair + (valid ? (unsigned)lane : 0u);
        myFrom = half ? fromB : fromA;
        myTo = half ? toB : toA;
        mySF = half ? (int)gw[10] : scanFrom;
        myST = half ? stB : stA;
        from = fromA < fromB ? fromA : fromB;
        to = toA > toB ? toA : toB;
        scanFrom = scanFrom < (int)gw[10] ? scanFrom : (int)gw[10];
        aEnd = stA > stB ? stA : stB;
      } else {
        valid = lane < nPairsInGroup && lane < 32;
      }
    }
    const HapRows hap = hapRows(p, pairIdx);
    const unsigned long long* rowA = hap.rowA;
    const unsigned long long* rowB = hap.rowB;

    const int nA = aEnd - from;
    const int nChunks = (nA + C - 1) / C;
    const bool single = nChunks <= 1;
    // Wave priority = how much of its group a wave still has in front of it.  Left alone, the two waves of a SIMD do not
    // share it evenly: the older one is served first and runs its groups in half the time of its partner (C3 windows:
    // 0.7 s against 1.4 s a group, per-group stamps of a diagnostic build) -- the same throughput while the queue is full,
    // but when it runs dry the favoured wave is done early and its partner finishes alone, on a SIMD that a lone wave
    // does not fill.  With the wave that has MORE left in front the two finish together: 4096 groups of the C3 shape (what
    // each of four GPUs gets) 2291 -> 1927 ms, 2048 groups 1023 -> 980, C2 1827 -> 1810 (same box).
    __builtin_amdgcn_s_setprio(3); // a fresh group: everything remains (pass B is about a third of it)

    int wordIdx = -1;
    unsigned long long xw = 0, aw = 0;
    // observation class of this lane's pair at site q: 0 het, 1 hom major, 2 hom minor
    // (obsIsZero / obsIsTwo of HMM.cpp:647-652 folded into a row select)
    auto obsClass = [&](const int q) -> int {
      const int wi = q >> 6;
      if (__builtin_expect(wi != wordIdx, 0)) { // once per 64 sites
        const unsigned long long wa = rowA[wi];
        const unsigned long long wb = rowB[wi];
        xw = wa ^ wb;
        aw = wa & wb;
        wordIdx = wi;
      }
      const int bit = q & 63;
      const int x = (int)((xw >> bit) & 1ull);
      const int t = (int)((aw >> bit) & 1ull);
      return x ? 0 : 1 + t;
    };
    auto prefetchEmis = [&](const int q) -> EmisRegs {
      EmisRegs r;
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const int idx = lane + i * kWave;
        r.v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (idx < NC * E4) {
          r.v[i] = p.emis3[(size_t)q * (NC * E4) + idx];
        }
      }
      return r;
    };
    auto commitEmis = [&](const int q, const EmisRegs& r) {
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const int idx = lane + i * kWave;
        if (idx < NC * E4) {
          emisLds[q & 1][idx] = r.v[i];
        }
      }
      __builtin_amdgcn_wave_barrier();
    };

    // Array mode: a site's emission rows go straight from global memory into ring slot (q & 1) by LDS-DMA -- no
    // staging registers, no ds_write (kept in registers from one iteration to the next they were spilled: a wait
    // for the load's round trip plus a scratch store at every site).  Asynchronous: counts in vmcnt and is visible
    // to this wave's LDS reads behind a vmcnt wait that covers it.  The slot's previous rows must no longer be read.
    auto stageEmis = [&](const int q) {
      const gchar_p src = uniformPtr(p.emis3 + (size_t)q * (NC * E4));
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const int idx = lane + i * kWave;
        if (idx < NC * E4) {
          dmaToLds((gf32x4_p)(src + (size_t)i * (kWave * sizeof(float4)) + laneOff), &emisLds[q & 1][i * kWave]);
        }
      }
    };
    // Table row of the step into `site` (RowIndexBlock: the rows of 64 consecutive sites in one VGPR, picked with v_readlane)
    RowIndexBlock stepRows;
    auto stepRowOf = [&](const int site) -> int { return stepRows.at(p.stepRow, p.S, lane, site); };
    // Wait for the emission rows requested one iteration ago (prefetchEmis) while the beta-row stores issued behind
    // them may still be in flight: vector memory operations retire in order, so "at most K4 outstanding" means the
    // older request is done.  Explicit, because the compiler cannot count a conditional store burst and would wait
    // for vmcnt(0) -- i.e. for the stores to reach HBM -- at every site.
    auto waitEmisRows = [&](const bool storesBehind) {
      constexpr unsigned n = (unsigned)K4A; // (only the compile-time-K loops call this)
      if (storesBehind && n < 64) {
        __builtin_amdgcn_s_waitcnt(0x0F70 | (n & 15u) | ((n >> 4) << 14));
      } else {
        waitVm0();
      }
    };

    float w[KA];
    Diag cycW; // diagnostic builds only: cycles parked in operand waits, cycles per code region
#if defined(FSMC_REGION_STAMPS)
    cycW.last = (unsigned)__builtin_readcyclecounter();
#endif
#if defined(FSMC_PHASE_STAMPS)
    // diagnostic build only: where a group's wall time goes (never enabled in the shipped library)
    long long cycB = 0, cycR = 0, cycA = 0;
    long long stamp = (long long)clock64();
#define FSMC_STAMP(acc)                                                                                                \
  do {                                                                                                                 \
    const long long now_ = (long long)clock64();                                                                       \
    (acc) += now_ - stamp;                                                                                             \
    stamp = now_;                                                                                                      \
  } while (0)
#else
#define FSMC_STAMP(acc) ((void)0)
#endif

    // Sequence mode, backward.  The vector carried from site to site is the STORED one (after the half-step).
    // betaGapStep: stage site q's rows (its fourth row is the homozygous emission of the gap (q-1, q)) and take
    // the un-normalised half-step across that gap.  betaSeqStep: the site step out of q = pos+1 (whose rows the
    // previous half-step left in the ring), then the half-step towards pos-1 unless pos is the window start.
    auto betaGapStep = [&](float (&b)[KA], const int q, const EmisRegs& rows) {
      commitEmis(q, rows);
      const int row = tRowGapB[q];
      beta_step<KT, KA, false, kSeqSyncLoads<SEQ, KT, MODE>>(K, b, w, tabs, row, &emisLds[q & 1][3 * E4], cycW);
    };
    auto betaSeqStep = [&](float (&b)[KA], const int pos) {
      const int q = pos + 1;
      const bool gap = pos > from;
      EmisRegs ev;
      if (gap) {
        ev = prefetchEmis(pos);
      }
      const int c = obsClass(q);
      const int row = tRowSiteB[q];
      beta_step<KT, KA, true, kSeqSyncLoads<SEQ, KT, MODE>>(K, b, w, tabs, row, &emisLds[q & 1][c * E4], cycW);
      if (gap) {
        betaGapStep(b, pos, ev);
      }
    };

    // ------------------------------------------------------------------ pass B
    {
      float b[KA];
      if constexpr (!kRotate) {
        beta_init<KT, KA>(K, p.K, b);
      }
      // Checkpoints (multi-chunk windows): beta at the first site of every chunk but the first -- slot j for site
      // from + j*C -- and at aEnd (slot nChunks) when the alpha sweep stops short of the window.  Pass B walks down,
      // so the next checkpoint is a countdown (no integer division per site).
      int ckJ = (aEnd < to) ? nChunks : nChunks - 1;
      int ckPos = (aEnd < to) ? aEnd : from + ckJ * C;
#if FSMC_DECODE_POOL
      // Where the rows of the chunk pass B is in stay (null: nowhere, pass A rebuilds them): one of the wave's own
      // resident buffers, or a buffer of the pool.  Decided once per chunk, when pass B enters it.
      float4* keep = nullptr;
      auto enterChunk = [&](const int j) {
        if (!pooled) {
          keep = j < nResident ? resBase + (size_t)j * p.chunkRows * vecF4 : nullptr;
          return;
        }
        keep = nullptr;
        if (j < p.poolCap) {
          // Lane 0 tries a few claim words, round robin over the pool (a cursor all waves advance): no wave ever
          // waits for another.  The buffer's last reader gave it back behind its final read, and this wave reads only
          // what it wrote itself, so claiming needs no ordering beyond the claim word's own.
          int got = -1;
          if (lane == 0) {
            for (int t = 0; t < kPoolProbes; ++t) {
              const unsigned c = __hip_atomic_fetch_add(&p.poolState[kPoolCursor], 1u, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT) % p.poolBuffers;
              unsigned expected = 0u;
              if (__hip_atomic_compare_exchange_strong(&p.poolState[kPoolClaims + c], &expected, 1u, __ATOMIC_RELAXED,
                                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                got = (int)c;
                break;
              }
            }
            // (one more vector store behind the emission rows than waitEmisRows counts: its "at most K4 outstanding" is
            //  only stricter for it -- vector memory operations retire in order -- and the returning atomics above have
            //  been waited for with vmcnt(0) anyway)
            poolTable[j] = got;
          }
          got = __builtin_amdgcn_readfirstlane(got);
          if (got >= 0) {
            keep = poolBase + (size_t)got * p.chunkRows * vecF4;
          }
        }
      };
      if (!single && ckJ < nChunks) {
        enterChunk(ckJ); // (a sweep that stops short of the window enters its last chunk at the checkpoint of aEnd)
      }
#endif
      // kCarryScale: c(s) = 1.0f / bsum(s) is the reciprocal that scaled the row of site s.  cUp = c(pos + 1) rides in
      // the spare float of a chunk row: the alpha sweep reads the row of odd offset r one site before it recomputes the
      // row of r + 1 (pass B walks down, so c(r + 1) is known when row r goes out; the pad of a chunk's last row is
      // never read).  cOwn = c(pos) rides in a checkpoint: the first site of a chunk has no stored row below it, and
      // checkpoint j IS beta of that site -- for chunk 0 and a one-chunk window, which have none, the row of `from`
      // goes to checkpoint slot 0 (the area has maxChunks + 2 slots, of which 1 .. nChunks are in use).
      // Bit-exact: the reader would compute c(pos) as 1.0f / bsum from beta_core_pk on the landed bits of pos + 1 with the
      // same operand rows; the writer fed the same function the same bits and divided by the same instruction sequence.
      // So the stored float is the float the reader would have produced.
      auto afterBeta = [&](const int pos, const float cUp = 0.f, const float cOwn = 0.f) -> bool { // true if a row went out
        if (single) {
          const int rel = pos - from;
          if (pos < aEnd && (!HALF || (rel & 1) || pos == aEnd - 1)) {
            store_vec<KT, KA>(K, chunkbuf + slotOf(rel) * vecF4, laneOff, b, cUp);
            return true;
          }
        } else {
          bool out = false;
          // (pos lies in chunk ckJ: the checkpoint countdown below IS the chunk pass B is in)
#if FSMC_DECODE_POOL
          // A resident chunk: the row stays, at its chunk-local slot.  keep != null implies pos < aEnd: enterChunk runs
          // for chunks 0 .. nChunks - 1 only -- at the start when the sweep covers the window, otherwise not before the
          // checkpoint of aEnd -- and never for chunk -1 (the countdown below stops at ckJ == 1).
          if (keep != nullptr) {
#else
          if (kResidentBuilt && ckJ < nResident && pos < aEnd) { // a resident chunk: the row stays, at its chunk-local slot
#endif
            const int relc = pos - ckPos;
            const int hiJ = ckPos + C < aEnd ? ckPos + C : aEnd;
            if (!HALF || (relc & 1) || pos == hiJ - 1) {
#if FSMC_DECODE_POOL
              store_vec<KT, KA>(K, keep + slotOf(relc) * vecF4, laneOff, b, cUp);
#else
              store_vec<KT, KA>(K, resBase + ((size_t)ckJ * p.chunkRows + slotOf(relc)) * vecF4, laneOff, b, cUp);
#endif
              out = true;
            }
          }
          if (__builtin_expect(pos == ckPos && ckJ >= 1, 0)) { // once per chunk
            store_vec<KT, KA>(K, ckpt + (size_t)ckJ * vecF4, laneOff, b, cOwn);
            ckJ -= 1;
            ckPos = from + ckJ * C;
#if FSMC_DECODE_POOL
            enterChunk(ckJ);
#endif
            out = true;
          }
          return out;
        }
        return false;
      };
      if constexpr (SEQ) {
        if (to - 1 > from) {
          betaGapStep(b, to - 1, prefetchEmis(to - 1));
        }
      }
      if constexpr (!kRotate) {
        afterBeta(to - 1);
      }
      if constexpr (SEQ) {
        for (int pos = to - 2; pos >= from; --pos) {
          betaSeqStep(b, pos);
          afterBeta(pos);
        }
      } else {
        if (to - 2 >= from) {
          stageEmis(to - 1);
        }
        if constexpr (kRotate) {
          // Rotated loop: the operand-free tail of a step (1/sum, the scaling multiply, the row store) runs while
          // the next step's first operands are in flight.  Carried from step to step: the un-normalised row w and
          // its sum; beta_init is the same thing with w = 1.0f (sum = K by sequential adds, HMM.cpp:887-897).
          float bsum = 0.f;
#pragma unroll
          for (int k = 0; k < K; ++k) {
            w[k] = (!kGhost<KT> || k < p.K) ? 1.0f : 0.f;
            bsum = bsum + w[k];
          }
          const float bsumInit = bsum;
          // DUAL: the lanes whose own window ends at site q start from beta = 1 there (HMM.cpp:887-897)
          auto openBeta = [&](const int q) {
            if constexpr (DUAL) {
              if (q == toA - 1 || q == toB - 1) {
                const bool sel = myTo - 1 == q;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                  w[k] = sel ? ((!kGhost<KT> || k < p.K) ? 1.0f : 0.f) : w[k];
                }
                bsum = sel ? bsumInit : bsum;
              }
            }
          };
          float cPrev = 1.0f; // kCarryScale: the reciprocal of the iteration before, c(q + 1)
          bool stored = false;
          for (int pos = to - 2; pos >= from; --pos) {
            const int q = pos + 1;
            openBeta(q);
            waitEmisRows(stored); // the rows of site q have landed
            __builtin_amdgcn_wave_barrier();
            if (pos - 1 >= from) {
              stageEmis(q - 1); // into the slot of site q + 1, whose step is over
            }
            const int row = stepRowOf(q);
            const int c = obsClass(q);
            const float4* e = &emisLds[q & 1][c * E4];
            const cfloat_p rs = rowSetOf<KT>(tabs, row);
            BetaOps<KT> ops;
            beta_issue_pk<KT>(ops, rs, e);
            FSMC_END(cycW, 0);
            if constexpr (kCarryScale) {
              const float cq = scale_pk<KT, KA>(b, w, bsum); // beta of site q, final
              stored = afterBeta(q, cPrev, cq);
              cPrev = cq;
            } else {
              scale_pk<KT, KA>(b, w, bsum); // beta of site q, final
              stored = afterBeta(q);
            }
            FSMC_END(cycW, 1);
            bsum = beta_core_pk<KT, KA, kGhost<KT>>(b, w, ops, rs, e, tabs.ghostMask, cycW);
          }
          openBeta(from);
          if constexpr (kCarryScale) {
            const float cq = scale_pk<KT, KA>(b, w, bsum);
            afterBeta(from, cPrev, cq);
            store_vec<KT, KA>(K, ckpt, laneOff, b, cq); // checkpoint slot 0: beta of the window's first site and its c
          } else {
            scale_pk<KT, KA>(b, w, bsum);
            afterBeta(from);
          }
        } else {
          for (int pos = to - 2; pos >= from; --pos) {
            const int q = pos + 1;
            waitVm0();
            __builtin_amdgcn_wave_barrier();
            if (pos - 1 >= from) {
              stageEmis(q - 1);
            }
            const int row = stepRowOf(q);
            const int c = obsClass(q);
            beta_step<KT, KA, true, kSeqSyncLoads<SEQ, KT, MODE>>(K, b, w, tabs, row, &emisLds[q & 1][c * E4], cycW);
            afterBeta(pos);
          }
        }
      }
    }

    FSMC_STAMP(cycB);
    // ------------------------------------------------------------------ pass A
    int cur = 4;      // open threshold level (0..3) or 4 = none
    int segStart = 0; // first site of the open segment
    float acc = 0.f;  // posteriorIBD
    float a[KA];

    auto emit = [&](const int s0, const int s1) {
#if defined(FSMC_DIAG_NOSMEM) || defined(FSMC_DIAG_NOEMIS) || defined(FSMC_DIAG_SAMEROW)
      if (s0 >= 0) { // garbage posteriors would flood the record buffer
        return;
      }
#endif
      emitIbdRecord<TRACK>(p, K, spsMem, tPi, tExpT, pairIdx, s0, s1, acc);
    };
    // LDS-DMA of one stored beta row (K4 x 1 KiB) into the landing zone: asynchronous, no VGPRs
    auto fetchBeta = [&](const float4* row) { // row: wave-uniform address of the stored vector
      const gchar_p base = uniformPtr(row);
#pragma unroll
      for (int k4 = 0; k4 < K4; ++k4) {
#if defined(__HIP_DEVICE_COMPILE__)
        __builtin_amdgcn_global_load_lds(rowSlot(base, k4, laneOff), &betaLds[k4 * kWave], 16, 0, 2 /* nt */);
#endif
      }
    };

    for (int j = 0; j < (nChunks > 0 ? nChunks : 0); ++j) {
      {
        // (two thirds of the work are left when pass A starts: levels 2, 1, 0 as the chunks go by)
        const int left = (8 * (nChunks - j)) / (3 * nChunks);
        if (left >= 2) {
          __builtin_amdgcn_s_setprio(2);
        } else if (left == 1) {
          __builtin_amdgcn_s_setprio(1);
        } else {
          __builtin_amdgcn_s_setprio(0);
        }
      }
      const int lo = from + j * C;
      const int hi = (lo + C < aEnd) ? lo + C : aEnd;
      // the rows of this chunk: kept by pass B (a resident chunk), or rebuilt below into the wave's chunk buffer
#if FSMC_DECODE_POOL
      // (pool: the entry pass B wrote for this chunk -- a vector load, the scalar cache does not see the wave's own store)
      int poolBuf = -1;
      if (pooled && !single && j < p.poolCap) {
        waitVm0();
        poolBuf = __builtin_amdgcn_readfirstlane(*(volatile int*)&poolTable[j]);
      }
      const bool resident = kResidentBuilt && !single && (pooled ? poolBuf >= 0 : j < nResident);
      float4* const cbuf = !resident ? chunkbuf
                                     : pooled ? poolBase + (size_t)poolBuf * p.chunkRows * vecF4
                                              : resBase + (size_t)j * p.chunkRows * vecF4;
      if (pooled && !single && !resident && lane == 0) {
        __hip_atomic_fetch_add(&p.poolState[kPoolRebuilt], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
#else
      const bool resident = kResidentBuilt && !single && j < nResident;
      float4* const cbuf = resident ? resBase + (size_t)j * p.chunkRows * vecF4 : chunkbuf;
#endif
      if (!single && !resident) {
        // park the carried alpha while the chunk's betas are rebuilt
        if (j > 0) {
          store_vec<KT, KA>(K, saveA, laneOff, a);
        }
        // (cUp: as in pass B's afterBeta -- the reciprocal that scaled the row of site + 1, kCarryScale)
        auto storeRow = [&](const int site, const float (&row)[KA], const float cUp = 0.f) -> bool { // true if the row went out
          const int rel = site - lo;
          if (!HALF || (rel & 1) || site == hi - 1) {
            store_vec<KT, KA>(K, chunkbuf + slotOf(rel) * vecF4, laneOff, row, cUp);
            return true;
          }
          return false;
        };
        if constexpr (kRotate) {
          // same rotation as pass B: (w, bsum) is the pending un-normalised row; a checkpoint is loaded as a row with
          // sum 1.0f (w * (1.0f / 1.0f) is an exact copy) and belongs to the next chunk (not stored here)
          float b[KA];
          float bsum = 0.f;
          int pos;
          if (hi == to) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
              w[k] = (!kGhost<KT> || k < p.K) ? 1.0f : 0.f;
              bsum = bsum + w[k];
            }
            pos = to - 2;
          } else {
            load_vec<KT, KA>(K, ckpt + (size_t)(j + 1) * vecF4, laneOff, w);
            bsum = 1.0f;
            pos = hi - 1;
          }
          if (pos >= lo) {
            stageEmis(pos + 1);
          }
          // DUAL: the lanes whose own window ends at site q start from beta = 1 there, as in pass B (HMM.cpp:887-897)
          auto reopenBeta = [&](const int q) {
            if constexpr (DUAL) {
              if (q == toA - 1 || q == toB - 1) {
                const bool sel = myTo - 1 == q;
                float ones = 0.f;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                  const float one = (!kGhost<KT> || k < p.K) ? 1.0f : 0.f;
                  w[k] = sel ? one : w[k];
                  ones = ones + one;
                }
                bsum = sel ? ones : bsum;
              }
            }
          };
          float cPrev = 1.0f; // kCarryScale: the reciprocal of the iteration before, c(q + 1)
          bool stored = false;
          for (; pos >= lo; --pos) {
            const int q = pos + 1;
            reopenBeta(q);
            waitEmisRows(stored); // the rows of site q have landed
            __builtin_amdgcn_wave_barrier();
            if (pos - 1 >= lo) {
              stageEmis(q - 1); // into the slot of site q + 1, whose step is over
            }
            const int row = stepRowOf(q);
            const int c = obsClass(q);
            const float4* e = &emisLds[q & 1][c * E4];
            const cfloat_p rs = rowSetOf<KT>(tabs, row);
            BetaOps<KT> ops;
            beta_issue_pk<KT>(ops, rs, e);
            FSMC_END(cycW, 0);
            if constexpr (kCarryScale) {
              const float cq = scale_pk<KT, KA>(b, w, bsum); // beta of site q, final
              stored = q < hi && storeRow(q, b, cPrev);
              cPrev = cq;
            } else {
              scale_pk<KT, KA>(b, w, bsum); // beta of site q, final
              stored = q < hi && storeRow(q, b);
            }
            FSMC_END(cycW, 1);
            bsum = beta_core_pk<KT, KA, kGhost<KT>>(b, w, ops, rs, e, tabs.ghostMask, cycW);
          }
          reopenBeta(pos + 1);
          scale_pk<KT, KA>(b, w, bsum);
          if (pos + 1 < hi) {
            storeRow(pos + 1, b, kCarryScale ? cPrev : 0.f);
          }
        } else {
          float b[KA];
          int pos;
          if (hi == to) {
            beta_init<KT, KA>(K, p.K, b);
            if constexpr (SEQ) {
              if (to - 1 > from) {
                betaGapStep(b, to - 1, prefetchEmis(to - 1));
              }
            }
            store_vec<KT, KA>(K, chunkbuf + slotOf(to - 1 - lo) * vecF4, laneOff, b);
            pos = to - 2;
          } else {
            load_vec<KT, KA>(K, ckpt + (size_t)(j + 1) * vecF4, laneOff, b);
            pos = hi - 1;
            if constexpr (SEQ) {
              commitEmis(hi, prefetchEmis(hi)); // the checkpoint is the stored vector of site hi: its rows next
            }
          }
          if constexpr (SEQ) {
            for (; pos >= lo; --pos) {
              betaSeqStep(b, pos);
              store_vec<KT, KA>(K, chunkbuf + (size_t)(pos - lo) * vecF4, laneOff, b);
            }
          } else {
            if (pos >= lo) {
              stageEmis(pos + 1);
            }
            for (; pos >= lo; --pos) {
              const int q = pos + 1;
              waitVm0();
              __builtin_amdgcn_wave_barrier();
              if (pos - 1 >= lo) {
                stageEmis(q - 1);
              }
              const int row = stepRowOf(q);
              const int c = obsClass(q);
              beta_step<KT, KA, true, kSeqSyncLoads<SEQ, KT, MODE>>(K, b, w, tabs, row, &emisLds[q & 1][c * E4], cycW);
              storeRow(pos, b);
            }
          }
        }
        if (j > 0) {
          load_vec<KT, KA>(K, saveA, laneOff, a);
        }
      }

      FSMC_END(cycW, 13);
      FSMC_STAMP(cycR);
      // the wave's own stores of this chunk's betas must have landed before the DMA reads them back
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      waitVm0();
      fetchBeta(cbuf);
      EmisRegs ev;
      if constexpr (SEQ) {
        ev = prefetchEmis(lo);
        commitEmis(lo, ev); // later sites are staged by the half-step of the site before them
      } else {
        // Array mode: the ring holds the rows of sites pos and pos + 1; after the combine of site pos its slot is
        // free and takes the rows of site pos + 2, which the vmcnt(0) wait of site pos + 1 covers.
        stageEmis(lo);
        if (lo + 1 < hi) {
          stageEmis(lo + 1);
        }
      }
      // table rows of the steps into the next sites, requested two sites ahead (a scalar load waited for at its use
      // costs the wave a round trip to L2 at every site)
      // every request so far (the first beta row, the first sites' emission rows) has landed: inside the loop the
      // emission registers are then only ever read behind one of its own vmcnt(0) waits, and the compiler adds none
      // kCarryScale: c of the site whose row the sweep recomputes next -- at a chunk's first site the pad of checkpoint j
      // (pass B put it there for kept and rebuilt chunks alike), afterwards the pad of the stored row one site below
      float cUp = 0.f;
      if constexpr (kCarryScale) {
        cUp = load_pad<KT>(ckpt + (size_t)j * vecF4, laneOff);
      }
      waitVm0();
      for (int pos = lo; pos < hi; ++pos) {
        // HALF: this site's beta row was not stored -- it is recomputed below from the row of site pos+1
        const bool rec = HALF && ((pos - lo) & 1) == 0 && pos + 1 < hi;

        if constexpr (SEQ) {
          if (pos < to - 1) {
            ev = prefetchEmis(pos + 1);
          }
        }
        const int c = obsClass(pos);
        const float4* e = &emisLds[pos & 1][c * E4];
        FSMC_END(cycW, 4);
        if (__builtin_expect(pos == from, 0)) {
          alpha_init<KT, KA>(K, a, tPi, e);
        } else {
          alpha_step<KT, KA, true, kSeqSyncLoads<SEQ, KT, MODE>>(K, a, w, tabs, stepRowOf(pos), e, cycW);
          if constexpr (DUAL) {
            // the lanes whose own window opens here start from pi * emission (HMM.cpp:736-747)
            if (pos == fromA || pos == fromB) {
              alpha_init<KT, KA>(K, w, tPi, e);
              const bool sel = myFrom == pos;
#pragma unroll
              for (int k = 0; k < K; ++k) {
                a[k] = sel ? w[k] : a[k];
              }
            }
          }
        }
        if constexpr (SEQ) {
          // what the reference's alpha buffer holds for this site: alpha after the un-normalised half-step
          // across the gap to the next site (HMM.cpp:764-767); the last site of the window keeps its alpha
          if (pos < to - 1) {
            commitEmis(pos + 1, ev);
            const int row = tRowGapF[pos + 1];
            alpha_step<KT, KA, false, kSeqSyncLoads<SEQ, KT, MODE>>(K, a, w, tabs, row, &emisLds[(pos + 1) & 1][3 * E4],
                                            cycW);
          }
        }

        // combine with beta of this site (landed in LDS) and normalise (HMM.cpp:672-691)
        waitVm0();
        __builtin_amdgcn_wave_barrier();
        FSMC_END(cycW, 8);
        float sumq = 0.f;
        if (rec) {
          // the landing zone holds beta of site pos+1: one beta step back gives this site's row (the same
          // operations, on the same bits, as the pass that stored its neighbours), combined from registers
          float b[KA];
          const int q = pos + 1;
          const int cq1 = obsClass(q);
          const int rowq = stepRowOf(q);
          const float4* eq = &emisLds[q & 1][cq1 * E4];
          auto readLanded = [&]() {
#pragma unroll
            for (int k4 = 0; k4 < K4; ++k4) {
              const float4 o = betaLds[k4 * kWave + lane];
              b[4 * k4] = o.x;
              if (4 * k4 + 1 < K) b[4 * k4 + 1] = o.y;
              if (4 * k4 + 2 < K) b[4 * k4 + 2] = o.z;
              if (4 * k4 + 3 < K) b[4 * k4 + 3] = o.w;
            }
          };
          {
            const cfloat_p rs = rowSetOf<KT>(tabs, rowq);
            BetaOps<KT> ops;
            beta_issue_pk<KT>(ops, rs, eq); // in flight while the landed row moves from LDS to registers
            readLanded();
            FSMC_END(cycW, 9);
            if constexpr (kCarryScale) {
              // c of this site came with the row below it (or the chunk's checkpoint): no sum, no division
              beta_core_pk<KT, KA, kGhost<KT>, false, false>(b, w, ops, rs, eq, tabs.ghostMask, cycW);
              scale_by_pk<KT, KA>(b, w, cUp);
            } else {
              const float bsum = beta_core_pk<KT, KA, kGhost<KT>>(b, w, ops, rs, eq, tabs.ghostMask, cycW);
              scale_pk<KT, KA>(b, w, bsum);
            }
            if constexpr (DUAL) {
              // the lanes whose own window ends at this site start from beta = 1 here (HMM.cpp:887-897), exactly what
              // pass B gave them (and did not store: the row of an even offset): 1.0f * (1.0f / sum of K ones)
              if (__builtin_expect(pos == toA - 1 || pos == toB - 1, 0)) {
                float ones = 0.f;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                  ones = ones + ((!kGhost<KT> || k < p.K) ? 1.0f : 0.f);
                }
                const float c1 = 1.0f / ones;
                const bool sel = myTo - 1 == pos;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                  const float init = ((!kGhost<KT> || k < p.K) ? 1.0f : 0.f) * c1;
                  b[k] = sel ? init : b[k];
                }
              }
            }
          }
          FSMC_END(cycW, 9);
#pragma unroll
          for (int k = 0; k < K; k += 2) {
            if (k + 1 < K) { // products two states at a time, the sum in state order
              const f32x2 av = {a[k], a[k + 1]};
              const f32x2 bv = {b[k], b[k + 1]};
              const f32x2 q = pmul(av, bv);
              w[k] = q.x;
              w[k + 1] = q.y;
              sumq = sumq + q.x;
              sumq = sumq + q.y;
            } else {
#pragma unroll
              for (int kk = k; kk < k + 2; ++kk) {
                if (kk < K) {
                  w[kk] = a[kk] * b[kk];
                  sumq = sumq + w[kk];
                }
              }
            }
          }
        } else {
          constexpr int kCB = 8; // states per block of the combine
          const int NB = (K + kCB - 1) / kCB;
          auto loadB = [&](const int blk, float4& b0, float4& b1) {
            b0 = betaLds[(2 * blk) * kWave + lane];
            b1 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (2 * blk + 1 < K4) {
              b1 = betaLds[(2 * blk + 1) * kWave + lane];
            }
          };
          float4 c0, c1;
          loadB(0, c0, c1);
#pragma unroll
          for (int blk = 0; blk < NB; ++blk) {
            float4 n0 = c0, n1 = c1;
            if (blk + 1 < NB) {
              loadB(blk + 1, n0, n1);
            }
#pragma unroll
            for (int i = 0; i < kCB; i += 2) {
              const int k = blk * kCB + i;
              if (k + 1 < K) {
                const f32x2 av = {a[k], a[k + 1]};
                const f32x2 bv = {pick(c0, c1, i), pick(c0, c1, i + 1)};
                const f32x2 q = pmul(av, bv);
                w[k] = q.x;
                w[k + 1] = q.y;
                sumq = sumq + q.x;
                sumq = sumq + q.y;
              } else {
#pragma unroll
                for (int ii = i; ii < i + 2; ++ii) {
                  const int kk = blk * kCB + ii;
                  if (kk < K) {
                    w[kk] = a[kk] * pick(c0, c1, ii);
                    sumq = sumq + w[kk];
                  }
                }
              }
            }
            if constexpr (kCarryScale) {
              if (blk == NB - 1) {
                cUp = pick(c0, c1, K - blk * kCB); // float K of the landed row: c of the site above
              }
            }
            __builtin_amdgcn_sched_barrier(0);
            c0 = n0;
            c1 = n1;
          }
        }
        const float cq = 1.0f / sumq;
        FSMC_END(cycW, 10);
        // every read of the landing zone has returned: request the next site's beta row
        waitLgkm0();
        if (MODE != kModeSums && !rec && pos + 1 < hi) {
          fetchBeta(cbuf + slotOf(pos + 1 - lo) * vecF4);
        }
        if constexpr (!SEQ && MODE != kModeSums) {
          if (pos + 2 < hi) {
            stageEmis(pos + 2); // this site's ring slot is free: its alpha step (and beta recompute) are over
          }
        }

        FSMC_END(cycW, 11);
        if (MODE == kModePerPair) {
          consumePerPair<KT, KA>(w, cq, coalLds, valid, pairIdx, pos, p);
        }

        if (MODE == kModeSums) {
          // HMM::augmentSumOverPairs (HMM.cpp:1052-1081): per site and state, the batch's posteriors are summed
          // over pairs in batch order (local fp32 sum from 0.f), then added to the accumulator.  The K x 64 tile
          // is transposed through LDS (row stride 65 floats: conflict-free both ways); lane j then owns state j.
          float* const tile = reinterpret_cast<float*>(betaLds);
          // this site's ring slot: its rows are no longer needed
          unsigned char* const cls = reinterpret_cast<unsigned char*>(&emisLds[pos & 1][0]);
#pragma unroll
          for (int k = 0; k < K; ++k) {
            tile[k * 65 + lane] = w[k] * cq;
          }
          if (p.flags & FSMC_WANT_MAJOR_MINOR_SUMS) {
            cls[lane] = (unsigned char)c;
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          // two states a lane in one walk over the pairs (K = 69: the five states beyond the first 64 ride along in lanes
          // 0..4 instead of costing a second walk); every state's sum still adds its pairs in batch order
          for (int kb = 0; kb < Kreal; kb += 2 * kWave) {
            const int kk0 = kb + lane, kk1 = kb + kWave + lane;
            const bool h0 = kk0 < Kreal, h1 = kk1 < Kreal;
            float* const acc0 = p.sums + (size_t)blockIdx.x * p.sumsSlot + (size_t)pos * Kreal + (h0 ? kk0 : 0);
            float* const acc1 = p.sums + (size_t)blockIdx.x * p.sumsSlot + (size_t)pos * Kreal + (h1 ? kk1 : 0);
            float s[2] = {0.f, 0.f}, s00[2] = {0.f, 0.f}, s01[2] = {0.f, 0.f}, s11[2] = {0.f, 0.f};
            if (round > 0) { // a later group of the batch: the running sums of the pairs before (this wave wrote them)
              if (p.flags & FSMC_WANT_SUMS) {
                if (h0) s[0] = acc0[0];
                if (h1) s[1] = acc1[0];
              }
              if (p.flags & FSMC_WANT_MAJOR_MINOR_SUMS) {
                if (h0) {
                  s00[0] = acc0[p.sumsPlane];
                  s01[0] = acc0[2 * p.sumsPlane];
                  s11[0] = acc0[3 * p.sumsPlane];
                }
                if (h1) {
                  s00[1] = acc1[p.sumsPlane];
                  s01[1] = acc1[2 * p.sumsPlane];
                  s11[1] = acc1[3 * p.sumsPlane];
                }
              }
            }
            const int t0 = (h0 ? kk0 : 0) * 65, t1 = (h1 ? kk1 : 0) * 65;
            // The walk over the batch's pairs, sixteen at a time: the tile values of sixteen pairs are read together
            // (one wait), then added one after the other -- the reference's order of additions (HMM.cpp:1054-1073).
            // As a loop of one pair a turn (rounds 1-3) every turn waited for its own two LDS reads and took a branch:
            // ~70 cycles a pair on a wave that runs alone.  The 00 / 01 / 11 split adds +0.f to the two sums a pair
            // does not belong to (x + 0.f == x for the non-negative sums) instead of branching on the pair's class.
            auto walk = [&](auto splitTag) {
              constexpr bool SPLIT = decltype(splitTag)::value;
              constexpr int kWalk = 16;
              auto add = [&](const float q0, const float q1, const int cv) {
                s[0] = s[0] + q0;
                s[1] = s[1] + q1;
                if constexpr (SPLIT) { // 0 het -> 01, 1 hom major -> 00, 2 hom minor -> 11
                  s11[0] = s11[0] + (cv == 2 ? q0 : 0.f);
                  s11[1] = s11[1] + (cv == 2 ? q1 : 0.f);
                  s00[0] = s00[0] + (cv == 1 ? q0 : 0.f);
                  s00[1] = s00[1] + (cv == 1 ? q1 : 0.f);
                  s01[0] = s01[0] + (cv == 0 ? q0 : 0.f);
                  s01[1] = s01[1] + (cv == 0 ? q1 : 0.f);
                }
              };
              int v = 0;
              for (; v + kWalk <= nPairsInGroup; v += kWalk) {
                float q0[kWalk], q1[kWalk];
                int cv[kWalk];
#pragma unroll
                for (int i = 0; i < kWalk; ++i) {
                  q0[i] = tile[t0 + v + i];
                  q1[i] = tile[t1 + v + i];
                  cv[i] = SPLIT ? (int)cls[v + i] : 0;
                }
#pragma unroll
                for (int i = 0; i < kWalk; ++i) {
                  add(q0[i], q1[i], cv[i]);
                }
              }
              for (; v < nPairsInGroup; ++v) {
                add(tile[t0 + v], tile[t1 + v], SPLIT ? (int)cls[v] : 0);
              }
            };
            if (p.flags & FSMC_WANT_MAJOR_MINOR_SUMS) {
              walk(std::true_type{});
            } else {
              walk(std::false_type{});
            }
            if (p.flags & FSMC_WANT_SUMS) {
              if (h0) acc0[0] = s[0];
              if (h1) acc1[0] = s[1];
            }
            if (p.flags & FSMC_WANT_MAJOR_MINOR_SUMS) {
              if (h0) {
                acc0[p.sumsPlane] = s00[0];
                acc0[2 * p.sumsPlane] = s01[0];
                acc0[3 * p.sumsPlane] = s11[0];
              }
              if (h1) {
                acc1[p.sumsPlane] = s00[1];
                acc1[2 * p.sumsPlane] = s01[1];
                acc1[3 * p.sumsPlane] = s11[1];
              }
            }
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
          waitLgkm0();
          __builtin_amdgcn_wave_barrier();
          if (pos + 1 < hi) {
            fetchBeta(cbuf + slotOf(pos + 1 - lo) * vecF4);
          }
          if constexpr (!SEQ) {
            if (pos + 2 < hi) {
              stageEmis(pos + 2);
            }
          }
        }

        if (MODE == kModeDump) {
          float* out = p.dumpOut + p.dumpOffsets[g] + (size_t)(pos - from) * Kreal * kWave + lane;
#pragma unroll
          for (int k = 0; k < K; ++k) {
            if (!kGhost<KT> || k < Kreal) {
              out[(size_t)k * kWave] = valid ? w[k] * cq : 0.f;
            }
          }
        }

        if (MODE == kModeIbd) {
          if (pos >= scanFrom) {
            // posterior of the states the scan needs
            // (the states beyond the scan's only feed the per-state sums of open segments: scaled there, by the
            //  lanes that are inside a segment)
            // Sum over the states below the threshold, k ascending from 0.f (HMM.cpp:1207-1224).  The loop leaves at
            // the first block of four states beyond the threshold -- one taken branch per site; a guard around every
            // block was seventeen of them (a taken branch costs this in-order wave ~100 cycles: the scan was 14 % of
            // the kernel).  Fully unrolled, so the register arrays stay statically indexed.  Inside the last block
            // the states beyond the threshold add +0.f, which leaves the (non-negative) sum unchanged.
            const unsigned nPost = p.stateThr;
            float s = 0.f;
            scanBlocks<KA, KT, K4A>(w, s, cq, launderScalar(nPost));
            int level = s >= p.thr[0] ? 0 : s >= p.thr[1] ? 1 : s >= p.thr[2] ? 2 : s >= p.thr[3] ? 3 : 4;
            if constexpr (DUAL) {
              if (!(pos >= mySF && pos < myST)) {
                level = 4; // outside this lane's own scan window
              }
            }
            // a change of level (or a drop below every threshold) closes the open segment at pos-1
            if (__builtin_expect(valid && cur != 4 && level != cur, 0)) {
              emit(segStart, pos - 1);
            }
            const bool opening = level != 4 && level != cur;
            if constexpr (TRACK) {
              // per-state posterior sums of the open segment (sum_posterior_per_state, HMM.cpp:1212-1229): kept
              // in the wave's workspace, touched only by the lanes that are inside a segment at this site
              if (level != 4) {
                // four blocks (sixteen states) per round trip: the loads of a round go out together.  A lane that
                // opens a segment at this site starts from zero: it clears its column first (once per segment), so
                // that the accumulation needs no select per state; 0.f + x is x, and a wave's own store to an
                // address is what its next load from it returns.  The products and sums go two states an instruction
                // (the same IEEE operations): this block is executed at every site that has ANY lane of the wave
                // inside a segment.
                // A member that runs ONE wave per SIMD has nobody to hide a round trip behind and the accumulation
                // registers to park other values in: all its blocks' loads go out together, one round trip a site
                // (K = 80 on the C2 shape: 0.73 -> 0.77, K = 100: 0.69 -> 0.72).
                constexpr int kG = 4;
                constexpr bool kOneTrip = minWavesPerSimd(KT) == 1;
                const gchar_p spsBase = uniformPtr(saveS); // scalar base + lane offset + immediate
                // (the two thresholds as values the compiler cannot prove loop-invariant, like the scan's: it
                //  otherwise hoists the compare of EVERY block out of the site loop as a lane mask in a scalar pair,
                //  spills them all and reloads two lanes of a spill register per block and site)
                const unsigned nAgeL = launderScalar(p.ageThr), nPostL = launderScalar(nPost);
                auto rounds = [&](auto inLds) {
                  constexpr bool LDS = decltype(inLds)::value;
                  auto loadBlock = [&](const int k4) -> float4 {
                    if constexpr (LDS) {
                      return spsDyn[k4 * kWave + lane];
                    } else {
                      const f32x4 t = *rowSlot(spsBase, k4, laneOff);
                      return make_float4(t.x, t.y, t.z, t.w);
                    }
                  };
                  // sv = the block's sums so far; adds this site's posteriors and writes the block back
                  auto addBlock = [&](const int k4, float4 sv) {
                    // blocks the scan already normalised are taken as they are (x * 1.0f is exact); states at or
                    // beyond the age threshold are never read back (segment_ages stops there)
                    const float sc = ((unsigned)(4 * k4) < nPostL) ? 1.0f : cq;
                    if (4 * k4 + 3 < K) {
                      const f32x2 scv = {sc, sc};
                      const f32x2 w01 = {w[4 * k4], w[4 * k4 + 1]}, w23 = {w[4 * k4 + 2], w[4 * k4 + 3]};
                      const f32x2 s01 = {sv.x, sv.y}, s23 = {sv.z, sv.w};
                      const f32x2 r01 = padd(s01, pmul(w01, scv)), r23 = padd(s23, pmul(w23, scv));
                      sv = make_float4(r01.x, r01.y, r23.x, r23.y);
                    } else {
                      sv.x = sv.x + w[4 * k4] * sc;
                      if (4 * k4 + 1 < K) sv.y = sv.y + w[4 * k4 + 1] * sc;
                      if (4 * k4 + 2 < K) sv.z = sv.z + w[4 * k4 + 2] * sc;
                      if (4 * k4 + 3 < K) sv.w = sv.w + w[4 * k4 + 3] * sc;
                    }
                    if constexpr (LDS) {
                      spsDyn[k4 * kWave + lane] = sv;
                    } else {
                      const f32x4 t = {sv.x, sv.y, sv.z, sv.w};
                      *rowSlot(spsBase, k4, laneOff) = t;
                    }
                  };
                  if (__builtin_expect(opening, 0)) {
#pragma unroll
                    for (int k4 = 0; k4 < K4; ++k4) {
                      if ((unsigned)(4 * k4) >= nAgeL) {
                        break;
                      }
                      if constexpr (LDS) {
                        spsDyn[k4 * kWave + lane] = make_float4(0.f, 0.f, 0.f, 0.f);
                      } else {
                        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                        *rowSlot(spsBase, k4, laneOff) = z;
                      }
                    }
                  }
                  if constexpr (kOneTrip && !LDS) {
                    float4 sv[K4];
#pragma unroll
                    for (int g4 = 0; g4 < K4; g4 += kG) {
                      if ((unsigned)(4 * g4) < nAgeL) { // (groups of four blocks under the age threshold)
#pragma unroll
                        for (int j = 0; j < kG; ++j) {
                          if (g4 + j < K4) {
                            sv[g4 + j] = loadBlock(g4 + j);
                          }
                        }
                      }
                    }
#pragma unroll
                    for (int g4 = 0; g4 < K4; g4 += kG) {
                      if ((unsigned)(4 * g4) < nAgeL) {
#pragma unroll
                        for (int j = 0; j < kG; ++j) {
                          if (g4 + j < K4) {
                            addBlock(g4 + j, sv[g4 + j]);
                          }
                        }
                      }
                    }
                  } else {
                    // four blocks (sixteen states) per round trip
#pragma unroll
                    for (int g4 = 0; g4 < K4; g4 += kG) {
                      if ((unsigned)(4 * g4) >= nAgeL) {
                        break;
                      }
                      float4 sv[kG];
#pragma unroll
                      for (int j = 0; j < kG; ++j) {
                        if (g4 + j < K4) {
                          sv[j] = loadBlock(g4 + j);
                        }
                      }
#pragma unroll
                      for (int j = 0; j < kG; ++j) {
                        if (g4 + j < K4) {
                          addBlock(g4 + j, sv[j]);
                        }
                      }
                    }
                  }
                };
                if constexpr (kSpsLdsBuilt<MODE, SEQ, DUAL>) {
                  if (spsInLds) { // (uniform over the launch)
                    rounds(std::true_type{});
                  } else {
                    rounds(std::false_type{});
                  }
                } else {
                  rounds(std::false_type{});
                }
              }
            }
            acc = (level == 4) ? 0.f : (opening ? s : acc + s);
            if (opening) {
              segStart = pos;
            }
            cur = level;
            if constexpr (DUAL) {
              if (__builtin_expect(pos == stA - 1 || pos == stB - 1, 0)) {
                if (pos == myST - 1) { // the last site of this lane's scan window closes its open segment
                  if (valid && cur != 4) {
                    emit(segStart, pos);
                  }
                  cur = 4;
                }
              }
            } else if (__builtin_expect(pos == aEnd - 1, 0)) {
              if (valid && cur != 4) {
                emit(segStart, pos);
              }
            }
          }
        }
        FSMC_END(cycW, 12);
      }
#if FSMC_DECODE_POOL
      if (pooled && resident) {
        // The chunk is swept: its buffer goes back to the pool, behind the last read of its rows (the LDS-DMA counts in
        // vmcnt).  Release order: the next owner may sit on another XCD, whose writes to the buffer must not meet this
        // wave's rows still on their way out of the L2.
        waitVm0();
        if (lane == 0) {
          __hip_atomic_exchange(&p.poolState[kPoolClaims + poolBuf], 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_fetch_add(&p.poolState[kPoolKept], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
#endif
      FSMC_STAMP(cycA);
    }
#if defined(FSMC_REGION_STAMPS)
    if (lane == 0 && p.phaseCycles) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        atomicAdd(&p.phaseCycles[8 + r], (unsigned long long)cycW.acc[r]);
      }
    }
#endif
#if defined(FSMC_DIAG_GROUP_TIMES)
    // diagnostic builds (tools/build_variant.sh <name> -DFSMC_DIAG_GROUP_TIMES; tools/analyse_group_times.py): one marker
    // record per group -- start = -1, end = the wave's slot, prob / post_mean = when the group ended / began (ms of the
    // 100 MHz clock), map = HW_ID and XCC_ID -- among the IBD records.  How the SIMD-sharing of the waves was found.
    if (MODE == kModeIbd && lane == 0) {
      const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
      const unsigned idx = atomicAdd(&p.counters[1], 1u);
      if (idx < p.recCap) {
        fsmc_ibd_record r;
        r.pair = pairIdx;
        r.start = -1;
        r.end = (int)blockIdx.x;
        r.prob = (float)((double)(t1 & 0xFFFFFFFFull) / 1e5);
        r.post_mean = (float)((double)(diagT0 & 0xFFFFFFFFull) / 1e5);
        r.map = __int_as_float((int)(__builtin_amdgcn_s_getreg(63492) & 0xFFFFu) |
                               (int)((__builtin_amdgcn_s_getreg(63508) & 0xFu) << 16));
        p.recs[idx] = r;
      }
    }
#endif
#if defined(FSMC_PHASE_STAMPS)
    if (lane == 0 && p.phaseCycles) {
      atomicAdd(&p.phaseCycles[0], (unsigned long long)cycB);
      atomicAdd(&p.phaseCycles[1], (unsigned long long)cycR);
      atomicAdd(&p.phaseCycles[2], (unsigned long long)cycA);
      atomicAdd(&p.phaseCycles[3], 1ull);
      atomicAdd(&p.phaseCycles[4], (unsigned long long)cycW.waitCycles);
    }
#endif
  }
}
