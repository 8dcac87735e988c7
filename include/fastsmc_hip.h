/*
 * fastsmc_hip.h -- C ABI of the MI355X (gfx950) pairwise-HMM decode library, libfastsmc_hip.so.
 *
 * This is the drop-in seam for ONE path of PalamaraLab/FastSMC: the batched pairwise HMM
 * decode (forward, backward, posterior combine) and its posterior consumers.  The reference
 * has no FFI for this path -- it is private methods of class HMM -- so each entry point
 * below names the reference call it stands in for (paths relative to ASMC_SRC/SRC):
 *
 *   fsmc_model_create      <- what HMM::HMM leaves behind for the path: DecodingQuantities
 *                             vectors + prepareEmissions rows        (HMM.cpp:65-127, 159-256)
 *   fsmc_haps_upload       <- Individual::genotype1/2 bit vectors consumed by makeBits
 *                                                                    (HMM.cpp:147-157)
 *   fsmc_decode_ibd        <- decodeBatch + writePerPairOutputFastSMC for every batch of a
 *                             work list                              (HMM.cpp:575-584, 624-633,
 *                                                                     639-1041, 1179-1357)
 *   fsmc_decode_posteriors <- decodeBatch; result = m_alphaBuffer     (HMM.cpp:639-722)
 *   fsmc_decode_per_pair   <- decodeBatch + writePerPairOutput        (HMM.cpp:1360-1458)
 *   fsmc_decode_sums       <- decodeBatch + augmentSumOverPairs       (HMM.cpp:1044-1085)
 *   fsmc_decode_pair_posteriors <- decodeBatch + the perPairPosteriors / sumOfPosteriors part of
 *                             writePerPairOutput, the tables ASMC::decodePairs hands out
 *                                                                    (HMM.cpp:1378-1392, ASMC.cpp:80-128)
 *   fsmc_decode_pair_minima <- decodeBatch + writePerPairOutput + the column-wise min / argmin of
 *                             DecodePairsReturnStruct::finaliseCalculations
 *                                                  (HMM.cpp:1360-1458, DecodePairsReturnStruct.hpp:105-118)
 *   fsmc_decode_pair_bins   <- decodeBatch + writePerPairOutput, then per pair the mean / min / argmin of the rows over
 *                             bins of sites (no counterpart in the reference: its callers reduce the rows in numpy)
 *   fsmc_decode_pair_cdf    <- decodeBatch, then per pair and site the running sum of the posterior over the states: tail
 *                             probabilities and quantile states (none: the reference's callers do this in numpy on
 *                             perPairPosteriors; the sum's order is the IBD scan's, HMM.cpp:1207-1224)
 *   fsmc_decode_pair_tail_summaries <- the tail probabilities of fsmc_decode_pair_cdf, summed over the pairs per site and
 *                             reduced over bins of sites per pair (none: the reference's callers do this in numpy)
 *   fsmc_decode_pair_loglik <- the forward half of decodeBatch, its per-site scaling sums kept (HMM.cpp:725-784); the
 *                             product of the sums, the pair's data likelihood, has no counterpart: the reference
 *                             uses every sum for 1.0f / sum and drops it
 *   fsmc_decode_pair_viterbi <- none: the reference decodes marginals only.  The forward step of decodeBatch
 *                             (HMM.cpp:787-830) with max in place of +, back-pointers and a traceback
 *   fsmc_decode_pair_samples <- none: the reference draws nothing.  The forward half of decodeBatch (HMM.cpp:725-784),
 *                             then backward sampling with the coefficients of the forward step's term (HMM.cpp:799-830)
 *   fsmc_decode_pair_transitions <- none: the reference keeps no two-slice quantity.  decodeBatch's forward vectors and
 *                             the three terms of its backward step (getPreviousBetaBatched, HMM.cpp:986-1014) joined
 *
 * Conventions: plain C types; host buffers are caller-owned, device buffers library-owned;
 * every function returns 0 on success or a negative FSMC_E* code and never exits or throws;
 * fsmc_last_error() describes the last failure of the context (or of context creation when
 * ctx == NULL).  One context per device; contexts are independent and may be driven from
 * different host threads/processes (one process per GPU).  There is NO CPU fallback: without
 * a usable HIP device every call fails with FSMC_ENODEVICE.
 */
#ifndef FASTSMC_HIP_H
#define FASTSMC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSMC_OK 0
#define FSMC_EINVAL (-1)    /* bad argument */
#define FSMC_ENODEVICE (-2) /* no HIP device / HIP runtime failure at start-up */
#define FSMC_EHIP (-3)      /* a HIP call failed; see fsmc_last_error */
#define FSMC_ENOMEM (-4)    /* device or host allocation failed */
#define FSMC_ESTATE (-5)    /* call sequence error (e.g. decode before upload) */
#define FSMC_EOVERFLOW (-6) /* caller's output buffer too small; *n_out holds the needed count */
#define FSMC_EUNSUPPORTED (-7)
#define FSMC_ERUNTIME (-8)  /* the device is there but this process cannot launch on it: two HIP runtimes loaded */

typedef struct fsmc_ctx fsmc_ctx;
typedef struct fsmc_model fsmc_model;

/* Constant inputs of the path.  All pointers are host memory, copied by fsmc_model_create. */
typedef struct {
  int32_t K;                /* states                          (DecodingQuantities::states) */
  int32_t S;                /* sites                           (Data::sites) */
  const float* pi;          /* [K] initialStateProb */
  const float* col_ratios;  /* [K] columnRatios, zero padded   (DecodingQuantities.cpp:299-303) */
  const float* exp_times;   /* [K] expectedTimes */
  int32_t n_rows;           /* rows of the four transition tables */
  const float* D;           /* [n_rows][K] Dvectors */
  const float* B;           /* [n_rows][K] Bvectors   (column K-1 unused) */
  const float* U;           /* [n_rows][K] Uvectors   (column K-1 unused) */
  const float* RR;          /* [n_rows][K] rowRatioVectors (column K-1 unused) */
  const int32_t* step_row;  /* [S] table row of key roundMorgans(gen[p]-gen[p-1]) for p>=1 (HMM.cpp:755,909) */
  const float* e1;          /* [S][K] emission1AtSite */
  const float* e0m1;        /* [S][K] emission0minus1AtSite */
  const float* e2m0;        /* [S][K] emission2minus0AtSite */
  uint32_t state_threshold; /* HMM::stateThreshold      (HMM.cpp:504-513) */
  uint32_t age_threshold;   /* HMM::ageThreshold        (HMM.cpp:101-105) */
  float probability_threshold; /* HMM::probabilityThreshold (HMM.cpp:96-99) */
  /* Sequence mode (DecodingParams::decodingSequence; HMM.cpp:760-770 forward, 915-925 backward): two transition
   * steps per site -- across the homozygous stretch since the previous site, then the site itself.  All zero /
   * NULL in array mode (step_row is then the only row index).  Arrays are [S], indexed by the later site q of
   * the gap (q-1, q); entry 0 unused:
   *   gap_row_f[q]  row of key roundMorgans(recDist_q - rate[q]),   site_row_f[q]  row of key rate[q]
   *   gap_row_b[q]  row of key roundMorgans(recDist_q - rate[q-1]), site_row_b[q]  row of key rate[q-1]
   * (recDist_q = roundMorgans(gen[q]-gen[q-1]), rate[p] = roundMorgans(recRateAtMarker[p])), and
   *   hom[q][K] = homozygousEmissionMap[roundPhysical(phys[q]-phys[q-1]-1)]. */
  int32_t sequence;
  const int32_t* gap_row_f;
  const int32_t* site_row_f;
  const int32_t* gap_row_b;
  const int32_t* site_row_b;
  const float* hom;
} fsmc_model_desc;

/* One haplotype pair: rows of the uploaded bit matrix.  Row 2*ind + (hap-1). */
typedef struct {
  uint32_t hap_a; /* the record's first haplotype  (PairObservations iInd/iHap) */
  uint32_t hap_b; /* the record's second haplotype (PairObservations jInd/jHap) */
} fsmc_pair;

/* A batch of <= 64 consecutive pairs that share one decode window -- the reference's batch
 * (HMM.cpp:555-636).  [from,to) is the padded decode window handed to decodeBatch;
 * [scan_from,scan_to) is the window the IBD scan covers (HMM.cpp:1199-1206).  Non-hashing
 * mode: from = scan_from = 0, to = scan_to = S. */
typedef struct {
  uint32_t first_pair; /* index into the pair list */
  uint32_t n_pairs;    /* 1..64 */
  uint32_t from, to;
  uint32_t scan_from, scan_to;
} fsmc_group;

/* One IBD segment as handed to HMM::writePairIBD (HMM.cpp:1110-1177). */
typedef struct {
  uint32_t pair;   /* index into the pair list */
  int32_t start;   /* first site */
  int32_t end;     /* last site, inclusive */
  float prob;      /* cumulative posterior ("posteriorIBD"); ibd_score = prob / (end-start+1) */
  float post_mean; /* getPosteriorMean of the per-state sums (0 if not requested) */
  float map;       /* getMAP of the per-state sums (0 if not requested) */
} fsmc_ibd_record;

#define FSMC_WANT_MEAN 1u /* DecodingParams::doPerPairPosteriorMean */
#define FSMC_WANT_MAP 2u  /* DecodingParams::doPerPairMAP */
#define FSMC_WANT_SUMS 4u /* DecodingParams::doPosteriorSums (fsmc_decode_sums) */
#define FSMC_WANT_MAJOR_MINOR_SUMS 8u /* doMajorMinorPosteriorSums */

/* ---- context ---- */
/* stream: an existing hipStream_t to launch on (e.g. torch's current stream), or NULL for a private one. */
int fsmc_ctx_create(int device_id, void* stream, fsmc_ctx** out);
void fsmc_ctx_destroy(fsmc_ctx* ctx);
const char* fsmc_last_error(const fsmc_ctx* ctx);
/* Device properties as seen by the library: CU count, and the number of resident decode waves it launches. */
int fsmc_ctx_info(const fsmc_ctx* ctx, int32_t* n_cu, int32_t* n_slots, uint64_t* hbm_bytes);
/* Diagnostic.  The library's scratch memory (the decode's workspace, the staging, row and accumulator buffers of the
 * entry points, the two pinned row buffers, fsmc_identify's per-call buffers) is allocated once and reused; a kernel
 * must write every cell of it before any kernel reads it.  FSMC_DIAG_SCRATCH_FILL=<0..255> in the environment makes an
 * entry point fill every scratch buffer it is about to use with that byte, the whole allocation, before anything it
 * writes there, so that a read of a cell not written in this call shows in the result (255: NaN / -1; 127: a huge finite
 * value; 128: a tiny negative float, a very negative integer).  The variable is read at every call; a value that is no
 * integer in 0..255 makes every such entry point return FSMC_EINVAL, nothing launched.  Results do not depend on it.
 * Returns the bytes filled on this context since it was created: 0 unless the variable was set. */
uint64_t fsmc_ctx_scratch_filled(const fsmc_ctx* ctx);
/* Workspace for the alpha/beta streaming (bytes).  A limit set here is the caller's statement about the job: a plan may
 * use all of it at once -- windows kept whole instead of chunked, resident chunks, long windows in the paired kernel.
 * 0 (default): the library's own policy.  The rows a decode cannot do without may take up to 80 % of the card (at least
 * 40 %); everything beyond them is EARNED: hipMalloc costs about 40 ms per GB on this driver, so a context starts with a
 * free allowance of 24 GB and every launch adds what an upgraded plan is expected to save of it (6 % of its estimated
 * kernel time, at the allocation rate) -- a run of seconds does not spend them allocating.  Growth is
 * amortised and every byte is paid for once: a bigger buffer is a new allocation of its whole size, so the plan is
 * upgraded only when the credit covers twice the buffer held (or the whole budget), and an allocation is debited from
 * the credit.  The buffer is kept for the life of the context. */
int fsmc_ctx_set_workspace_limit(fsmc_ctx* ctx, uint64_t bytes);
/* The caller announces the work the context's coming launches will decode -- pair-sites (pairs x sites of their decode
 * windows) of a model of `states` states: what the reference's HMM::decodeAll knows when it starts (its job's pair
 * range, HMM.cpp:310-321).  Under the library's own workspace policy (no limit set) the credit of the whole job is
 * then there at the first launch: a job long enough to pay for the card allocates it once, at its start, instead of
 * growing into it; a short job stays small.  The announced launches earn nothing again.  No effect with a limit set.
 * pair_sites = 0 ends the announced job (HMM::finishDecoding, HMM.cpp:515-524): what is left of the announcement -- an
 * estimate that was too high, a job that stopped early -- is forgotten and its unspent credit taken back.  The credit
 * of announcements is capped at the device's memory. */
int fsmc_ctx_expect_work(fsmc_ctx* ctx, double pair_sites, int32_t states);
/* Tuning: sites between beta checkpoints when a decode window does not fit the workspace (0 = automatic:
 * max(512, ceil(sqrt(window))), 2048 for the wave-group kernel, rounded up to 16).  Results do not depend on it. */
int fsmc_ctx_set_chunk_sites(fsmc_ctx* ctx, uint32_t sites);
/* Tuning: beta stride of the IBD decode and of the sums over pairs.  1 = every beta row of a chunk goes through HBM
 * (8K bytes per pair-site); 2 = every second row does and the alpha sweep recomputes the others from their successor
 * (4K bytes per pair-site, half a sweep more arithmetic); 0 = automatic: 2 where that kernel exists (array mode,
 * K <= 128) -- for the sums only when the launch has at least as many batches as the chip holds waves (a wave alone on
 * its SIMD only gets the recomputed half sweep on top) --, else 1.  Results do not depend on it.
 * fsmc_ctx_last_beta_stride reports what the last IBD or sums launch used. */
int fsmc_ctx_set_beta_stride(fsmc_ctx* ctx, uint32_t stride);
int fsmc_ctx_last_beta_stride(const fsmc_ctx* ctx, int32_t* stride);
/* How the last launch was laid out: sites per chunk (= the longest window when every beta row fitted), chunks per
 * window, resident waves. */
int fsmc_ctx_last_plan(const fsmc_ctx* ctx, int32_t* chunk_sites, int32_t* max_chunks, int32_t* n_slots);
/* Chunked windows (longer than a wave's workspace holds) rebuild every chunk's beta rows from a checkpoint -- one of the
 * decode's 3.5 sweeps -- except for the window's first chunks, whose rows the backward pass can leave in the workspace
 * ("resident chunks").  chunks = -1 (default): as many as the workspace allows (the limit if one is set, otherwise what
 * the context has earned: see fsmc_ctx_set_workspace_limit); 0: none; n: at most n.  Results do not depend on it. */
int fsmc_ctx_set_resident_chunks(fsmc_ctx* ctx, int32_t chunks);
int fsmc_ctx_last_resident_chunks(const fsmc_ctx* ctx, int32_t* chunks);
/* The chunk pool.  Where the number of resident chunks is left to the library (-1 above) and is neither none nor all of
 * them, the resident buffers of all waves of a launch form one pool: a wave claims a buffer for a chunk when its backward
 * pass reaches it, rebuilds the chunk if none is free, and gives the buffer back once the forward sweep has passed the
 * chunk.  The same memory then keeps more chunks, because the waves of a launch that runs several rounds do not hold
 * their rows at the same time.  mode = -1 (default): in IBD launches with more than twice as many groups as resident
 * waves; 0: never (every wave keeps its own buffers); 1: also in launches of one or two rounds and in the sums over pairs.  phi_percent: a window asks for a buffer for its first
 * ceil(phi_percent / 100 x resident chunks) chunks (100 ... 100000, 0 = the default).  Results do not depend on any of it.
 * fsmc_ctx_last_chunk_pool (after the launch has completed; it waits for the context's stream): the pool's buffers
 * (0: the last launch kept the static layout), the chunks whose rows were kept and those that were rebuilt -- of the
 * last kernel launch where a call makes several -- and the buffers still claimed, 0 after every launch. */
int fsmc_ctx_set_chunk_pool(fsmc_ctx* ctx, int32_t mode, uint32_t phi_percent);
int fsmc_ctx_last_chunk_pool(fsmc_ctx* ctx, uint32_t* buffers, uint32_t* kept, uint32_t* rebuilt, uint32_t* outstanding);
/* Two half-groups per wavefront.  A group of at most 32 pairs (a hashing-mode batch of the reference's default size)
 * fills half a wave; with pairing = 1 (default) the IBD decode puts two such groups with nearby windows on one wave,
 * each lane still decoded over its own group's windows (results do not depend on it); half-full groups that find no
 * partner ride in the same kernel as items of their own.  0 = never.
 * fsmc_ctx_last_items: wave work items of the last IBD launch when it paired groups, 0 when it ran them as uploaded. */
int fsmc_ctx_set_pairing(fsmc_ctx* ctx, uint32_t mode);
int fsmc_ctx_last_items(const fsmc_ctx* ctx, int32_t* n_items);
/* Two waves per decode window.  The consumers without state across sites (fsmc_decode_posteriors, fsmc_decode_per_pair,
 * fsmc_decode_sums*) of a model of at most 128 states in array mode: a launch of at most half as many groups (batches of
 * the sums) as the chip holds waves gives every group a workgroup of two waves -- alpha runs up from the window's first
 * site in one while beta runs down from its last in the other, each stores its rows as far as the middle and combines
 * with the other's beyond it (HMM.cpp:672-691, 725-1041: one alpha step, one beta step and one combine per site, the
 * same operations in the same order: results do not depend on it) -- provided the whole windows' rows fit the
 * workspace.  0 (default) = automatic, 1 = never.  fsmc_ctx_last_waves_per_window: 2 if the last such launch did. */
int fsmc_ctx_set_two_wave_windows(fsmc_ctx* ctx, uint32_t mode);
int fsmc_ctx_last_waves_per_window(const fsmc_ctx* ctx, int32_t* waves);
/* 1 when the last IBD launch kept the open segments' per-state posterior sums (FSMC_WANT_MEAN / FSMC_WANT_MAP:
 * HMM.cpp:1212-1229) in LDS instead of the workspace: a launch of fewer wavefronts than the chip's LDS can give
 * (K/4 + 1) KiB each beside the kernel's own -- a small job, whose waves would wait out every round trip of those sums
 * to L2.  The results do not depend on it. */
int fsmc_ctx_last_segment_sums_in_lds(const fsmc_ctx* ctx, int32_t* in_lds);
/* Tuning: groups of the work list that fsmc_decode_pair_posteriors decodes, transposes and copies out at a time (a
 * "slice"); device memory, the pinned row buffers and nothing else are sized by it.  0 (default) = automatic: as many
 * groups as a quarter of the card (or the workspace limit) and its free memory hold of the slice's dump and rows.
 * Results do not depend on it.  fsmc_ctx_last_pair_posterior_slices: slices of the last such call. */
int fsmc_ctx_set_pair_posterior_slice(fsmc_ctx* ctx, uint32_t groups);
int fsmc_ctx_last_pair_posterior_slices(const fsmc_ctx* ctx, int32_t* slices);
/* The same for fsmc_decode_pair_minima: groups whose mean / MAP rows the device holds at a time.  0 (default) =
 * automatic: as many groups as a quarter of the card (or the workspace limit) and half its free memory hold of rows
 * (64 * S * 4 bytes a group and output).  Results do not depend on it. */
int fsmc_ctx_set_pair_minima_slice(fsmc_ctx* ctx, uint32_t groups);
int fsmc_ctx_last_pair_minima_slices(const fsmc_ctx* ctx, int32_t* slices);
/* The same for fsmc_decode_pair_bins.  0 (default) = automatic: as many groups as a quarter of the card (or the
 * workspace limit) and half its free memory hold of rows and binned outputs (64 * 4 bytes * (S a row kind + n_bins an
 * output) a group).  Results do not depend on it. */
int fsmc_ctx_set_pair_bins_slice(fsmc_ctx* ctx, uint32_t groups);
int fsmc_ctx_last_pair_bins_slices(const fsmc_ctx* ctx, int32_t* slices);
/* The same for fsmc_decode_pair_cdf.  0 (default) = automatic: as many groups as a quarter of the card (or the
 * workspace limit) and half its free memory hold of staging and rows (64 * K * S * 4 bytes a group of staging plus
 * 64 * S * 4 bytes a group and output).  Results do not depend on it. */
int fsmc_ctx_set_pair_cdf_slice(fsmc_ctx* ctx, uint32_t groups);
int fsmc_ctx_last_pair_cdf_slices(const fsmc_ctx* ctx, int32_t* slices);
/* The same for fsmc_decode_pair_tail_summaries.  0 (default) = automatic: as many groups as a quarter of the card (or the
 * workspace limit) and half its free memory hold of staging, tail rows and binned outputs (64 * K * S * 4 bytes a group
 * of staging plus 64 * 4 bytes * (S + n_bins a bin output) a group and cut).  Results do not depend on it. */
int fsmc_ctx_set_pair_tail_slice(fsmc_ctx* ctx, uint32_t groups);
int fsmc_ctx_last_pair_tail_slices(const fsmc_ctx* ctx, int32_t* slices);
/* The same for fsmc_decode_pair_loglik.  0 (default) = automatic: as many groups as a quarter of the card (or the
 * workspace limit) and half its free memory hold of outputs (64 * 12 bytes * (1 + n_bins) a group): in practice the
 * whole work list.  Results do not depend on it. */
int fsmc_ctx_set_pair_loglik_slice(fsmc_ctx* ctx, uint32_t groups);
int fsmc_ctx_last_pair_loglik_slices(const fsmc_ctx* ctx, int32_t* slices);
/* The same for fsmc_decode_pair_viterbi.  0 (default) = automatic: as many groups as a quarter of the card (or the
 * workspace limit) and half its free memory hold of outputs (64 * (S + 12) bytes a group).  Results do not depend on
 * it. */
int fsmc_ctx_set_pair_viterbi_slice(fsmc_ctx* ctx, uint32_t groups);
int fsmc_ctx_last_pair_viterbi_slices(const fsmc_ctx* ctx, int32_t* slices);
/* The same for fsmc_decode_pair_samples.  0 (default) = automatic: as many groups as a quarter of the card (or the
 * workspace limit) and half its free memory hold of outputs (64 * n_samples * S bytes a group).  Results do not depend
 * on it. */
int fsmc_ctx_set_pair_samples_slice(fsmc_ctx* ctx, uint32_t groups);
int fsmc_ctx_last_pair_samples_slices(const fsmc_ctx* ctx, int32_t* slices);
/* The same for fsmc_decode_pair_transitions.  0 (default) = automatic: as many groups as a quarter of the card (or the
 * workspace limit) and half its free memory hold of outputs (64 * 8 bytes * (S + n_bins) a group).  Results do not
 * depend on it. */
int fsmc_ctx_set_pair_transitions_slice(fsmc_ctx* ctx, uint32_t groups);
int fsmc_ctx_last_pair_transitions_slices(const fsmc_ctx* ctx, int32_t* slices);
/* Which kernel the last launch ran: 16 ... 128 = the lane-per-pair kernel compiled for that many states (the exact
 * members 69, 50, 100, or the padded members 16, 32, 48, 64, 80, 96, 112, 128); the wave-group kernel (128 < K <= 1024):
 * 1048 / 1064 / 1080 = four waves per group of 48 / 64 / 80 states (K <= 192 / 256 / 320), 6064 / 7064 / 8064 = six /
 * seven / eight waves of 64 states (K <= 384 / 448 / 512), 8080 / 8096 / 8128 = eight waves of 80 / 96 / 128 states
 * (K <= 640 / 768 / 1024); 0 = the any-K kernel (1024 < K <= 4096: a pair's K-vectors live in the workspace instead of
 * registers -- the same results, far from the roofline). */
int fsmc_ctx_last_kernel(const fsmc_ctx* ctx, int32_t* member);

/* ---- resident inputs ---- */
int fsmc_model_create(fsmc_ctx* ctx, const fsmc_model_desc* desc, fsmc_model** out);
void fsmc_model_destroy(fsmc_model* m);
/* bits: [n_haps][ceil(n_sites/64)] little-endian words, site s at bit (s % 64) of word s / 64. */
int fsmc_haps_upload(fsmc_ctx* ctx, const uint64_t* bits, uint32_t n_haps, uint32_t n_sites);
/* The work list: pairs and the groups (batches) that partition them in order. */
int fsmc_worklist_upload(fsmc_ctx* ctx, const fsmc_pair* pairs, size_t n_pairs, const fsmc_group* groups,
                         size_t n_groups);

/* ---- the hot path, split so that timing can exclude transfers ---- */
/* Launch the IBD decode of the resident work list (asynchronous on the context's stream). */
int fsmc_decode_ibd_launch(fsmc_ctx* ctx, const fsmc_model* m, uint32_t flags);
/* Wait, copy back and order the records like the reference writes them (batch, pair in batch, site).
 * If cap is too small returns FSMC_EOVERFLOW with *n_out = needed. */
int fsmc_decode_ibd_fetch(fsmc_ctx* ctx, fsmc_ibd_record* out, size_t cap, size_t* n_out);
/* Block until the stream is idle. */
/* ---- identification step (scope row f1; replaces the word loop of FastSMC::run, FastSMC.cpp:118-235, with
 * HASHING/SeedHash.hpp:29-136, ExtendHash.hpp:26-128, Match.hpp:29-83, Utils.cpp:22-34) ----
 * Which haplotype pairs of the job share 64-site words over at least min_m centimorgans.  A pair's matching words
 * are merged into one interval while no more than `gap` words in a row are missing; a word whose number of distinct
 * values / n_haps is not above `skip` extends every open interval instead of being compared. */
typedef struct {
  uint32_t window_size;  /* Data::windowSize (haplotypes per side of a job's square), Data.cpp:62-80 */
  uint32_t w_i, w_j;     /* 1-based window numbers of the job */
  int32_t last_job;      /* jobInd == jobs (SeedHash.hpp:97) */
  int32_t j_above_diag;  /* Data::is_j_above_diag */
} fsmc_job_window;

typedef struct {
  uint32_t hap_a, hap_b; /* rows of the word matrix, hap_a < hap_b */
  uint32_t from, to;     /* first site of the first matching word, last site of the last one (Match.hpp:42-52) */
  uint32_t flush_word;   /* word at which the reference's ExtendHash would have reported it (n_words: at the end) */
} fsmc_candidate;

/* words: [n_haps][n_words] host, word w of haplotype h (bit s%64 of word s/64 = allele of site s); global_ids:
 * [n_haps] haplotype numbers in the whole file (2 * sample line + 0/1); gen_pos: [n_sites] Morgans.  Fills `out` with
 * the candidates ordered by (flush_word, hap_a * n_haps + hap_b) -- the order in which fastsmc_amd hands them to
 * HMM::decodeFromHashing.  FSMC_EOVERFLOW: cap too small, *n_out = the number of candidates.
 * gap: any value >= 0.  A gap of n_words or more can never run out before the last word, so every such value means
 * the same as n_words and is taken as n_words (flush_word is then n_words for every candidate). */
int fsmc_identify(fsmc_ctx* ctx, const uint64_t* words, uint32_t n_haps, uint32_t n_words, const uint32_t* global_ids,
                  const fsmc_job_window* job, const float* gen_pos, uint32_t n_sites, int32_t gap, float skip,
                  float min_m, fsmc_candidate* out, size_t cap, size_t* n_out);
/* The other knobs of the reference's identification step (DecodingParams.hpp: hashingWordSize, haploid, max_seeds,
 * constReadAhead); fsmc_identify is fsmc_identify_ex with {64, 1, 0, 10}.
 *   word_size   sites per word, 1..64: word w of a haplotype holds sites w*word_size .. +word_size-1 in its LOW bits
 *               (Individuals.hpp:39-50); from/to and the centimorgan test count in these words.
 *   haploid     0: matches are keyed by INDIVIDUAL pairs (ExtendHash.hpp:47-70: haplotype ids rounded down to the
 *               individual, rows 2k and 2k+1 of the matrix): any of the (up to four) haplotype pairs of the job extends
 *               the pair's one interval, the two haplotypes of one individual form a pair, and the candidate names
 *               rows (2 * ind_a, 2 * ind_b), ind_a <= ind_b (locationToPair).  n_haps must be even.
 *   max_seeds   != 0: a seed with more than max_seeds haplotypes is split by the NEXT word, and again, while the words
 *               read ahead last (SeedHash.hpp:41-85): only the pairs that also share those words are extended, to the
 *               last word looked at.
 *   read_ahead  words buffered ahead of the current one, 1..32 (FastSMC.cpp:186-195: while word c is processed
 *               min(n_words, c + read_ahead) words have been read); bounds the splitting above. */
typedef struct {
  uint32_t word_size;
  uint32_t haploid;
  int32_t max_seeds;
  uint32_t read_ahead;
} fsmc_identify_opts;
int fsmc_identify_ex(fsmc_ctx* ctx, const uint64_t* words, uint32_t n_haps, uint32_t n_words,
                     const uint32_t* global_ids, const fsmc_job_window* job, const float* gen_pos, uint32_t n_sites,
                     int32_t gap, float skip, float min_m, const fsmc_identify_opts* opts, fsmc_candidate* out,
                     size_t cap, size_t* n_out);
/* After an fsmc_identify that returned FSMC_EOVERFLOW (*n_out = the count): the complete candidate list of that call, in
 * emission order -- it was finished and kept on the device, so the caller allocates *n_out records and fetches them
 * instead of running the identification a second time.  The kept list is released by the fetch. */
int fsmc_identify_fetch(fsmc_ctx* ctx, fsmc_candidate* out, size_t cap, size_t* n_out);

int fsmc_sync(fsmc_ctx* ctx);
/* Device time (ms, hipEvent) of the last decode call's kernel(s) -- a call of several launches (the sums of more batches
 * than fit one launch) from its first launch to the end of its last, the plane additions in between included; valid
 * after a sync/fetch. */
int fsmc_last_kernel_ms(fsmc_ctx* ctx, float* ms);

/* Diagnostic: shader-clock cycles summed over waves since the last call, {pass B, beta rebuild, alpha sweep,
 * groups}; all zero unless the library was built with -DFSMC_PHASE_STAMPS (never the shipped build). */
int fsmc_phase_cycles(fsmc_ctx* ctx, uint64_t* out, size_t n);

/* Convenience: upload work list + launch + fetch. */
int fsmc_decode_ibd(fsmc_ctx* ctx, const fsmc_model* m, const fsmc_pair* pairs, size_t n_pairs,
                    const fsmc_group* groups, size_t n_groups, uint32_t flags, fsmc_ibd_record* out, size_t cap,
                    size_t* n_out);

/* Posterior of every pair of the resident work list over its group's window, in the reference's batch layout
 * per group: out[group][pos - from][k][lane 0..63], i.e. group g starts at out + offsets[g] floats where
 * offsets[g] = 64*K*sum_{h<g}(to_h - from_h).  Lanes >= n_pairs are zero.  out_floats = capacity of out. */
int fsmc_decode_posteriors(fsmc_ctx* ctx, const fsmc_model* m, float* out, size_t out_floats);

/* writePerPairOutput: mean[n_pairs][S] = sum_k post*exp_times[k]; map[n_pairs][S] = first argmax_k post.
 * Either may be NULL.  Requires whole-sequence groups (from = 0, to = S), as in the reference (HMM.cpp:1378). */
int fsmc_decode_per_pair(fsmc_ctx* ctx, const fsmc_model* m, const float* exp_coal_times, float* mean, int32_t* map);

/* writePerPairOutput's posterior tables (HMM.cpp:1378-1392; DecodePairsReturnStruct::perPairPosteriors and
 * sumOfPosteriors) for the resident work list, in the layout the API hands out:
 *   post_rows[i][k * S + pos] = posterior(pair i, pos, k) * exp_coal_times[k]   (one fp32 multiply; HMM.cpp:1382)
 *   sum[k * S + pos]          = ((sum[k * S + pos] + v_0) + v_1) + ...          (the same values, added pair after pair
 *                               in work-list order onto what the caller passes in)
 * post_rows: n_pairs pointers to [K][S] floats each, or NULL; sum: [K][S], read AND written, or NULL; at least one of
 * the two.  Several calls over consecutive parts of a pair list, each continuing the sum of the one before, give the
 * bits of one call over the whole list.  The work list goes through the device in slices of groups
 * (fsmc_ctx_set_pair_posterior_slice), the rows leave through pinned buffers while the next slice decodes: memory is
 * bounded by the slice, and with sum alone only [K][S] floats cross the bus each way.  Requires whole-sequence groups
 * (from = 0, to = S; FSMC_EINVAL otherwise), as in the reference. */
int fsmc_decode_pair_posteriors(fsmc_ctx* ctx, const fsmc_model* m, const float* exp_coal_times,
                                float* const* post_rows, float* sum);

/* Per site, the smallest posterior mean / MAP state over the pairs of the resident work list and which pair has it:
 * what DecodePairsReturnStruct::finaliseCalculations computes from the [pairs][sites] matrices of writePerPairOutput
 * (DecodePairsReturnStruct.hpp:105-118), without those matrices leaving the device.  Exactly that loop in work-list
 * order: pair 0 seeds (best, arg); pair i replaces them only when v_i < best (a strict fp32 / int32 compare: ties keep
 * the earlier pair, -0.f does not beat +0.f, a NaN never replaces anything and a NaN seed stays); arg = pair_base + i.
 *   min_mean / argmin_mean: [S] each, both or neither; min_map / argmin_map: [S] each, both or neither; at least one
 *   pair of outputs.
 *   pair_base == 0: the first pair of the work list is the seed, what the arrays hold is ignored.
 *   pair_base  > 0: the arrays are the state of a chain that earlier calls began (over pairs 0 .. pair_base - 1 of a
 *                   longer list) and this call continues: a carried value that ties with a new one stays.  Several
 *                   calls over consecutive parts of a list give the bits of one call over the whole list.
 * The work list goes through the device in slices of groups (fsmc_ctx_set_pair_minima_slice); 4 * S bytes per output
 * cross the bus each way (in: only when pair_base > 0).  fsmc_last_kernel_ms spans every decode and every reduction of
 * the call.  FSMC_EINVAL: no output pair or half of one; a group that is not the whole sequence (from = 0, to = S), as
 * in the reference; pair_base + n_pairs beyond INT32_MAX. */
int fsmc_decode_pair_minima(fsmc_ctx* ctx, const fsmc_model* m, const float* exp_coal_times, uint64_t pair_base,
                            float* min_mean, int32_t* argmin_mean, int32_t* min_map, int32_t* argmin_map);

/* Per pair of the resident work list, summaries over bins of sites of the rows fsmc_decode_per_pair would write
 * (mean[i][t], map[i][t]), without those rows leaving the device.  bin_edges: n_bins + 1 int32 values, strictly ascending,
 * 0 <= bin_edges[0], bin_edges[n_bins] <= S; bin b is sites [bin_edges[b], bin_edges[b + 1]), n of them; sites outside
 * [bin_edges[0], bin_edges[n_bins]) belong to no bin.  Outputs, [n_pairs][n_bins] each (work-list order) or NULL:
 *   bin_mean: the mean of mean[i][t] over the bin in a defined fp64 order: slot j (0 <= j < 64) starts at +0.0 and adds
 *     (double)mean[i][t] for t = bin_edges[b] + j, + 64, ... in ascending order; then for stride = 32, 16, 8, 4, 2, 1:
 *     a[j] = a[j] + a[j + stride] for j < stride; the result is (float)(a[0] / (double)n): one fp64 divide, one
 *     round-to-nearest conversion.
 *   bin_min_mean / bin_argmin_mean (both or neither): the smallest mean[i][t] of the bin under `<` and the lowest
 *     absolute site index t that has it (numpy's argmin on the slice; a NaN in the bin wins, lowest site first).
 *   bin_min_map / bin_argmin_map (both or neither): the same for the MAP state.
 * The mean rows are decoded only when a mean output is asked for, the MAP rows only when a MAP output is.  The work list
 * goes through the device in slices of groups (fsmc_ctx_set_pair_bins_slice), which are independent; 4 * n_bins bytes a
 * pair and output cross the bus.  fsmc_last_kernel_ms spans every decode and every reduction of the call (with several
 * slices also the copies of their outputs in between).  FSMC_EINVAL: null times or edges; no output; a minimum without
 * its argmin or the reverse; n_bins == 0; edges not strictly ascending or outside [0, S]; a group that is not the whole
 * sequence (from = 0, to = S). */
int fsmc_decode_pair_bins(fsmc_ctx* ctx, const fsmc_model* m, const float* exp_coal_times, const int32_t* bin_edges,
                          size_t n_bins, float* bin_mean, float* bin_min_mean, int32_t* bin_argmin_mean,
                          int32_t* bin_min_map, int32_t* bin_argmin_map);

/* Per pair of the resident work list, the likelihood of the pair's observations under the model, from the forward sweep
 * alone: one of the decode's three sweeps, no beta rows, no workspace (fsmc_pair_loglik.h; lane-per-pair kernels, K <=
 * 128).  For a pair whose group is the whole sequence let sum[t] (fp32) be the scaling sum of the forward vector at site
 * t: the `sums` of calculateScalingBatch at HMM.cpp:745 and 776-779, accumulated from 0.f over k ascending in separately
 * rounded adds (ghost states add +0).  Array mode: sum[0] comes from pi * emission and sum[t] from the step into site t.
 * Sequence mode: the un-normalised half-step across the gap contributes no sum of its own; sum[t] is the sum after the
 * site step that follows it (HMM.cpp:760-779).  The likelihood, the product of the sums, is carried as a mantissa /
 * exponent pair so that the result is bit-reproducible:
 *     m = 1.0 (fp64); e = 0 (int32)
 *     for t = 0 .. S-1, ascending:
 *         m = m * (double)sum[t]                                       -- one fp64 multiply, round to nearest
 *         if (m != 0 && isfinite(m)) { m = frexp(m, &de); e += de; }   -- exact
 *   mant[i] (float64, in [0.5, 1), or 0 / inf / NaN) and expo[i] (int32), [n_pairs] each in work-list order.  The
 *     log-likelihood is log(mant) + expo * ln 2, formed by the caller in fp64: a zero sum gives -inf, a NaN stays a NaN.
 *   bin_mant[i * n_bins + b], bin_expo[i * n_bins + b]: the same recurrence started afresh at m = 1, e = 0 at site
 *     bin_edges[b] and taken at site bin_edges[b + 1] - 1: the conditional likelihood of the bin's observations given
 *     everything before it.  Sites outside every bin count towards the total only; the total is a chain of its own over
 *     all sites, not a combination of the bins.
 * mant / expo: both or neither; bin_mant / bin_expo: both or neither, and only with edges; one pair of outputs at least.
 * bin_edges: n_bins + 1 int32 values under the rules of fsmc_decode_pair_bins; read only with the bin outputs.  The work
 * list goes through the device in slices of groups (fsmc_ctx_set_pair_loglik_slice), which are independent; 12 bytes a
 * pair and output cross the bus.  fsmc_ctx_last_kernel reports the member; fsmc_last_kernel_ms spans the call's launches
 * (with several slices also the copies of their outputs in between).  FSMC_EINVAL, nothing touched: a mantissa without
 * its exponent or the reverse; no output; bin outputs without edges, n_bins == 0, edges not strictly ascending or outside
 * [0, S]; a group that is not the whole sequence (from = 0, to = S); a model of more than 128 states (the wave-group
 * and any-K kernels have no forward-only member). */
int fsmc_decode_pair_loglik(fsmc_ctx* ctx, const fsmc_model* m, const int32_t* bin_edges, size_t n_bins, double* mant,
                            int32_t* expo, double* bin_mant, int32_t* bin_expo);

/* Per pair of the resident work list, the single most probable JOINT state sequence of the pair under the model (the
 * Viterbi path) and its probability, from a max-product forward sweep with back-pointers and a traceback
 * (fsmc_pair_viterbi.h; lane-per-pair kernels: K <= 128, array mode, whole-sequence groups).  The map of
 * fsmc_decode_per_pair is the per-site argmax of the marginals; this is the argmax over whole paths.  The transition is
 * semiseparable with non-negative entries, so max distributes over the forward step's recurrences as + does.  The
 * contract; every operation is one separately rounded IEEE fp32 operation, every comparison exactly the one written:
 *     site 0:   v[k] = pi[k] * em0[k]
 *     site t >= 1, from the scaled vector p of site t-1, table row step_row[t]:
 *       suffix maximum, k descending:  mC[K-1] = p[K-1], cI[K-1] = K-1;
 *           for k = K-2 .. 0:  if (p[k] >= mC[k+1]) (mC[k], cI[k]) = (p[k], k) else = (mC[k+1], cI[k+1])
 *       MU = 0.f, uI = 0
 *       for k = 0 .. K-1 ascending:
 *           d = D[k] * p[k]
 *           if k >= 1:  cand = U[k-1] * p[k-1];  car = cR[k-1] * MU
 *                       if (car >= cand) MU = car  (uI stays)  else (MU, uI) = (cand, k-1)
 *                       (best, arg) = (MU, uI);  if (d > best) (best, arg) = (d, k)
 *           else        (best, arg) = (d, 0)
 *           if k < K-1: l = B[k] * mC[k+1];  if (l > best) (best, arg) = (l, cI[k+1])
 *           v[k] = em_t[k] * best;   psi[t][k] = arg
 *     every site: sum[t] = ((0.f + v[0]) + v[1]) + ...  (k ascending);  delta_t = v * (1.0f / sum[t])
 *     end:      x[S-1] = the smallest k with delta_{S-1}[k] > every earlier one (strict >, k ascending)
 *               x[t-1] = psi[t][x[t]]   for t = S-1 .. 1
 *     P(path, observations): m = 1.0, e = 0; for t ascending: (m, e) <- (m, e) * (double)sum[t], the recurrence of
 *               fsmc_decode_pair_loglik; then once more with (double)delta_{S-1}[x[S-1]]
 *   em_t is the emission row of the pair's observation class at site t.  On equal values the smaller predecessor index
 *   wins everywhere.  Ghost states of a padded kernel member (p = 0, zero table entries) are never chosen.
 *   states[i * S + t] = x[t] (uint8, in [0, K)); mant[i] (float64) and expo[i] (int32): the probability as in
 *     fsmc_decode_pair_loglik, log(mant) + expo * ln 2 its logarithm; [n_pairs] in work-list order.
 *   A pair whose mantissa is 0 or not finite (a zero scaling sum somewhere) has mantissa and exponent as defined; its
 *     states only lie in [0, K).  The other pairs of its group are exact.
 * states may be NULL (the probabilities alone: no second sweep, no traceback); mant / expo: both or neither; one output
 * at least.  A wave keeps K bytes of back-pointers a pair and site in the decode's workspace; a sequence whose
 * back-pointers do not fit is swept in chunks: a first sweep leaves a checkpoint a chunk, then chunk by chunk from the
 * end a second sweep rebuilds the chunk's back-pointers and the traceback walks it (fsmc_ctx_set_chunk_sites and
 * fsmc_ctx_set_workspace_limit are honoured, fsmc_ctx_last_plan and fsmc_ctx_last_kernel report; results do not depend
 * on them).  The work list goes through the device in slices of groups (fsmc_ctx_set_pair_viterbi_slice), which are
 * independent; the state rows leave through pinned buffers.  fsmc_last_kernel_ms spans the call's launches (with several
 * slices also the copies in between).  FSMC_EINVAL, nothing touched: a mantissa without its exponent or the reverse; no
 * output; a group that is not the whole sequence (from = 0, to = S); a model of more than 128 states; a sequence-mode
 * model (its half-step doubles the trellis). */
int fsmc_decode_pair_viterbi(fsmc_ctx* ctx, const fsmc_model* m, uint8_t* states, double* mant, int32_t* expo);

/* Per pair of the resident work list, n_samples state sequences drawn from the JOINT posterior over state sequences
 * given the pair's observations: forward filtering with backward sampling (fsmc_pair_samples.h; lane-per-pair kernels:
 * K <= 128, array mode, whole-sequence groups).  The Viterbi path is one point without spread, the marginals have spread
 * without dependence between neighbouring sites; these are whole tracks with the right joint law.  The transition is
 * semiseparable, so the weights of the predecessors of a state cost O(K): they are the coefficients of delta_t[i] in the
 * forward step's term for state j (HMM.cpp:799-830); the emission of t+1 is common to all i and drops out.  The
 * contract; every operation is one separately rounded IEEE fp32 operation.  delta_t is the scaled forward vector of
 * site t, exactly what fsmc_decode_pair_loglik's kernel holds after its scaling (the reference's alpha):
 *     uniform of (seed, pair, sample r, site t):
 *       Philox4x32-10, key = (seed & 0xffffffff, seed >> 32),
 *       counter = (t >> 2, r, hap_a, hap_b)          (the pair's two fields of the work list, as stored)
 *       u = float(out[t & 3] >> 8) * 2^-24           (exact, in [0, 1))
 *     pick(w[0..K-1], u):
 *       c[-1] = 0.f;  c[i] = c[i-1] + w[i]   for i ascending
 *       x = u * c[K-1]
 *       state = min(K-1, #{ i in [0, K) : c[i] <= x })   (exactly this comparison; K the model's states)
 *     site S-1:  w[i] = delta_{S-1}[i];   x[S-1] = pick(w, u(S-1))
 *     site t = S-2 .. 0, with j = x[t+1] and D, B, U the table row step_row[t+1], cR the column ratios:
 *       i > j:   w[i] = B[j] * delta_t[i]
 *       i = j:   w[j] = D[j] * delta_t[j]
 *       i < j:   g = 1.f at i = j-1;   for i = j-2 .. 0:  g = g * cR[i+1]
 *                w[i] = (U[i] * delta_t[i]) * g
 *       x[t] = pick(w, u(t))
 *   states[(i * n_samples + r) * S + t] = x[t] of sample r (uint8, in [0, K)), i in work-list order.
 *   A chosen state always has w > 0 (c[i] > x >= c[i-1]): every sampled path is one the model allows.  Ghost states of a
 *     padded kernel member (delta = 0, zero table entries) have w = +0 and are never counted and never chosen.
 *   A sample depends on (seed, hap_a, hap_b, r, t) and the data only: not on list order, groups, slices, flushes, chunk
 *     length, workspace or shard.  A pair listed twice gets the same rows; (a, b) and (b, a) are different streams.
 *   A pair with a zero scaling sum somewhere (NaN vectors) only has states in [0, K).  The other pairs of its group are
 *     exact.
 * A wave keeps 4 K bytes of forward vector a pair and site in the decode's workspace; a sequence whose vectors do not fit
 * is swept in chunks: a first sweep leaves a checkpoint a chunk, then chunk by chunk from the end a second sweep rebuilds
 * the chunk's vectors and the sampler walks it down (fsmc_ctx_set_chunk_sites and fsmc_ctx_set_workspace_limit are
 * honoured, fsmc_ctx_last_plan and fsmc_ctx_last_kernel report; results do not depend on them).  The work list goes
 * through the device in slices of groups (fsmc_ctx_set_pair_samples_slice), which are independent; the state rows leave
 * through pinned buffers.  fsmc_last_kernel_ms spans the call's launches (with several slices also the copies in
 * between).  FSMC_EINVAL, nothing touched: n_samples outside 1 ... 64; states NULL; a group that is not the whole
 * sequence (from = 0, to = S); a model of more than 128 states; a sequence-mode model (its half-step doubles the
 * trellis). */
int fsmc_decode_pair_samples(fsmc_ctx* ctx, const fsmc_model* m, int32_t n_samples, uint64_t seed, uint8_t* states);

/* Per pair of the resident work list and site t, the posterior probability, given all of the pair's observations, that
 * the state at site t is lower (p_down) or higher (p_up) than the state at site t-1: the two-slice posterior summed
 * below and above the diagonal (fsmc_pair_transitions.h; lane-per-pair kernels: K <= 128, array mode, whole-sequence
 * groups).  The marginals carry no dependence between neighbouring sites, the Viterbi path no uncertainty, and counting
 * over sampled paths costs n samples for 1 / sqrt(n); this is exact and costs about one decode.  The transition is
 * semiseparable: the backward step already forms, per state k of site t-1, the mass moving to lower states (BL[k]),
 * staying (D[k] * vec[k]) and moving to higher states (BU[k]) (getPreviousBetaBatched, HMM.cpp:986-1014).  The contract;
 * every operation is one separately rounded IEEE fp32 operation.  delta_t is the scaled forward vector of site t,
 * exactly what fsmc_decode_pair_loglik's kernel holds after its scaling (the reference's alpha).  b_t is the scaled
 * backward vector of the reference (backwardBatch, HMM.cpp:882-940): b_{S-1}[k] = 1.f * (1.0f / sum) with sum over the
 * model's K states; going down, one backward step in the order (BL + D * vec) + BU, then the scaling:
 *     site t = S-1 .. 1, with D, B, U, RR the table row step_row[t] and e the emission of the pair's class at site t:
 *       vec[k] = b_t[k] * e[k]
 *       BU[K-1] = 0.f;  BU[k] = U[k] * vec[k+1] + RR[k] * BU[k+1]       (k descending)
 *       BL[0]   = 0.f;  BL[k] = BL[k-1] + B[k-1] * vec[k-1]            (k ascending)
 *       down = up = stay = 0.f;  for k ascending over the model's K states:
 *         down = down + delta_{t-1}[k] * BL[k]
 *         stay = stay + delta_{t-1}[k] * (D[k] * vec[k])
 *         up   = up   + delta_{t-1}[k] * BU[k]
 *       z = (down + stay) + up;   r = 1.0f / z
 *       p_down[t] = down * r;     p_up[t] = up * r
 *     p_down[0] = p_up[0] = 0.f.
 *   down_rows[i * S + t] = p_down[t], up_rows[i * S + t] = p_up[t] of pair i in work-list order; 1 - p_down - p_up is
 *     the probability of no change.
 *   bin_down[i * n_bins + b] = the sum of (double)p_down[t] over the sites t of [bin_edges[b], bin_edges[b+1]), rounded
 *     once to float, in the fp64 order of bin_tail_length (fsmc_decode_pair_tail_summaries): 64 slots starting at +0.0,
 *     slot s adds the sites e[b] + s, + 64, ... ascending, then the tree a[s] = a[s] + a[s + stride] for stride = 32 ...
 *     1.  No weights, no divide: the expected number of downward changes in the bin.  bin_up likewise.
 *   Ghost states of a padded kernel member (delta = 0, zero table entries) contribute +0.f products and change nothing;
 *     the first scaling of b uses the model's K.
 *   A pair with a zero scaling sum somewhere gives whatever IEEE gives (NaN).  The other pairs of its group are exact.
 *   The results depend on the pair and the data only: not on list order, groups, slices, flushes, chunk length or
 *     workspace.
 * Any of the four outputs may be NULL, one at least must be given; with bin outputs only, the rows never leave the
 * device.  The workspace is fsmc_decode_pair_samples': forward vectors in chunks with checkpoints
 * (fsmc_ctx_set_chunk_sites and fsmc_ctx_set_workspace_limit are honoured, fsmc_ctx_last_plan and fsmc_ctx_last_kernel
 * report; results do not depend on them).  The work list goes through the device in slices of groups
 * (fsmc_ctx_set_pair_transitions_slice), which are independent; the rows leave through pinned buffers.
 * fsmc_last_kernel_ms spans the call's launches (with several slices also the copies in between).  FSMC_EINVAL, nothing
 * touched: all four outputs NULL; bin outputs without edges, or edges that are not strictly ascending inside [0, S]; a
 * group that is not the whole sequence (from = 0, to = S); a model of more than 128 states; a sequence-mode model.
 * FSMC_ENOMEM, nothing launched: the workspace limit does not hold one wave's rows. */
int fsmc_decode_pair_transitions(fsmc_ctx* ctx, const fsmc_model* m, float* down_rows, float* up_rows,
                                 const int32_t* bin_edges, int32_t n_bins, float* bin_down, float* bin_up);

/* Per pair of the resident work list and site, where the posterior mass lies, without the [K][S] tables leaving the
 * device.  post[k] is the pair's normalised fp32 posterior at the site over the model's K states (not multiplied by any
 * time).  In fp32 and in ascending k only, one add a state (the IBD scan's order, HMM.cpp:1207-1224):
 *   cdf[0] = 0.f + post[0];  cdf[k] = cdf[k-1] + post[k]
 *   tail_rows[j][i * S + t] = cdf[c - 1] for the cut c = tail_states[j], 1 <= c <= K: the probability that pair i
 *     coalesced in one of the first c states at site t.  c = K is allowed; the result is then 1 give or take an ulp.
 *   quantile_rows[j][i * S + t] = the smallest k with cdf[k] >= q under an fp32 compare, q = quantiles[j], 0 < q <= 1;
 *     K - 1 if no state reaches q (rounding can leave cdf[K-1] < 1; a NaN never compares true and gives K - 1 too).
 * Up to 8 cuts and up to 8 quantiles a call, one at least in total, in any order, duplicates allowed.  tail_rows[j] and
 * quantile_rows[j] each point at [n_pairs][S] caller memory in work-list order; every output is independent.  The work
 * list goes through the device in slices of groups (fsmc_ctx_set_pair_cdf_slice); a slice's rows leave through pinned
 * buffers while the next slice decodes; 4 bytes a pair-site and output cross the bus.  fsmc_last_kernel_ms spans every
 * decode and every reduction of the call.  FSMC_EINVAL: no output at all; more than 8 of either kind; a null array where
 * its count is non-zero; a null row pointer; a cut outside [1, K]; a quantile that is not finite or outside (0, 1]; a
 * group that is not the whole sequence (from = 0, to = S). */
int fsmc_decode_pair_cdf(fsmc_ctx* ctx, const fsmc_model* m, const int32_t* tail_states, size_t n_tail,
                         float* const* tail_rows, const float* quantiles, size_t n_quantiles,
                         int32_t* const* quantile_rows);

/* The tail probabilities of fsmc_decode_pair_cdf reduced over the pairs of the resident work list and over bins of sites,
 * without the [n_pairs][S] tail rows leaving the device.  tail[j][i][t] is exactly tail_rows[j][i * S + t] of
 * fsmc_decode_pair_cdf: the fp32 running sum cdf[c - 1] of pair i's posterior at site t, ascending k, one fp32 add a
 * state, for the cut c = tail_states[j], 1 <= c <= K.  Up to 8 cuts a call, one at least, duplicates allowed.  Outputs
 * (any may be NULL, one at least):
 *   tail_sum: [n_tail][S] float64, read AND written: tail_sum[j * S + t] = ((tail_sum[j * S + t] + (double)tail[j][0][t])
 *     + (double)tail[j][1][t]) + ..., one fp64 add a pair, in work-list order, onto what the caller passes in (pass
 *     zeros to start a sum).  Several calls over consecutive parts of a pair list, each continuing the array of the one
 *     before, give the bits of one call over the whole list; so do the slices of one call.
 *   bin_tail_mean: [n_tail][n_pairs][n_bins] float32: the mean of tail[j][i][t] over bin b, sites [bin_edges[b],
 *     bin_edges[b + 1]), n of them, in the defined fp64 order of fsmc_decode_pair_bins' bin_mean: slot s (0 <= s < 64)
 *     starts at +0.0 and adds (double)tail[j][i][t] for t = bin_edges[b] + s, + 64, ... in ascending order; then for
 *     stride = 32, 16, 8, 4, 2, 1: a[s] = a[s] + a[s + stride] for s < stride; the result is (float)(a[0] / (double)n).
 *   bin_tail_length: the same shape: the same slots and the same tree over (double)tail[j][i][t] *
 *     (double)site_weights[t] (the fp64 product of two floats is exact, so a fused multiply-add gives the same bits);
 *     the result is (float)a[0], no divide.  With site_weights[t] the centimorgans site t stands for this is the pair's
 *     expected length below the cut in the bin.
 * bin_edges: n_bins + 1 int32 values under the rules of fsmc_decode_pair_bins (strictly ascending, within [0, S]; sites
 * outside [bin_edges[0], bin_edges[n_bins]) belong to no bin); read only with a bin output.  site_weights: [S] finite
 * floats; read only with bin_tail_length.  The work list goes through the device in slices of groups
 * (fsmc_ctx_set_pair_tail_slice); 8 * S bytes a cut cross the bus each way for tail_sum and 4 * n_bins bytes a pair, cut
 * and bin output come back.  fsmc_last_kernel_ms spans every decode and every reduction of the call (with bin outputs
 * and several slices also the copies of their cells in between).  FSMC_EINVAL: no output; no cut or more than 8; a cut
 * outside [1, K]; a bin output without edges, n_bins == 0, edges not strictly ascending or outside [0, S];
 * bin_tail_length without site_weights; a weight that is not finite; a group that is not the whole sequence (from = 0,
 * to = S). */
int fsmc_decode_pair_tail_summaries(fsmc_ctx* ctx, const fsmc_model* m, const int32_t* tail_states, size_t n_tail,
                                    double* tail_sum, const int32_t* bin_edges, size_t n_bins, float* bin_tail_mean,
                                    const float* site_weights, float* bin_tail_length);

/* augmentSumOverPairs: sums[S][K] += sum over the pairs of the work list of the posterior
 * (and the 00/01/11 split when the pointers are non-NULL).  Whole-sequence groups only. */
int fsmc_decode_sums(fsmc_ctx* ctx, const fsmc_model* m, float* sums, float* sums00, float* sums01, float* sums11);
/* The same for reference batches of more than 64 pairs (DecodingParams.cpp:301 allows any multiple of 8): the reference
 * sums a whole batch over its pairs, in order, and then adds it (HMM.cpp:1054-1073).  Batch b is the consecutive groups
 * batch_first_group[b] .. batch_first_group[b+1]-1 (n_batches + 1 entries, the first 0, the last the number of groups):
 * they are decoded in turn and share one running sum, so the result is the reference's bit for bit.
 * fsmc_decode_sums treats every group as a batch of its own. */
int fsmc_decode_sums_batches(fsmc_ctx* ctx, const fsmc_model* m, const uint32_t* batch_first_group, size_t n_batches,
                             float* sums, float* sums00, float* sums01, float* sums11);

#ifdef __cplusplus
}
#endif
#endif
