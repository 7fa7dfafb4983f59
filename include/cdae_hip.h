/* cdae_hip.h — C ABI of libcdae_hip.so, the MI355X (gfx950) implementation of the CDAE training hot path.
 *
 * The reference (jasonyaw/CDAE, "libcf") has no FFI: its boundary is C++ template duck-typing —
 * Solver<Model> and Evaluation<Model> instantiated with Model = libcf::CDAE
 * (/root/reference/src/solver/solver.hpp:11-46, src/model/evaluation.hpp:113-181,
 * apps/yelp/yelp.cpp:168-199).  This header is the plain-C surface that sits *underneath* that
 * class: the repo's own host C++ (src/model/recsys/cdae.hpp, same class name and methods as the
 * reference) forwards each Model-concept call to exactly one entry point below, and CHECKs the status
 * so that the reference's abort-on-error convention (glog CHECK / LOG(FATAL)) is preserved.
 *
 *   reference interface (file:line)                         entry point
 *   -------------------------------------------------------------------------------------------
 *   CDAE::CDAE(const CDAEConfig&)        cdae.hpp:39-74      cdae_hip_create
 *   RecsysModelBase::reset               recsys_model_base.hpp:29-34
 *                                                            cdae_hip_set_interactions
 *   CDAE::reset (parameter init)         cdae.hpp:109-134    cdae_hip_init_params / cdae_hip_set_param
 *   CDAE::train_one_iteration            cdae.hpp:136-146    cdae_hip_train_epoch
 *     get_corrputed_input                cdae.hpp:361-371      (device, include/cdae_rng.h)
 *     sample_negative_item               recsys_model_base.hpp:46-57  (device, include/cdae_rng.h)
 *     train_one_user_corruption          cdae.hpp:198-358      (device kernels; explicit-input form:
 *                                                           cdae_hip_train_one_user_corruption)
 *     train_one_user_corruption with the shared parameters frozen
 *                                        cdae.hpp:198-358    cdae_hip_fold_in_rows
 *   CDAE::get_hidden_values              cdae.hpp:373-416    cdae_hip_encode
 *   CDAE::data_loss                      cdae.hpp:78-101     cdae_hip_data_loss
 *   CDAE::penalty_loss                   cdae.hpp:103-107    cdae_hip_penalty_loss
 *   CDAE::recommend (all users, top-k)   cdae.hpp:162-196    cdae_hip_recommend_all
 *   CDAE::recommend (any rated sets)     cdae.hpp:162-196    cdae_hip_recommend_rows, cdae_hip_eval_topn_rows (batched),
 *                                                            cdae_hip_recommend_user (one user)
 *   CDAE::recommend (allow list, exclusions apart from the inputs)
 *                                        cdae.hpp:162-196    cdae_hip_recommend_rows_filtered
 *   CDAE::recommend (place of named items in the whole list)
 *                                        cdae.hpp:162-196    cdae_hip_full_rank_rows
 *   CDAE::get_output_values              cdae.hpp:418-426    cdae_hip_score_rows
 *   TOPN_Evaluation::evaluate            evaluation.hpp:113-181, evaluate_rec_list :183-219
 *                                                            cdae_hip_set_test_rows + cdae_hip_eval_topn
 *   (item neighbours by dot / cosine; no reference counterpart)
 *                                                            cdae_hip_similar_items
 *   (data-parallel exchange; no reference counterpart)       cdae_hip_delta_*, cdae_hip_comm_*, cdae_hip_exchange_*,
 *                                                            cdae_hip_multi_* (Solver<CDAE>::train on N GPUs)
 *
 * Conventions: every function returns 0 on success, non-zero on failure; cdae_hip_last_error()
 * returns a thread-local message for the last failure.  No exceptions cross the boundary.  All
 * pointers are HOST pointers unless the name says `device`.  The library owns all device memory.
 * A handle is used from one host thread at a time (internally it owns one worker thread that issues the
 * sampling + sorting launches of the coming batches; cdae_hip_destroy joins it).  Parameters are fp32 row-major with the row
 * stride returned by cdae_hip_row_stride() (64, 128, 256 or 512 floats — the smallest that holds
 * num_dim; pad lanes are 0, or 1 in the AdaGrad accumulators, and stay so).
 */
#ifndef CDAE_HIP_H_
#define CDAE_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: cdae_hip_config.linear_function (in what was tail padding of the uint32 block: zero the struct before filling it),
 *    parameters CDAE_P_UU / CDAE_P_UU_AG; pipelined delta exchange entry points */
/* 3: cdae_hip_debug_sample_batch (integer-parity test hook), cdae_hip_recommend_user
 * 4: library-owned RCCL communicator + exchange schedule (cdae_hip_comm_*, cdae_hip_exchange_*), cdae_hip_multi_*
 * 5: cdae_hip_create_mf (IMF / BPR handles), CDAE_P_UB / CDAE_P_UB_AG, item-rows layout of cdae_hip_multi_*
 * 6: cdae_hip_set_profiling_families
 * 7: default batch_users capped at 256 (was 512); cdae_hip_default_batch_users, cdae_hip_batch_users; cdae_hip_user_order (IMF / BPR
 *    block schedules train in activity-grouped order; their default is one user per block)
 * 8: cdae_hip_full_output_plan
 * 9: cdae_hip_set_test_rows, cdae_hip_eval_topn, cdae_hip_multi_eval_topn (TOPN metrics on the device)
 * 10: IMF / BPR handles created with batch_users = 0 train the certified block of their model (cdae_hip_mf_default_batch_users: 16 / 8
 *     users on the BASELINE-sized data sets, was 1); BPR's phase U carries the positive item's row from pair to pair
 * 11: schedule of the user-sharded layout: cdae_hip_delta_set_combine (CDAE_COMBINE_GLOBAL_ACC), cdae_hip_multi_set_schedule
 *     (relay warm-up epochs on the single-GPU schedule, users per shard of the exchanged steps, combine rule); the drop-in IMF / BPR
 *     classes pass batch_users = 1 (the reference loop) unless CDAE_BATCH_USERS says otherwise
 * 12: cdae_hip_decode_plan, cdae_hip_set_decode_fused (which launches the sampled decode + hidden-gradient step of a handle is made of);
 *     cdae_hip_multi_steps_per_epoch, cdae_hip_multi_train_steps (a range of the exchanged steps of an epoch: what bench.py times)
 *     added under 12 (no existing entry point or structure changed): cdae_hip_recommend_rows, cdae_hip_eval_topn_rows, CDAE_NO_USER —
 *     batched top-k and TOPN for rated sets the caller supplies
 *     added under 12 (no existing entry point or structure changed): cdae_hip_score_rows, CDAE_RANK_CANDIDATES_MAX — batched scores and
 *     ranks of candidate sets the caller supplies
 *     also under 12, the version unchanged (a test hook beside cdae_hip_debug_sample_batch; nothing existing changed): cdae_hip_debug_row_pack
 *     also under 12, the version unchanged (a new entry point; nothing existing changed): cdae_hip_full_rank_rows — exact ranks of named
 *     items in a row's whole list (full-catalogue Recall@k / NDCG@k / MRR / AUC without sampling)
 *     also under 12, the version unchanged (new entry points; nothing existing changed): cdae_hip_fold_in_rows, cdae_hip_set_guest_nodes,
 *     cdae_hip_guest_nodes, CDAE_GUEST_USER — batched fold-in of user nodes for rows outside the training set, and a guest table that serves the fitted nodes
 *     to the rows entry points
 *     also under 12, the version unchanged (a new entry point; nothing existing changed): cdae_hip_recommend_rows_filtered — batched top-k
 *     with an item allow list for the call and per-row exclusions that are not inputs (or inputs that are not exclusions)
 *     also under 12, the version unchanged (a new entry point; nothing existing changed): cdae_hip_similar_items, CDAE_ITEMS_OUTPUT /
 *     CDAE_ITEMS_INPUT, CDAE_SIM_DOT / CDAE_SIM_COSINE — batched top-k item neighbours of named items by dot product or cosine
 *     also under 12, the version unchanged (new entry points; nothing existing changed): cdae_als_config, cdae_hip_create_als,
 *     cdae_hip_als_half_step, cdae_hip_als_solve_rows, cdae_hip_als_gram, CDAE_ALS_USERS / CDAE_ALS_ITEMS — WRMF fitted by alternating
 *     least squares, conjugate gradients per row on the matrix cores
 *     also under 12, the version unchanged (new entry points; nothing existing changed): cdae_warp_config, cdae_hip_create_warp,
 *     cdae_hip_warp_search, cdae_hip_warp_record_choices, cdae_hip_warp_choices, CDAE_WARP_MAX_TRY — WARP: rank-weighted pairwise
 *     matrix factorisation whose negatives are searched for on the device
 *     also under 12, the version unchanged (new entry points; nothing existing changed): cdae_fism_config, cdae_hip_create_fism,
 *     cdae_hip_fism_plan, cdae_hip_fism_set_resident — FISM: factored item similarity, the user's rows kept on chip for a visit
 *     also under 12, the version unchanged (a new entry point; nothing existing changed): cdae_hip_create_fism_pair — FISMauc, the
 *     pairwise form of FISM on the FISM handle
 *     also under 12, the version unchanged (new entry points; nothing existing changed): cdae_hip_als_set_confidence,
 *     cdae_hip_als_solve_rows_weighted, cdae_hip_als_objective — per-pair confidence weights for WRMF and the objective its
 *     half-steps minimise */
#define CDAE_HIP_ABI_VERSION 12

/* numeric values follow libcf::LossType (/root/reference/src/model/loss.hpp:10-18) */
#define CDAE_LOSS_SQUARE 0u
#define CDAE_LOSS_CROSS_ENTROPY 5u

/* parameter ids (/root/reference/src/model/recsys/cdae.hpp:430-439) */
#define CDAE_P_W 0u      /* items x K  : input embedding and, when !asymmetric, tied decoder  */
#define CDAE_P_W_AG 1u   /* AdaGrad accumulator of W                                          */
#define CDAE_P_V 2u      /* items x K  : decoder when asymmetric                              */
#define CDAE_P_V_AG 3u
#define CDAE_P_WU 4u     /* users x K  : per-user input node (north-star "V_u"), cdae.hpp:434 */
#define CDAE_P_WU_AG 5u
#define CDAE_P_B 6u      /* K          : hidden bias                                          */
#define CDAE_P_B_AG 7u
#define CDAE_P_BP 8u     /* items      : output bias b_prime                                  */
#define CDAE_P_BP_AG 9u
#define CDAE_P_UU 10u     /* users x K  : per-user gate on the input sum, linear_function only, cdae.hpp:437 */
#define CDAE_P_UU_AG 11u
#define CDAE_P_UB 12u     /* users      : user bias ub_ of the IMF / BPR handles (imf.hpp:132); not allocated for CDAE */
#define CDAE_P_UB_AG 13u
#define CDAE_P_COUNT 14u

typedef struct cdae_hip_config {
  uint32_t struct_size;      /* sizeof(cdae_hip_config), for ABI checking                  */
  uint32_t num_dim;          /* CDAEConfig::num_dim          cdae.hpp:19                   */
  uint32_t num_neg;          /* CDAEConfig::num_neg          cdae.hpp:26                   */
  uint32_t num_corruptions;  /* CDAEConfig::num_corruptions  cdae.hpp:22                   */
  uint32_t loss_type;        /* CDAE_LOSS_*                  cdae.hpp:17                   */
  uint32_t using_adagrad;    /* cdae.hpp:20 (0 -> plain SGD with L2)                       */
  uint32_t asymmetric;       /* cdae.hpp:23                                                */
  uint32_t user_factor;      /* cdae.hpp:24                                                */
  uint32_t linear;           /* cdae.hpp:25 (identity hidden activation)                   */
  uint32_t scaled;           /* cdae.hpp:27 (input scale 1/(1-q))                          */
  uint32_t tanh_act;         /* cdae.hpp:30                                                */
  uint32_t batch_users;      /* users whose encode sees the same parameter snapshot; 1 ==  */
                             /* the reference's strictly sequential schedule; 0 -> default */
                             /* (cdae_hip_default_batch_users: num_users/160 rounded down   */
                             /* to 32, within [32, 256] — the accuracy envelope's bound)    */
  uint32_t full_output;      /* 1: every unrated item is a negative with target 0 (north-star */
                             /* extension; num_neg is ignored): dense decode on the MFMA cores, */
                             /* per-block summed decoder gradient            */
  uint32_t linear_function;  /* cdae.hpp:29: h = Uu[u] (.) (scale * sum W[k]) + b + Wu[u], Uu trained */
                             /* (fills what used to be alignment padding: struct_size is unchanged)   */
  double lambda;             /* cdae.hpp:15 */
  double learn_rate;         /* cdae.hpp:16 */
  double corruption_ratio;   /* cdae.hpp:21 */
  double beta;               /* cdae.hpp:28 */
} cdae_hip_config;

typedef struct cdae_hip_stats {
  double wall_seconds;       /* host wall-clock of the call, stream-synchronised            */
  uint64_t users;            /* user-corruption units trained                               */
  uint64_t examples;         /* (user, output item) pairs decoded = sum (1+num_neg) n_u     */
  uint64_t batches;
  /* accumulated HIP-event milliseconds per kernel family; filled only when profiling is on */
  double ms_sample, ms_sort, ms_encode, ms_decode, ms_hidden, ms_input;
  uint64_t launches_decode;
} cdae_hip_stats;

typedef struct cdae_hip cdae_hip_t;

const char* cdae_hip_last_error(void);
int cdae_hip_abi_version(void);

int cdae_hip_create(const cdae_hip_config* cfg, int device_id, cdae_hip_t** out);
int cdae_hip_destroy(cdae_hip_t* h);

/* CSR of the training interactions: row_ptr[num_users+1], col_idx[nnz] sorted ascending and unique
 * inside each row (the reference's uid -> {iid -> label} hashtable, data-inl.hpp:414-429, with the
 * always-1 labels of yelp.cpp:60-66 dropped).  Copied; the caller keeps its arrays.  A call refused for its arguments (a
 * malformed row, an owned-user range outside the users, a batch whose Z would exceed 2 GiB or whose list 2^32 examples) leaves the
 * handle with the data set and parameters it had; a call that fails later (a device allocation) leaves it without a data set. */
int cdae_hip_set_interactions(cdae_hip_t* h, uint64_t num_users, uint64_t num_items,
                              const int64_t* row_ptr, const uint32_t* col_idx);

uint32_t cdae_hip_row_stride(const cdae_hip_t* h);

/* The batch_users a handle created with batch_users = 0 takes for `num_users` users (chosen at cdae_hip_set_interactions):
 * num_users / 160 rounded down to a multiple of 32, within [32, CDAE_DEFAULT_BATCH_USERS_MAX].  The upper bound is the largest
 * size for which the driver-run accuracy tests hold the Recall@10 / loss-curve tolerance against the strictly sequential
 * reference schedule (cdae.hpp:136-146) at the BASELINE shapes; larger values are accepted when asked for explicitly and are
 * a throughput setting outside that envelope.  cdae_hip_batch_users: the value a handle is using (0 before
 * cdae_hip_set_interactions when the default was asked for). */
#define CDAE_DEFAULT_BATCH_USERS_MAX 256u
uint32_t cdae_hip_default_batch_users(uint64_t num_users);
uint32_t cdae_hip_batch_users(const cdae_hip_t* h);

/* Which launches the SAMPLED step's decode (cdae.hpp:225-293) and hidden-gradient sum (cdae.hpp:240,248,277,285) of this handle are
 * made of, chosen at cdae_hip_set_interactions from the data set and batch_users (0 before it):
 *   *hot_rows   item rows that take a wavefront of their own (the most popular: >= 48 expected positives per batch);
 *   *late_rows  the first of them (at most 64) whose hidden-gradient terms the per-user finish adds itself instead of the gather;
 *   *fused      1: decode and gather are ONE launch (the gather waits, example by example, for the g of rows that finish early
 *               and never for the late rows); 0: two launches.  Either order gives the same bits.
 * Any pointer may be NULL. */
int cdae_hip_decode_plan(const cdae_hip_t* h, uint32_t* hot_rows, uint32_t* late_rows, uint32_t* fused);
/* allow = 0: this handle takes the two separate launches (same bits).  REQUIRED for handles whose training calls may be in flight on the
 * SAME device at the same time as another handle's (two models trained from two threads; the logical shards of cdae_hip_multi_* with
 * equal device ids, for which the library does it itself): inside the fused launch the gather wavefronts hold their slots while they wait
 * for rows of the same launch, and with two such launches on one device each can keep the other's row workgroups from being dispatched
 * — the waits are bounded and end in an error from cdae_hip_synchronize, not in a hang, but the epoch is lost.  One handle per device
 * at a time (the reference's own use: one model, one training loop) needs nothing. */
int cdae_hip_set_decode_fused(cdae_hip_t* h, int allow);

/* Which launches the full-output decode (cdae_hip_config.full_output; the reference has no counterpart: its training decode is
 * always sampled, cdae.hpp:217-293) of this handle is made of, once cdae_hip_set_interactions has run — for a caller that prices
 * the kernel families cdae_hip_get_stats times (bench.py: which of the three products are inside the "decode" family):
 *   CDAE_PLAN_FUSED_DECODE  K <= 256: forward product, loss' and hidden-gradient product in one launch (full_decode_fused_kernel)
 *   CDAE_PLAN_GEMM2_TN      K > 256: hg = G D read from G^T and the row-major decoder image (gemm_tn_bf16_kernel; GEMM 1 writes no G)
 *   CDAE_PLAN_ROWS_FUSED    K > 256, >= 32768 items: dD = G^T Z and the row steps in one launch (gemm3_rows_fused_kernel),
 *                           timed in the "input" family — the "decode" family then holds two of the three products
 * 0 for a sampled-decode handle. */
#define CDAE_PLAN_FUSED_DECODE 1u
#define CDAE_PLAN_GEMM2_TN 2u
#define CDAE_PLAN_ROWS_FUSED 4u
uint32_t cdae_hip_full_output_plan(const cdae_hip_t* h);

/* A data-parallel rank holds only its own users (rows re-based to 0).  The random streams of
 * include/cdae_rng.h are keyed by GLOBAL user id = offset + local row, so a sharded run draws the
 * same masks and negatives as a single-GPU run over all users.  Default 0. */
int cdae_hip_set_user_id_offset(cdae_hip_t* h, uint64_t global_id_of_local_user_0);

/* reset(): W, V, Wu ~ U(-1,1) * 4*sqrt(6/(I+K)), accumulators 1e-4, biases 0 (cdae.hpp:109-134),
 * drawn from the CDAE_STREAM_INIT counter stream of include/cdae_rng.h.  Wu rows are keyed by GLOBAL user id
 * (cdae_hip_set_user_id_offset): a shard initialises its rows to what a single-GPU run would. */
int cdae_hip_init_params(cdae_hip_t* h, uint64_t seed);

/* dense [rows x num_dim] (or [n]) fp32 host arrays, unpadded */
int cdae_hip_set_param(cdae_hip_t* h, uint32_t which, const float* host, size_t count);
int cdae_hip_get_param(cdae_hip_t* h, uint32_t which, float* host, size_t count);
/* The device array itself (row stride cdae_hip_row_stride(), padded_count elements).  The pointer is WRITABLE: the call marks the
 * full-output path's bf16 images of the decoder stale, so a caller that writes parameters through it trains on what it wrote (write
 * before the next training call, not during one).  Refused for the user-indexed arrays (Wu, Uu, user bias) of an IMF / BPR handle with
 * batch_users > 1, whose rows are stored in training order (cdae_hip_user_order), not by user id. */
int cdae_hip_param_device_ptr(cdae_hip_t* h, uint32_t which, void** device_ptr, size_t* padded_count);

/* One pass over users [u_begin, u_end) x num_corruptions in batches of batch_users
 * (train_one_iteration, cdae.hpp:136-146).  train_epoch == train_users over all users. */
int cdae_hip_train_epoch(cdae_hip_t* h, uint64_t seed, uint32_t epoch, cdae_hip_stats* stats);
int cdae_hip_train_users(cdae_hip_t* h, uint64_t seed, uint32_t epoch, uint64_t u_begin,
                         uint64_t u_end, cdae_hip_stats* stats);
/* Asynchronous forms.  enqueue_users = train_users without the final host synchronisation (several calls
 * queue back to back on the library's stream; the call returns when its batches are QUEUED, and since round 6 it paces
 * itself on the side streams: before it queues a batch it looks, for at most 200 us, whether that batch's sampled and
 * sorted lists are complete, so that the training stream need not wait for them — a call of n batches returns about
 * two batches before the device has trained them, not n); prefetch_users runs only the sampling + sorting of the leading
 * batch(es) of a range on the side stream(s) — as many as the library looks ahead: one, or two where the second
 * prep lane is on — so that it overlaps whatever the caller does next (e.g. the RCCL all-reduce of the
 * data-parallel exchange); later train/enqueue calls for the same (seed, epoch) starting at the same user
 * pick the prepared batches up, one-batch calls included.  collect_stats synchronises and returns the counters (and, with profiling
 * on, the HIP-event kernel times) accumulated since the previous train_users / collect_stats. */
int cdae_hip_enqueue_users(cdae_hip_t* h, uint64_t seed, uint32_t epoch, uint64_t u_begin, uint64_t u_end);
int cdae_hip_prefetch_users(cdae_hip_t* h, uint64_t seed, uint32_t epoch, uint64_t u_begin, uint64_t u_end);
int cdae_hip_collect_stats(cdae_hip_t* h, cdae_hip_stats* stats);

/* The reference's public per-user step with the caller's own corrupted input set,
 * train_one_user_corruption(uid, input_set, output_set) (cdae.hpp:198-200; output_set is the user's
 * train row), plus the negatives the reference would draw at cdae.hpp:217-220.  Known-answer tests use it
 * to feed fixed masks and negatives (duplicates allowed, processed in the given order). */
int cdae_hip_train_one_user_corruption(cdae_hip_t* h, uint64_t uid, const uint32_t* input_items,
                                       size_t n_input, const uint32_t* negative_items, size_t n_negative);
/* Developer/benchmark aid: period 0 = off; k >= 1 = HIP events (on the stream each kernel is launched on) around the
 * kernel families of every k-th batch; cdae_hip_stats.ms_* / launches_decode then cover the sampled batches only. */
int cdae_hip_set_profiling(cdae_hip_t* h, int period);
/* ... restricted to the families in `mask` (bit CDAE_FAMILY_*; default all): an event pair costs ~6 us of stream time, so a
 * benchmark times only the family its roofline needs inside its timed region. */
#define CDAE_FAMILY_SAMPLE 0
#define CDAE_FAMILY_SORT 1
#define CDAE_FAMILY_ENCODE 2
#define CDAE_FAMILY_DECODE 3
#define CDAE_FAMILY_HIDDEN 4
#define CDAE_FAMILY_INPUT 5
int cdae_hip_set_profiling_families(cdae_hip_t* h, uint32_t mask);
int cdae_hip_synchronize(cdae_hip_t* h);

/* Test hook for the INTEGER work of the path (bit-exact parity, tests/test_gpu_integer.py): runs the sampling, the
 * item sort and the segmentation of ONE batch — users [u_begin, u_begin + n_users) (n_users <= batch_users),
 * corruption `cidx` — exactly as cdae_hip_train_users would (get_corrputed_input cdae.hpp:361-371, sample_negative_item
 * recsys_model_base.hpp:46-57 / cdae.hpp:217-220) and copies the example lists back instead of training on them:
 *   ex_item / ex_val [E]          user-major: per user its n_u train items, then its n_u * num_neg negatives;
 *                                 val = example index << 32 | slot | target << 30 | is_input << 31
 *   sorted_item / sorted_val [E]  the same list stably sorted by item (user order inside an item); sorted_val also
 *                                 carries dup_prev << 28 | dup_next << 29 (neighbour in the row is the same user's)
 *   seg_begin / seg_end [num_items]   sorted range of every item (0, 0 for items without examples)
 *   dup_of_pos / dup_of_ex [E]    correction-row number of every second-or-later duplicate negative, by sorted
 *                                 position / by example (0xFFFFFFFF elsewhere); the numbering itself is arbitrary
 * E = (1 + num_neg) * (train items of the batch's users) (full_output: the positives only); *n_examples is the
 * capacity of the arrays on entry and E on return.  Any output pointer may be NULL. */
int cdae_hip_debug_sample_batch(cdae_hip_t* h, uint64_t seed, uint32_t epoch, uint64_t u_begin, uint32_t n_users,
                                uint32_t cidx, uint32_t* ex_item, uint64_t* ex_val, uint32_t* sorted_item,
                                uint64_t* sorted_val, uint32_t* seg_begin, uint32_t* seg_end, uint32_t* dup_of_pos,
                                uint32_t* dup_of_ex, uint64_t* n_examples);

/* Test hook beside cdae_hip_debug_sample_batch (tests/test_gpu_row_pack.py): prepares the same ONE batch the way training would and
 * copies back its ROW PACK — the rows of the decode's four-rows-per-wavefront role, i.e. popularity ranks [hot_rows, num_items)
 * (cdae_hip_decode_plan), ordered by this batch's segment length, longest first, so that the four rows of a wavefront end together.
 * out_records holds *n_records records of four uint32 each on return: {item, sorted begin, sorted end, popularity rank}; the count is
 * num_items - hot_rows rounded up to a multiple of four, the fill records are {0, 0, 0, 0xFFFFFFFF}.  The order among rows of equal
 * length is arbitrary.  *n_records is the capacity of out_records (in records) on entry; 0 on return for a handle or batch that has
 * no pack (num_dim > 256, full_output, IMF / BPR, item shards, a batch without examples).  out_records may be NULL. */
int cdae_hip_debug_row_pack(cdae_hip_t* h, uint64_t seed, uint32_t epoch, uint64_t u_begin, uint32_t n_users, uint32_t cidx,
                            uint32_t* out_records, uint64_t* n_records);

/* z for `n` users (get_hidden_values, cdae.hpp:373-416).  mode 0: full train row, scale 1 (the
 * inference form, cdae.hpp:169); mode 1: training corruption of (seed, epoch, corruption 0) with the
 * configured scale.  Z is [n x num_dim] fp32 on the host.  `uids` is any list: any user any number of times, in any order.
 * The input sum takes the order cdae_hip_recommend_rows documents (groups of `unit` consecutive positions of the row, each group's
 * kept rows added from 0 in ascending position, the group sums added from 0 in group order); the finish, element by element in fp32:
 * acc = acc * Uu[u] (linear_function only, a rounded product), h = fmaf(acc, scale, b) — ONE rounding —, h = h + Wu[u]
 * (user_factor only), z = act(h).  Both are part of the contract (tests/encode_ref.py restates them).
 * Training encodes a batch of more than 768 users with exactly these two launches.  A batch of at most 768 users takes one launch
 * (encode_users_kernel) with 16 wavefronts per user: wavefront w adds the group sums w, w + 16, w + 32, ... from 0 in that order,
 * then the 16 wavefront sums are added from 0 in wavefront order, and the finish is the one above.  For a row of at most 16 groups
 * (1024 items at unit 64) that is the same sum in the same order; beyond 16 groups it is a different association of the same
 * terms, so the training z of such a row may differ from cdae_hip_encode(mode 1) in the last bits. */
int cdae_hip_encode(cdae_hip_t* h, uint64_t seed, uint32_t epoch, int mode, const uint32_t* uids,
                    size_t n, float* Z);

/* data_loss (cdae.hpp:78-101) with the CDAE_STREAM_LOSS_CORRUPT masks; penalty_loss (cdae.hpp:103-107) */
int cdae_hip_data_loss(cdae_hip_t* h, uint64_t seed, uint32_t epoch, double* out);
int cdae_hip_penalty_loss(cdae_hip_t* h, double* out);

/* recommend() for users [u_begin, u_end): top-k unrated items by W'[i].z + b'[i], descending score,
 * ties -> lower item id first (heap.hpp:44-52 + utils.hpp:16-19 with ascending scan order).  num_dim <= 256 and topk <= 16
 * run on the matrix cores (all users of a chunk per launch); any other combination — and any item count — takes the
 * general one-workgroup-per-user path.
 * A user with fewer than topk unrated items gets them all, in that order, and 0xFFFFFFFF in every surplus place, on both
 * paths and through the item-rows merge of cdae_hip_multi_recommend_all (the reference's heap returns a shorter list there,
 * cdae.hpp:181-188); a rated item is never returned.
 * out is [(u_end-u_begin) x topk] uint32 on the host. */
int cdae_hip_recommend_all(cdae_hip_t* h, uint64_t u_begin, uint64_t u_end, uint32_t topk,
                           uint32_t* out);

/* TOPN_Evaluation::evaluate (evaluation.hpp:113-181) with evaluate_rec_list (evaluation.hpp:183-219) on the device: the top-`topk`
 * list of EVERY user over the items outside the user's train row (what cdae_hip_recommend_all returns) is scored against the
 * user's validation row without leaving the GPU.  cdae_hip_set_test_rows hands the validation rows over once per data set — CSR
 * over the handle's users, items ascending and unique inside a row (the uid -> {iid} table evaluation.hpp:118-120 rebuilds on
 * every call); copied.  cdae_hip_eval_topn returns
 *   rets[8] = P@1 P@5 P@10 R@1 R@5 R@10 MAP@5 MAP@10, each the sum over the users WITH test items of r / (number of such users),
 *             added in user order: the bits of the reference's sequential loop (evaluation.hpp:160-166) in fp64;
 *   hits[3] = hits in the first 1 / 5 / 10 places summed over all users (integers; may be NULL);
 *   ids_out = the [num_users x topk] table itself (may be NULL: then nothing but 16 numbers crosses PCIe).
 * topk is what the evaluation asks recommend() for (10, evaluation.hpp:145); only the first 20 places are scored (:186). */
int cdae_hip_set_test_rows(cdae_hip_t* h, const int64_t* test_row_ptr, const uint32_t* test_col);
int cdae_hip_eval_topn(cdae_hip_t* h, uint32_t topk, double* rets8, uint64_t* hits3, uint32_t* ids_out);

/* recommend(uid, topk, rated_item_set) (cdae.hpp:162-196) for a rated set that is NOT the user's train row: the hidden
 * layer is encoded from `rated_items` (scale 1, cdae.hpp:169) and exactly those items are excluded (cdae.hpp:177-179).
 * Items need not be sorted; duplicates are an error.  out is [topk] uint32 on the host. */
int cdae_hip_recommend_user(cdae_hip_t* h, uint64_t uid, const uint32_t* rated_items, size_t n_rated, uint32_t topk,
                            uint32_t* out);

/* recommend(uid, topk, rated_item_set) for MANY rated sets at once, none of which has to be a train row: the test-phase protocol
 * (rated = train + validation), fold-in of held-out users, serving of sessions that changed since training.
 *   rows     row_ptr[n_rows + 1] / col: a host CSR of rated sets, items ascending and unique inside a row (validated: an unsorted,
 *            duplicate or out-of-range item is an error that names the row); a row may be empty.  cdae_hip_recommend_rows with n_rows == 0 succeeds and touches nothing
 *            (cdae_hip_eval_topn_rows with n_rows == 0 has no row with targets: its error below).
 *   uids     uids[r] = the local user whose Wu row (and Uu row under linear_function) row r takes; any user any number of times.
 *            CDAE_NO_USER: the row has no user node — a Wu row of zeros that is still added and a Uu row of ones, i.e. the arithmetic
 *            of a real user with those rows.  uids == NULL: every row is CDAE_NO_USER.  CDAE_GUEST_USER(i): node i of the handle's guest
 *            table (below: cdae_hip_set_guest_nodes, cdae_hip_fold_in_rows) — an error when i is at or beyond the table's size or no
 *            table is set.  Any other id >= num_users is an error.
 *   hidden   get_hidden_values(uid, rated_set) with scale 1 (cdae.hpp:169, :373-416): z = act(sum_{k in row} W[k] (.) Uu[uid] + b + Wu[uid]);
 *            corruption_ratio == 1 encodes the empty input (:168-172) and still excludes the row.
 *   order    of the input sum (part of the contract): the one cdae_hip_encode(mode 0) takes for a train row — groups of `unit`
 *            consecutive items (the handle's work-unit size: unit = 64 when min(batch_users, num_users) <= 1024, else 128 — so a handle
 *            with batch_users > 1024 but at most 1024 users sums in groups of 64), each group summed from 0 in ascending item order, the group sums added from 0 in group order.  A row equal to a handle's train row therefore has that
 *            handle's inference z, and its list, bit for bit.
 *   ranking  exactly cdae_hip_recommend_all's: descending score, equal scores by ascending item id, the row's own items never
 *            returned, 0xFFFFFFFF in the surplus places of a row with fewer than topk items left (cdae_hip_recommend_user refuses such
 *            a set; one short row must not fail a batch).  topk in [1, num_items]; num_dim <= 256 and topk <= 16 run on the matrix
 *            cores, anything else on the general path.
 *   out      out_ids [n_rows x topk]; out_scores NULL or [n_rows x topk]: the fp32 score the path computed for every listed item,
 *            -INFINITY in the sentinel places.
 * cdae_hip_eval_topn_rows scores those lists on the device against per-row target sets (a second CSR over the same n_rows, items
 * ascending and unique, empty rows allowed) by the rules of cdae_hip_eval_topn: rets8 = the eight means over the rows WITH targets,
 * added in row order; hits3 (may be NULL) = integer hits in the first 1 / 5 / 10 places; ids_out (may be NULL) = the lists.  No row
 * with targets is an error.
 * Refused: IMF / BPR handles (the score does not depend on the rated set), item shards, calls before cdae_hip_set_interactions.
 * The caller's arrays are copied into grow-only device buffers of the handle (freed with it): a steady-state call allocates nothing.
 * Rows are taken in chunks (at most 32 768 per launch group) with one host synchronisation per chunk that returns results. */
#define CDAE_NO_USER 0xFFFFFFFFu
int cdae_hip_recommend_rows(cdae_hip_t* h, uint64_t n_rows, const uint32_t* uids, const int64_t* row_ptr, const uint32_t* col,
                            uint32_t topk, uint32_t* out_ids, float* out_scores);
int cdae_hip_eval_topn_rows(cdae_hip_t* h, uint64_t n_rows, const uint32_t* uids, const int64_t* row_ptr, const uint32_t* col,
                            const int64_t* target_row_ptr, const uint32_t* target_col, uint32_t topk, double* rets8, uint64_t* hits3,
                            uint32_t* ids_out);

/* get_output_values(z, idx) (cdae.hpp:418-426) for MANY rows at once: the model's scores of the items the caller NAMES, and their
 * ranks among themselves — re-ranking of a retrieved candidate set, sampled-candidate evaluation (one held-out positive among ~100
 * sampled negatives, HR@k / NDCG@k from the positive's rank), held-out loss over any items.
 *   rows, uids, hidden, order of the input sum
 *            exactly cdae_hip_recommend_rows's, validated alike and encoded by the same launches: the z of a row is bit for bit the
 *            z cdae_hip_recommend_rows ranks from (CDAE_NO_USER, uids == NULL and corruption_ratio == 1 mean what they mean there).
 *   candidates
 *            cand_row_ptr[n_rows + 1] / cand_col: a second host CSR over the same rows, items ascending and unique inside a row
 *            (validated: an unsorted, duplicate or out-of-range candidate is an error that names the row); a row may be empty.  A
 *            candidate MAY be one of the row's rated items and is scored like any other: exclusion is the caller's business, as in
 *            get_output_values.
 *   out_scores
 *            [cand_row_ptr[n_rows]]: out_scores[p] = the fp32 D[cand_col[p]] . z_r + b'[cand_col[p]] of the row r that position p
 *            belongs to (D = V when asymmetric, else W; the output is linear, as in the reference).  Required when there is at least
 *            one candidate.
 *   position independence
 *            the score of (row, item) is a function of z_r, D[item] and b'[item] only: the same bits whatever else the call holds —
 *            other candidates, other rows, the pair's place in its row, the chunking.  One contraction order per row stride
 *            (cdae_hip_row_stride() = 64 NI floats, NI = 1, 2, 4, 8): lane l of a 64-lane wavefront owns elements [l NI, (l + 1) NI) and
 *            computes p_l = z[l NI] * D[l NI], then p_l = p_l + z[l NI + i] * D[l NI + i] for i = 1 .. NI - 1 in ascending i, every
 *            product and every sum rounded to fp32 on its own (no fused multiply-add); the 64 p_l are added as a balanced tree over
 *            neighbouring lanes — (p_0 + p_1), (p_2 + p_3), ... then pairs of those, and so on for six levels, each level adding the
 *            two halves of a block of 2, 4, 8, 16, 32, 64 consecutive lanes; b'[item] is added last, once.
 *   out_ranks
 *            NULL or [cand_row_ptr[n_rows]]: out_ranks[p] = the number of candidates of the same row that precede p in
 *            cdae_hip_recommend_all's total order — a strictly greater score, or an equal score and a lower item id; 0 is the best.
 *            Computed on the device from the very fp32 scores out_scores reports, so ranks and scores agree by construction.  With
 *            out_ranks a row of more than CDAE_RANK_CANDIDATES_MAX candidates is an error that names the row, raised before anything
 *            is launched.  Scores alone have no such cap: a row may list all num_items.
 * n_rows == 0 succeeds and touches nothing; rows without any candidate succeed and write nothing.
 * Refused (the handle stays usable): IMF / BPR handles, item shards, calls before cdae_hip_set_interactions, a null out_scores with
 * candidates present.
 * The caller's arrays are copied into grow-only device buffers of the handle (freed with it): a steady-state call allocates nothing.
 * Work is taken in chunks of at most 32 768 rows and at most 65 536 candidates (whole candidate rows while they fit; a longer row is
 * cut into chunks of 65 536), with one host synchronisation per chunk. */
#define CDAE_RANK_CANDIDATES_MAX 4096u
int cdae_hip_score_rows(cdae_hip_t* h, uint64_t n_rows, const uint32_t* uids, const int64_t* row_ptr, const uint32_t* col,
                        const int64_t* cand_row_ptr, const uint32_t* cand_col, float* out_scores, uint32_t* out_ranks);

/* Where does a named item stand in a row's WHOLE list?  The exact rank of every target item among ALL items outside the row's rated
 * set — what full-catalogue Recall@k / NDCG@k / MRR / AUC are computed from, for any k, without sampling candidates.
 *   rows, uids, hidden, order of the input sum
 *            exactly cdae_hip_recommend_rows's, validated alike and encoded by the same launches: the z of a row is bit for bit the
 *            z cdae_hip_recommend_rows ranks from (CDAE_NO_USER, uids == NULL and corruption_ratio == 1 mean what they mean there).
 *   targets  target_row_ptr[n_rows + 1] / target_col: a second host CSR over the same rows, items ascending and unique inside a row
 *            (validated: an unsorted, duplicate or out-of-range target is an error that names the row); a row may be empty.  A target
 *            that is one of its row's rated items is an error that names the row, raised before anything is launched: a rated item
 *            has no place in the list.  There is no cap on the targets of a row: it may name every one of its unrated items.
 *   out_ranks
 *            [target_row_ptr[n_rows]], required when there is at least one target: out_ranks[p] = the number of items OUTSIDE the
 *            row's rated set that precede target p in cdae_hip_recommend_all's total order — a strictly greater score, or an equal
 *            score and a lower item id.  The row's other targets count like any other item.  0 is the head of the list: the rank is
 *            the place the item takes in that row's cdae_hip_recommend_rows list of unbounded length.
 *   out_scores
 *            NULL or [target_row_ptr[n_rows]]: the fp32 score the counting used for the target.
 *   which arithmetic (part of the contract)
 *            Two sweeps over the catalogue: the first learns the targets' scores, the second counts against them; both compute every
 *            score the way the top-k kernel of the same num_dim does, so ranks and scores agree by construction.
 *            num_dim <= 256: the scores are the matrix-core top-k path's, bit for bit — the same contraction length per num_dim
 *            (32 / 64 / 128 / 200 / 256 for num_dim <= 32 / 64 / 128 / 200 / 256), the same chain of v_mfma_f32_32x32x2_f32 over the
 *            same operands in the same order, b' added last.  For every topk <= 16, an id that cdae_hip_recommend_rows lists at
 *            place j, given as a target, gets rank j and the listed score, bit for bit.
 *            num_dim > 256: the scores are the general path's (a fused multiply-add chain over the lane's elements, the wavefront
 *            sum, b' added last), and the same holds for every topk.
 *            (A score that is NaN has no place in the order; its rank is unspecified.)
 *   position independence
 *            a row's ranks and scores do not depend on what else the call holds, on its place in the call, or on the chunking.
 * n_rows == 0 succeeds and touches nothing; rows without targets succeed and write nothing.
 * Refused (the handle stays usable): IMF / BPR handles, item shards, calls before cdae_hip_set_interactions, a null out_ranks with
 * targets present.
 * The caller's arrays are copied into grow-only device buffers of the handle (freed with it): a steady-state call allocates nothing.
 * Rows are taken in chunks of at most 32 768 (fewer once a chunk holds 4 194 304 targets) with one host synchronisation per chunk;
 * on the matrix cores a row with n targets takes ceil(n / 16) columns of the counting launches, at most 32 768 columns per launch.
 * Cost: two sweeps of the decoder per chunk plus 16 compares per (column, item). */
int cdae_hip_full_rank_rows(cdae_hip_t* h, uint64_t n_rows, const uint32_t* uids, const int64_t* row_ptr, const uint32_t* col,
                            const int64_t* target_row_ptr, const uint32_t* target_col, uint32_t* out_ranks, float* out_scores);

/* cdae_hip_recommend_rows with the excluded set cut loose from the input set, and an item allow list: a category page ("top 10 among
 * these 600 items"), items that must not be listed but were never inputs (shown and ignored, out of stock, blocked), and repeat
 * consumption (a rated item may be listed again).
 *   rows, uids, hidden, order of the input sum
 *            exactly cdae_hip_recommend_rows's, validated alike and encoded by the same launches: the z of a row is bit for bit the
 *            z cdae_hip_recommend_rows ranks from (CDAE_NO_USER, CDAE_GUEST_USER(i), uids == NULL and corruption_ratio == 1 mean what
 *            they mean there).  Neither excl nor allow enters z.
 *   excl     excl_row_ptr[n_rows + 1] / excl_col: a second host CSR over the same rows, items ascending and unique inside a row
 *            (validated: an unsorted, duplicate or out-of-range item is an error that names the row); a row may be empty.
 *            excl_row_ptr == NULL: no extra exclusions.  An excluded item may also be rated; it may also lie outside the allow list,
 *            where it has no effect.
 *   exclude_rated
 *            != 0: a row's rated items are excluded as in cdae_hip_recommend_rows.  0: they are candidates like any other item; the
 *            row's list then comes from all (allowed) items minus excl.
 *   allow    allow_items[n_allow]: ONE list for the whole call, ascending and unique (an unsorted, duplicate or out-of-range id is an
 *            error that names the position).  allow_items == NULL (then n_allow must be 0): the whole catalogue.  allow_items != NULL
 *            with n_allow == 0 is an error.
 *   result   row r's list is the first topk items of its candidate set C_r = allow \ excl_r (\ rated_r when exclude_rated) in
 *            cdae_hip_recommend_all's total order: descending score, equal scores by ascending ORIGINAL item id.  out_ids holds
 *            original item ids; a row with |C_r| < topk gets 0xFFFFFFFF in the surplus places (-INFINITY in out_scores, which may be
 *            NULL).  topk in [1, num_items] whatever the allow list's size.
 *   which arithmetic (part of the contract)
 *            the path is chosen as for cdae_hip_recommend_rows: num_dim <= 256 and topk <= 16 run on the matrix cores, anything else
 *            on the general path.  On either path the score of (row, item) is the bits that path of cdae_hip_recommend_rows computes
 *            for that pair: with excl == NULL, allow == NULL and exclude_rated != 0 the call returns cdae_hip_recommend_rows' ids and
 *            scores bit for bit; with a filter it returns the list cdae_hip_recommend_rows would give at unbounded length with the
 *            items outside C_r deleted, scores bit for bit.  (With an allow list the sweep runs over a packed copy of the allowed
 *            decoder rows, made once per call and rebuilt by every call; a score does not depend on where its decoder row sits.)
 *   position independence
 *            a row's list and scores do not depend on what else the call holds, on the row's place in the call, or on the chunking.
 * n_rows == 0 succeeds and touches nothing.
 * Refused (the handle stays usable): IMF / BPR handles, item shards, calls before cdae_hip_set_interactions.  Every validation error is
 * raised before anything is launched.
 * The caller's arrays, the allow list's inverse and the packed decoder rows live in grow-only device buffers of the handle (freed with
 * it): a steady-state call allocates nothing.  Rows are taken in chunks of at most 32 768 (the general path's chunk is that of
 * cdae_hip_recommend_rows' general path, sized by the swept item count) with one host synchronisation per chunk. */
int cdae_hip_recommend_rows_filtered(cdae_hip_t* h, uint64_t n_rows, const uint32_t* uids, const int64_t* row_ptr, const uint32_t* col,
                                     const int64_t* excl_row_ptr, const uint32_t* excl_col, int exclude_rated,
                                     const uint32_t* allow_items, uint64_t n_allow,
                                     uint32_t topk, uint32_t* out_ids, float* out_scores);

/* The item page: the topk items closest to each of many named items, by dot product or cosine over one of the model's item tables —
 * the similar_items of a matrix-factorisation library, and the offline build of an item-to-item table.  The reference has no
 * counterpart; this comment is the definition.
 *   queries  query_items[n_queries]: any item, any number of times, in any order.  An id >= num_items is an error that names the
 *            position.  n_queries == 0 succeeds and touches nothing.
 *   table    T [num_items x num_dim].  CDAE_ITEMS_OUTPUT: D, the rows the scores are made of (V when asymmetric, else W);
 *            CDAE_ITEMS_INPUT: W, the rows the encoder sums.  On an IMF / BPR handle both name the item factors iv_ (CDAE_P_W).
 *            Biases take no part.  A full_output handle is served from its fp32 rows like any other.
 *   score    CDAE_SIM_DOT: s(q, i) = T[i] . T[q].  CDAE_SIM_COSINE: s(q, i) = N[i] . N[q], N being T normalised row by row:
 *            ss_i is accumulated in fp64 in one fixed order — lane l of 64 owns elements [l NI, (l + 1) NI) of the row stride
 *            (cdae_hip_row_stride() = 64 NI; pad elements are zero) and adds its squares in ascending order,
 *            p = p + (double)x * (double)x from p = 0; the 64 partials are added as the balanced tree over neighbouring lanes that
 *            cdae_hip_score_rows documents — n_i = (float)sqrt(ss_i), and N[i][k] = T[i][k] / n_i, a correctly rounded fp32
 *            division (the library is built without fast-math).  A row with ss_i == 0 normalises to zeros, so every score with it is
 *            +0.0, never NaN.  A row's normalised form depends on that row alone.
 *   which arithmetic (part of the contract)
 *            the dot product is the arithmetic of the path, chosen as everywhere: num_dim <= 256 and topk <= 16 run
 *            recommend_all's matrix-core chain with the table row as the A operand, the query row as the B operand and a bias of
 *            +0.0 added last; anything else runs the general path's fused multiply-add chain over the lane's elements, the
 *            wavefront sum, + 0.0.  On either path s(q, i) has the bits of s(i, q): the products commute and the chain order is
 *            the same.
 *   candidates
 *            C_q = allow \ excl_q (\ {q} when exclude_self != 0).  allow_items[n_allow]: ONE list for the whole call, ascending and
 *            unique; NULL with n_allow == 0 is the whole catalogue, a non-NULL list with n_allow == 0 is an error — exactly
 *            cdae_hip_recommend_rows_filtered's rules and error texts.  excl_row_ptr[n_queries + 1] / excl_col: a host CSR over the
 *            queries, items ascending and unique inside a row (validated; an error names the row); NULL: none.  The query's own
 *            vector never depends on allow or excl: a query outside the allow list is served like any other.
 *   result   the first topk items of C_q in cdae_hip_recommend_all's total order: descending score, equal scores by ascending
 *            ORIGINAL item id; surplus places hold 0xFFFFFFFF / -INFINITY.  topk in [1, num_items].  out_scores may be NULL.
 *   position independence
 *            a query's list and scores do not depend on what else the call holds, on its place in the call, or on the chunking.
 * Refused (the handle stays usable): item shards, calls before cdae_hip_set_interactions, an unknown table or metric.  Every validation
 * error is raised before anything is launched.
 * The table image of a call (the allowed and / or normalised rows; CDAE_SIM_DOT without an allow list sweeps the handle's table in
 * place) is made once per call and rebuilt by every call.  Everything lives in grow-only device buffers of the handle (freed with it): a
 * steady-state call allocates nothing.  Queries are taken in chunks of at most 32 768 (the general path's chunk is that of
 * cdae_hip_recommend_rows' general path, sized by the swept item count) with one host synchronisation per chunk. */
#define CDAE_ITEMS_OUTPUT 0u   /* D: V when asymmetric, else W — the rows the scores are made of */
#define CDAE_ITEMS_INPUT  1u   /* W: the rows the encoder sums */
#define CDAE_SIM_DOT    0u
#define CDAE_SIM_COSINE 1u
int cdae_hip_similar_items(cdae_hip_t* h, uint64_t n_queries, const uint32_t* query_items,
                           uint32_t table, uint32_t metric, int exclude_self,
                           const int64_t* excl_row_ptr, const uint32_t* excl_col,
                           const uint32_t* allow_items, uint64_t n_allow,
                           uint32_t topk, uint32_t* out_ids, float* out_scores);

/* Fold-in: fit the user node of MANY rows that are no train rows, with everything shared frozen — the strong-generalisation protocol
 * (train on some users; for an unseen user fit only their own node on part of their history, rank the rest), and the warm re-fit of a
 * user whose session changed.  This is train_one_user_corruption (cdae.hpp:198-358) with every update of a shared parameter removed:
 * W, V, b and b' are read, never written; all that moves is the row's own (wu, wu_ag) and, under linear_function, (uu, uu_ag).
 *   rows     row_ptr[n_rows + 1] / col: a host CSR as for cdae_hip_recommend_rows (items ascending and unique inside a row, validated alike:
 *            the error names the row); a row may be empty.  A row that holds all num_items items is an error that names the row, raised
 *            before anything is launched: the negative sampler needs an unrated item.
 *   start    the node row r starts from, chosen by uids[r] exactly as the rows entry points choose a row's node:
 *              a local user              copies of that user's Wu / Wu_ag / Uu / Uu_ag rows (the handle's own rows are not written);
 *              CDAE_NO_USER, uids NULL   wu = 0, uu = 1, both accumulators 1e-4 (reset()'s values, cdae.hpp:109-134);
 *              CDAE_GUEST_USER(i)        node i of the guest table (continue an earlier fit).
 *   stream   s = stream_id_base + r takes the place of the global user id in cdae_rng_key (include/cdae_rng.h).
 *   loop     with R the row's items, n = |R|, m = n num_neg: for e = epoch_begin .. epoch_begin + n_epochs - 1, and inside it for
 *            c = 0 .. num_corruptions - 1:
 *              kept  = the R[pos] with cdae_keep(cdae_rng_draw(key(seed, e, s, CDAE_STREAM_CORRUPT), c n + pos), thr);
 *              S     = sum_{j in kept} W[j], unscaled;
 *              h     = scale S ((.) uu under linear_function) + b (+ wu under user_factor);  z = act(h) with the reference's clamps,
 *                      z' = act'(z) (cdae.hpp:208-215);
 *              N_i   = cdae_sample_negative(key(seed, e, s, CDAE_STREAM_NEGATIVE), c m + i, R, n, num_items) for i < m: the draws
 *                      training makes for a user with id s and that row;
 *              hg    = sum_{j in R} loss'(D[j].z + b'[j], 1) D[j] + sum_i loss'(D[N_i].z + b'[N_i], 0) D[N_i], D = V when asymmetric,
 *                      else W; every term from the frozen rows, a duplicate negative counted once per occurrence;
 *              delta = hg (.) z';
 *              user_factor:      one AdaGrad (or SGD) step of (wu, wu_ag) with gradient delta + lambda wu (cdae.hpp:317-331);
 *              linear_function:  one step of (uu, uu_ag) with gradient lambda uu + delta (.) S, S unscaled as in the reference
 *                                (cdae.hpp:295-299, :340, :351-357);
 *              both gradients formed from the values before either step.
 *            An empty row takes no step and returns its start node; n_epochs == 0 returns the start nodes.
 *   contract the handle's parameters are not written.  A row's result is a function of (its items, its start node, s, seed, the epoch
 *            range, the frozen parameters) only: the same bits whatever else the call holds, wherever the row sits, however the call is
 *            chunked, and on every repeat (a fixed summation order, no atomics).  No particular order is promised beyond that.
 *   out      out_wu / out_wu_ag / out_uu / out_uu_ag: each NULL or [n_rows x num_dim] on the host.  Without linear_function out_uu /
 *            out_uu_ag are written with ones / 1e-4; without user_factor out_wu / out_wu_ag with zeros / 1e-4.
 *   install  != 0: after the WHOLE call has succeeded the guest table is exactly the n_rows fitted nodes, row r as guest r — on the
 *            device, nothing crosses PCIe for it, and only then: a row may start from the guest slot another row of the same call
 *            replaces.  On any error the table is as it was.  (The library keeps an installing call's fitted rows in a second set of
 *            arrays and EXCHANGES that set with the table at the end instead of copying into it: such a call holds n_rows staged
 *            rows, not one chunk's, and the two sets reach their steady sizes after two installing calls of a given size.)
 * n_rows == 0 succeeds and touches nothing, except that with install it clears the table.
 * Refused (the handle stays usable): IMF / BPR handles, item shards, calls before cdae_hip_set_interactions, full_output handles (their
 * decode is dense; a dense fold-in is not implemented), a handle with neither user_factor nor linear_function (nothing to fit).
 * The caller's arrays are copied into grow-only device buffers of the handle (freed with it): a steady-state call allocates nothing.
 * Rows are taken in chunks of at most 32 768, ONE launch per chunk for all its epochs, one host synchronisation per chunk.
 *
 * The guest table: a second user table the handle owns — four device arrays [n_guests x row stride] (wu, wu_ag, uu, uu_ag), grow-only,
 * freed with the handle, dropped by cdae_hip_set_interactions.  cdae_hip_recommend_rows, cdae_hip_eval_topn_rows, cdae_hip_score_rows,
 * cdae_hip_full_rank_rows and cdae_hip_fold_in_rows resolve uids[r] = CDAE_GUEST_USER(i) to guest i.  cdae_hip_set_guest_nodes replaces
 * the table by n_guests host rows ([n_guests x num_dim] each; a NULL array stands for zeros / 1e-4 / ones / 1e-4); n_guests == 0 clears
 * it.  cdae_hip_guest_nodes: its size.  A handle with more than 0x7FFFFFFF users refuses a table (its user ids need the top bit), and
 * the refusals of cdae_hip_fold_in_rows apply. */
#define CDAE_GUEST_USER(i) (0x80000000u | (uint32_t)(i))
int cdae_hip_fold_in_rows(cdae_hip_t* h, uint64_t n_rows, const uint32_t* uids, const int64_t* row_ptr, const uint32_t* col,
                          uint64_t seed, uint32_t epoch_begin, uint32_t n_epochs, uint64_t stream_id_base, int install,
                          float* out_wu, float* out_wu_ag, float* out_uu, float* out_uu_ag);
int cdae_hip_set_guest_nodes(cdae_hip_t* h, uint64_t n_guests, const float* wu, const float* wu_ag, const float* uu, const float* uu_ag);
uint64_t cdae_hip_guest_nodes(const cdae_hip_t* h);

/* ---- data-parallel exchange (north star: RCCL all-reduce of the shared W / W' / bias gradients;
 * Wu never leaves its GPU).  Each rank trains its own users from a common snapshot, then
 *   cdae_hip_delta_begin   : snapshot the shared parameters
 *   ... cdae_hip_train_users ...
 *   cdae_hip_delta_compute : delta = current - snapshot, packed in one device buffer together with a
 *                            per-row touch indicator
 *   <all-reduce(sum) of that buffer by the caller, e.g. torch.distributed over RCCL>
 *   cdae_hip_delta_apply   : current = snapshot + combine(summed delta)
 * Layout of the buffer: cdae_hip_delta_device_ptr(). */
/* All four delta calls are stream-ordered on the library's HIP stream (cdae_hip_stream) and do not block the
 * host; run the all-reduce on that stream, or synchronise (cdae_hip_synchronize) before touching the buffer
 * from another one. */
int cdae_hip_stream(cdae_hip_t* h, void** hip_stream);
int cdae_hip_delta_begin(cdae_hip_t* h);
int cdae_hip_delta_compute(cdae_hip_t* h);
int cdae_hip_delta_device_ptr(cdae_hip_t* h, void** device_ptr, size_t* count_floats);
#define CDAE_DELTA_SUM 0u         /* current = snapshot + sum over ranks (summed gradients; default)      */
#define CDAE_DELTA_TOUCH_MEAN 1u  /* item rows / #ranks that touched them, hidden bias / world_size      */
int cdae_hip_delta_apply(cdae_hip_t* h, uint32_t world_size, uint32_t rule);

/* Pipelined form of the same exchange (sum rule): the all-reduce of one period's deltas overlaps the next period's
 * training, and the other ranks' part is folded in one period late.  After cdae_hip_delta_begin() (agreed state A = current):
 *   cdae_hip_delta_stage : send = recv = current - A ; snap = current
 *   (caller all-reduces the recv buffer, cdae_hip_delta_recv_device_ptr, n floats, asynchronously; the buffer is
 *    compact: the matrices' pad columns are not exchanged)
 *   cdae_hip_delta_merge : A += recv ; current = A + (current - snap)     (before the next _stage)
 * A moves only by the all-reduced sums, so it is the same BITS on every rank; when nothing was trained between a stage and
 * its merge (synchronous exchange, final flush) every rank ends with current == A, bit for bit.
 * Stream-ordered on cdae_hip_stream like the calls above.  (cdae_hip_exchange_* below drive these with a library-owned
 * RCCL communicator; these entry points remain for hosts that bring their own collective.) */
int cdae_hip_delta_stage(cdae_hip_t* h);
/* How _merge folds the all-reduced buffer in (set it before the first _stage, or between a _merge and the next _stage):
 *   CDAE_COMBINE_SUM         (default) the algebra above: the replicas' accumulated steps are summed.
 *   CDAE_COMBINE_GLOBAL_ACC  AdaGrad handles only (others keep the sum): per (parameter, accumulator) pair the replicas exchange their
 *       accumulator growth — exactly their sum of squared gradients, cdae.hpp:254 — and their step with their own preconditioner taken
 *       back out, (current - A) * (beta + sqrt(acc)); _merge takes ONE step with the accumulator that has seen every replica:
 *       A_acc += sum ; A += sum / (beta + sqrt(A_acc))  (cdae_exchange_algebra.h pipe_pair).  Same buffers, same all-reduce. */
#define CDAE_COMBINE_SUM 0u
#define CDAE_COMBINE_GLOBAL_ACC 1u
int cdae_hip_delta_set_combine(cdae_hip_t* h, uint32_t combine);
int cdae_hip_delta_recv_device_ptr(cdae_hip_t* h, void** device_ptr, size_t* count_floats);
int cdae_hip_delta_merge(cdae_hip_t* h);
int cdae_hip_delta_merge_stage(cdae_hip_t* h);   /* _merge of the previous period then _stage of this one, in one pass */

/* ---- the sibling SGD models IMF and BPR on the same handle type (yelp.cpp:122-165 --method=MF / BPR) ----
 *   IMF::reset / BPR::reset        imf.hpp:57-69                cdae_hip_set_interactions + cdae_hip_init_params
 *   IMF::train_one_iteration       imf.hpp:71-86 (+ :88-115)    cdae_hip_train_epoch / _train_users
 *   BPR::train_one_iteration       bpr.hpp:56-70 (+ :72-106)    (same; pairwise = 1)
 *   RecsysModelBase::recommend     recsys_model_base.hpp:77-104 cdae_hip_recommend_all   (score = ub + ib + uv . iv, imf.hpp:117-119)
 * Parameters through cdae_hip_get/set_param: CDAE_P_WU / _WU_AG = uv_ / uv_ag_ (users x K), CDAE_P_W / _W_AG = iv_ / iv_ag_
 * (items x K), CDAE_P_UB / _UB_AG = ub_ / ub_ag_, CDAE_P_BP / _BP_AG = ib_ / ib_ag_.  loss_type: 0 SQUARE, 1 LOGISTIC, 2 LOG,
 * 3 HINGE, 5 CROSS_ENTROPY (loss.hpp:10-18; what yelp.cpp lets these models choose).  batch_users: users whose chains run
 * concurrently against the block-start item rows; 1 == the reference's strictly sequential loop.  data_loss / penalty_loss are
 * 0 for these models, as in the reference (ModelBase defaults, model_base.hpp:36-45); cdae_hip_encode, the explicit-input step
 * and the full-output decode do not apply. */
/* Training order.  A CDAE handle, and an IMF / BPR handle with one user per block (batch_users = 1: what the drop-in classes
 * src/model/recsys/imf.hpp / bpr.hpp pass by default), visit the users in id order like the reference.
 * An IMF / BPR handle with batch_users > 1 (the block schedule: what batch_users = 0 selects on BASELINE-sized data sets, a throughput setting beyond it) trains them in ACTIVITY-GROUPED order — users
 * sorted by train-row length, cut into blocks of batch_users, the blocks visited in a fixed pseudo-random order — because a block
 * lasts as long as its most active user's serial chain.  cdae_hip_user_order returns that order: out[position] = user id
 * (count = num_users; the identity for every other handle).  The random streams, cdae_hip_train_users' range and
 * cdae_hip_debug_sample_batch's window are in POSITIONS; get / set_param and recommend_all are by user id as everywhere. */
int cdae_hip_user_order(cdae_hip_t* h, uint32_t* out, size_t count);

typedef struct cdae_mf_config {
  uint32_t struct_size;      /* sizeof(cdae_mf_config)                                   */
  uint32_t num_dim;          /* IMFConfig::num_dim          imf.hpp:19                   */
  uint32_t num_neg;          /* imf.hpp:20                                               */
  uint32_t loss_type;        /* imf.hpp:17 / bpr.hpp:17                                  */
  uint32_t using_adagrad;    /* imf.hpp:22                                               */
  uint32_t using_bias_term;  /* imf.hpp:21                                               */
  uint32_t pairwise;         /* 0: IMF (pointwise instances), 1: BPR (pairs)             */
  uint32_t batch_users;      /* 1: the reference's sequential loop; > 1: block schedule  */
                             /* in activity-grouped order (cdae_hip_user_order).  0 ->   */
                             /* cdae_hip_mf_default_batch_users(num_users, pairwise)      */
  double lambda;             /* imf.hpp:16                                               */
  double learn_rate;         /* imf.hpp:14                                               */
  double beta;               /* imf.hpp:15                                               */
} cdae_mf_config;
/* The default blocks (batch_users = 0): the largest sizes measured INSIDE the sampled CDAE path's accuracy bound — Recall@10 within
 * +-0.002 of the sequential loop at every epoch as a mean over six seeds, against fp64 fixtures of the loop at ML-10M shape K=200
 * (tests/test_gpu_mf.py; tools/mf_envelope.py has the other sizes and Yelp shape) — chosen when the data set is known
 * (cdae_hip_set_interactions):
 *   IMF  16 users per block from 8 192 users on (measured at 10 000 and 70 000 users; 32 users per block sit up to +0.0035, 64 up to
 *        +0.005): 43 x the loop's users/s at ML-10M shape;
 *   BPR   8 users per block from 65 536 users on (70 000 users: inside the bound; 10 000 users: +0.003 in the first two epochs, so
 *        smaller data sets keep the loop): 22 x the loop's users/s.  Since ABI 10 a BPR user's pairs see their shared positive item's
 *        row as the loop leaves it between them (a private copy carried through phase U); before, every block size was 0.008 low
 *        in the first two epochs.
 * Smaller data sets train one user per block: the reference loop itself. */
#define CDAE_IMF_DEFAULT_BATCH_USERS 16u
#define CDAE_IMF_DEFAULT_MIN_USERS 8192u
#define CDAE_BPR_DEFAULT_BATCH_USERS 8u
#define CDAE_BPR_DEFAULT_MIN_USERS 65536u
uint32_t cdae_hip_mf_default_batch_users(uint64_t num_users, uint32_t pairwise);
int cdae_hip_create_mf(const cdae_mf_config* cfg, int device_id, cdae_hip_t** out);

/* ---- WRMF: weighted-regularised matrix factorisation fitted by alternating least squares (Hu, Koren, Volinsky, "Collaborative
 * filtering for implicit feedback datasets"; the reference's src/model/recsys/wrmf.hpp, als.hpp), on the same handle type ----
 * Binary interactions R (the train CSR): preference 1 and confidence 1 + alpha on a stored pair, preference 0 and confidence 1
 * elsewhere.  The user half-step, with the item table Y frozen and R_u the items of row u, solves for every user with interactions
 *     G   = Y^T Y                                          (K x K, once per half-step)
 *     A_u = G + alpha * sum_{i in R_u} y_i y_i^T + lambda * I
 *     b_u = (1 + alpha) * sum_{i in R_u} y_i
 *     x_u <- CG(A_u, b_u, start = the current x_u, cg_steps iterations)
 * and the item half-step is the same over the transposed CSR with G = X^T X of the user table the user half-step has just written.
 * An epoch is the user half-step followed by the item half-step (wrmf.hpp:102-109); a row without interactions is left as it is
 * (wrmf.hpp:111-116).  CG is the textbook loop, A_u is never formed (A_u p = G p + alpha sum_i y_i (y_i . p) + lambda p):
 *     r = b - A x; p = r; rs = r.r; then cg_steps times: Ap; a = rs / (p.Ap); x += a p; r -= a Ap; rs' = r.r; p = r + (rs'/rs) p
 * and a row whose rs falls below 1e-20 stops with the x it has.  One half-step is exactly parallel: no learning rate, no sampling,
 * no order between rows; a row's result does not depend on the rows solved beside it, and the same state gives the same bits.
 *
 * There is deliberately NO switch for the reference's literal train_one_index (wrmf.hpp:66-100).  It omits the Y^T Y term, so every
 * unobserved pair is unweighted, and its system lambda * I + scalar * sum y y^T is so ill-conditioned that a truncated fp32 CG on it
 * differs from fp64 by up to 1e-1 on this repository's test fixtures (measured with numpy): nothing a GPU kernel could be held to.
 *
 * alpha is WRMFConfig::scalar; lambda and num_dim are the reference's; cdae_hip_init_params draws Random() * 0.001
 * (wrmf.hpp:47-48) from the CDAE_STREAM_INIT stream with the keys of the IMF tables.  The factors live where IMF's do — CDAE_P_WU
 * users x K, CDAE_P_W items x K, biases zero — so cdae_hip_recommend_all, cdae_hip_eval_topn and cdae_hip_similar_items serve the
 * handle as they serve IMF; the accumulator ids (_AG), CDAE_P_UB and CDAE_P_BP hold the constants init_params writes and nothing
 * reads them.  Unlike the SGD handles, rows without interactions and rows with every item are legal in set_interactions.
 *   cdae_hip_train_epoch    both half-steps; seed and epoch are ignored (nothing is drawn); stats.users = num_users, stats.batches = 2
 *   cdae_hip_train_users    the full range only
 * A partial range, cdae_hip_enqueue_users, cdae_hip_prefetch_users, cdae_hip_debug_sample_batch and cdae_hip_debug_row_pack are
 * refused (a half-step needs every row); everything that refuses an IMF / BPR handle refuses this one with the same text;
 * data_loss / penalty_loss are 0. */
typedef struct cdae_als_config {
  uint32_t struct_size;      /* sizeof(cdae_als_config)                                  */
  uint32_t num_dim;          /* WRMFConfig::num_dim                                      */
  uint32_t cg_steps;         /* CG iterations per row and half-step; 0 -> 3              */
  uint32_t reserved;         /* 0                                                        */
  double lambda;             /* WRMFConfig::lambda                                       */
  double alpha;              /* WRMFConfig::scalar: confidence 1 + alpha on a stored pair */
} cdae_als_config;
#define CDAE_ALS_DEFAULT_CG_STEPS 3u
#define CDAE_ALS_USERS 0u
#define CDAE_ALS_ITEMS 1u
int cdae_hip_create_als(const cdae_als_config* cfg, int device_id, cdae_hip_t** out);
int cdae_hip_als_half_step(cdae_hip_t* h, uint32_t side);
/* The user-side solve for rows the caller supplies (users outside the training set, against the frozen item table): a host CSR over
 * n_rows rows, validated exactly as cdae_hip_recommend_rows validates its rated sets; x0 NULL (zeros) or [n_rows x num_dim];
 * out_x [n_rows x num_dim]; cg_steps 0 = the handle's.  A row without items returns its start vector.  The handle's parameters are
 * not written.  Chunks of at most 32 768 rows; n_rows == 0 succeeds and touches nothing; every validation error is raised before
 * a launch.  The train rows with x0 = the current user factors return the bits cdae_hip_als_half_step(CDAE_ALS_USERS) would write. */
int cdae_hip_als_solve_rows(cdae_hip_t* h, uint64_t n_rows, const int64_t* row_ptr, const uint32_t* col, const float* x0,
                            uint32_t cg_steps, float* out_x);
/* G = T^T T of the current user (CDAE_ALS_USERS) or item (CDAE_ALS_ITEMS) table as the half-steps compute it, [num_dim x num_dim]
 * row-major: a test hook (the same table gives the same bits on every call). */
int cdae_hip_als_gram(cdae_hip_t* h, uint32_t side, float* out, size_t count);
/* Per-pair confidence weights (the paper's c_ui = 1 + alpha * r_ui with r_ui a play count, a dwell time, a log-scaled count).  w is one
 * fp32 value per stored pair in the order of the train CSR's col, each finite and >= 0.  A stored pair keeps preference 1 and gets
 * confidence 1 + alpha * w; everything else keeps preference 0 and confidence 1.  The user half-step becomes
 *     A_u = G + alpha * sum_{i in R_u} w_ui y_i y_i^T + lambda * I,     b_u = sum_{i in R_u} (1 + alpha * w_ui) y_i
 * with the same CG loop and the same 1e-20 stop; the item half-step is the same over the item-major CSR with the weights carried
 * through the same permutation.  A pair with w = 0 is legal: it adds y_i to b and nothing to the sparse part of A.  A handle that was
 * never given weights runs the binary kernel; w = 1 everywhere is the binary model (the same bits wherever the sums are exact).
 *   count must equal the interaction count of the last cdae_hip_set_interactions; the values are copied.
 *   w == NULL with count == 0 returns the handle to binary.
 *   A negative, NaN or infinite value, a wrong count, a handle without a data set or a non-WRMF handle is refused before anything is
 *   written, and the handle keeps the weights it had.  A new cdae_hip_set_interactions drops the weights: the new data set is binary. */
int cdae_hip_als_set_confidence(cdae_hip_t* h, const float* w, size_t count);
/* cdae_hip_als_solve_rows with one weight per entry of col (the CALLER's weights, not the handle's): the same chunks, validation and
 * zero-row behaviour; a weight that is negative or not finite is refused before a launch.  w == NULL gives exactly the bits of
 * cdae_hip_als_solve_rows.  The train rows and train weights with x0 = the current user factors return the bits
 * cdae_hip_als_half_step(CDAE_ALS_USERS) would write. */
int cdae_hip_als_solve_rows_weighted(cdae_hip_t* h, uint64_t n_rows, const int64_t* row_ptr, const uint32_t* col, const float* w,
                                     const float* x0, uint32_t cg_steps, float* out_x);
/* The objective the half-steps minimise, for the current tables under the handle's current confidences (a binary handle: w = 1):
 *     out2[0] = sum_{all u,i} c_ui (p_ui - x_u . y_i)^2         out2[1] = lambda (|X|^2 + |Y|^2)
 * It is never formed densely: with s = x_u . y_i, the sum of s^2 over ALL pairs is <X^T X, Y^T Y>_F, a stored pair adds
 * c (1 - s)^2 - s^2, and the penalty is lambda (trace X^T X + trace Y^T Y).  The Grams are the half-steps' (fp32), s is an fp32 dot
 * product, everything else is accumulated in fp64 in a fixed order: the same state gives the same bits on every call.  No parameter is
 * written.  cdae_hip_data_loss and cdae_hip_penalty_loss of a WRMF handle stay 0. */
int cdae_hip_als_objective(cdae_hip_t* h, double* out2);

/* ---- WARP: rank-weighted pairwise matrix factorisation (Weston, Bengio, Usunier, "WSABIE"; the reference's src/model/recsys/warp.hpp,
 * `class WARP : public IMF`), on the same handle type --------------------------------------------------------------------------------
 * For users in order, for every positive i of the user in row order, with items_left = num_items - n_u:
 *     yui = s(i)                                    once per positive: NOT refreshed between its num_neg pairs
 *     for k < num_neg:
 *         draw candidates j_0, j_1, ... until s(j_t) > yui - 1 (strict, fp32) or CDAE_WARP_MAX_TRY draws are made; cnt = t + 1
 *         cnt >= CDAE_WARP_MAX_TRY: the pair is skipped (a violator found at the 500th draw too)
 *         g = loss'(yui - s(j), 1) * l[items_left / cnt]      integer division; l[idx] = H_{idx + 1}, the harmonic numbers
 *         uv_u, iv_i, iv_j step as BPR's do, all three from the pre-step values, with 2 lambda regularisation; AdaGrad divides by
 *         sqrt(acc) — no beta — and biases are part of no step
 * s(x) = ib[x] + uv_u . iv_x (ub cancels on both sides of the test).  Candidate t of pair (p, k) of a user is
 * cdae_sample_negative(key, (p * num_neg + k) * CDAE_WARP_MAX_TRY + t, row, n_u, num_items) on the CDAE_STREAM_NEGATIVE key that
 * IMF / BPR use (include/cdae_rng.h); candidates past the first violator are never looked at.  The rank weights are filled by
 * cdae_hip_set_interactions: the fp64 recurrence, rounded once to fp32.
 * Parameters live where IMF's do and cdae_hip_init_params draws them as for IMF (Random() * 0.01, accumulators 1e-4, biases 0, the same
 * stream keys), so cdae_hip_recommend_all, cdae_hip_eval_topn, cdae_hip_similar_items and get / set_param serve the handle as they
 * serve an IMF handle; everything that refuses an IMF / BPR handle refuses this one with the same text.  cdae_hip_debug_sample_batch
 * and cdae_hip_debug_row_pack are refused: there is no example list before the step.
 * loss_type: the five losses of cdae_mf_config (the reference's default is HINGE).  batch_users: 1 (and 0, which selects 1) is the
 * reference loop.  A value above 1 is the block schedule of IMF / BPR in cdae_hip_user_order's activity-grouped order: one wavefront per
 * user of the block searches and steps its user vector against the block-start item rows, then every item row takes its pairs' steps in
 * (user, pair) order.  A block of ONE user (the last of a range whose length is 1 modulo batch_users) runs the reference loop.  No block
 * size has been measured for accuracy, so none is a default.
 * The stats of a training call: users = the users of the range; examples = 2 * num_neg * (their train items), the two list places of
 * every pair whether its search trained it or skipped it; batches = blocks, and under batch_users = 1 one per user. */
typedef struct cdae_warp_config {
  uint32_t struct_size;      /* sizeof(cdae_warp_config)                                 */
  uint32_t num_dim;          /* WARPConfig::num_dim (10)                                 */
  uint32_t num_neg;          /* WARPConfig::num_neg (5)                                  */
  uint32_t loss_type;        /* CDAE_LOSS_*: 0, 1, 2, 3 (HINGE, the default), 5          */
  uint32_t using_adagrad;    /* WARPConfig::using_adagrad (1)                            */
  uint32_t batch_users;      /* 0 or 1: the reference loop; > 1: block schedule          */
  double lambda;             /* WARPConfig::lambda (0.1)                                 */
  double learn_rate;         /* WARPConfig::learn_rate (0.1)                             */
} cdae_warp_config;
#define CDAE_WARP_MAX_TRY 500u
int cdae_hip_create_warp(const cdae_warp_config* cfg, int device_id, cdae_hip_t** out);
/* The search of every (position, positive, k) of training positions [pos_begin, pos_end) against the current parameters, with the draws
 * of (seed, epoch); nothing is trained.  out_item[q] / out_cnt[q] with q = (row offset of the positive from pos_begin's first positive)
 * * num_neg + k; cnt = CDAE_WARP_MAX_TRY and item = 0xFFFFFFFF: exhausted.  out_margin (may be NULL): s(j) - (s(i) - 1) of the chosen
 * candidate (0 where exhausted).  count must be the range's pair count; it is checked before any launch.  Hard-negative mining for a
 * caller, and the hook that pins the search: the training kernels call the same device function.  One wavefront per user, chunks of
 * at most 8 192 users. */
int cdae_hip_warp_search(cdae_hip_t* h, uint64_t seed, uint32_t epoch, uint64_t pos_begin, uint64_t pos_end,
                         uint32_t* out_item, uint32_t* out_cnt, float* out_margin /* may be NULL */, size_t count);
/* With recording on, a training call leaves the (item, cnt) of every pair of the users it trained, in position order (skipped pairs as
 * above), in a buffer of nnz * num_neg pairs allocated by the first on = 1; pairs of users no call has trained since read 0xFFFFFFFF / 0.
 * Off by default; off costs nothing.  cdae_hip_warp_choices copies the whole record out (count = nnz * num_neg). */
int cdae_hip_warp_record_choices(cdae_hip_t* h, uint32_t on);
int cdae_hip_warp_choices(cdae_hip_t* h, uint32_t* out_item, uint32_t* out_cnt, size_t count);

/* ---- FISM: factored item similarity (Kabbur, Ning, Karypis, "FISM: Factored Item Similarity Models for Top-N Recommender Systems",
 * KDD'13; the reference's src/model/recsys/fism.hpp), on the same handle type ------------------------------------------------------
 * A user is the sum of the input rows P[j] of their items, an item is scored against a second table Q: there is no user table.
 * For users in id order, with R_u in CSR order, n = n_u:
 *     s_pos = (n - 1)^-alpha, and 0 when n = 1;  s_neg = n^-alpha        fp64 pow, rounded once to fp32 (a table filled by
 *                                                                         cdae_hip_set_interactions)
 *     x = sum_{j in R_u} P[j]                                  fp32, at the start of the visit
 *     for p < n, i = R_u[p]; for k <= num_neg:
 *         k = 0: item i, label 1, rated, s = s_pos
 *         k >= 1: item = cdae_sample_negative(key, p * num_neg + (k - 1), row, n, num_items), s = s_neg
 *                 (the CDAE_STREAM_NEGATIVE key and draw index of IMF; label -1 for LOG, else 0)
 *         v    = rated ? x - P[i] : x                          fism.hpp:210-216
 *         pred = [bu[u] + bi[item]] + s * (v . Q[item])        biases only with using_bias_term
 *         g    = loss'(pred, label)
 *         bu[u], bi[item] step on g + lambda * b               fism.hpp:113-124
 *         every j in R_u (j != i when rated): P[j] steps on g * s * Q[item] + lambda * P[j]   (Q[item] before its own step)   :140-149
 *         Q[item] steps on g * s * v + lambda * Q[item]        :151-164
 *         x += sum_j (P[j] after - P[j] before)                :148, 165
 * AdaGrad is acc += grad^2; p -= lr * grad / sqrt(acc) — no beta; with using_adagrad = 0 plain SGD.  cdae_hip_init_params draws P and
 * Q as Random() * 0.001 (fism.hpp:66, 68) on the init stream with the keys of CDAE_P_W and CDAE_P_V; accumulators 1e-4, biases 0.
 * ONE deliberate difference from the reference: it keeps x_ as a users x K table built at reset (:70-77), moves x_[u] only by u's own
 * steps (:165) and reads it in recommend (:183), so x_[u] goes stale with every other user's step on a shared row and is never
 * refreshed.  Here x is the sum of the CURRENT rows at the start of each visit, carried exactly as above inside the visit, and serving
 * computes it from the rated set it is given: the paper's algorithm, no user table, servable for rows outside the training set.  There
 * is no switch for the stale table.  Not taken from the reference: using_factor_term = 0, and using_global_mean (predict never reads it).
 * Parameters: P = CDAE_P_W / _W_AG, Q = CDAE_P_V / _V_AG, bi = CDAE_P_BP / _BP_AG, bu = CDAE_P_UB / _UB_AG; CDAE_P_WU, _UU and _B are
 * not allocated.  loss_type: 0 (SQUARE, the default), 2 (LOG), 5 (CROSS_ENTROPY); LOGISTIC and HINGE are refused.  batch_users: 0 or 1,
 * the loop; a block schedule is not built.
 * Training: cdae_hip_train_epoch, _train_users (any sub-range) and _enqueue_users run the loop, one launch per window of users holding
 * at most window_instances instances (a user is never cut); stats.users / examples / batches = users trained, sum (1 + num_neg) n_u,
 * launches.  cdae_hip_set_interactions accepts rows without items on a FISM handle (a row with every item is refused as for the SGD
 * handles).  A user without train items (n = 0; s_pos does not exist) takes no step: it is counted in stats.users, adds 0 to
 * stats.examples, and bu[u] and its accumulator keep their bits; the kernel passes it over before the visit's first load, and a window
 * of such users alone is still one launch.  data_loss and penalty_loss return 0 as for IMF.  Refused: debug_sample_batch, debug_row_pack, encode,
 * train_one_user_corruption, fold_in_rows (nothing to fit), recommend_user (cdae_hip_recommend_rows serves any rated set), the delta /
 * exchange calls, the ALS and WARP calls.
 * Serving: z = n^-alpha * sum_{j in rated} P[j] (n the size of the rated set; 0 for an empty one), D = Q, b' = bi, through the sweeps
 * of every list-producing entry point: cdae_hip_recommend_all and _eval_topn (the train rows), _recommend_rows, _eval_topn_rows,
 * _score_rows, _full_rank_rows, _recommend_rows_filtered (any rated sets; uids are validated and not otherwise read) and
 * _similar_items (CDAE_ITEMS_INPUT = P, CDAE_ITEMS_OUTPUT = Q).  bu is constant within a row and is left out of served scores.  A
 * candidate that is in its row's rated set (score_rows, exclude_rated = 0) is scored from the full x, not leave-one-out. */
typedef struct cdae_fism_config {
  uint32_t struct_size;      /* sizeof(cdae_fism_config)                                 */
  uint32_t num_dim;          /* FISMConfig::num_dim (10)                                 */
  uint32_t num_neg;          /* FISMConfig::num_neg (5)                                  */
  uint32_t loss_type;        /* CDAE_LOSS_*: 0 (SQUARE, the default), 2, 5               */
  uint32_t using_adagrad;    /* FISMConfig::using_adagrad (1)                            */
  uint32_t using_bias_term;  /* FISMConfig::using_bias_term (1)                          */
  uint32_t batch_users;      /* 0 or 1: the loop                                         */
  uint32_t reserved;         /* 0                                                        */
  double lambda;             /* FISMConfig::lambda (0.01)                                */
  double learn_rate;         /* SGDConfig::learn_rate (0.1)                              */
  double alpha;              /* FISMConfig::alpha (1); a real number here                */
} cdae_fism_config;
int cdae_hip_create_fism(const cdae_fism_config* cfg, int device_id, cdae_hip_t** out);
/* resident_rows: how many of a user's rows the training kernel keeps on chip for a whole visit at this handle's num_dim (0: every row
 * streams through memory; 0 before cdae_hip_set_interactions).  window_instances: the instances one launch holds at most. */
int cdae_hip_fism_plan(const cdae_hip_t* h, uint32_t* resident_rows, uint64_t* window_instances);
/* allow = 0: every row streams through memory.  Both settings give the same bits (as cdae_hip_set_decode_fused). */
int cdae_hip_fism_set_resident(cdae_hip_t* h, int allow);

/* ---- FISMauc: the pairwise (ranking) form of FISM from the same paper (the reference's src/model/recsys/fism_pair.hpp), on a FISM
 * handle.  It takes cdae_fism_config as it stands (reserved stays 0) and everything of a FISM handle but the training loop: the scale
 * table, the residency plan (cdae_hip_fism_plan, _fism_set_resident), the launch windows, the negative stream, rows without items, the
 * serving encode and every sweep behind it, and every FISM refusal.
 * For users in id order, with R_u in CSR order, n = n_u and s = (n - 1)^-alpha (FISM's s_pos: 0 for a lone positive):
 *     x = sum_{r in R_u} P[r]                                  fp32, at the start of the visit (FISM's order)
 *     for p < n, i = R_u[p]; for k < num_neg:
 *         j    = cdae_sample_negative(key, p * num_neg + k, row, n, num_items)     FISM's key (CDAE_STREAM_NEGATIVE) and draw index
 *         v    = x - P[i]                                      the current x; P[i] takes no step while i is the positive
 *         d    = [bi[i] - bi[j]] + s * (v . (Q[i] - Q[j]))     biases only with using_bias_term; no bu anywhere
 *         g    = loss'(d, 1)
 *         bi[i] steps on g + lambda * bi[i];  bi[j] steps on -g + lambda * bi[j]
 *         every r in R_u, r != i: P[r] steps on g * s * (Q[i] - Q[j]) + lambda * P[r]   (both Q rows from before their own steps)
 *         Q[i] steps on g * s * v + lambda * Q[i];  Q[j] steps on -g * s * v + lambda * Q[j]
 *         x += sum_r (P[r] after - P[r] before)
 * Both predictions are formed at the CURRENT parameters for every pair: a negative that repeats inside a positive sees its earlier step.
 * AdaGrad without beta from accumulators of 1e-4, or plain SGD; cdae_hip_init_params as for FISM.
 * Taken from fism_pair.hpp: the structure of the step (:110-160), the (n - 1)^-alpha scale for BOTH items of the pair (:137, 147, 148)
 * and the Q gradients on x - P[i].  Deliberately different from it (the file does not compile as it stands: it includes a path that
 * does not exist): it never overrides predict_user_item_rating, so its negative prediction is always 0 — here d is the difference of
 * two real predictions; it forms the positive's prediction once, before the loop over negatives, and keeps it while the parameters
 * move — here every pair reads the current Q[i], bi[i] and x; its AdaGrad accumulators start at 0, so a zero gradient divides 0 by 0
 * — here 1e-4; it declares bu and never steps it — here there is no bu: it cancels in d, and CDAE_P_UB / _UB_AG are not allocated (asking
 * for them is refused); it keeps the stale x_ table that the FISM handle already declined.
 * loss_type: 0 (SQUARE, the paper's (1 - d)^2, the default) or 2 (LOG of the difference: the BPR criterion).  CROSS_ENTROPY (5) is
 * refused: at label 1 its gradient is LOG's.  LOGISTIC and HINGE are refused as for FISM.  batch_users: 0 or 1.
 * Training: as for FISM, one launch per window of users holding at most window_instances PAIRS (a user is never cut).  stats.examples
 * is the number of pairs, num_neg * nnz of the range; stats.users and stats.batches as for FISM.  A user with n = 0 takes no step and is
 * counted; a user with n = 1 has an empty neighbourhood (s = 0, v = 0) and its pairs still step bi and the lambda terms.  data_loss and
 * penalty_loss return 0.  Both residency settings give the same bits.
 * Serving: exactly a FISM handle's (z = n^-alpha * sum of the rated rows of P, D = Q, b' = bi). */
int cdae_hip_create_fism_pair(const cdae_fism_config* cfg, int device_id, cdae_hip_t** out);

/* ---- library-owned RCCL communicator and exchange schedule (one process per GPU: bench.py --gpus N) -----------------
 * The all-reduce of the staged deltas runs inside the library, on its own communicator and HIP stream, overlapped with the
 * training kernels; the host application only distributes the 128-byte unique id (any channel: bench.py uses a gloo
 * broadcast) and calls _exchange_step after every enqueued batch.  period 0: synchronous exchange at every step (stage,
 * all-reduce, merge); period k >= 1: pipelined — every k steps the accumulated delta is staged and reduced asynchronously,
 * the other ranks' part is merged k steps later.  _exchange_flush reduces and merges what is outstanding: afterwards every
 * rank holds the same shared parameters.  A handle without a communicator behaves as a one-rank group.
 * _exchange_time_all_reduce: seconds per all-reduce of the exchange buffer with the device otherwise idle (call it before
 * the deltas matter: it flushes, and restarts the exchange from the current parameters). */
#define CDAE_COMM_ID_BYTES 128
int cdae_hip_comm_unique_id(void* out, size_t bytes);
int cdae_hip_comm_init_rank(cdae_hip_t* h, int world_size, int rank, const void* unique_id, size_t bytes);
int cdae_hip_exchange_configure(cdae_hip_t* h, int period);
int cdae_hip_exchange_step(cdae_hip_t* h);
int cdae_hip_exchange_flush(cdae_hip_t* h);
int cdae_hip_exchange_time_all_reduce(cdae_hip_t* h, int repeats, double* seconds);

/* ---- several user shards behind one handle (one process, N GPUs): what Solver<CDAE>::train (solver-inl.hpp:51-55) drives
 * when src/model/recsys/cdae.hpp is given CDAE_DEVICES=0,1,... ------------------------------------------------------------
 * device_ids all distinct: one shard per GPU, one host thread per shard during an epoch, RCCL communicator from
 * ncclCommInitAll.  device_ids all equal: logical shards of ONE GPU — same schedule, the all-reduce is a fixed-order sum kernel
 * (tests, accuracy envelope).  Users are cut into contiguous ranges balanced by interactions; Wu / Wu_ag stay on their
 * shard; get/set_param address the global matrices.  Every entry point mirrors its single-handle namesake. */
typedef struct cdae_hip_multi cdae_hip_multi_t;
/* How the shards divide the model (set before _set_interactions):
 *   CDAE_LAYOUT_USERS      (default) user shards + exchange of shared-parameter deltas, as described above.
 *   CDAE_LAYOUT_ITEM_ROWS  every shard owns a contiguous range of ITEM rows — W / W_ag / (V / V_ag) / b' and the decode over them —
 *       and sees every user; b is replicated and stepped identically everywhere; the user node (Wu, Uu) is sharded by contiguous
 *       USER ranges (the owner's rows of a batch ride the first all-reduce).  Per batch two all-reduces of [batch_users x row_stride]
 *       floats cross the shards (the input sums of the encode, the hidden gradient); no item-row parameter ever does.  The schedule
 *       is the single-GPU schedule EXACTLY (same steps, same order; only the two sums are associated differently), so this layout
 *       has no accuracy cost — for the sampled decode (every shard samples the batch's whole example list against the whole rows and
 *       keeps the examples of its rows; one shard is the single handle bit for bit) and for the full-output decode (BASELINE
 *       configs[4]: 1 M items x K=512, whose dense delta would be 2 GB).  _shard() reports item ranges in this layout. */
#define CDAE_LAYOUT_USERS 0u
#define CDAE_LAYOUT_ITEM_ROWS 1u
int cdae_hip_multi_set_layout(cdae_hip_multi_t* m, uint32_t layout);
int cdae_hip_multi_create(const cdae_hip_config* cfg, int n_shards, const int* device_ids, cdae_hip_multi_t** out);
int cdae_hip_multi_destroy(cdae_hip_multi_t* m);
int cdae_hip_multi_num_shards(const cdae_hip_multi_t* m);
int cdae_hip_multi_shard(cdae_hip_multi_t* m, int shard, cdae_hip_t** handle, uint64_t* u_begin, uint64_t* u_end);
int cdae_hip_multi_set_interactions(cdae_hip_multi_t* m, uint64_t num_users, uint64_t num_items, const int64_t* row_ptr,
                                    const uint32_t* col_idx);
int cdae_hip_multi_init_params(cdae_hip_multi_t* m, uint64_t seed);
int cdae_hip_multi_set_exchange(cdae_hip_multi_t* m, int period);
/* The whole schedule of CDAE_LAYOUT_USERS (ABI 11).  An epoch e of `train_epoch` runs in two parts:
 *   RELAY  the first  R = clamp((relay_epochs - e) * num_users, 0, num_users)  users (fractions of an epoch allowed) are trained on the
 *          SINGLE-GPU schedule — Solver<CDAE>::train's order (cdae.hpp:136-146): users 0, 1, 2, ... in blocks of the handles'
 *          batch_users, every item row's chain sequential — by the shard that holds them, and the shared block is handed from shard to
 *          shard when the range crosses a cut (one device-to-device copy of [W | W_ag | b' | ... ] per shard and epoch; the other GPUs
 *          wait).  The blocks restart at every shard cut (the cuts balance interactions, they are not multiples of batch_users), so the
 *          trajectory is the single-GPU SCHEDULE — bit for bit one handle walked range by range — not the single handle's own block grid.
 *          It costs a single GPU's time and has the single-GPU schedule's accuracy: the warm-up that DESIGN.md §7 measured to
 *          bring the exchanged steps back towards the envelope (young AdaGrad accumulators are what the summed steps overshoot on).
 *   EXCHANGE  the remaining users of every shard, `sync_batch_users` (0 = the handles' batch_users) per shard and step, deltas
 *          exchanged every step (period 0) or pipelined (period k), folded in by `combine` (CDAE_COMBINE_*).
 * cdae_hip_multi_set_exchange(m, p) changes the PERIOD only: combine rule, sync_batch_users and relay_epochs stay as the last
 * set_schedule left them (a fresh handle: CDAE_COMBINE_SUM, 0, 0.0). */
typedef struct cdae_multi_schedule {
  int32_t period;
  uint32_t combine;
  uint32_t sync_batch_users;
  uint32_t reserved;
  double relay_epochs;
} cdae_multi_schedule;
int cdae_hip_multi_set_schedule(cdae_hip_multi_t* m, const cdae_multi_schedule* schedule);
int cdae_hip_multi_train_epoch(cdae_hip_multi_t* m, uint64_t seed, uint32_t epoch, cdae_hip_stats* stats);
/* users [u_begin, u_end) only — CDAE_LAYOUT_ITEM_ROWS (every shard sees every user); the user-sharded layout trains whole epochs */
int cdae_hip_multi_train_users(cdae_hip_multi_t* m, uint64_t seed, uint32_t epoch, uint64_t u_begin, uint64_t u_end,
                               cdae_hip_stats* stats);
/* User-sharded layout: the exchanged part of an epoch is `steps_per_epoch` steps (every shard trains sync_batch_users — or batch_users — of
 * its users, then the exchange).  cdae_hip_multi_train_steps runs steps [step_begin, step_end) of epoch `epoch` WITHOUT the relay part and
 * ends with a flush (replicas identical): a measurement hook — bench.py times K steps with it; training goes through train_epoch. */
uint64_t cdae_hip_multi_steps_per_epoch(const cdae_hip_multi_t* m);
int cdae_hip_multi_train_steps(cdae_hip_multi_t* m, uint64_t seed, uint32_t epoch, uint64_t step_begin, uint64_t step_end,
                               cdae_hip_stats* stats);
int cdae_hip_multi_data_loss(cdae_hip_multi_t* m, uint64_t seed, uint32_t epoch, double* out);
int cdae_hip_multi_penalty_loss(cdae_hip_multi_t* m, double* out);
int cdae_hip_multi_recommend_all(cdae_hip_multi_t* m, uint64_t u_begin, uint64_t u_end, uint32_t topk, uint32_t* out);
/* cdae_hip_eval_topn for a sharded model: the shards' lists are merged on the host (cdae_hip_multi_recommend_all), the eight means
 * are summed there in user order (same expressions and order of additions as the single-handle kernels) */
int cdae_hip_multi_eval_topn(cdae_hip_multi_t* m, const int64_t* test_row_ptr, const uint32_t* test_col, uint32_t topk,
                             double* rets8, uint64_t* hits3, uint32_t* ids_out);
int cdae_hip_multi_get_param(cdae_hip_multi_t* m, uint32_t which, float* host, size_t count);
int cdae_hip_multi_set_param(cdae_hip_multi_t* m, uint32_t which, const float* host, size_t count);

#ifdef __cplusplus
}
#endif
#endif /* CDAE_HIP_H_ */
