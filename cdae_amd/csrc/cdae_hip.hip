// cdae_hip.hip — host side of libcdae_hip.so: the C ABI of include/cdae_hip.h on top of the kernels
// in cdae_kernels.hpp.  gfx950 only; no CPU fallback: every entry point needs a HIP device and fails
// loudly without one.
#include <hip/hip_runtime.h>

#include <cstring>   // rocprim's texture_cache_iterator needs ::memset declared first

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <type_traits>
#include <utility>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "../../include/cdae_hip.h"
#include "cdae_internal.hpp"
#include "cdae_dev_buf.h"
#include "cdae_kernels.hpp"
#include "cdae_full_kernels.hpp"
#include "cdae_recommend_kernels.hpp"
#include "cdae_foldin_kernels.hpp"
#include "cdae_sort_kernels.hpp"
#include "cdae_mf_kernels.hpp"
#include "cdae_als_kernels.hpp"
#include "cdae_warp_kernels.hpp"
#include "cdae_fism_kernels.hpp"
#include "cdae_fism_pair_kernels.hpp"

#ifdef CDAE_DECODE_TIMING
#define CDAE_TOUCHED_ARG ((uint32_t*)nullptr)     // the timing build borrows `touched` for its stamps
#else
#define CDAE_TOUCHED_ARG h->d_touched
#endif

namespace {

thread_local std::string g_err;

int fail(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return 1;
}

#define HIPCHK(expr)                                                                           \
  do {                                                                                         \
    hipError_t e__ = (expr);                                                                   \
    if (e__ != hipSuccess)                                                                     \
      return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
  } while (0)

#define CHK(expr)            \
  do {                       \
    int rc__ = (expr);       \
    if (rc__) return rc__;   \
  } while (0)

}  // namespace

// DevBuf's memory (cdae_dev_buf.h): the only hipMalloc / hipFree of a handle's device memory
int cdae::mem::acquire(void** p, size_t bytes) {
  HIPCHK(hipMalloc(p, bytes));
  return 0;
}
int cdae::mem::release(void* p) {
  HIPCHK(hipFree(p));
  return 0;
}

namespace {

// launch `KERNEL<NI>` for the handle's NI (elements of a K-vector per lane)
#define DISPATCH_NI(ni, KERNEL, grid, block, shmem, stream, ...)                                  \
  do {                                                                                            \
    switch (ni) {                                                                                 \
      case 1: hipLaunchKernelGGL(KERNEL<1>, grid, block, shmem, stream, __VA_ARGS__); break;      \
      case 2: hipLaunchKernelGGL(KERNEL<2>, grid, block, shmem, stream, __VA_ARGS__); break;      \
      case 4: hipLaunchKernelGGL(KERNEL<4>, grid, block, shmem, stream, __VA_ARGS__); break;      \
      default: hipLaunchKernelGGL(KERNEL<8>, grid, block, shmem, stream, __VA_ARGS__); break;     \
    }                                                                                             \
  } while (0)
// f(std::integral_constant<int, NI>) for the handle's NI, where a launch names further template arguments or only the kernel's
// address is wanted (hipFuncSetAttribute)
template <class F> auto dispatch_ni(uint32_t ni, F&& f) {
  if (ni == 1) return f(std::integral_constant<int, 1>{});
  if (ni == 2) return f(std::integral_constant<int, 2>{});
  if (ni == 4) return f(std::integral_constant<int, 4>{});
  return f(std::integral_constant<int, 8>{});
}

// f(std::integral_constant<int, NCH>) for the contraction length NCH of the matrix-core sweeps (recommend_mfma_kernel,
// full_rank_mfma_kernel) at num_dim K <= 256: the one place that maps num_dim to it
template <class F> auto dispatch_nch(uint32_t K, F&& f) {
  if (K <= 32) return f(std::integral_constant<int, 4>{});
  if (K <= 64) return f(std::integral_constant<int, 8>{});
  if (K <= 128) return f(std::integral_constant<int, 16>{});
  if (K <= 200) return f(std::integral_constant<int, 25>{});
  return f(std::integral_constant<int, 32>{});
}

// b.alloc(n), then n elements copied from the host
template <class T> int dev_upload(DevBuf<T>& b, const T* src, size_t n) {
  CHK(b.alloc(n));
  HIPCHK(hipMemcpy(b.p, src, n * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

constexpr uint32_t MF_SEQ_USERS = 256;     // IMF / BPR sequential default: users per launch window (cdae_hip::mf_seq)
// batches above this many users take the two-launch encode (a workgroup of 16 wavefronts per user is mostly idle wavefronts;
// full-output: 512 users -7 % per step with one launch, 1024 +2 %, 2048 +11 %; sampled: equal at 1024, +4 % at 2048)
constexpr uint32_t ENCODE_USERS_MAX = 768;
enum Family { F_SAMPLE = 0, F_SORT, F_ENCODE, F_DECODE, F_HIDDEN, F_INPUT, F_COUNT };

struct Span { int family; hipEvent_t a, b; };

}  // namespace

struct cdae_hip {
  cdae_hip_config cfg{};
  int device = 0;
  hipStream_t stream = nullptr;
  uint64_t U = 0, I = 0;
  uint32_t K = 0, Kp = 0, NI = 1, B = 0;
  uint64_t uid_offset = 0;
  cdae::HyperParams hp{};

  std::vector<int64_t> h_row_ptr;
  DevBuf<int64_t> d_row_ptr;
  DevBuf<uint32_t> d_col;
  DevBuf<uint32_t> d_item_order;
  uint32_t hot_rows = 0;            // decode: rows [0, hot_rows) of item_order get a wavefront of their own
  // late rows (cdae_kernels.hpp DecodeLate): the first late_rows of them leave their hidden-gradient terms to hidden_finish_kernel
  uint32_t late_rows = 0;
  DevBuf<float> d_Ghot;             // [B][LATE_MAX]
  DevBuf<uint32_t> d_hotdup;        // [B][LATE_MAX]
  DevBuf<uint32_t> d_late_bits;     // [(I + 31) / 32] bitmap of the late rows' items
  uint32_t late_words = 0;
  bool fused_decode = false;        // decode + gather as ONE launch (decode_gather_kernel); CDAE_DECODE_UNFUSED turns it off (developer switch)
  bool fused_possible = false;      // ... what set_interactions found possible; fused_decode = fused_possible && allow_fused
  bool allow_fused = true;          // cdae_hip_set_decode_fused: off for handles whose launches may overlap another handle's on the same device
  // device error word: raised by a gather wavefront of the fused launch (bit 0) or a workgroup of bucket_sort_kernel (bit 1) that gave up
  // waiting; checked after every synchronisation of the main stream.  HOST memory mapped into the device (the kernels write it on the
  // error path only): the check is a plain read, not a 30 us device-to-host copy behind every synchronize
  uint32_t* h_err = nullptr;        // host address (a slot of the process-wide pool below: one mapped page per device, not one per handle)
  int err_slot = -1;
  uint32_t* d_fused_err = nullptr;  // the same word as the device sees it
  cdae::FusedGeom fused_geo{};      // geometry of this handle's fused launch (set at the first one)
  bool fused_geo_set = false;
  bool row_pack = true;             // the four-row role takes its rows from ExBuf::pack (CDAE_ROW_PACK=0, developer switch: popularity order as before)
  std::vector<float> h_pack_len;    // [I - hot_rows] expected lengths of the packed rows, longest first: one synthetic draw from h_rank_len (fused launch: balancing packed groups)
  std::vector<float> h_rank_len;    // [I] expected examples per batch of the row of popularity rank r (fused launch: balancing the four-row groups over the SIMDs)
  DevBuf<uint32_t> d_cold_map;      // [decode workgroups x 4] four-row group of every wavefront of the fused launch's row workgroups (0xFFFFFFFF: none)
  uint32_t num_cus = 256;
  cdae::DecodeLate decode_late() const { return cdae::DecodeLate{d_Ghot, d_hotdup, late_rows}; }
  cdae::LateFinish late_finish() { return cdae::LateFinish{d_Ghot, d_hotdup, d_item_order, d_D0, d_dup_corr, late_rows}; }
  // developer switches, read once in cdae_hip_create (DESIGN.md lists them)
  bool full_unfused = false;        // CDAE_FULL_UNFUSED: full-output decode as three separate GEMMs
  std::vector<uint32_t> h_unit_ptr;     // prefix of work units (<= hp.unit_pos positives each) per user
  DevBuf<uint32_t> d_rank_of;           // [I] inverse of d_item_order
  DevBuf<uint32_t> d_unit_user;         // [total units] user of every unit (kernels' unit -> user look-up)
  DevBuf<uint32_t> d_unit_ptr;
  uint32_t unit_cap = 0;                // most units in any window of batch_users users
  DevBuf<float> d_Hpart;                // [unit_cap][Kp] encode partial sums
  DevBuf<uint32_t> d_uptr_tmp;          // per-call prefix for cdae_hip_encode's arbitrary user lists

  // shared (item-side) parameters, one allocation: [W | W_ag | (V | V_ag) | bp | bp_ag | b | b_ag]
  DevBuf<float> d_shared;
  size_t n_shared = 0, n_matrix = 0;
  size_t off[CDAE_P_COUNT] = {0};
  size_t cnt[CDAE_P_COUNT] = {0};   // padded element counts
  DevBuf<float> d_Wu, d_Wu_ag;
  DevBuf<float> d_Uu, d_Uu_ag;          // linear_function only: [U][Kp] per-user gate (cdae.hpp:437-438)
  DevBuf<float> d_Ssum;                 // linear_function only: [B][Kp] unscaled input sums of the batch (Uu step)
  DevBuf<float> d_delta_rows;           // linear_function only: [B][Kp] Uu[u] (.) delta_u (what the input rows receive)

  // batch workspace
  uint64_t Ecap = 0;
  // example lists are kept in NSETS sets: batch q uses set q % NSETS.  Batch t+1 (and, with the second prep lane, t+2) is
  // sampled and sorted on a prep stream while batch t trains
  struct ExBuf {
    DevBuf<uint32_t> item; DevBuf<uint64_t> val;                  // user-major example list
    DevBuf<uint32_t> sorted_item; DevBuf<uint64_t> sorted_val;         // the same, stably sorted by item
    DevBuf<uint32_t> seg;                                         // [2*I]: first | one-past-last sorted position per item
    DevBuf<uint16_t> key16, sorted_key16;                             // 16-bit sort keys when I <= 65536 (rocPRIM then runs onesweep)
    DevBuf<uint32_t> dup_of_pos, dup_of_ex;                          // duplicate-negative correction rows (segment_kernel)
    DevBuf<uint32_t> dup_count;
    // counting sort (cdae_sort_kernels.hpp): per-item counts / prefix / (unused cursor), item-bucketed values, per-tile counts
    DevBuf<uint32_t> item_count, prefix, rank; DevBuf<uint64_t> bucketed;
    DevBuf<uint32_t> tile_hist, block_total;                             // (`rank` holds the in-block item prefix)
    DevBuf<uint32_t> wg_state;                                       // bucket_sort_kernel: one word per item range (cleared by the sample kernel)
    DevBuf<uint32_t> cells, cell_flag;                               // ... and its cells [ranges][units][BKC_SLOTS], filled by sample_kernel; overflow word
    uint32_t cell_tag = 0;                                           // (host) the tag of the batch last prepared into this set
    DevBuf<cdae::RowRecord> pack;                                    // row_pack_kernel: the batch's rows of the four-row decode role by this batch's length (empty: handle without the role)
    hipEvent_t ready = nullptr, released = nullptr;
  } ex[3];
  static constexpr int NSETS = 3;
  hipStream_t prep2 = nullptr;          // second prep lane (batches with odd sequence number), or nullptr: one lane, look-ahead 1
  bool prep2_own = false;               // prep2 is a stream of its own (else it aliases `aux`)
  bool prep2_auto = false;              // use the second lane only for batches of at most PREP2_AUTO_MAX_USERS users
  DevBuf<float> d_D0;                   // decoder matrix at batch start (hidden-gradient gather)
  uint32_t dup_stripes = 1;             // counters the correction rows are numbered from (cdae_kernels.hpp DUP_STRIPES)
  DevBuf<float> d_dup_corr; uint32_t dup_cap = 0;      // [dup_cap][Kp] hidden-gradient corrections of duplicate negatives
  DevBuf<float> d_HGpart;               // [8][B][Kp] per-XCD partial hidden gradients
  // full-output decode (MFMA path): bf16 operand copies and the dense gradient, padded to 128-multiples
  uint32_t Bp = 0, Ip = 0;
  DevBuf<__bf16> d_Zb, d_ZTb, d_Db, d_DTb, d_Gb, d_GTb;
  DevBuf<float> d_dD;
  DevBuf<uint8_t> d_has_in;             // [I]: item has a kept input in the block being stepped (set by full_positive_fixup_kernel, cleared by full_rows_inputs_kernel)
  DevBuf<uint32_t> d_iota;              // 0..B: identity unit prefix (fused full-output path: one hg partial row per user)
  DevBuf<uint32_t> d_bits_train;        // [NSETS][B x ceil(I/32)] rated-item bitmap of the batch (targets of the fused full-output decode), per example-buffer set
  size_t bits_stride = 0;
  uint32_t full_slices = 1;
  // Full-output path, item spaces below 32768 (full_rows_kernel): the row step writes the bf16 images of every decoder row it
  // has just stepped and the encode writes those of z, so a steady-state batch needs no conversion launch.  db_valid: d_Db / d_DTb
  // hold the CURRENT decoder (cleared by everything else that writes parameters); zb_rows: rows of d_Zb / columns of d_ZTb that may
  // be non-zero (the encode only writes the batch's users: a shorter batch takes the zero-filling conversion kernel once)
  bool db_valid = false;
  bool db_rows_valid = false;           // item spaces >= 32768: d_Db (only) holds the current decoder — the batch starts with a bf16 -> bf16 transposition
  uint32_t zb_rows = 0xFFFFFFFFu;
  // full-output, small item spaces: blocks of at most this many users run on ONE stream, the b recurrence as leading workgroups of the
  // GEMM 3 launch (first half of the users) and of the row launch (the rest) (CDAE_FULL_ONE_STREAM_MAX; 0 = always the two-stream
  // order).  Measured (Yelp shape K=50 / ML-10M shape K=200, ms per block, two streams -> one): 64 users 0.074 -> 0.051, 256: 0.076 ->
  // 0.055, 512: 0.083 -> 0.067 / 0.124 -> 0.106, 1024: 0.099 -> 0.088 / 0.145 -> 0.132, 2048: - / 0.197 -> 0.188, 4096: - / 0.327 -> 0.327
  // — a hand-off between two streams costs ~15 us, the recurrence 41 ns per user
  uint32_t full_one_stream_max = 2048;
  hipStream_t aux = nullptr;            // full-output path: the hidden-bias recurrence beside GEMM 3
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_delta = nullptr;
  bool join_pending = false;            // full-output path: the aux stream's b recurrence of the last batch has not been joined yet
  hipStream_t prep = nullptr;           // sampling + sorting of the next batch
  DevBuf<char> d_sort_tmp; size_t sort_tmp_bytes = 0, sort_tmp_stride = 0;   // two workspaces, one per prep lane
  DevBuf<float> d_Z, d_Dz, d_HG, d_G;
  DevBuf<uint32_t> d_touched;
  DevBuf<double> d_scalar;              // [8] reduction results; lives as long as the handle (cdae_hip_create)
  DevBuf<unsigned long long> d_trace;   // CDAE_WAVE_TRACE (developer aid): owns hp.trace; lives as long as the handle
  DevBuf<uint32_t> d_uids;
  // Grow-only workspaces of the evaluation and serving entry points (grow-only: ensure()): a steady-state call allocates nothing
  DevBuf<uint32_t> d_rec;               // the lists of one chunk
  DevBuf<float> d_score;                // recommend, general path: score rows when num_items * 4 B exceed the LDS
  DevBuf<float> d_zeval, d_hpart_eval;  // evaluation workspace: [users][Kp] hidden rows, [units][Kp] encode partial sums
  DevBuf<uint32_t> d_bits;              // recommend: rated-item bitmap
  // TOPN metrics on the device (cdae_hip_set_test_rows / cdae_hip_eval_topn): the validation rows as CSR, per-user metric terms
  DevBuf<int64_t> d_test_ptr; DevBuf<uint32_t> d_test_col; DevBuf<double> d_topn_pu, d_topn_out;
  uint64_t test_users_with_rows = 0;
  // cdae_hip_recommend_rows / cdae_hip_eval_topn_rows: the caller's rated sets (CSR + user of every row), target sets and per-row metric
  // terms; grow-only (capacities in rows / items), so a steady-state call allocates nothing
  DevBuf<int64_t> d_rows_ptr, d_rows_tptr;
  DevBuf<uint32_t> d_rows_uid, d_rows_col, d_rows_tcol;
  DevBuf<double> d_rows_pu;
  DevBuf<double> d_rows_out;            // [16]: the eight means, then the three hit counts
  // cdae_hip_score_rows: the candidate CSR, the tile table of the call, the scores and ranks of one chunk (grow-only, freed with the handle)
  DevBuf<int64_t> d_cand_ptr;
  DevBuf<uint32_t> d_cand_col, d_cand_rank;
  DevBuf<uint2> d_cand_tiles;
  DevBuf<float> d_cand_score;
  std::vector<uint2> h_cand_tiles;      // host image of the tile table: alive until the call's last synchronisation
  // cdae_hip_full_rank_rows: the target CSR, its bit rows for one chunk, the virtual-row table of the call, the target scores and
  // ranks of one chunk (grow-only, freed with the handle)
  DevBuf<int64_t> d_fr_tptr;
  DevBuf<uint32_t> d_fr_tcol, d_fr_tbits, d_fr_rank;
  DevBuf<uint2> d_fr_vrows;
  DevBuf<float> d_fr_tscore;
  std::vector<uint2> h_fr_vrows;        // host image of the virtual-row table: alive until the call's last synchronisation
  // cdae_hip_recommend_rows_filtered: the excl CSR, the allow list, its inverse (item -> place, [num_items]) and the packed copy of the
  // allowed decoder rows and of their b' (rebuilt by every call that has an allow list); grow-only, freed with the handle
  DevBuf<int64_t> d_flt_eptr;
  DevBuf<uint32_t> d_flt_ecol, d_flt_allow, d_flt_pos;
  DevBuf<float> d_flt_D, d_flt_bp;
  // cdae_hip_similar_items: the queries, the row_ptr that makes them a one-item-per-row CSR (0, 1, 2, ...), the table image of the call
  // (gathered and / or normalised rows; rebuilt by every call that needs one) and the +0.0 bias (zero-filled where it grows, never
  // written again); the excl CSR, the allow list and its inverse share d_flt_*.  Grow-only, freed with the handle
  DevBuf<uint32_t> d_sim_q;
  DevBuf<int64_t> d_sim_iota;
  DevBuf<float> d_sim_T, d_sim_zero;
  // WRMF handles (cdae_hip_create_als, cdae_als_kernels.hpp): the item-major CSR built once per data set (users ascending inside a
  // column; dropped with the interaction state), the Gram matrix [Kp x Kp] of the frozen table and its per-slice partials, and the
  // start vectors / solutions of one chunk of cdae_hip_als_solve_rows (its CSR shares d_rows_ptr / d_rows_col).  Grow-only.
  DevBuf<int64_t> d_tptr; DevBuf<uint32_t> d_tcol;
  DevBuf<float> d_als_G, d_als_part, d_als_x, d_als_out;
  // per-pair confidence weights (cdae_hip_als_set_confidence): user-major in the order of d_col, item-major in the order of d_tcol; null
  // = a binary handle (dropped with the data set).  d_als_rw: the weights of one cdae_hip_als_solve_rows_weighted call.  d_als_G2: the
  // second Gram of cdae_hip_als_objective; d_als_obj: its per-row terms, then <Gx, Gy>_F and the two traces.
  DevBuf<float> d_als_w, d_als_tw, d_als_rw, d_als_G2;
  DevBuf<double> d_als_obj;
  uint32_t als_steps = 0; float als_alpha = 0.f, als_lambda = 0.f;
  double als_lambda_cfg = 0.;            // lambda as configured (the objective's penalty is formed in fp64)
  // WARP handles (cdae_hip_create_warp, cdae_warp_kernels.hpp): the rank weights l[num_items] (cdae_warp_host.h, filled per data set); the
  // record of the last training calls' choices, [nnz * num_neg] by position, allocated by the first cdae_hip_warp_record_choices(1) and
  // dropped with the data set; the outputs of one chunk of cdae_hip_warp_search (grow-only)
  DevBuf<float> d_warp_l, d_warp_out_margin;
  DevBuf<uint32_t> d_warp_rec_item, d_warp_rec_cnt, d_warp_out_item, d_warp_out_cnt;
  bool warp_record = false;
  // FISM handles (cdae_hip_create_fism, cdae_fism_kernels.hpp): scale[n] = n^-alpha for n <= num_items (cdae_fism_host.h, filled per data
  // set: s_pos = scale[n - 1], s_neg = scale[n], serving scale[size of the rated set]); whether the first rows of a visit stay on chip
  DevBuf<float> d_fism_scale;
  double fism_alpha = 1.; bool fism_resident = true;
  bool fism_pair = false;        // FISMauc (cdae_hip_create_fism_pair, cdae_fism_pair_kernels.hpp): the pair loop; no user bias is allocated
  // Guest table (cdae_hip_set_guest_nodes, cdae_hip_fold_in_rows with install): a second user table, rows wu | wu_ag | uu | uu_ag of
  // [n_guests x Kp] each, that the rows entry points address as CDAE_GUEST_USER(i).  d_fold: the staging rows the fold-in kernel writes
  // (a chunk's, or the whole call's when it installs); installing EXCHANGES the two sets, so a failed call leaves the table as it was.
  // Grow-only, freed with the handle.  d_fold_long: the long rows' slots of every chunk of a call (cdae_foldin_kernels.hpp).
  DevBuf<float> d_guest[4]; uint64_t n_guests = 0;
  DevBuf<float> d_fold[4];
  DevBuf<uint32_t> d_fold_long;
  std::vector<uint32_t> h_fold_long;    // host image of that list: alive until the call's last synchronisation
  std::vector<size_t> h_fold_long_off;  // where every chunk's slots begin in it (kept here so that a steady-state call allocates no host memory either)
  int sort_bits = 1;
  // prep worker: the ~12 launches that sample + sort a batch are issued by a second host thread (the training loop was bound by
  // the HOST's launch rate: ~21 runtime calls x 4.5 us per batch on one thread)
  struct PrepJob { int set; uint64_t s0; uint32_t nb, cidx; uint64_t E; uint64_t seed; uint32_t epoch; int lane; uint64_t prof_q; };
  bool prep_threaded = true;            // CDAE_PREP_THREAD=0: issue everything from the caller's thread
  std::thread worker;
  std::mutex job_mu;
  std::condition_variable job_cv;
  std::condition_variable issued_cv;    // worker -> caller: jobs_issued advanced (await_prep_upto sleeps here after a short spin)
  std::deque<PrepJob> jobs;
  bool worker_stop = false;
  uint64_t jobs_submitted = 0;          // (caller's thread only)
  std::atomic<uint64_t> jobs_issued{0}; // jobs whose launches + `ready` record have been issued (worker -> caller)
  std::atomic<int> worker_failed{0};
  std::string worker_error;             // valid once worker_failed != 0
  std::mutex prof_mu;                   // spans / event pool are touched by both threads when profiling
  bool encode_two_launches = false;     // CDAE_ENCODE_TWO_LAUNCHES: the training encode as encode_partial + encode_finish (developer switch)
  bool debug_skip_prep = false;         // CDAE_DEBUG_SKIP_PREP (timing experiment only: batches reuse stale example lists -> WRONG results)
  // bucket_sort_kernel (cdae_sort_kernels.hpp): the default item-major ordering — one narrow launch; item ranges cut at set_interactions
  bool bucket_sort = false;
  uint32_t bucket_ranges = 0;
  DevBuf<uint32_t> d_bucket_cut;        // [bucket_ranges + 1] item ids
  bool bucket_attr_set = false;         // dynamic-LDS attribute set on this handle's device
  DevBuf<uint16_t> d_range_of;          // [I] item -> range (sample_kernel routes every example into its range's cell); empty: the sort scans the key list
  uint32_t cell_units = 0;              // units the cells are allocated for (the most of any batch)
  bool counting_sort = false;           // tile counting sort on the prep stream (cdae_sort_kernels.hpp) instead of rocPRIM: num_items <= TILE_SORT_MAX_ITEMS
  bool tile_attr_set = false;           // dynamic LDS above 64 KiB allowed for the two tile kernels (per handle: the attribute is per device)
  bool gemm3_attr_set[8] = {false, false, false, false, false, false, false, false};   // launch_gemm_lds: dynamic-LDS attribute set on this handle's device, per epilogue
  bool gemmw_attr_set[8] = {false, false, false, false, false, false, false, false};   // ... of the 256 x 256-tile kernel
  bool gemm_narrow = false;             // CDAE_GEMM_NARROW: never the 256 x 256-tile kernel (A/B switch)
  bool gemm1_tiled = false;             // CDAE_GEMM1_TILED: GEMM 1 as the 256 x 256-tile kernel where gemm1_loss_duo_kernel would run (A/B switch)
  bool gemm1_duo_attr_set[2] = {false, false};   // dynamic-LDS attribute of gemm1_loss_duo_kernel<LOSS> set on this handle's device
  bool fused_attr_set = false;          // dynamic-LDS attribute of this handle's full_decode_fused_kernel instance set (one K and loss per handle)
  bool gemm2_nt = false;                // CDAE_GEMM2_NT: hg = G D from G and D^T (gemm_nt_bf16_ldsw_kernel) where gemm_tn_bf16_kernel would read G^T and D (A/B switch)
  bool gemm_tn_attr_set = false;        // dynamic-LDS attribute of gemm_tn_bf16_kernel set on this handle's device
  bool rows_separate = false;           // CDAE_FULL_ROWS_SEPARATE: GEMM 3 and the row step as two launches where gemm3_rows_fused_kernel would run (A/B switch)
  bool fused_rows_attr_set[2][2] = {};      // dynamic-LDS attribute of gemm3_rows_fused_kernel<ADA, KH> set on this handle's device
  int rows_fused_kh = 2;                // CDAE_FULL_ROWS_KH: workgroups per item tile of the fused row step (1 | 2)

  // data-parallel exchange
  DevBuf<float> d_base, d_delta, d_recv, d_snap;   // agreed state, staged delta, all-reduced delta, parameters at the last stage
  void* xchg = nullptr; void (*xchg_free)(void*) = nullptr;   // communicator + schedule of the exchange (cdae_multi.hip)
  uint32_t delta_combine = CDAE_COMBINE_SUM;                  // cdae_hip_delta_set_combine: how staged deltas are folded in (cdae_exchange_algebra.h)
  // IMF / BPR handles (cdae_hip_create_mf, cdae_mf_kernels.hpp): 0 = CDAE, 1 = IMF, 2 = BPR; 3 = WRMF by ALS (cdae_hip_create_als):
  // IMF's tables and serving, no sampled step — every training path that asks `mf == 2 ? BPR : IMF` is refused before it is reached;
  // 4 = WARP (cdae_hip_create_warp): IMF's tables and serving, BPR's batch workspace, its own step (compute_batch_warp);
  // 5 = FISM (cdae_hip_create_fism): two item tables (an asymmetric handle's W and V), no user table, no example lists, its own loop
  // (fism_enqueue) and its own encode in front of the sweeps (fism_encode); with fism_pair (cdae_hip_create_fism_pair) the pair loop
  uint32_t mf = 0, mf_bias = 1;
  // IMF / BPR, batch_users = 1 (the library default: the reference's strictly sequential loop): the users are still taken one after the
  // other and every instance still steps the user vector and the item row(s) in place — but LAUNCHES cover MF_SEQ_USERS users: one
  // sampling launch for all of them (the draws are keyed by user, not by batch) and one mf_user_kernel<IN_PLACE> launch in which a
  // single wavefront walks them in order.  Through round 3 every user was a batch of its own: a sampling launch, a library sort and
  // a segment pass nobody read, ~20 runtime calls.  h->B is then the launch window (capacities, plans); cdae_hip_batch_users still
  // answers 1 and the stats count one block per user.
  bool mf_seq = false;
  bool mf_auto = false;                 // IMF / BPR handle created with batch_users = 0: the block size is chosen per data set (set_interactions)
  bool prep_force_sort = false;         // cdae_hip_debug_sample_batch: the item-major lists are wanted although training would not read them
  // IMF / BPR block schedule (batch_users > 1): the users are trained in ACTIVITY-GROUPED order — sorted by train-row length, cut
  // into blocks of batch_users, the blocks visited in a fixed pseudo-random order — because a block lasts as long as its most active
  // user's serial chain (a heavy-tailed mix made every block as slow as its heaviest user: 3 ms against 0.24 ms for the average
  // one).  user_perm[position] = user id, user_inv its inverse; everything on the device is indexed by POSITION, the C ABI by user
  // id (get / set_param, recommend_all map through them).  Empty: identity (CDAE; IMF / BPR with one user per block = the reference order).
  std::vector<uint32_t> user_perm, user_inv;
  uint32_t ex_per_pos = 1;              // examples of the batch's item-sorted list per train interaction (CDAE: 1 + num_neg)
  DevBuf<float> d_ub, d_ub_ag;   // [U] user bias and its accumulator
  DevBuf<float> d_UVpre;                // [instances of a batch][Kp]: user vector before each instance's step (phase I input)
  // item-sharded layout (cdae_multi.hip): this handle holds item rows [item0, item0 + I) of I_global; every user,
  // possibly with no local item.  The two per-user sums that cross shards live in d_Hsum (input sums) and d_HG (hidden gradient).
  bool item_shard = false; uint64_t item0 = 0, I_global = 0;
  DevBuf<uint32_t> d_gpos;              // item shard: per user (length of the whole row, position of the first local item): the dropout stream's index space
  DevBuf<float> d_Hsum;
  DevBuf<float> d_hsum_eval;            // item shard, evaluation: [users][SHARD_BLOCKS x Kp] input-sum all-reduce buffer of a chunk
  DevBuf<float> d_rec_score;            // the scores of d_rec's lists (item-sharded top-k merge, the rows entry points' out_scores)
  uint64_t fs_prepped = 0;              // item-sharded training: batches whose example lists have been prepared (buffer set = parity)
  // item shard: users [own_u0, own_u1) keep their private rows (Wu, Wu_ag, Uu, Uu_ag) HERE, table row 0 = user own_u0 (SURVEY.md
  // §8(e): the user node is sharded by user; the rows of a batch's users reach the other shards through the input-sum all-reduce)
  uint64_t own_u0 = 0, own_u1 = ~0ull;
  uint64_t wu_rows() const { return item_shard ? std::min<uint64_t>(own_u1, U) - std::min<uint64_t>(own_u0, U) : U; }
  // item shard, SAMPLED decode: the WHOLE train rows with global item ids — negatives are drawn from all I_global items and
  // rejected against the whole row, the example list keeps the single-GPU layout (work units over the whole rows)
  const int64_t* g_row_ptr_src = nullptr; const uint32_t* g_col_src = nullptr;   // (set_item_shard_global -> the next set_interactions)
  std::vector<int64_t> h_grow_ptr;
  std::vector<uint32_t> h_gunit_ptr;
  DevBuf<int64_t> d_grow_ptr; DevBuf<uint32_t> d_gcol, d_gunit_ptr, d_gunit_user;
  bool shard_sampled() const { return item_shard && !cfg.full_output; }

  bool skip_ready_wait = false;         // compute_batch: enqueue_users has seen the set's `ready` event complete on the host (no wait packet on the main stream)
  uint32_t host_pace_us = 200;          // enqueue_users: how long the caller's thread looks for a batch's lists to be complete before it leaves the wait to the device (0: always the device; CDAE_HOST_PACE_US, developer switch)
  uint64_t seq = 0;                     // batches enqueued so far; batch q uses example-buffer set q % NSETS
  // sets (seq + t) % NSETS, t < pre_n, already hold (or have queued) the prepared batches pre[t] (cdae_hip_prefetch_users)
  struct PreBatch { uint64_t s0, seed; uint32_t nb, cidx, epoch; };
  PreBatch pre[2] = {};
  uint32_t pre_n = 0;
  uint64_t acc_users = 0, acc_examples = 0, acc_batches = 0;   // since the last stats collection
  int profiling = 0;                    // 0 off; k >= 1: HIP events around the kernel families of every k-th batch
  uint32_t prof_mask = 0xFFFFFFFFu;     // ... of the families whose bit is set (cdae_hip_set_profiling_families)
  uint64_t prof_q = 0;                  // sequence number of the batch being enqueued (sampling of the profile)
  std::vector<Span> spans;
  std::vector<hipEvent_t> pool;

  float* P(uint32_t which) {
    if (which == CDAE_P_WU) return d_Wu;
    if (which == CDAE_P_WU_AG) return d_Wu_ag;
    if (which == CDAE_P_UU) return d_Uu;
    if (which == CDAE_P_UU_AG) return d_Uu_ag;
    if (which == CDAE_P_UB) return d_ub;
    if (which == CDAE_P_UB_AG) return d_ub_ag;
    return cnt[which] ? d_shared + off[which] : nullptr;
  }
  float* dec() { return cfg.asymmetric ? P(CDAE_P_V) : P(CDAE_P_W); }
  float* dec_ag() { return cfg.asymmetric ? P(CDAE_P_V_AG) : P(CDAE_P_W_AG); }
  float* delta_rows() { return cfg.linear_function ? d_delta_rows : d_HG; }
};

namespace {

// Full-output path: the hidden-bias recurrence of a batch runs on the aux stream and is joined as LATE as possible — right
// before the next batch's encode_finish (the first consumer of b and of the delta buffer), so that the next batch's input
// gather and the bf16 copies of D overlap its tail.  Every other entry point that touches parameters or the main stream
// joins first.
int join_aux(cdae_hip* h) {
  if (h->join_pending) {
    HIPCHK(hipStreamWaitEvent(h->stream, h->ev_join, 0));
    h->join_pending = false;
  }
  return 0;
}

// Device error words: ONE page of mapped host memory per device and process, a slot per handle (a pinned, mapped allocation per handle
// is a system-wide resource; hundreds of handles in one process — a test session — should not each hold one).
struct ErrPool {
  static constexpr int SLOTS = 1024;
  uint32_t* host = nullptr; uint32_t* dev = nullptr;
  std::vector<char> used;
};
std::mutex g_err_mu;
ErrPool g_err_pool[64];
int err_slot_acquire(int device, uint32_t** host, uint32_t** dev, int* slot) {
  std::lock_guard<std::mutex> lk(g_err_mu);
  if (device < 0 || device >= 64) return fail("device id %d outside the error-word pool", device);
  ErrPool& p = g_err_pool[device];
  if (!p.host) {
    HIPCHK(hipHostMalloc((void**)&p.host, ErrPool::SLOTS * sizeof(uint32_t), hipHostMallocMapped));
    HIPCHK(hipHostGetDevicePointer((void**)&p.dev, p.host, 0));
    p.used.assign(ErrPool::SLOTS, 0);
  }
  for (int i = 0; i < ErrPool::SLOTS; ++i)
    if (!p.used[i]) { p.used[i] = 1; p.host[i] = 0u; *host = p.host + i; *dev = p.dev + i; *slot = i; return 0; }
  return fail("more than %d live handles on device %d", ErrPool::SLOTS, device);
}
void err_slot_release(int device, int slot) {
  std::lock_guard<std::mutex> lk(g_err_mu);
  if (device >= 0 && device < 64 && slot >= 0 && g_err_pool[device].host) g_err_pool[device].used[slot] = 0;
}

// After the main stream has been synchronised: the handle's device error word.  Bit 0: a gather wavefront of a fused launch
// (decode_gather_kernel) gave up waiting for a g; bit 1: a workgroup of bucket_sort_kernel gave up waiting for the ranges in front of it.
// Both waits rest on workgroups being dispatched in index order and are bounded, so that a broken assumption is an error, not a hang.
int fused_check(cdae_hip* h) {
  if (!h->d_fused_err || !(h->fused_decode || h->bucket_sort)) return 0;
  const uint32_t err = *(volatile uint32_t*)h->h_err;
  if (err) {
    *(volatile uint32_t*)h->h_err = 0u;
    return fail("%s%s: workgroups not dispatched in index order, or a launch that was skipped?  The parameters of this handle are no longer valid",
                (err & 1u) ? "fused decode + gather launch: a gather wavefront gave up waiting for its g; " : "",
                (err & 2u) ? "bucket_sort_kernel: a workgroup gave up waiting for the ranges in front of it" : "");
  }
  return 0;
}

// Events between the library's own streams order work on ONE device: they need no system-scope fence.  A default HIP event
// writes back and invalidates the caches when it is recorded — measured here as ~14 us of idle main stream per batch around
// the `released` record and ~3 us at the `ready` wait (profiles/r02_wave_timeline_256.txt: 86 us of kernels in a 100 us step).
// CDAE_EVENT_SYSTEM_FENCE=1 restores the default.  (The exchange's events in cdae_multi.hip stay system-scope: RCCL peers read.)
inline unsigned sync_event_flags() {      // (the environment is read at every call: per handle, not per process)
  const bool sys = DEV_ENV("CDAE_EVENT_SYSTEM_FENCE") != nullptr;
  return sys ? (unsigned)hipEventDisableTiming : (unsigned)(hipEventDisableTiming | hipEventDisableSystemFence);
}
inline unsigned timing_event_flags() {
  const bool sys = DEV_ENV("CDAE_EVENT_SYSTEM_FENCE") != nullptr;
  return sys ? (unsigned)hipEventDefault : (unsigned)hipEventDisableSystemFence;
}

int get_event(cdae_hip* h, hipEvent_t* ev) {
  {
    std::lock_guard<std::mutex> lk(h->prof_mu);
    if (!h->pool.empty()) { *ev = h->pool.back(); h->pool.pop_back(); return 0; }
  }
  HIPCHK(hipEventCreateWithFlags(ev, timing_event_flags()));
  return 0;
}
struct Prof {   // RAII-less helper: begin()/end() around one kernel family launch, on the stream it is launched on
  cdae_hip* h; Span s; bool on; hipStream_t st;
  int begin(cdae_hip* hh, int family, hipStream_t stream, uint64_t q = ~0ull /* batch sequence number; default: the caller thread's prof_q */) {
    if (q == ~0ull) q = hh->prof_q;
    h = hh; on = hh->profiling > 0 && ((hh->prof_mask >> family) & 1u) && q % (uint64_t)hh->profiling == 0; st = stream; if (!on) return 0;
    s.family = family;
    CHK(get_event(h, &s.a)); CHK(get_event(h, &s.b));
    HIPCHK(hipEventRecord(s.a, st));
    return 0;
  }
  int end() {
    if (!on) return 0;
    HIPCHK(hipEventRecord(s.b, st));
    std::lock_guard<std::mutex> lk(h->prof_mu);
    h->spans.push_back(s);
    return 0;
  }
};

int collect_profile(cdae_hip* h, cdae_hip_stats* st) {
  double ms[F_COUNT] = {0};
  uint64_t launches[F_COUNT] = {0};
  std::lock_guard<std::mutex> lk(h->prof_mu);
  for (Span& s : h->spans) {
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, s.a, s.b));
    ms[s.family] += t;
    launches[s.family]++;
    h->pool.push_back(s.a); h->pool.push_back(s.b);
  }
  h->spans.clear();
  if (st) {
    st->ms_sample = ms[F_SAMPLE]; st->ms_sort = ms[F_SORT]; st->ms_encode = ms[F_ENCODE];
    st->ms_decode = ms[F_DECODE]; st->ms_hidden = ms[F_HIDDEN]; st->ms_input = ms[F_INPUT];
    st->launches_decode = launches[F_DECODE];
  }
  return 0;
}

// Every device buffer that a data set owns, listed ONCE: f(buffers...) is called for the three example-buffer sets and then for the
// handle's own.  A new buffer is added HERE only.  Not in the list: d_scalar and d_trace, which cdae_hip_create allocates and which
// live as long as the handle — their destructors free them.
template <class F> void visit_data_set_bufs(cdae_hip* h, F&& f) {
  for (auto& b : h->ex)
    f(b.item, b.val, b.sorted_item, b.sorted_val, b.seg, b.dup_of_pos, b.dup_of_ex, b.dup_count, b.key16, b.sorted_key16,
      b.item_count, b.prefix, b.rank, b.bucketed, b.tile_hist, b.block_total, b.wg_state, b.cells, b.cell_flag, b.pack);
  f(h->d_row_ptr, h->d_col, h->d_item_order, h->d_shared, h->d_Wu, h->d_Wu_ag, h->d_D0, h->d_HGpart, h->d_sort_tmp,
    h->d_unit_ptr, h->d_Hpart, h->d_uptr_tmp, h->d_Zb, h->d_ZTb, h->d_Db, h->d_DTb, h->d_Gb, h->d_GTb, h->d_dD, h->d_has_in,
    h->d_Z, h->d_Dz, h->d_HG, h->d_G, h->d_touched, h->d_uids, h->d_base, h->d_delta, h->d_recv, h->d_snap,
    h->d_dup_corr, h->d_unit_user, h->d_iota, h->d_bits_train,
    h->d_Uu, h->d_Uu_ag, h->d_Ssum, h->d_delta_rows, h->d_Hsum,
    h->d_gpos, h->d_ub, h->d_ub_ag, h->d_UVpre, h->d_rank_of, h->d_grow_ptr, h->d_gcol, h->d_gunit_ptr, h->d_gunit_user,
    h->d_test_ptr, h->d_test_col, h->d_topn_pu, h->d_topn_out, h->d_bucket_cut, h->d_range_of,
    h->d_Ghot, h->d_hotdup, h->d_late_bits, h->d_cold_map, h->d_rows_out, h->d_tptr, h->d_tcol,
    // the grow-only workspaces of the evaluation and serving entry points
    h->d_rec, h->d_rec_score, h->d_score, h->d_bits, h->d_zeval, h->d_hpart_eval, h->d_hsum_eval,
    h->d_rows_ptr, h->d_rows_uid, h->d_rows_col, h->d_rows_tptr, h->d_rows_pu, h->d_rows_tcol,
    h->d_cand_ptr, h->d_cand_col, h->d_cand_tiles, h->d_cand_score, h->d_cand_rank,
    h->d_fr_tptr, h->d_fr_tcol, h->d_fr_tbits, h->d_fr_vrows, h->d_fr_tscore, h->d_fr_rank,
    h->d_flt_eptr, h->d_flt_ecol, h->d_flt_allow, h->d_flt_pos, h->d_flt_D, h->d_flt_bp,
    h->d_sim_q, h->d_sim_iota, h->d_sim_T, h->d_sim_zero,
    h->d_guest[0], h->d_guest[1], h->d_guest[2], h->d_guest[3], h->d_fold[0], h->d_fold[1], h->d_fold[2], h->d_fold[3],
    h->d_fold_long, h->d_als_G, h->d_als_part, h->d_als_x, h->d_als_out, h->d_als_w, h->d_als_tw, h->d_als_rw, h->d_als_G2, h->d_als_obj,
    h->d_warp_l, h->d_warp_rec_item, h->d_warp_rec_cnt, h->d_warp_out_item, h->d_warp_out_cnt, h->d_warp_out_margin,
    h->d_fism_scale);
}
// Drops every one of them; the first release error is returned after all have been dropped.
int drop_data_set_bufs(cdae_hip* h) {
  int rc = 0;
  visit_data_set_bufs(h, [&](auto&... b) { ((rc = b.drop() || rc), ...); });
  return rc;
}

void free_all(cdae_hip* h) {
  (void)drop_data_set_bufs(h);        // (errors ignored: the handle goes away; before the streams and events do)
  for (auto& b : h->ex) {
    if (b.ready) (void)hipEventDestroy(b.ready);
    if (b.released) (void)hipEventDestroy(b.released);
  }
  if (h->h_err) { err_slot_release(h->device, h->err_slot); h->h_err = nullptr; h->d_fused_err = nullptr; h->err_slot = -1; }
  if (h->prep) (void)hipStreamDestroy(h->prep);
  if (h->prep2 && h->prep2_own) (void)hipStreamDestroy(h->prep2);
  if (h->aux) (void)hipStreamDestroy(h->aux);
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  if (h->ev_delta) (void)hipEventDestroy(h->ev_delta);
  for (hipEvent_t e : h->pool) (void)hipEventDestroy(e);
  for (Span& s : h->spans) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
  if (h->stream) (void)hipStreamDestroy(h->stream);
}

int await_prep(cdae_hip* h);     // (prep worker, below)
void stop_prep_worker(cdae_hip* h);
int quiesce(cdae_hip* h) {
  CHK(await_prep(h));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (h->prep) HIPCHK(hipStreamSynchronize(h->prep));
  if (h->prep2) HIPCHK(hipStreamSynchronize(h->prep2));
  if (h->aux) HIPCHK(hipStreamSynchronize(h->aux));
  return 0;
}

int free_interaction_state(cdae_hip* h) {
  CHK(drop_data_set_bufs(h));
  h->db_valid = false; h->db_rows_valid = false; h->zb_rows = 0xFFFFFFFFu;
  h->n_guests = 0;
  h->warp_record = false;
  return 0;
}

// one batch of train_one_user_corruption for users [s0, s0+nb), corruption cidx
struct Batch { uint64_t s0; uint32_t nb; uint32_t cidx; uint64_t E; };

inline uint32_t units_of(const cdae_hip* h, const Batch& b) { return h->h_unit_ptr[b.s0 + b.nb] - h->h_unit_ptr[b.s0]; }
// item shard, sampled decode: units over the WHOLE rows (sample_kernel, hidden_gather_kernel)
inline uint32_t gunits_of(const cdae_hip* h, const Batch& b) { return h->h_gunit_ptr[b.s0 + b.nb] - h->h_gunit_ptr[b.s0]; }

// Rows [0, decode_hot_rows) take a wavefront of their own in the K <= 256 decode launches; the others go four to a wavefront.
inline uint32_t decode_hot_rows(const cdae_hip* h) { return std::min<uint32_t>(h->hot_rows, (uint32_t)h->I); }
// Handles whose batches get a row pack (row_pack_kernel): the sampled K <= 256 decode of a single handle.  An item shard's decode takes
// its rows in popularity order (pack == nullptr): its step is paced by the exchange, not by this launch.
inline bool packs_rows(const cdae_hip* h) { return h->row_pack && h->K <= 256 && !h->mf && !h->cfg.full_output && !h->item_shard; }
// ... and the batches of such a handle that have one: every batch prep_batch ordered (an explicit input set is ordered by its caller)
inline cdae::RowRecord* pack_of(const cdae_hip* h, const cdae_hip::ExBuf& x, uint64_t E) { return packs_rows(h) && E > 0 ? x.pack.p : nullptr; }

// The item-major order of a batch's example list: x.item / x.val (or the 16-bit keys, or the sample kernel's cells) into x.sorted_val and
// the segment tables.  prep_batch calls it on a prep stream behind the sampling launch; a WARP handle, whose lists exist only after
// phase U, on the training stream (compute_batch_warp) — it takes the library sort on the 32-bit keys, VOID key included.
// void_key: the key of examples that belong to no row of this handle (sorted last: no segment, no duplicate marks), or 0xFFFFFFFF
int order_examples(cdae_hip* h, cdae_hip::ExBuf& x, uint64_t E, hipStream_t st, void* sort_tmp, uint32_t n_units, bool bucket, bool use_cells,
                   uint32_t void_key) {
  using namespace cdae;
  const uint32_t I = (uint32_t)h->I;
  const dim3 seg_grid((uint32_t)((E + 256 * SEG_PER_THREAD - 1) / (256 * SEG_PER_THREAD)));
  if (E == 0) {
    // nothing to order
  } else if (h->mf_seq && !h->prep_force_sort) {
    // the in-place loop reads the user-major list only: no item-major order, no segment table
  } else if (bucket) {
    // item-major order, segment tables, duplicate marks: ONE narrow launch (cdae_sort_kernels.hpp bucket_sort_kernel)
    if (!h->bucket_attr_set) {
      HIPCHK(hipFuncSetAttribute((const void*)bucket_sort_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)BK_LDS_BYTES));
      h->bucket_attr_set = true;
    }
    hipLaunchKernelGGL(bucket_sort_kernel, dim3(h->bucket_ranges), dim3(BK_THREADS), BK_LDS_BYTES, st, (const uint16_t*)x.key16, (const uint64_t*)x.val,
                       (uint32_t)E, (const uint32_t*)h->d_bucket_cut, x.wg_state, (const uint32_t*)(use_cells ? x.cells.p : nullptr), n_units,
                       (const uint32_t*)x.cell_flag, x.cell_tag, x.seg, x.seg + I, (const uint32_t*)h->d_rank_of,
                       x.seg + 2 * (size_t)I, x.seg + 3 * (size_t)I, x.sorted_val, x.bucketed, x.dup_count, h->dup_cap, x.dup_of_pos, x.dup_of_ex,
                       h->dup_stripes, h->d_fused_err);
  } else if (h->counting_sort) {
    // item-major order by counting, four launches (cdae_sort_kernels.hpp)
    const uint32_t n_tiles = (uint32_t)((E + TILE_EX - 1) / TILE_EX);
    const size_t tile_lds = (size_t)I * sizeof(uint32_t);
    if (tile_lds + 1024 > 64 * 1024 && !h->tile_attr_set) {
      HIPCHK(hipFuncSetAttribute((const void*)tile_hist_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_lds));
      HIPCHK(hipFuncSetAttribute((const void*)tile_scatter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_lds + 1024));
      h->tile_attr_set = true;
    }
    hipLaunchKernelGGL(tile_hist_kernel, dim3(n_tiles), dim3(TILE_THREADS), tile_lds / 2 + 4, st, x.item, (uint32_t)E, I, x.tile_hist);
    hipLaunchKernelGGL(item_tile_scan_kernel, dim3((I + 255) / 256), dim3(256), 0, st, x.tile_hist, n_tiles, I, x.item_count, x.rank, x.block_total);
    hipLaunchKernelGGL(tile_scatter_kernel, dim3(n_tiles), dim3(TILE_THREADS), tile_lds + 128 * sizeof(uint32_t), st, x.item, x.val,
                       (uint32_t)E, I, x.tile_hist, x.item_count, x.rank, x.block_total, x.prefix, x.seg, x.seg + I, x.dup_count, x.bucketed,
                       (const uint32_t*)h->d_rank_of, x.seg + 2 * (size_t)I, x.seg + 3 * (size_t)I);
    hipLaunchKernelGGL(segment_sort_kernel, dim3((I + SEGSORT_ITEMS - 1) / SEGSORT_ITEMS), dim3(SEGSORT_THREADS), 0, st, I, x.prefix, x.bucketed,
                       x.sorted_val, x.item_count, x.dup_count, h->dup_cap, x.dup_of_pos, x.dup_of_ex, h->dup_stripes);
  } else if (x.key16) {
    // 16-bit keys: rocPRIM picks onesweep (2 digit passes) instead of block sort + log2(tiles) merge passes
    HIPCHK(rocprim::radix_sort_pairs(sort_tmp, h->sort_tmp_bytes, x.key16.p, x.sorted_key16.p, x.val.p, x.sorted_val.p,
                                     (size_t)E, 0u, (unsigned)h->sort_bits, st));
    hipLaunchKernelGGL(segment_kernel<uint16_t>, seg_grid, dim3(256), 0, st, x.sorted_key16, x.sorted_val, (uint32_t)E,
                       x.seg, x.seg + I, x.dup_count, h->dup_cap, x.dup_of_pos, x.dup_of_ex, h->dup_stripes,
                       (const uint32_t*)h->d_rank_of, x.seg + 2 * (size_t)I, x.seg + 3 * (size_t)I, void_key);
  } else {
    HIPCHK(rocprim::radix_sort_pairs(sort_tmp, h->sort_tmp_bytes, x.item.p, x.sorted_item.p, x.val.p, x.sorted_val.p,
                                     (size_t)E, 0u, (unsigned)h->sort_bits, st));
    hipLaunchKernelGGL(segment_kernel<uint32_t>, seg_grid, dim3(256), 0, st, x.sorted_item, x.sorted_val, (uint32_t)E,
                       x.seg, x.seg + I, x.dup_count, h->dup_cap, x.dup_of_pos, x.dup_of_ex, h->dup_stripes,
                       (const uint32_t*)h->d_rank_of, x.seg + 2 * (size_t)I, x.seg + 3 * (size_t)I, void_key);
  }
  return 0;
}

// K1 + sort on the prep stream into example-buffer set `b`
// lane 1: the second prep stream with the second half of the sort workspace (two batches are prepared side by side)
int prep_batch(cdae_hip* h, int b, const Batch& bt, uint64_t seed, uint32_t epoch, int lane = 0, uint64_t prof_q = ~0ull) {
  using namespace cdae;
  cdae_hip::ExBuf& x = h->ex[b];
  hipStream_t st = lane ? h->prep2 : h->prep;
  void* sort_tmp = (char*)h->d_sort_tmp + (lane ? h->sort_tmp_stride : 0);
  const uint32_t I = (uint32_t)h->I;
  Prof pr;
  HIPCHK(hipStreamWaitEvent(st, x.released, 0));               // the batch that last used this set is done with it
  if (h->mf == 4u) {
    // WARP: nothing to draw — the items of a pair are chosen in phase U (warp_user_kernel) and ordered behind it on the training
    // stream (compute_batch_warp).  Only the per-batch clears of the block schedule: the by-item segment tables, the duplicate counters
    if (!h->mf_seq) {
      HIPCHK(hipMemsetAsync(x.seg, 0, 2 * (size_t)I * sizeof(uint32_t), st));
      HIPCHK(hipMemsetAsync(x.dup_count, 0, cdae::DUP_STRIPES * sizeof(uint32_t), st));
    }
    HIPCHK(hipEventRecord(x.ready, st));
    return 0;
  }
  CHK(pr.begin(h, F_SAMPLE, st, prof_q));
  const bool shs = h->shard_sampled();
  const uint32_t n_units = shs ? gunits_of(h, bt) : units_of(h, bt);
  const bool bucket = h->bucket_sort && x.key16;      // bucket_sort_kernel writes every entry of the segment tables itself: nothing to clear
  const bool use_cells = bucket && x.cells && n_units <= h->cell_units;   // sample_kernel routes the examples into the ranges' cells
  if (use_cells) x.cell_tag = x.cell_tag + 1u ? x.cell_tag + 1u : 1u;     // a fresh non-zero tag per batch: nobody has to clear the overflow word
  if (n_units == 0) {            // (an item shard none of whose rows the batch's users rated: only the per-batch clears)
    HIPCHK(hipMemsetAsync(x.seg, 0, 4 * (size_t)I * sizeof(uint32_t), st));
    HIPCHK(hipMemsetAsync(x.dup_count, 0, cdae::DUP_STRIPES * sizeof(uint32_t), st));
  } else if (h->mf) {
    hipLaunchKernelGGL(mf_sample_kernel, dim3((n_units + 3) / 4), dim3(256), 0, st, h->hp, h->mf == 2 ? 1u : 0u, h->d_row_ptr, h->d_col,
                       h->d_unit_ptr + bt.s0, n_units, bt.s0, bt.nb, seed, epoch, x.item, x.val, x.key16, x.seg, bucket ? 0u : 2u * I, x.dup_count,
                       x.dup_of_ex, h->d_unit_user, x.wg_state);
  } else if (shs) {
    // item shard, sampled decode: the single-GPU example list of the batch from the WHOLE rows, other shards' examples VOID
    hipLaunchKernelGGL(sample_kernel, dim3((n_units + 3) / 4), dim3(256), 0, st, h->hp, h->d_grow_ptr, h->d_gcol,
                       h->d_gunit_ptr + bt.s0, n_units, bt.s0, bt.nb, bt.cidx, seed, epoch, x.item, x.val, x.key16,
                       x.seg, h->counting_sort || bucket ? 0u : 4u * I, x.dup_count, x.dup_of_ex, h->d_gunit_user,
                       x.wg_state, (const uint32_t*)nullptr, (uint32_t)h->item0, I, (uint32_t)h->I_global,
                       (const uint16_t*)(use_cells ? h->d_range_of.p : nullptr), (const uint32_t*)h->d_bucket_cut, h->bucket_ranges,
                       use_cells ? x.cells : (uint32_t*)nullptr, x.cell_flag, x.cell_tag);
  } else
  hipLaunchKernelGGL(sample_kernel, dim3((n_units + 3) / 4), dim3(256), 0, st, h->hp, h->d_row_ptr, h->d_col,
                     h->d_unit_ptr + bt.s0, n_units, bt.s0, bt.nb, bt.cidx, seed, epoch, x.item, x.val, x.key16,
                     x.seg, h->counting_sort || bucket ? 0u : 4u * I, x.dup_count, x.dup_of_ex, h->d_unit_user,
                     x.wg_state, (const uint32_t*)h->d_gpos, 0u, 0u, 0u,
                     (const uint16_t*)(use_cells ? h->d_range_of.p : nullptr), (const uint32_t*)h->d_bucket_cut, h->bucket_ranges,
                     use_cells ? x.cells : (uint32_t*)nullptr, x.cell_flag, x.cell_tag);
  CHK(pr.end());
  CHK(pr.begin(h, F_SORT, st, prof_q));
  CHK(order_examples(h, x, bt.E, st, sort_tmp, n_units, bucket, use_cells, shs ? I : 0xFFFFFFFFu));
  if (RowRecord* const pack = pack_of(h, x, bt.E))
    hipLaunchKernelGGL(row_pack_kernel, dim3(1), dim3(ROW_PACK_THREADS), 0, st, (const uint32_t*)h->d_item_order, (const uint32_t*)(x.seg + 2 * (size_t)I),
                       (const uint32_t*)(x.seg + 3 * (size_t)I), decode_hot_rows(h), I, pack);
  CHK(pr.end());
  if (h->cfg.full_output && h->d_bits_train) {
    // fused full-output decode: its targets — one bit per (batch user, item) — depend on the data set only, so they are
    // built here, beside the previous batch's training, instead of in front of the decode (memset + kernel: 22 us per batch)
    const uint32_t words = (I + 31) / 32;
    uint32_t* bits = h->d_bits_train + (size_t)b * h->bits_stride;
    hipLaunchKernelGGL(rated_bits_kernel, dim3((bt.nb + 3) / 4), dim3(256), 0, st, h->d_row_ptr, h->d_col, bt.s0, bt.nb, words, bits);
  }
  HIPCHK(hipEventRecord(x.ready, st));
  HIPCHK(hipGetLastError());
  return 0;
}

// Geometry of the fused launch (decode_gather_kernel), once per handle.
// packed: the groups hold the batch's rows by length (row_pack_kernel) — group q the 4q-th .. (4q+3)-th longest
int fused_geometry(cdae_hip* h, uint32_t hot, uint32_t I, bool packed) {
  using namespace cdae;
  FusedGeom g{};
  g.hot_wgs = (hot + 3) / 4;
  // The four-row groups are dealt to (CU, SIMD) bins so that every SIMD gets about the same number of example steps (longest group first,
  // each to the lightest bin): a group lasts as long as its longest row, the SIMDs are VALU-bound on these wavefronts, and in index
  // order (round 5) the SIMDs that held the most popular groups finished 10-15 us after the others — which every gather wavefront of
  // this launch then waits for.  Workgroup b's wavefront w runs on SIMD w of CU b mod S (observed placement: only the balance depends
  // on it): the k-th group of bin (cu, w) goes to workgroup cu + k S.  The popular rows' CUs take no group.
  const uint32_t n_groups = (I - hot + 3) / 4, S = h->num_cus;
  std::vector<float> len(n_groups, 0.f);
  if (packed) {
    // Packed group q lasts as long as the 4q-th longest row of the batch: an ORDER STATISTIC of the lengths, not a rank's mean (in the
    // tail the means are flat while the sorted lengths run from ~30 down to ~3).  One synthetic batch stands for all: Poisson draws
    // from the rows' means, fixed seed, sorted.  Scheduling only — no result depends on it.
    if (h->h_pack_len.size() != (size_t)(I - hot)) {
      std::mt19937_64 rng(0x9E3779B97F4A7C15ull);
      h->h_pack_len.resize(I - hot);
      for (uint32_t r = hot; r < I; ++r)
        h->h_pack_len[r - hot] = (float)std::poisson_distribution<uint32_t>(std::max((double)h->h_rank_len[r], 1e-6))(rng);
      std::sort(h->h_pack_len.begin(), h->h_pack_len.end(), std::greater<float>());
    }
    for (uint32_t q = 0; q < n_groups; ++q) len[q] = h->h_pack_len[4 * (size_t)q];
  } else
  for (uint32_t q = 0; q < n_groups; ++q)
    for (uint32_t j = 0; j < 4 && hot + 4 * q + j < I; ++j) len[q] = std::max(len[q], h->h_rank_len[hot + 4 * q + j]);
  std::vector<uint32_t> by_len(n_groups);
  std::iota(by_len.begin(), by_len.end(), 0u);
  std::stable_sort(by_len.begin(), by_len.end(), [&](uint32_t a, uint32_t b2) { return len[a] > len[b2]; });
  const uint32_t cu0 = std::min(g.hot_wgs, S > 8 ? S - 8 : 0u);                 // CUs [0, cu0) belong to the popular rows
  const uint32_t n_bins = (S - cu0) * 4;
  std::vector<std::vector<uint32_t>> bin(n_bins);
  {
    // lightest bin first: a heap of (load, bin)
    using Ent = std::pair<float, uint32_t>;
    std::vector<Ent> heap;
    for (uint32_t i = 0; i < n_bins; ++i) heap.push_back({0.f, i});
    auto cmp = [](const Ent& a, const Ent& b2) { return a.first > b2.first || (a.first == b2.first && a.second > b2.second); };
    std::make_heap(heap.begin(), heap.end(), cmp);
    for (uint32_t k = 0; k < n_groups; ++k) {
      const uint32_t q = by_len[k];
      std::pop_heap(heap.begin(), heap.end(), cmp);
      Ent e = heap.back();
      bin[e.second].push_back(q);
      e.first += 4.f + len[q];                                                    // (+ a wavefront's fixed cost: prologue, epilogue)
      heap.back() = e;
      std::push_heap(heap.begin(), heap.end(), cmp);
    }
  }
  size_t rounds_cold = 0;
  for (auto& v : bin) rounds_cold = std::max(rounds_cold, v.size());
  // cold round k of CU cu is workgroup index cu + k S
  g.decode_wgs = (uint32_t)std::max<size_t>(rounds_cold, 1) * S;
  std::vector<uint32_t> map((size_t)g.decode_wgs * 4, 0xFFFFFFFFu);
  for (uint32_t i = 0; i < n_bins; ++i) {
    const uint32_t cu = cu0 + i / 4, w = i % 4;
    for (size_t k = 0; k < bin[i].size(); ++k) map[((size_t)k * S + cu) * 4 + w] = bin[i][k];
  }
  CHK(h->d_cold_map.alloc(map.size()));
  HIPCHK(hipMemcpy(h->d_cold_map, map.data(), map.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  g.cold_map = h->d_cold_map;
  h->fused_geo = g;
  h->fused_geo_set = true;
  return 0;
}

// K3 on the main stream: the decode of example-buffer set `x` over this handle's item rows (shared by the single-handle step and
// the sampled item-shard step)
// fused != nullptr: the fused launch (decode_gather_kernel) with these gather arguments; the caller then launches no hidden_gather_kernel
// pack: the set's row pack of this batch (pack_of), or nullptr: rows in popularity order
int launch_decode(cdae_hip* h, cdae_hip::ExBuf& x, const cdae::GatherArgs* fused = nullptr, const cdae::RowRecord* pack = nullptr) {
  using namespace cdae;
  hipStream_t st = h->stream;
  const uint32_t I = (uint32_t)h->I;
  const dim3 blk(256);
  const dim3 grid_rows((I + 3) / 4);
#define DECODE_TAIL h->d_item_order, x.seg + 2 * (size_t)I, x.seg + 3 * (size_t)I, x.sorted_val, h->d_Z, h->dec(), h->dec_ag(), \
                    h->P(CDAE_P_BP), h->P(CDAE_P_BP_AG), h->d_HG, h->d_G, h->d_D0, h->d_touched, x.dup_of_pos, h->d_dup_corr, pack_arg
#define DECODE_ARGS h->hp, DECODE_TAIL
#define DECODE_LA(NI_, L_, A_)                                                                                       \
  do {                                                                                                               \
    if (pad) hipLaunchKernelGGL((decode_rows_kernel<NI_, L_, A_, true>), grid_rows, blk, 0, st, DECODE_ARGS);        \
    else hipLaunchKernelGGL((decode_rows_kernel<NI_, L_, A_, false>), grid_rows, blk, 0, st, DECODE_ARGS);           \
  } while (0)
#define DECODE_NI(NI_)                                          \
  do {                                                          \
    if (ce && ada) DECODE_LA(NI_, 5, true);                     \
    else if (ce) DECODE_LA(NI_, 5, false);                      \
    else if (ada) DECODE_LA(NI_, 0, true);                      \
    else DECODE_LA(NI_, 0, false);                              \
  } while (0)
  // K <= 256: hot rows one per wavefront, all others four per wavefront (NV float4 pieces + NT tail scalars per lane)
#define DECODE_HY(NV_, NT_)                                                                                           \
  do {                                                                                                                \
    if (fused) {                                                                                                       \
      if (ce && ada) hipLaunchKernelGGL((decode_gather_kernel<NV_, NT_, 5, true>), grid_fu, blk, 0, st, h->hp, hot, geo, late, *fused, DECODE_TAIL);   \
      else if (ce) hipLaunchKernelGGL((decode_gather_kernel<NV_, NT_, 5, false>), grid_fu, blk, 0, st, h->hp, hot, geo, late, *fused, DECODE_TAIL);    \
      else if (ada) hipLaunchKernelGGL((decode_gather_kernel<NV_, NT_, 0, true>), grid_fu, blk, 0, st, h->hp, hot, geo, late, *fused, DECODE_TAIL);    \
      else hipLaunchKernelGGL((decode_gather_kernel<NV_, NT_, 0, false>), grid_fu, blk, 0, st, h->hp, hot, geo, late, *fused, DECODE_TAIL);            \
    }                                                                                                                  \
    else if (ce && ada) hipLaunchKernelGGL((decode_hybrid_kernel<NV_, NT_, 5, true>), grid_hy, blk, 0, st, h->hp, hot, late, DECODE_TAIL);   \
    else if (ce) hipLaunchKernelGGL((decode_hybrid_kernel<NV_, NT_, 5, false>), grid_hy, blk, 0, st, h->hp, hot, late, DECODE_TAIL);    \
    else if (ada) hipLaunchKernelGGL((decode_hybrid_kernel<NV_, NT_, 0, true>), grid_hy, blk, 0, st, h->hp, hot, late, DECODE_TAIL);    \
    else hipLaunchKernelGGL((decode_hybrid_kernel<NV_, NT_, 0, false>), grid_hy, blk, 0, st, h->hp, hot, late, DECODE_TAIL);            \
  } while (0)
#define DECODE_HY_NT(NV_)                                                                        \
  do {                                                                                           \
    if (nt == 1) DECODE_HY(NV_, 1); else if (nt == 2) DECODE_HY(NV_, 2); else DECODE_HY(NV_, 4); \
  } while (0)
  {
    const bool ce = h->cfg.loss_type == CDAE_LOSS_CROSS_ENTROPY, ada = h->cfg.using_adagrad != 0, pad = h->K < h->Kp;
    const uint32_t K = h->K;
    const RowRecord* const pack_arg = K <= 256 ? pack : nullptr;        // (decode_rows_kernel has no four-row role)
    if (K <= 256) {
      const uint32_t hot = decode_hot_rows(h);
      const uint32_t waves = hot + (I - hot + 3) / 4;
      const dim3 grid_hy((waves + 3) / 4);
      const DecodeLate late = h->decode_late();
      // fused launch (decode_gather_kernel): [popular rows] [the other rows] [gather]
      if (fused && !h->fused_geo_set) CHK(fused_geometry(h, hot, I, pack != nullptr));
      const FusedGeom geo = h->fused_geo;
      const dim3 grid_fu(geo.decode_wgs + (fused ? 8u * ((fused->n_units + 3u) / 4u) : 0u));
      const uint32_t nv = K / 64, tail = K % 64;
      const uint32_t nt = tail == 0 ? 0u : (tail < 16 ? 1u : (tail < 32 ? 2u : 4u));   // 16 nt > tail: room for b'
      if (nt == 0) {
        switch (nv) { case 1: DECODE_HY(1, 0); break; case 2: DECODE_HY(2, 0); break; case 3: DECODE_HY(3, 0); break; default: DECODE_HY(4, 0); break; }
      } else {
        switch (nv) { case 0: DECODE_HY_NT(0); break; case 1: DECODE_HY_NT(1); break; case 2: DECODE_HY_NT(2); break; default: DECODE_HY_NT(3); break; }
      }
    } else {
      switch (h->NI) { case 1: DECODE_NI(1); break; case 2: DECODE_NI(2); break; case 4: DECODE_NI(4); break; default: DECODE_NI(8); break; }
    }
  }
#undef DECODE_HY_NT
#undef DECODE_HY
#undef DECODE_LA
#undef DECODE_NI
#undef DECODE_ARGS
#undef DECODE_TAIL
  HIPCHK(hipGetLastError());
  return 0;
}

// Tail of the sampled step, shared by the single handle (compute_batch) and the item shard (fs_phase2): delta from hg, the Wu / Uu
// steps, then the input rows with the strictly sequential hidden-bias recurrence as leading workgroups (both need only delta).
// hg = HG + `parts` slabs of HGpart over the unit prefix uptr (an item shard: parts 0, d_HG already holds the all-reduced hg);
// uu_b: the batch's gathered Uu rows (item shard); pr: the caller's open F_HIDDEN span, or nullptr (no profiling of the tail).
int sampled_tail(cdae_hip* h, cdae_hip::ExBuf& x, uint64_t s0, uint32_t nb, const uint32_t* uptr, uint32_t n_units, uint32_t parts,
                 const float* uu_b, const cdae::LateFinish& late, Prof* pr) {
  using namespace cdae;
  hipStream_t st = h->stream;
  const uint32_t I = (uint32_t)h->I;
  const dim3 blk(256);
  DISPATCH_NI(h->NI, hidden_finish_kernel, dim3(nb), blk, 0, st, h->hp, uptr, n_units, s0, nb, h->d_HGpart, h->d_Dz, h->d_HG,
              h->d_Wu, h->d_Wu_ag, parts, h->d_Uu, h->d_Uu_ag, h->d_Ssum, h->d_delta_rows, uu_b, late);
  if (pr) { CHK(pr->end()); CHK(pr->begin(h, F_INPUT, st)); }
  const uint32_t bias_blocks = (h->Kp + 255u) / 256u;
  DISPATCH_NI(h->NI, input_rows_kernel, dim3(bias_blocks + (I + 3) / 4), blk, 0, st, h->hp, h->d_item_order, x.seg + 2 * (size_t)I, x.seg + 3 * (size_t)I,
              x.sorted_val, h->d_Z, h->d_HG, h->d_G, h->P(CDAE_P_W), h->P(CDAE_P_W_AG), CDAE_TOUCHED_ARG, nb, h->P(CDAE_P_B),
              h->P(CDAE_P_B_AG), h->delta_rows());
  if (pr) CHK(pr->end());
  HIPCHK(hipEventRecord(x.released, st));
  HIPCHK(hipGetLastError());
  return 0;
}

// K2..K5 on the main stream from example-buffer set `b`.
// explicit_in != nullptr: single user whose example list (already sorted into set b) and input set come from the caller
int compute_batch(cdae_hip* h, int b, const Batch& bt, uint64_t seed, uint32_t epoch,
                  const uint32_t* explicit_in = nullptr, uint32_t n_explicit = 0) {
  using namespace cdae;
  cdae_hip::ExBuf& x = h->ex[b];
  hipStream_t st = h->stream;
  const uint32_t I = (uint32_t)h->I, nb = bt.nb;
  const uint64_t s0 = bt.s0;
  const dim3 blk(256);
  const dim3 grid_users((nb + 3) / 4), grid_rows((I + 3) / 4);
  Prof pr;

  h->hp.trace_odd = (uint32_t)(h->seq & 1);
  CHK(pr.begin(h, F_ENCODE, st));
  // explicit mode: one user, one unit (the caller's lists need not follow the num_neg proportion)
  const uint32_t n_units = explicit_in ? 1u : units_of(h, bt);
  const uint32_t* uptr = explicit_in ? h->d_uptr_tmp : h->d_unit_ptr + s0;
  const dim3 grid_units((n_units + 3) / 4);
  // The fused launch (decode + gather, decode_gather_kernel): plain batches of a handle that has late rows.  The batch's encode then
  // fills G with G_PENDING (the gather wavefronts wait on it), whichever encode form runs.
  const bool fused = h->fused_decode && !explicit_in && n_units > 0u && bt.E > 0u && bt.E < (1ull << 32);
  float* const ghot = h->late_rows ? h->d_Ghot.p : nullptr;
  uint32_t* const gfill = fused ? reinterpret_cast<uint32_t*>(h->d_G.p) : nullptr;
  const uint32_t n_fill = fused ? (uint32_t)bt.E : 0u;
  if (!explicit_in && !h->encode_two_launches && nb <= ENCODE_USERS_MAX) {
    // one launch: a workgroup per user (encode_users_kernel)
    DISPATCH_NI(h->NI, encode_users_kernel, dim3(nb), dim3(ENC_WAVES * WAVE), 0, st, h->hp, h->d_row_ptr, h->d_col, h->P(CDAE_P_W), uptr, s0, nb,
                bt.cidx, seed, epoch, h->d_Wu, h->P(CDAE_P_B), h->d_Z, h->d_Dz, h->d_HG, h->d_Uu, h->d_Ssum,
                (BF16_T*)nullptr, (BF16_T*)nullptr, 0u, (float*)nullptr, (const float*)nullptr, (const float*)nullptr, (const uint32_t*)nullptr,
                ghot, h->d_hotdup, gfill, n_fill);
  } else {
    DISPATCH_NI(h->NI, encode_partial_kernel, grid_units, blk, 0, st, h->hp, h->d_row_ptr, h->d_col, h->P(CDAE_P_W), uptr, n_units,
                (const uint32_t*)nullptr, s0, nb, 1, CDAE_STREAM_CORRUPT, bt.cidx, seed, epoch, h->d_Hpart, explicit_in, n_explicit,
                explicit_in ? (const uint32_t*)nullptr : (const uint32_t*)h->d_unit_user);
    DISPATCH_NI(h->NI, encode_finish_kernel, grid_users, blk, 0, st, h->hp, h->d_Hpart, uptr, h->d_Wu, h->P(CDAE_P_B),
                (const uint32_t*)nullptr, s0, nb, 1, h->d_Z, h->d_Dz, h->d_HG, h->d_Uu, h->d_Ssum,
                (BF16_T*)nullptr, (BF16_T*)nullptr, 0u, ghot, h->d_hotdup, gfill, n_fill);
  }
  CHK(pr.end());

  if (!h->skip_ready_wait) HIPCHK(hipStreamWaitEvent(st, x.ready, 0));
  const GatherArgs ga{h->d_row_ptr, uptr, n_units, s0, nb, x.item, h->d_G, h->d_D0, h->d_HGpart, explicit_in ? (uint32_t)bt.E : 0u, x.dup_of_ex,
                      h->d_dup_corr, explicit_in ? (const uint32_t*)nullptr : (const uint32_t*)h->d_unit_user,
                      h->late_rows ? (const uint32_t*)h->d_late_bits : (const uint32_t*)nullptr, h->late_words, h->d_fused_err};
  CHK(pr.begin(h, F_DECODE, st));
  CHK(launch_decode(h, x, fused ? &ga : nullptr, explicit_in ? nullptr : pack_of(h, x, bt.E)));
  CHK(pr.end());

  CHK(pr.begin(h, F_HIDDEN, st));
  if (!fused)
    DISPATCH_NI(h->NI, hidden_gather_kernel, dim3(8 * ((n_units + 3) / 4)), blk, 0, st, h->hp, ga.row_ptr, uptr, n_units, s0, nb,
                x.item, h->d_G, h->d_D0, h->d_HGpart, ga.explicit_examples, x.dup_of_ex, h->d_dup_corr, ga.unit_user,
                ga.late_bits, ga.late_words);
  return sampled_tail(h, x, s0, nb, uptr, n_units, 8u, nullptr, h->late_finish(), &pr);
}

// LDS-staged NT GEMM: the 256 x 128 three-stage kernel where the rows allow it (M % 256 == 0), else the 128 x 128 one.
template <int EPI>
int launch_gemm_lds(cdae_hip* h, hipStream_t st, const __bf16* A, const __bf16* Bm, uint32_t M, uint32_t N, uint32_t Kd, uint32_t lda,
                    uint32_t ldb, uint32_t kps, const cdae::GemmEpilogue& ep, uint32_t splits, uint32_t mode) {
  using namespace cdae;
  const uint32_t Nt = (N + 127) / 128;
  if (M % 256 == 0 && N % 256 == 0 && !h->gemm_narrow) {
    // 256 x 256 tiles (round 3): 128 flop per byte staged into LDS instead of 85
    if (!h->gemmw_attr_set[EPI]) {
      HIPCHK(hipFuncSetAttribute((const void*)gemm_nt_bf16_ldsw_kernel<EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gemmw_lds_bytes()));
      h->gemmw_attr_set[EPI] = true;
    }
    const GemmGrid gg{M / 256, N / 256, splits, mode};
    hipLaunchKernelGGL((gemm_nt_bf16_ldsw_kernel<EPI>), dim3(gg.workgroups()), dim3(512), gemmw_lds_bytes(), st, A, Bm, M, N, Kd, lda, ldb,
                       kps, ep, gg);
    return 0;
  }
  if (M % 256 == 0) {
    if (!h->gemm3_attr_set[EPI]) {     // per handle: the attribute belongs to the (function, device) pair
      HIPCHK(hipFuncSetAttribute((const void*)gemm_nt_bf16_lds3_kernel<EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gemm3s_lds_bytes()));
      h->gemm3_attr_set[EPI] = true;
    }
    const GemmGrid gg{M / 256, Nt, splits, mode};
    hipLaunchKernelGGL((gemm_nt_bf16_lds3_kernel<EPI>), dim3(gg.workgroups()), dim3(512), gemm3s_lds_bytes(), st, A, Bm, M, N, Kd, lda, ldb,
                       kps, ep, gg);
  } else {
    const GemmGrid gg{M / 128, Nt, splits, mode};
    hipLaunchKernelGGL((gemm_nt_bf16_lds_kernel<EPI>), dim3(gg.workgroups() + (EPI == EPI_STORE ? ep.bias_blocks : 0u)), dim3(256), 0, st, A, Bm, M, N,
                       Kd, lda, ldb, kps, ep, gg);
  }
  return 0;
}

// contraction split of GEMM 2 (hg = G D, K > 256 / unfused path): about 2048 workgroups in all, splits a multiple of 64 items
uint32_t gemm2_k_per_split(const cdae_hip* h) {
  const uint32_t tiles2 = ((h->Kp + 127) / 128) * (h->Bp / 128);
  const uint32_t want = std::max<uint32_t>(1, std::min<uint32_t>(h->Ip / 64, (2048 + tiles2 - 1) / tiles2));
  return (((h->Ip + want - 1) / want + 63) / 64) * 64;
}

// GEMM 2 of the K > 256 path from G^T and the row-major decoder image (gemm_tn_bf16_kernel): then GEMM 1 writes no G and nothing reads D^T
bool gemm2_tn_path(const cdae_hip* h) {
  // (rows and columns of GEMM 1 in multiples of 256: it is then the 256 x 256-tile kernel, whose loss epilogue knows how to leave G out)
  return h->Kp > 256 && h->Kp % 256 == 0 && h->Bp % 256 == 0 && h->Ip % 256 == 0 && !h->gemm_narrow && !h->gemm2_nt;
}
// GEMM 3 + row step in one launch (gemm3_rows_fused_kernel): Kp = 512 over item spaces >= 32768, i.e. BASELINE configs[4]'s path
bool rows_fused_path(const cdae_hip* h) {
  return h->Kp == 512 && h->I >= 32768 && h->Ip % cdae::FR_ITEMS == 0 && !h->rows_separate;
}
int launch_rows_fused(cdae_hip* h, hipStream_t st, const cdae_hip::ExBuf& x, uint32_t nb, __bf16* Db) {
  using namespace cdae;
  const uint32_t I = (uint32_t)h->I;
#define FR_LAUNCH(ADA_, KH_)                                                                                                              \
  do {                                                                                                                                    \
    if (!h->fused_rows_attr_set[ADA_][KH_ - 1]) {                                                                                         \
      HIPCHK(hipFuncSetAttribute((const void*)gemm3_rows_fused_kernel<ADA_, KH_>, hipFuncAttributeMaxDynamicSharedMemorySize,             \
                                 (int)fused_rows_lds_bytes<KH_>()));                                                                      \
      h->fused_rows_attr_set[ADA_][KH_ - 1] = true;                                                                                       \
    }                                                                                                                                     \
    const uint32_t tiles = h->Ip / FR_ITEMS, grid = KH_ == 1 ? tiles : 16u * ((tiles + 7u) / 8u);                                         \
    hipLaunchKernelGGL((gemm3_rows_fused_kernel<ADA_, KH_>), dim3(grid), dim3(256 / KH_), fused_rows_lds_bytes<KH_>(), st, h->hp,         \
                       (const __bf16*)h->d_ZTb, (const __bf16*)h->d_GTb, h->Bp, h->Bp, nb, (const uint8_t*)h->d_has_in,                   \
                       h->d_dD, h->dec(), h->dec_ag(),                                                                                    \
                       h->P(CDAE_P_BP), h->P(CDAE_P_BP_AG), h->d_touched, Db, h->Ip);                                                     \
  } while (0)
  if (h->cfg.using_adagrad) { if (h->rows_fused_kh == 1) FR_LAUNCH(true, 1); else FR_LAUNCH(true, 2); }
  else { if (h->rows_fused_kh == 1) FR_LAUNCH(false, 1); else FR_LAUNCH(false, 2); }
#undef FR_LAUNCH
  // the rows kept as inputs (tied weights: one step with dD + the summed input gradient)
  DISPATCH_NI(h->NI, full_rows_inputs_kernel, dim3((I + 255) / 256), dim3(256), 0, st, h->hp, h->d_has_in, (const uint32_t*)x.seg, (const uint32_t*)(x.seg + I),
              (const uint64_t*)x.sorted_val, (const float*)h->delta_rows(), (const float*)h->d_dD, h->P(CDAE_P_W), h->P(CDAE_P_W_AG), Db, (__bf16*)nullptr, h->Ip);
  return 0;
}

// The unfused (K > 256, or CDAE_FULL_UNFUSED) forward product with its loss epilogue, the positive fix-up and the hidden-gradient
// product of one block — shared by the single-handle step (compute_batch_full) and the item shard's phase 1 (fs_phase1: the same
// launches over the shard's own item rows).  *parts / *rows: the slabs of HGpart holding the partial hg and their row count.
int full_products_k512(cdae_hip* h, hipStream_t st, cdae_hip::ExBuf& x, const Batch& bt, uint32_t nb, uint32_t* parts, uint32_t* rows) {
  using namespace cdae;
  const uint32_t I = (uint32_t)h->I, Kp = h->Kp, Bp = h->Bp, Ip = h->Ip;
  const dim3 blk(256);
  const bool tn2 = gemm2_tn_path(h);                                      // GEMM 2 reads G^T and D: no G, no D^T
  GemmEpilogue ep{};
  ep.bp = h->P(CDAE_P_BP); ep.G = tn2 ? (__bf16*)nullptr : h->d_Gb; ep.ldg = Ip; ep.GT = h->d_GTb; ep.ldgt = Bp;
  ep.rows_live = nb; ep.cols_live = I; ep.loss_type = h->cfg.loss_type;
  // GEMM 1: Y = Z D^T (+ b'), g = loss'(y, 0) -> G [Bp x Ip] (unless GEMM 2 reads G^T), G^T [Ip x Bp]
  if (tn2 && Kp == 512 && !h->gemm1_tiled) {
    // the z rows of 256 users in registers, only D staged, the two wavefronts of a SIMD in opposite phases — one contracts while the
    // other runs its loss epilogue (gemm1_loss_duo_kernel): G^T alone, which is all GEMM 2 (TN) and GEMM 3 read
    const uint32_t user_tiles = Bp / 256, n_tiles = Ip / 128;
    const uint32_t item_groups = std::min<uint32_t>(((std::max<uint32_t>(1u, 256u / user_tiles) + 7u) / 8u) * 8u, ((n_tiles + 7u) / 8u) * 8u);
    const uint32_t tiles_per_group = (n_tiles + item_groups - 1) / item_groups;
    const dim3 grid(8u * user_tiles * ((item_groups + 7u) / 8u));
    const bool ce = h->cfg.loss_type == CDAE_LOSS_CROSS_ENTROPY;
    if (!h->gemm1_duo_attr_set[ce]) {
      if (ce) HIPCHK(hipFuncSetAttribute((const void*)gemm1_loss_duo_kernel<5>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gemm1_duo_lds_bytes()));
      else HIPCHK(hipFuncSetAttribute((const void*)gemm1_loss_duo_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gemm1_duo_lds_bytes()));
      h->gemm1_duo_attr_set[ce] = true;
    }
    if (ce)
      hipLaunchKernelGGL(gemm1_loss_duo_kernel<5>, grid, dim3(512), gemm1_duo_lds_bytes(), st, (const __bf16*)h->d_Zb, (const __bf16*)h->d_Db,
                         (const float*)h->P(CDAE_P_BP), h->d_GTb, Bp, nb, I, Ip, user_tiles, item_groups, tiles_per_group);
    else
      hipLaunchKernelGGL(gemm1_loss_duo_kernel<0>, grid, dim3(512), gemm1_duo_lds_bytes(), st, (const __bf16*)h->d_Zb, (const __bf16*)h->d_Db,
                         (const float*)h->P(CDAE_P_BP), h->d_GTb, Bp, nb, I, Ip, user_tiles, item_groups, tiles_per_group);
  } else
    CHK(launch_gemm_lds<EPI_LOSS>(h, st, h->d_Zb, h->d_Db, Bp, Ip, Kp, Kp, Kp, Kp, ep, 1, 0));
  HIPCHK(hipStreamWaitEvent(st, x.ready, 0));
  if (bt.E)
    hipLaunchKernelGGL(full_positive_fixup_kernel, dim3((uint32_t)((bt.E + 15) / 16)), blk, 0, st, x.item, x.val, (uint32_t)bt.E,
                       (uint32_t)h->cfg.loss_type, (const float*)h->d_Z, (const float*)h->dec(), Kp, (const float*)h->P(CDAE_P_BP),
                       tn2 ? (__bf16*)nullptr : h->d_Gb, Ip, h->d_GTb, Bp, rows_fused_path(h) ? h->d_has_in : (uint8_t*)nullptr);
  // GEMM 2: hg = G D  (contraction over items, split).  Every split stores its partial [Bp x Kp] product into its own slab of
  // HGpart and the consumer adds the slabs in fixed order: deterministic (the first version accumulated with fp32 atomics into
  // HG, whose order — and therefore rounding — changed from run to run)
  const uint32_t kps = gemm2_k_per_split(h);
  GemmEpilogue e2{};
  const uint32_t splits = (Ip + kps - 1) / kps;
  e2.Cout = h->d_HGpart; e2.ldc = Kp; e2.split_stride = (size_t)Bp * Kp;
  if (tn2) {                                                     // sum over items of G^T[item][user] D[item][k]: both images as they are
    const GemmGrid gg{Bp / 256, Kp / 256, splits, 2};
    if (!h->gemm_tn_attr_set) {
      HIPCHK(hipFuncSetAttribute((const void*)gemm_tn_bf16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gemm_tn_lds_bytes()));
      h->gemm_tn_attr_set = true;
    }
    hipLaunchKernelGGL(gemm_tn_bf16_kernel, dim3(gg.workgroups()), dim3(512), gemm_tn_lds_bytes(), st,
                       (const __bf16*)h->d_GTb, (const __bf16*)h->d_Db, Bp, Kp, Ip, Bp, Kp, kps, e2, gg);
  } else {
    CHK(launch_gemm_lds<EPI_STORE>(h, st, h->d_Gb, h->d_DTb, Bp, Kp, Ip, Ip, Ip, kps, e2, splits, 2));
  }
  *parts = splits; *rows = Bp;
  return 0;
}

// The fused full-output decode (K <= 256; cdae_full_kernels.hpp full_decode_fused_kernel): forward product, loss' against the targets of
// example-buffer set b — one bit per (batch user, item), built by prep_batch — and the hidden gradient in one launch, which leaves hg
// as h->full_slices slabs of HGpart.  Shared by the single handle and the item shard (its own item rows); the caller has waited for
// the set's `ready` event.
int launch_full_fused(cdae_hip* h, hipStream_t st, int b, uint32_t nb) {
  using namespace cdae;
  const uint32_t I = (uint32_t)h->I, Kp = h->Kp, Bp = h->Bp, Ip = h->Ip;
  const uint32_t words = (I + 31) / 32, slices = h->full_slices, tiles = Ip / (32 * FUSED_SUB);   // staged steps of 64 items
  const uint32_t* bits = h->d_bits_train + (size_t)b * h->bits_stride;
  const uint32_t tps = (tiles + slices - 1) / slices;
  const dim3 grid(slices, Bp / 128), blk(256);
  const size_t lds = full_fused_lds_bytes(Kp);
  if ((uint64_t)Ip * Bp > 0xFFFFFFFFull) return fail("full-output decode: G^T of %u x %u exceeds 2^32 elements; lower batch_users", Ip, Bp);
#define FUSED_LAUNCH2(NKS_, L_)                                                                                                         \
  do {                                                                                                                                  \
    if (!h->fused_attr_set) {      /* per handle (the attribute belongs to the (function, device) pair): a runtime call per batch otherwise */ \
      HIPCHK(hipFuncSetAttribute((const void*)full_decode_fused_kernel<NKS_, L_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
      h->fused_attr_set = true;                                                                                                          \
    }                                                                                                                                     \
    hipLaunchKernelGGL((full_decode_fused_kernel<NKS_, L_>), grid, blk, lds, st, h->hp, h->d_Zb, h->d_Db, h->d_DTb, Ip, h->P(CDAE_P_BP), \
                       bits, words, nb, tps, h->d_GTb, Bp, h->d_HGpart);                                                     \
  } while (0)
#define FUSED_LAUNCH(NKS_)                                                                       \
  do {                                                                                           \
    if (h->cfg.loss_type == CDAE_LOSS_CROSS_ENTROPY) FUSED_LAUNCH2(NKS_, 5); else FUSED_LAUNCH2(NKS_, 0); \
  } while (0)
  switch (Kp) { case 64: FUSED_LAUNCH(4); break; case 128: FUSED_LAUNCH(8); break; default: FUSED_LAUNCH(16); break; }
#undef FUSED_LAUNCH2
#undef FUSED_LAUNCH
  return 0;
}

// Two-stream tail of the full-output step, shared by the single handle (compute_batch_full) and the item shard (fs_phase2).  The aux
// stream takes what needs hg only — delta_u, the Wu / Uu steps, then the strictly sequential hidden-bias recurrence (2048 users x
// 58 ns) — beside GEMM 3 on the main stream; the row steps wait for delta, and the recurrence is joined by its next consumer (join_aux).
// (Round 4 measured GEMM 2 on the aux stream too, BESIDE the fused row launch of the K = 512 path, which needs G^T and Z^T only — two
// bf16 images of the decoder, swapped per block: 5.0 ms per 1024-user block against 4.75 in order.  The two launches stretch each
// other — GEMM 2 + hidden layer 1.2 -> 3.7 ms, row launch 2.3 -> 3.8 — because GEMM 2's LDS fill and the row launch's streams share
// the L2s and the fabric, and a CU holds one or the other, not both (139 KiB / 2 x 72 KiB of LDS).  Removed.)
struct FullTail {
  uint32_t hg_parts, hg_rows;   // hg = HG + hg_parts slabs of HGpart, hg_rows rows each (an item shard: 0 slabs, d_HG holds the all-reduced hg)
  const float* uu_b;            // item shard: the batch's gathered Uu rows, else nullptr
  bool write_images;            // full_rows_kernel / full_rows_wave_kernel leave the bf16 images of the rows they step (the fused row step always does)
  uint64_t prof_q;              // batch sequence number the profiling spans are sampled by
  Prof* decode_span;            // the caller's open F_DECODE span, ended behind GEMM 3, or nullptr
};
int full_tail(cdae_hip* h, cdae_hip::ExBuf& x, uint64_t s0, uint32_t nb, const FullTail& a) {
  using namespace cdae;
  hipStream_t st = h->stream;
  const uint32_t I = (uint32_t)h->I, Kp = h->Kp, Bp = h->Bp, Ip = h->Ip;
  const dim3 blk(256);
  const bool rows_fused = rows_fused_path(h);                             // GEMM 3 + row step in one launch (Kp = 512, >= 32768 items)
  __bf16* const img = a.write_images ? h->d_Db.p : nullptr;
  Prof pr;
  HIPCHK(hipEventRecord(h->ev_fork, st));
  HIPCHK(hipStreamWaitEvent(h->aux, h->ev_fork, 0));
  CHK(pr.begin(h, F_HIDDEN, h->aux, a.prof_q));
  DISPATCH_NI(h->NI, hidden_finish_kernel, dim3(nb), blk, 0, h->aux, h->hp, (const uint32_t*)h->d_iota, a.hg_rows, s0, nb, h->d_HGpart,
              h->d_Dz, h->d_HG, h->d_Wu, h->d_Wu_ag, a.hg_parts, h->d_Uu, h->d_Uu_ag, h->d_Ssum, h->d_delta_rows, a.uu_b);
  CHK(pr.end());
  HIPCHK(hipEventRecord(h->ev_delta, h->aux));
  hipLaunchKernelGGL(hidden_bias_kernel, dim3((Kp + 255u) / 256u), blk, 0, h->aux, h->hp, nb, h->d_HG, h->P(CDAE_P_B), h->P(CDAE_P_B_AG));
  HIPCHK(hipEventRecord(h->ev_join, h->aux));
  if (!rows_fused) {      // GEMM 3: dD = G^T Z, contraction over the batch's users (rows_fused: the product stays in the accumulators of the row-step launch)
    GemmEpilogue e3{};
    e3.Cout = h->d_dD; e3.ldc = Kp;
    CHK(launch_gemm_lds<EPI_STORE>(h, st, h->d_GTb, h->d_ZTb, Ip, Kp, Bp, Bp, Bp, Bp, e3, 1, 1));
  }
  if (a.decode_span) CHK(a.decode_span->end());

  HIPCHK(hipStreamWaitEvent(st, h->ev_delta, 0));
  CHK(pr.begin(h, F_INPUT, st, a.prof_q));
  if (rows_fused)      // dD = G^T Z and the row steps from its accumulators, the row-major bf16 image left current
    CHK(launch_rows_fused(h, st, x, nb, h->d_Db));
  else if (I >= 32768u)     // rows are plentiful and mostly without kept inputs: one wavefront per row (the row-major image only)
    DISPATCH_NI(h->NI, full_rows_wave_kernel, dim3((I + 3) / 4), blk, 0, st, h->hp, x.seg, x.seg + I, x.sorted_val, h->delta_rows(),
                h->d_dD, h->d_GTb, Bp, nb, h->P(CDAE_P_W), h->P(CDAE_P_W_AG), h->P(CDAE_P_V), h->P(CDAE_P_V_AG), h->P(CDAE_P_BP),
                h->P(CDAE_P_BP_AG), h->d_touched, img);
  else
    DISPATCH_NI(h->NI, full_rows_kernel, dim3(I), blk, 0, st, h->hp, x.seg, x.seg + I, x.sorted_val, h->delta_rows(),
                h->d_dD, h->d_GTb, Bp, nb, h->P(CDAE_P_W), h->P(CDAE_P_W_AG), h->P(CDAE_P_V), h->P(CDAE_P_V_AG), h->P(CDAE_P_BP),
                h->P(CDAE_P_BP_AG), (float*)nullptr, (float*)nullptr, h->d_touched,
                img, a.write_images ? h->d_DTb : (__bf16*)nullptr, a.write_images ? Ip : 0u);
  CHK(pr.end());
  // which bf16 images of the decoder the row step left current: both (full_rows_kernel), or the row-major one
  h->db_valid = a.write_images && I < 32768u;
  h->db_rows_valid = rows_fused || (a.write_images && I >= 32768u);
  h->join_pending = true;                                      // the aux stream (b recurrence) is joined by its next consumer: join_aux
  HIPCHK(hipEventRecord(x.released, st));
  HIPCHK(hipGetLastError());
  return 0;
}

// Full-output decode of one batch (MFMA path, cdae_full_kernels.hpp).  The example list holds the positives only.
int compute_batch_full(cdae_hip* h, int b, const Batch& bt, uint64_t seed, uint32_t epoch) {
  using namespace cdae;
  cdae_hip::ExBuf& x = h->ex[b];
  hipStream_t st = h->stream;
  const uint32_t I = (uint32_t)h->I, nb = bt.nb, Kp = h->Kp, Bp = h->Bp, Ip = h->Ip;
  const uint64_t s0 = bt.s0;
  const dim3 blk(256);
  const dim3 grid_users((nb + 3) / 4);
  const uint32_t n_units = units_of(h, bt);
  const uint32_t* uptr = h->d_unit_ptr + s0;
  Prof pr;

  CHK(pr.begin(h, F_ENCODE, st));
  const bool two_launches = h->encode_two_launches || nb > ENCODE_USERS_MAX;
  if (two_launches) {
    DISPATCH_NI(h->NI, encode_partial_kernel, dim3((n_units + 3) / 4), blk, 0, st, h->hp, h->d_row_ptr, h->d_col, h->P(CDAE_P_W), uptr,
                n_units, (const uint32_t*)nullptr, s0, nb, 1, CDAE_STREAM_CORRUPT, bt.cidx, seed, epoch, h->d_Hpart,
                (const uint32_t*)nullptr, 0u, (const uint32_t*)h->d_unit_user);
  }
  // bf16 copies D, D^T (rows >= I zero) of this batch: like the input gather they need the previous batch's row steps but not
  // its b recurrence, which may still be running on the aux stream — joined behind them, in front of its first consumer.
  // Small item spaces: converted together with Z behind the encode instead (one launch less; a launch is ~9 us there)
  // Round 3: for item spaces below 32768 the row step (full_rows_kernel) leaves the bf16 images of the decoder behind and the
  // encode writes those of z: no conversion launch in the steady state.  D is converted here only when something else wrote the
  // parameters (init, set_param, an exchange), Z only when the batch is shorter than the rows the images may hold.
  const bool rows_fused = rows_fused_path(h);                             // GEMM 3 + row step in one launch (Kp = 512, >= 32768 items)
  const bool rows_write_images = I < 32768u;
  const bool rows_write_db = !rows_write_images;                          // full_rows_wave_kernel: the row-major image only
  const bool need_d = !(rows_write_images && h->db_valid) && !(rows_write_db && h->db_rows_valid);
  const bool tn2 = gemm2_tn_path(h);                                      // GEMM 2 reads G^T and D: no G, no D^T
  if (rows_write_db && h->db_rows_valid && !tn2)                          // D^T from the bf16 rows the row step left (2 GB instead of 4 at 1 M x 512)
    hipLaunchKernelGGL(bf16_transpose_kernel, dim3(Kp / 64, Ip / 64), blk, 0, st, (const __bf16*)h->d_Db, I, Kp, Ip, h->d_DTb);
  const bool z_in_encode = h->zb_rows == nb;
  const bool pair_copy = Ip <= 65536 && need_d && !z_in_encode;
  if (need_d && !pair_copy) hipLaunchKernelGGL(to_bf16_transpose_kernel, dim3(Kp / 64, Ip / 64), blk, 0, st, h->dec(), I, Kp, Kp, Ip, h->d_Db, h->d_DTb);
  CHK(join_aux(h));
  __bf16* zb = z_in_encode ? h->d_Zb.p : nullptr;
  __bf16* ztb = z_in_encode ? h->d_ZTb.p : nullptr;
  if (two_launches) {
    DISPATCH_NI(h->NI, encode_finish_kernel, grid_users, blk, 0, st, h->hp, h->d_Hpart, uptr, h->d_Wu, h->P(CDAE_P_B),
                (const uint32_t*)nullptr, s0, nb, 1, h->d_Z, h->d_Dz, h->d_HG, h->d_Uu, h->d_Ssum, zb, ztb, Bp);
  } else {                       // one launch: a workgroup per user (encode_users_kernel)
    DISPATCH_NI(h->NI, encode_users_kernel, dim3(nb), dim3(ENC_WAVES * WAVE), 0, st, h->hp, h->d_row_ptr, h->d_col, h->P(CDAE_P_W), uptr, s0, nb,
                bt.cidx, seed, epoch, h->d_Wu, h->P(CDAE_P_B), h->d_Z, h->d_Dz, h->d_HG, h->d_Uu, h->d_Ssum, zb, ztb, Bp);
  }
  CHK(pr.end());

  CHK(pr.begin(h, F_DECODE, st));
  // bf16 operand copies Z, Z^T (rows >= nb zero) where the encode did not write them
  if (pair_copy)
    hipLaunchKernelGGL(to_bf16_transpose_pair_kernel, dim3(Kp / 64, Ip / 64 + Bp / 64), blk, 0, st, (const float*)h->dec(), I, Ip, h->d_Db, h->d_DTb,
                       (const float*)h->d_Z, nb, Bp, h->d_Zb, h->d_ZTb, Kp, Kp);
  else if (!z_in_encode)
    hipLaunchKernelGGL(to_bf16_transpose_kernel, dim3(Kp / 64, Bp / 64), blk, 0, st, h->d_Z, nb, Kp, Kp, Bp, h->d_Zb, h->d_ZTb);
  h->zb_rows = nb;
  const bool fused = Kp <= 256 && !h->full_unfused;
  uint32_t hg_parts = 0, hg_rows = nb;           // slabs of HGpart holding hg and their row count
  if (fused) {
    HIPCHK(hipStreamWaitEvent(st, x.ready, 0));
    CHK(launch_full_fused(h, st, b, nb));
    hg_parts = h->full_slices;
  } else {
    CHK(full_products_k512(h, st, x, bt, nb, &hg_parts, &hg_rows));
  }
  // Small item spaces, short blocks (round 4): everything on ONE stream, the b recurrence as the leading workgroups of the row launch
  // (full_rows_kernel's bias role).  A hand-off between two streams through an event costs ~15 us on this part against 2.7 us for
  // a launch boundary (tools/grid_barrier_cost.hip), and at <= one_stream_max users per block the recurrence (41 ns per user) is
  // shorter than the two hand-offs that would put it beside the row step.
  const bool one_stream = !rows_fused && I < 32768u && nb <= h->full_one_stream_max && !h->cfg.linear_function;   // (the gate's rows receive Uu (.) delta, b the plain delta)
  if (one_stream) {
    Prof pa;
    CHK(pa.begin(h, F_HIDDEN, st));
    DISPATCH_NI(h->NI, hidden_finish_kernel, dim3(nb), blk, 0, st, h->hp, (const uint32_t*)h->d_iota, hg_rows, s0, nb, h->d_HGpart, h->d_Dz,
                h->d_HG, h->d_Wu, h->d_Wu_ag, hg_parts, h->d_Uu, h->d_Uu_ag, h->d_Ssum, h->d_delta_rows);
    CHK(pa.end());
    GemmEpilogue e3{};
    e3.Cout = h->d_dD; e3.ldc = Kp;
    // the b recurrence (41 ns per user, strictly in user order) in two parts: the first half of the block's users as leading workgroups
    // of the GEMM 3 launch, the rest as leading workgroups of the row launch — each launch then lasts about as long as its own work
    uint32_t bias_u0 = 0;
    if (Ip % 256 != 0 && nb >= 64) {     // (launch_gemm_lds then takes the 128 x 128 kernel, the one that can host a bias role)
      bias_u0 = nb / 2;
      e3.bias_blocks = (Kp + 255u) / 256u; e3.bias_nb = bias_u0; e3.bias_delta = h->d_HG; e3.bias_b = h->P(CDAE_P_B); e3.bias_b_ag = h->P(CDAE_P_B_AG);
      e3.bias_hp = h->hp;
    }
    CHK(launch_gemm_lds<EPI_STORE>(h, st, h->d_GTb, h->d_ZTb, Ip, Kp, Bp, Bp, Bp, Bp, e3, 1, 1));
    CHK(pr.end());
    CHK(pr.begin(h, F_INPUT, st));
    const uint32_t bias_blocks = (Kp + 255u) / 256u;
    DISPATCH_NI(h->NI, full_rows_kernel, dim3(bias_blocks + I), blk, 0, st, h->hp, x.seg, x.seg + I, x.sorted_val, h->delta_rows(),
                h->d_dD, h->d_GTb, Bp, nb, h->P(CDAE_P_W), h->P(CDAE_P_W_AG), h->P(CDAE_P_V), h->P(CDAE_P_V_AG), h->P(CDAE_P_BP),
                h->P(CDAE_P_BP_AG), h->P(CDAE_P_B), h->P(CDAE_P_B_AG), h->d_touched,
                rows_write_images ? h->d_Db : (__bf16*)nullptr, rows_write_images ? h->d_DTb : (__bf16*)nullptr, Ip, bias_u0, (const float*)h->d_HG);
    h->db_valid = rows_write_images;
    h->db_rows_valid = false;
    CHK(pr.end());
    HIPCHK(hipEventRecord(x.released, st));
    HIPCHK(hipGetLastError());
    return 0;
  }
  return full_tail(h, x, s0, nb, FullTail{hg_parts, hg_rows, nullptr, true, h->prof_q, &pr});
}

// IMF / BPR: one block of users (cdae_mf_kernels.hpp).  A block of one user is the reference loop itself (in place).
int compute_batch_mf(cdae_hip* h, int b, const Batch& bt) {
  using namespace cdae;
  cdae_hip::ExBuf& x = h->ex[b];
  hipStream_t st = h->stream;
  const uint32_t I = (uint32_t)h->I, nb = bt.nb;
  // in place = the reference loop: a block of one user, or (mf_seq) a launch window of users that ONE wavefront walks in order
  const bool in_place = nb == 1 || h->mf_seq;
  const dim3 blk(in_place ? 64 : 256), grid_users(in_place ? 1 : (nb + 3) / 4);
  Prof pr;
  HIPCHK(hipStreamWaitEvent(st, x.ready, 0));
  CHK(pr.begin(h, F_DECODE, st));
#define MF_USER(NI_, PAIR_, INP_)                                                                                                   \
  hipLaunchKernelGGL((mf_user_kernel<NI_, PAIR_, INP_>), grid_users, blk, 0, st, h->hp, h->mf_bias, h->d_row_ptr, bt.s0, nb, x.item, \
                     h->d_Wu, h->d_Wu_ag, h->d_ub, h->d_ub_ag, h->P(CDAE_P_W), h->P(CDAE_P_W_AG), h->P(CDAE_P_BP), h->P(CDAE_P_BP_AG), \
                     h->d_UVpre, h->d_G)
#define MF_USER_NI(NI_)                                                              \
  do {                                                                               \
    if (h->mf == 2) { if (in_place) MF_USER(NI_, true, true); else MF_USER(NI_, true, false); }     \
    else { if (in_place) MF_USER(NI_, false, true); else MF_USER(NI_, false, false); }              \
  } while (0)
  switch (h->NI) { case 1: MF_USER_NI(1); break; case 2: MF_USER_NI(2); break; case 4: MF_USER_NI(4); break; default: MF_USER_NI(8); break; }
#undef MF_USER_NI
#undef MF_USER
  CHK(pr.end());
  if (!in_place) {
    CHK(pr.begin(h, F_INPUT, st));
    DISPATCH_NI(h->NI, mf_item_kernel, dim3((I + 3) / 4), blk, 0, st, h->hp, h->mf_bias, h->d_item_order, x.seg, x.seg + I, x.sorted_val,
                h->d_UVpre, h->d_G, h->P(CDAE_P_W), h->P(CDAE_P_W_AG), h->P(CDAE_P_BP), h->P(CDAE_P_BP_AG));
    CHK(pr.end());
  }
  HIPCHK(hipEventRecord(x.released, st));
  HIPCHK(hipGetLastError());
  return 0;
}

// WARP: one block of users (cdae_warp_kernels.hpp).  In place (a block of one user, or the sequential launch window) the one launch is the
// reference loop.  The block schedule: phase U searches, steps the user vectors and writes the block's pair records; the item-major order
// of those records can only be made now, on this stream (VOID keys of the skipped pairs included); phase I is mf_item_kernel, BPR's record
// format without bias steps.
int compute_batch_warp(cdae_hip* h, int b, const Batch& bt, uint64_t seed, uint32_t epoch) {
  using namespace cdae;
  cdae_hip::ExBuf& x = h->ex[b];
  hipStream_t st = h->stream;
  const uint32_t I = (uint32_t)h->I, nb = bt.nb;
  const bool in_place = nb == 1 || h->mf_seq;
  const dim3 blk(in_place ? 64 : 256), grid_users(in_place ? 1 : (nb + 3) / 4);
  uint32_t* const rec_item = h->warp_record ? h->d_warp_rec_item.p : nullptr;
  uint32_t* const rec_cnt = h->warp_record ? h->d_warp_rec_cnt.p : nullptr;
  Prof pr;
  HIPCHK(hipStreamWaitEvent(st, x.ready, 0));
  CHK(pr.begin(h, F_DECODE, st));
  dispatch_ni(h->NI, [&](auto ni) {
    constexpr int NI = decltype(ni)::value;
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid_users, blk, 0, st, h->hp, (const int64_t*)h->d_row_ptr, (const uint32_t*)h->d_col, bt.s0, nb, seed, epoch,
                         (const float*)h->d_warp_l, h->d_Wu.p, h->d_Wu_ag.p, h->P(CDAE_P_W), h->P(CDAE_P_W_AG), (const float*)h->P(CDAE_P_BP),
                         x.item.p, x.val.p, h->d_UVpre.p, h->d_G.p, rec_item, rec_cnt);
    };
    if (in_place) launch(warp_user_kernel<NI, true>); else launch(warp_user_kernel<NI, false>);
  });
  CHK(pr.end());
  if (!in_place) {
    CHK(pr.begin(h, F_SORT, st));
    CHK(order_examples(h, x, bt.E, st, h->d_sort_tmp, 0u, false, false, I));
    CHK(pr.end());
    CHK(pr.begin(h, F_INPUT, st));
    DISPATCH_NI(h->NI, mf_item_kernel, dim3((I + 3) / 4), blk, 0, st, h->hp, 0u, h->d_item_order, x.seg, x.seg + I, x.sorted_val,
                h->d_UVpre, h->d_G, h->P(CDAE_P_W), h->P(CDAE_P_W_AG), h->P(CDAE_P_BP), h->P(CDAE_P_BP_AG));
    CHK(pr.end());
  }
  HIPCHK(hipEventRecord(x.released, st));
  HIPCHK(hipGetLastError());
  return 0;
}

// z for nb users: a contiguous range [u0, u0+nb) (d_uids == nullptr) or the list d_uids (prefix in d_uptr_tmp)
int encode_chunk(cdae_hip* h, const uint32_t* d_uids, uint64_t u0, uint32_t nb, int mode, uint32_t stream_id,
                 uint32_t cidx, uint64_t seed, uint32_t epoch, uint32_t n_units_list = 0, float* z_out = nullptr,
                 float* hpart = nullptr, uint32_t hpart_cap = 0) {
  if (h->item_shard) return fail("an item shard encodes in phases under the multi-shard handle (its rows and its users' private rows are partial)");
  const uint32_t n_units = d_uids ? n_units_list : h->h_unit_ptr[u0 + nb] - h->h_unit_ptr[u0];
  const uint32_t* uptr = d_uids ? h->d_uptr_tmp : h->d_unit_ptr + u0;
  if (!hpart) { hpart = h->d_Hpart; hpart_cap = h->unit_cap; }
  if (n_units > hpart_cap) return fail("%u work units exceed the capacity %u", n_units, hpart_cap);
  DISPATCH_NI(h->NI, cdae::encode_partial_kernel, dim3((n_units + 3) / 4), dim3(256), 0, h->stream, h->hp, h->d_row_ptr, h->d_col,
              h->P(CDAE_P_W), uptr, n_units, d_uids, u0, nb, mode, stream_id, cidx, seed, epoch, hpart,
              (const uint32_t*)nullptr, 0u, d_uids ? (const uint32_t*)nullptr : (const uint32_t*)h->d_unit_user);
  DISPATCH_NI(h->NI, cdae::encode_finish_kernel, dim3((nb + 3) / 4), dim3(256), 0, h->stream, h->hp, hpart, uptr, h->d_Wu,
              h->P(CDAE_P_B), d_uids, u0, nb, mode, z_out ? z_out : h->d_Z, (float*)nullptr, (float*)nullptr, h->d_Uu, (float*)nullptr);
  HIPCHK(hipGetLastError());
  return 0;
}

// Evaluation workspace (data_loss, recommend): z rows and encode partial sums for up to EVAL_CHUNK users per launch — the
// training workspace holds only batch_users of them, far too few wavefronts to fill the chip.
constexpr uint32_t EVAL_CHUNK = 32768;
// item shard: blocks of [users x Kp] floats in the input-sum all-reduce buffer: the input sums, then — the user node being sharded by
// user — the batch's Wu rows (user_factor) and Uu rows (linear_function) contributed by their owner
constexpr uint32_t SHARD_BLOCKS = 3;
inline uint32_t shard_blocks_of(const cdae_hip* h) { return 1u + (h->cfg.user_factor ? 1u : 0u) + (h->cfg.linear_function ? 1u : 0u); }
int ensure_eval_ws(cdae_hip* h, uint32_t users, uint32_t units) {
  CHK(h->d_zeval.ensure(users, h->Kp));
  return h->d_hpart_eval.ensure(units, h->Kp);
}

inline bool is_user_indexed(uint32_t which) {
  return which == CDAE_P_WU || which == CDAE_P_WU_AG || which == CDAE_P_UU || which == CDAE_P_UU_AG || which == CDAE_P_UB || which == CDAE_P_UB_AG;
}
int copy_param_out(cdae_hip* h, uint32_t which, float* host, size_t count) {
  float* d = h->P(which);
  if (!d) return count == 0 ? 0 : fail("parameter %u is not allocated in this configuration", which);
  const bool vec = (which == CDAE_P_BP || which == CDAE_P_BP_AG || which == CDAE_P_UB || which == CDAE_P_UB_AG);
  const size_t rows = (which == CDAE_P_WU || which == CDAE_P_WU_AG || which == CDAE_P_UU || which == CDAE_P_UU_AG) ? (size_t)h->wu_rows() : ((which == CDAE_P_B || which == CDAE_P_B_AG) ? 1 : h->I);
  if (vec) {
    const size_t want = (which == CDAE_P_UB || which == CDAE_P_UB_AG) ? h->U : h->I;
    if (count != want) return fail("parameter %u has %llu elements, got %zu", which, (unsigned long long)want, count);
    HIPCHK(hipMemcpyAsync(host, d, count * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  } else {
    if (count != rows * h->K) return fail("parameter %u has %zu elements, got %zu", which, rows * h->K, count);
    if (rows == 0) return 0;
    HIPCHK(hipMemcpy2DAsync(host, h->K * sizeof(float), d, h->Kp * sizeof(float), h->K * sizeof(float), rows,
                            hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

}  // namespace

extern "C" {

const char* cdae_hip_last_error(void) { return g_err.c_str(); }
int cdae_hip_abi_version(void) { return CDAE_HIP_ABI_VERSION; }

int cdae_hip_create(const cdae_hip_config* cfg, int device_id, cdae_hip_t** out) {
  if (!cfg || !out) return fail("null argument");
  if (cfg->struct_size != sizeof(cdae_hip_config)) return fail("cdae_hip_config size mismatch: got %u, want %zu", cfg->struct_size, sizeof(cdae_hip_config));
  if (cfg->num_dim == 0 || cfg->num_dim > 512) return fail("num_dim must be in [1, 512], got %u", cfg->num_dim);
  if (cfg->loss_type != CDAE_LOSS_SQUARE && cfg->loss_type != CDAE_LOSS_CROSS_ENTROPY)
    return fail("loss_type %u unsupported: CDAE's linear output only works with SQUARE (0) and CROSS_ENTROPY (5); "
                "LOGISTIC aborts in the reference (loss.hpp:96)", cfg->loss_type);
  if (cfg->num_corruptions == 0) return fail("num_corruptions must be >= 1");
  if (cfg->scaled && !(cfg->corruption_ratio < 1.0)) return fail("scaled input needs corruption_ratio < 1");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device_id < 0 || device_id >= ndev) return fail("device %d not available (%d HIP devices)", device_id, ndev);
  HIPCHK(hipSetDevice(device_id));
  if (cfg->full_output > 1u) return fail("bad full_output");
  if (cfg->batch_users > cdae::SLOT_MASK) return fail("batch_users %u exceeds the example word's slot field (2^28 - 1)", cfg->batch_users);
  cdae_hip* h = new cdae_hip();
  h->cfg = *cfg;
  h->device = device_id;
  h->K = cfg->num_dim;
  h->NI = cfg->num_dim <= 64 ? 1 : (cfg->num_dim <= 128 ? 2 : (cfg->num_dim <= 256 ? 4 : 8));
  h->Kp = 64u * h->NI;
  h->B = cfg->batch_users ? cfg->batch_users : 1024u;
  h->full_unfused = DEV_ENV("CDAE_FULL_UNFUSED") != nullptr;
  h->gemm_narrow = DEV_ENV("CDAE_GEMM_NARROW") != nullptr;
  h->rows_separate = DEV_ENV("CDAE_FULL_ROWS_SEPARATE") != nullptr;
  h->gemm2_nt = DEV_ENV("CDAE_GEMM2_NT") != nullptr;
  h->gemm1_tiled = DEV_ENV("CDAE_GEMM1_TILED") != nullptr;
  if (const char* e = DEV_ENV("CDAE_FULL_ROWS_KH")) h->rows_fused_kh = std::atoi(e) == 1 ? 1 : 2;
  if (const char* v = DEV_ENV("CDAE_FULL_ONE_STREAM_MAX")) h->full_one_stream_max = (uint32_t)std::strtoul(v, nullptr, 10);
  h->debug_skip_prep = DEV_ENV("CDAE_DEBUG_SKIP_PREP") != nullptr;
  if (const char* ev = DEV_ENV("CDAE_ROW_PACK")) h->row_pack = std::atoi(ev) != 0;
  h->encode_two_launches = DEV_ENV("CDAE_ENCODE_TWO_LAUNCHES") != nullptr;
  if (const char* ev = DEV_ENV("CDAE_PREP_THREAD")) h->prep_threaded = std::atoi(ev) != 0;
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e != hipSuccess) { delete h; return fail("hipStreamCreate failed: %s", hipGetErrorString(e)); }
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->prep, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->aux, hipStreamNonBlocking);
  {
    // Second prep lane.  Sampling + sorting a batch is a chain of ~12 small launches, ~95 us on the prep stream whatever the
    // batch size; once a training step is shorter than that the decode waits for `ready` (profiles/r02_wave_timeline_256.txt: 15 us
    // per step at 256 users).  Two lanes prepare consecutive batches side by side.  Measured (tools/ab_bench.py, same box):
    // 128 users per batch 0.0972 -> 0.0755 ms per step, 256: 0.0995 -> 0.0942, 512: 0.1409 -> 0.1429 (the prep kernels then
    // only take issue slots from a step that was not waiting for them).  Default "auto": on up to 384 users per batch, on the
    // handle's aux stream (idle in the sampled path; an exchange's collective shares it).  CDAE_PREP2 = off | aux | own | auto.
    const char* sel = DEV_ENV("CDAE_PREP2");
    if (sel && !std::strcmp(sel, "own")) { if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->prep2, hipStreamNonBlocking); h->prep2_own = true; }
    else if (sel && !std::strcmp(sel, "aux")) h->prep2 = h->aux;
    else if (sel && !std::strcmp(sel, "off")) h->prep2 = nullptr;
    else { h->prep2 = h->aux; h->prep2_auto = true; }
    if (const char* hp_ = DEV_ENV("CDAE_HOST_PACE_US")) h->host_pace_us = (uint32_t)std::max(0, std::atoi(hp_));
  }
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_fork, sync_event_flags());
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_join, sync_event_flags());
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_delta, sync_event_flags());
  if (e != hipSuccess) { free_all(h); delete h; return fail("stream/event setup failed: %s", hipGetErrorString(e)); }
  if (int rc = h->d_scalar.alloc(8)) { free_all(h); delete h; return rc; }
  cdae::HyperParams& hp = h->hp;
  hp.lambda = (float)cfg->lambda; hp.lr = (float)cfg->learn_rate; hp.beta = (float)cfg->beta;
  hp.scale = cfg->scaled ? (float)(1.0 / (1.0 - cfg->corruption_ratio)) : 1.f;     // cdae.hpp:202-205
  hp.num_neg = cfg->full_output ? 0u : cfg->num_neg;     // full output: the example list holds the positives only
  hp.loss_type = cfg->loss_type;
  hp.adagrad = cfg->using_adagrad; hp.asymmetric = cfg->asymmetric; hp.user_factor = cfg->user_factor;
  hp.linear = cfg->linear; hp.tanh_act = cfg->tanh_act; hp.linear_function = cfg->linear_function;
  hp.keep_thr = cdae_keep_threshold(cfg->corruption_ratio);
  hp.uid_offset = 0; hp.num_items = 0; hp.K = h->K; hp.Kp = h->Kp;
  hp.own_u0 = 0; hp.own_u1 = ~0ull;
  if (DEV_ENV("CDAE_WAVE_TRACE")) {      // developer aid (tools/wave_trace.py): the last training batch's wavefront timeline
    (void)h->d_trace.alloc(4 * cdae::TRACE_CAP);      // (no trace where this fails)
    hp.trace = h->d_trace;
    if (hp.trace) (void)hipMemset(hp.trace, 0, 4 * cdae::TRACE_CAP * sizeof(unsigned long long));
  }
  hp.debug_skip = DEV_ENV("CDAE_DEBUG_SKIP_ROLES") ? (uint32_t)std::strtoul(DEV_ENV("CDAE_DEBUG_SKIP_ROLES"), nullptr, 10) : 0u;
  hp.debug_rank = DEV_ENV("CDAE_DEBUG_RANK") ? (uint32_t)std::strtoul(DEV_ENV("CDAE_DEBUG_RANK"), nullptr, 10) : 0u;
  *out = h;
  return 0;
}

int cdae_hip_destroy(cdae_hip_t* h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  stop_prep_worker(h);
  (void)hipStreamSynchronize(h->stream);
  if (h->hp.trace) {      // records of the LAST batch every slot saw
    std::vector<unsigned long long> rec(4 * cdae::TRACE_CAP);
    (void)hipMemcpy(rec.data(), h->hp.trace, rec.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    if (FILE* f = std::fopen(DEV_ENV("CDAE_WAVE_TRACE"), "wb")) { std::fwrite(rec.data(), sizeof(unsigned long long), rec.size(), f); std::fclose(f); }
  }
  if (h->xchg && h->xchg_free) { h->xchg_free(h->xchg); h->xchg = nullptr; }
  free_all(h);
  delete h;
  return 0;
}

int cdae_hip_create_mf(const cdae_mf_config* mc, int device_id, cdae_hip_t** out) {
  if (!mc || !out) return fail("null argument");
  if (mc->struct_size != sizeof(cdae_mf_config)) return fail("cdae_mf_config size mismatch: got %u, want %zu", mc->struct_size, sizeof(cdae_mf_config));
  if (mc->loss_type > 3u && mc->loss_type != CDAE_LOSS_CROSS_ENTROPY)
    return fail("loss_type %u unsupported: SQUARE (0), LOGISTIC (1), LOG (2), HINGE (3), CROSS_ENTROPY (5)", mc->loss_type);
  if (mc->num_neg == 0) return fail("num_neg must be >= 1");
  cdae_hip_config c = cdae_hip_config();
  c.struct_size = sizeof(c);
  c.num_dim = mc->num_dim; c.num_neg = mc->num_neg; c.num_corruptions = 1;
  c.loss_type = CDAE_LOSS_SQUARE;                          // (validated above; the MF kernels read hp.loss_type, set below)
  c.using_adagrad = mc->using_adagrad; c.user_factor = 1;
  // default (cdae_hip_mf_default_batch_users): the largest block measured inside the +-0.002 mean-over-seeds Recall@10 bound against the
  // sequential loop (imf.hpp:71-115, bpr.hpp:56-106; DESIGN.md §8b, tests/test_gpu_mf.py) at the BASELINE shapes, one user per block
  // — the reference loop itself — on data sets smaller than the ones it was measured on.  Larger blocks are a throughput setting
  // (batch_users = 0: decided in cdae_hip_set_interactions, where the number of users is known — cdae_hip_mf_default_batch_users)
  c.batch_users = mc->batch_users ? mc->batch_users : 1u;
  c.lambda = mc->lambda; c.learn_rate = mc->learn_rate; c.corruption_ratio = 0.; c.beta = mc->beta;
  CHK(cdae_hip_create(&c, device_id, out));
  cdae_hip* h = *out;
  h->mf = mc->pairwise ? 2u : 1u;
  h->mf_bias = mc->using_bias_term ? 1u : 0u;
  h->mf_auto = mc->batch_users == 0u;
  if (c.batch_users == 1u) { h->mf_seq = true; h->B = MF_SEQ_USERS; }
  h->hp.loss_type = mc->loss_type;
  h->hp.lambda = (float)(2.0 * mc->lambda);                // imf.hpp:92-95, bpr.hpp:78-82: the gradients regularise with 2 * lambda
  return 0;
}

int cdae_hip_create_als(const cdae_als_config* ac, int device_id, cdae_hip_t** out) {
  if (!ac || !out) return fail("null argument");
  if (ac->struct_size != sizeof(cdae_als_config)) return fail("cdae_als_config size mismatch: got %u, want %zu", ac->struct_size, sizeof(cdae_als_config));
  if (!(ac->lambda >= 0.0) || !(ac->alpha >= 0.0)) return fail("lambda and alpha must be >= 0");
  cdae_hip_config c = cdae_hip_config();
  c.struct_size = sizeof(c);
  c.num_dim = ac->num_dim; c.num_neg = 1; c.num_corruptions = 1;
  c.loss_type = CDAE_LOSS_SQUARE; c.user_factor = 1;
  c.batch_users = 1u;                                       // (no block schedule, no training order: rows are stored by user id)
  c.lambda = ac->lambda; c.learn_rate = 0.; c.corruption_ratio = 0.; c.beta = 1.;
  CHK(cdae_hip_create(&c, device_id, out));
  cdae_hip* h = *out;
  h->mf = 3u; h->mf_bias = 0u;
  h->mf_seq = true; h->B = MF_SEQ_USERS;
  h->als_steps = ac->cg_steps ? ac->cg_steps : CDAE_ALS_DEFAULT_CG_STEPS;
  h->als_alpha = (float)ac->alpha; h->als_lambda = (float)ac->lambda; h->als_lambda_cfg = ac->lambda;
  return 0;
}

int cdae_hip_create_warp(const cdae_warp_config* wc, int device_id, cdae_hip_t** out) {
  if (!wc || !out) return fail("null argument");
  if (wc->struct_size != sizeof(cdae_warp_config)) return fail("cdae_warp_config size mismatch: got %u, want %zu", wc->struct_size, sizeof(cdae_warp_config));
  if (wc->loss_type > 3u && wc->loss_type != CDAE_LOSS_CROSS_ENTROPY)
    return fail("loss_type %u unsupported: SQUARE (0), LOGISTIC (1), LOG (2), HINGE (3), CROSS_ENTROPY (5)", wc->loss_type);
  if (wc->num_neg == 0) return fail("num_neg must be >= 1");
  cdae_hip_config c = cdae_hip_config();
  c.struct_size = sizeof(c);
  c.num_dim = wc->num_dim; c.num_neg = wc->num_neg; c.num_corruptions = 1;
  c.loss_type = CDAE_LOSS_SQUARE;                          // (validated above; the WARP kernels read hp.loss_type, set below)
  c.using_adagrad = wc->using_adagrad; c.user_factor = 1;
  c.batch_users = wc->batch_users ? wc->batch_users : 1u;  // no block size has been measured for accuracy: the default is the reference loop
  c.lambda = wc->lambda; c.learn_rate = wc->learn_rate; c.corruption_ratio = 0.;
  c.beta = 0.;                                             // warp.hpp:107-109 divide by sqrt(acc) alone (WARPConfig::beta is never read)
  CHK(cdae_hip_create(&c, device_id, out));
  cdae_hip* h = *out;
  h->mf = 4u; h->mf_bias = 0u;                             // biases are part of the score and of no step (warp.hpp:93-94, 112-113)
  if (c.batch_users == 1u) { h->mf_seq = true; h->B = MF_SEQ_USERS; }
  h->hp.loss_type = wc->loss_type;
  h->hp.lambda = (float)(2.0 * wc->lambda);                // warp.hpp:95-97: the gradients regularise with 2 * lambda
  return 0;
}

int cdae_hip_create_fism_pair(const cdae_fism_config* fc, int device_id, cdae_hip_t** out) {
  if (!fc || !out) return fail("null argument");
  if (fc->struct_size != sizeof(cdae_fism_config)) return fail("cdae_fism_config size mismatch: got %u, want %zu", fc->struct_size, sizeof(cdae_fism_config));
  if (fc->loss_type == CDAE_LOSS_CROSS_ENTROPY)
    return fail("loss_type CROSS_ENTROPY (5) is refused on a pairwise FISM handle: at label 1, the only label a pair has, its gradient is "
                "LOG's; SQUARE (0), LOG (2)");
  CHK(cdae_hip_create_fism(fc, device_id, out));             // (every other refusal is FISM's)
  (*out)->fism_pair = true;
  return 0;
}

int cdae_hip_create_fism(const cdae_fism_config* fc, int device_id, cdae_hip_t** out) {
  if (!fc || !out) return fail("null argument");
  if (fc->struct_size != sizeof(cdae_fism_config)) return fail("cdae_fism_config size mismatch: got %u, want %zu", fc->struct_size, sizeof(cdae_fism_config));
  if (fc->batch_users > 1u)
    return fail("batch_users %u: a FISM block schedule (several users' visits at once) is not built; 0 or 1 is the loop", fc->batch_users);
  if (fc->loss_type == 1u) return fail("loss_type LOGISTIC (1) is refused: the reference CHECK-aborts on it (loss.hpp:96); SQUARE (0), LOG (2), CROSS_ENTROPY (5)");
  if (fc->loss_type == 3u)
    return fail("loss_type HINGE (3) is refused: its gradient jumps, and a FISM trajectory cannot be pinned across the jump; SQUARE (0), LOG (2), CROSS_ENTROPY (5)");
  if (fc->loss_type != CDAE_LOSS_SQUARE && fc->loss_type != 2u && fc->loss_type != CDAE_LOSS_CROSS_ENTROPY)
    return fail("loss_type %u unsupported: SQUARE (0), LOG (2), CROSS_ENTROPY (5)", fc->loss_type);
  if (fc->num_neg == 0) return fail("num_neg must be >= 1");
  if (!(fc->alpha >= 0.0) || !(fc->alpha <= 64.0)) return fail("alpha must be in [0, 64], got %g", fc->alpha);
  cdae_hip_config c = cdae_hip_config();
  c.struct_size = sizeof(c);
  c.num_dim = fc->num_dim; c.num_neg = fc->num_neg; c.num_corruptions = 1;
  c.loss_type = CDAE_LOSS_SQUARE;                          // (validated above; the FISM kernel reads hp.loss_type, set below)
  c.using_adagrad = fc->using_adagrad;
  c.asymmetric = 1;                                        // two item tables: P = W (what a rated set sums), Q = V (what the sweeps read)
  c.batch_users = 1u;
  c.lambda = fc->lambda; c.learn_rate = fc->learn_rate; c.corruption_ratio = 0.;
  c.beta = 0.;                                             // fism.hpp:119-120, 145, 161 divide by sqrt(acc) alone
  CHK(cdae_hip_create(&c, device_id, out));
  cdae_hip* h = *out;
  h->mf = 5u; h->mf_bias = fc->using_bias_term ? 1u : 0u;
  h->mf_seq = true; h->B = MF_SEQ_USERS;
  h->hp.loss_type = fc->loss_type;                         // (hp.lambda is lambda itself: fism.hpp:113-114, 142, 154)
  h->fism_alpha = fc->alpha;
  return 0;
}

uint32_t cdae_hip_row_stride(const cdae_hip_t* h) { return h ? h->Kp : 0; }
uint32_t cdae_hip_mf_default_batch_users(uint64_t U, uint32_t pairwise) {
  if (pairwise) return U >= CDAE_BPR_DEFAULT_MIN_USERS ? CDAE_BPR_DEFAULT_BATCH_USERS : 1u;
  return U >= CDAE_IMF_DEFAULT_MIN_USERS ? CDAE_IMF_DEFAULT_BATCH_USERS : 1u;
}
uint32_t cdae_hip_default_batch_users(uint64_t U) {
  return (uint32_t)std::min<uint64_t>(CDAE_DEFAULT_BATCH_USERS_MAX, std::max<uint64_t>(32, (U / 160) & ~(uint64_t)31));
}
int cdae_hip_user_order(cdae_hip_t* h, uint32_t* out, size_t count) {
  if (!h || !h->d_shared || !out) return fail("set_interactions must be called first");
  if (count != h->U) return fail("user order has %llu entries, got %zu", (unsigned long long)h->U, count);
  for (uint64_t pos = 0; pos < h->U; ++pos) out[pos] = h->user_perm.empty() ? (uint32_t)pos : h->user_perm[pos];
  return 0;
}
int cdae_hip_set_decode_fused(cdae_hip_t* h, int allow) {
  if (!h) return fail("null handle");
  h->allow_fused = allow != 0;
  h->fused_decode = h->fused_possible && h->allow_fused;
  return 0;
}

int cdae_hip_decode_plan(const cdae_hip_t* h, uint32_t* hot_rows, uint32_t* late_rows, uint32_t* fused) {
  if (!h) return fail("null handle");
  const bool set = h->d_shared != nullptr;
  if (hot_rows) *hot_rows = set && h->K <= 256 && !h->mf && !h->cfg.full_output ? h->hot_rows : 0u;
  if (late_rows) *late_rows = set ? h->late_rows : 0u;
  if (fused) *fused = set && h->fused_decode ? 1u : 0u;
  return 0;
}

uint32_t cdae_hip_batch_users(const cdae_hip_t* h) { return !h || (h->cfg.batch_users == 0 && h->U == 0) ? 0 : (h->mf_seq ? 1u : h->B); }
uint32_t cdae_hip_full_output_plan(const cdae_hip_t* h) {
  if (!h || !h->cfg.full_output || h->U == 0) return 0;
  if (h->Kp <= 256 && !h->full_unfused) return CDAE_PLAN_FUSED_DECODE;
  return (gemm2_tn_path(h) ? CDAE_PLAN_GEMM2_TN : 0u) | (rows_fused_path(h) ? CDAE_PLAN_ROWS_FUSED : 0u);
}

int cdae_hip_set_user_id_offset(cdae_hip_t* h, uint64_t offset) {
  if (!h) return fail("null handle");
  h->uid_offset = offset; h->hp.uid_offset = offset;
  return 0;
}

namespace {
void adopt_plan(cdae_hip* h, const cdae::plan::Args& a, cdae::plan::Plan& p, uint32_t cfg_batch_users);
int upload_data_set(cdae_hip* h, const cdae::plan::Plan& p, const int64_t* grp, const uint32_t* gcl);
}  // namespace

// Three steps.  1: the arguments are checked and the data-set plan is built (cdae_dataset_plan.h: host arithmetic alone) — every refusal
// that the arguments and the handle's configuration decide falls here, and leaves the handle with the data set and parameters it had.
// 2: the handle is quiesced, its old data set freed, the plan's numbers copied onto it.  3: allocations, uploads, fills, one synchronise.
int cdae_hip_set_interactions(cdae_hip_t* h, uint64_t U, uint64_t I, const int64_t* row_ptr, const uint32_t* col) {
  if (!h || !row_ptr || (!col && U && row_ptr[U])) return fail("null argument");
  if (h->shard_sampled() && (!h->g_row_ptr_src || !h->g_col_src)) return fail("an item shard of the sampled decode needs the whole rows (set_item_shard_global)");
  if (h->shard_sampled() && h->mf) return fail("the item-sharded layout is CDAE's");
  if (U == 0 || I == 0) return fail("empty interaction matrix (%llu users, %llu items)", (unsigned long long)U, (unsigned long long)I);
  if (I >= (1ull << 30) || U >= (1ull << 30)) return fail("at most 2^30 users and items");
  if (row_ptr[0] != 0) return fail("row_ptr[0] must be 0");
  cdae::plan::Args a;
  a.U = U; a.I = I; a.row_ptr = row_ptr; a.col = col;
  a.kind = h->mf; a.full_output = h->cfg.full_output; a.asymmetric = h->cfg.asymmetric; a.item_shard = h->item_shard;
  a.K = h->K; a.Kp = h->Kp; a.num_neg = h->hp.num_neg;
  a.I_global = h->I_global; a.own_u0 = h->own_u0; a.own_u1 = h->own_u1;
  uint32_t cfg_batch_users = h->cfg.batch_users;
  a.mf_seq = h->mf_seq; a.batch_users = h->B;
  if (h->mf && h->mf_auto) {
    cfg_batch_users = cdae_hip_mf_default_batch_users(U, h->mf == 2u ? 1u : 0u);
    a.mf_seq = cfg_batch_users == 1u;
    a.batch_users = a.mf_seq ? MF_SEQ_USERS : cfg_batch_users;
  }
  // default: ~U/160 users per parameter snapshot, in [32, 256].  256 is the largest size whose Recall@10 shows no systematic
  // offset against the strictly sequential reference schedule (paired multi-seed study at ML-10M shape, DESIGN.md §2: 384 and
  // 512 sit 0.001-0.002 low); tests/test_gpu_accuracy.py certifies exactly this value at the BASELINE shapes.
  if (cfg_batch_users == 0) a.batch_users = cdae_hip_default_batch_users(U);
  if (const char* ev = DEV_ENV("CDAE_DECODE_HOT_POS")) a.hot_pos = std::atof(ev);
  if (const char* ev = DEV_ENV("CDAE_DECODE_LATE_POS")) a.late_pos = std::atof(ev);
  a.no_late_rows = DEV_ENV("CDAE_NO_LATE_ROWS") != nullptr;      // round 5's arithmetic (developer switch)
  // opt-in (CDAE_SORT_COUNTING=1): measured slower than rocPRIM's onesweep beside the training kernels (profiles/r02_*)
  // opt-in (CDAE_SORT_TILE=1).  Measured (profiles/r02_tile_sort.txt): the four launches take 72 us against rocPRIM's ten launches / ~100 us
  // per batch on the prep stream, yet the training step is the same within 1 % at 256 users and 3 % slower at 512 — the prep
  // stream runs beside the training kernels, and what counts there is how much it disturbs them, not its own length
  // (round 4: the tile kernels skip VOID examples, so a sampled item shard can take them too — there the prep chain is NOT hidden
  // behind a look-ahead lane and the library sort's launches and fills are the larger part of it)
  a.sort_tile = DEV_ENV("CDAE_SORT_TILE") != nullptr;
  // the bucket sort is the DEFAULT since round 5.  CDAE_SORT_LIBRARY (developer build): the library sort + segment_kernel everywhere
  // (the A/B side of the bit-equality tests); CDAE_SORT_SCAN: the bucket sort without its cells
  a.sort_library = DEV_ENV("CDAE_SORT_LIBRARY") != nullptr;
  a.sort_scan = DEV_ENV("CDAE_SORT_SCAN") != nullptr;
  // the whole rows of a sampled item shard were lent for ONE call (set_item_shard_global): the call that hands them to the plan consumes them
  const int64_t* const grp = h->g_row_ptr_src;
  const uint32_t* const gcl = h->g_col_src;
  if (h->shard_sampled()) { a.whole_row_ptr = grp; h->g_row_ptr_src = nullptr; h->g_col_src = nullptr; }
  cdae::plan::Plan p;
  const std::string refusal = cdae::plan::build(a, p);
  if (!refusal.empty()) return fail("%s", refusal.c_str());

  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  // nothing may still be reading the old data set: a prefetched batch in the prep worker's queue or in the prep streams included
  CHK(quiesce(h));
  CHK(free_interaction_state(h));
  adopt_plan(h, a, p, cfg_batch_users);
  return upload_data_set(h, p, grp, gcl);
}

namespace {

// step 2: the plan's numbers onto the handle (the old data set is gone, nothing of the new one is on the device yet)
void adopt_plan(cdae_hip* h, const cdae::plan::Args& a, cdae::plan::Plan& p, uint32_t cfg_batch_users) {
  const uint64_t U = a.U, I = a.I;
  h->cfg.batch_users = cfg_batch_users; h->mf_seq = a.mf_seq; h->B = a.batch_users;
  h->U = U; h->I = I; h->hp.num_items = (uint32_t)I;
  if (h->item_shard) { h->own_u0 = h->hp.own_u0 = p.own_u0; h->own_u1 = h->hp.own_u1 = p.own_u1; }
  h->hp.unit_pos = p.unit_pos;
  h->user_perm = std::move(p.act.user_perm); h->user_inv = std::move(p.act.user_inv);
  h->h_row_ptr.assign(p.row_ptr, p.row_ptr + U + 1);
  h->hot_rows = p.split.hot_rows; h->late_rows = p.split.late_rows; h->late_words = (uint32_t)((I + 31) / 32);
  h->h_rank_len = std::move(p.split.rank_len);
  h->fused_geo_set = false;
  std::memcpy(h->off, p.params.off, sizeof h->off); std::memcpy(h->cnt, p.params.cnt, sizeof h->cnt);
  h->n_matrix = p.params.n_matrix; h->n_shared = p.params.n_shared;
  h->ex_per_pos = p.ex_per_pos; h->Ecap = p.Ecap;
  if (h->shard_sampled()) h->h_grow_ptr.assign(a.whole_row_ptr, a.whole_row_ptr + U + 1); else h->h_grow_ptr.clear();
  h->h_gunit_ptr = std::move(p.gunit_ptr);
  h->seq = 0; h->pre_n = 0;
  h->counting_sort = p.counting_sort;
  h->bucket_sort = p.bucket.on; h->bucket_ranges = p.bucket.on ? (uint32_t)p.bucket.cut.size() - 1 : 0u; h->cell_units = 0;
  h->h_unit_ptr = std::move(p.unit_ptr); h->unit_cap = p.unit_cap;
  h->sort_bits = p.sort_bits;
}

// step 3: everything on the device — the rows, the orders, the parameter block, the batch workspace (WRMF: its item-major CSR instead)
int upload_data_set(cdae_hip* h, const cdae::plan::Plan& p, const int64_t* grp, const uint32_t* gcl) {
  const uint64_t U = h->U, I = h->I;
  const uint32_t B = p.B;
  const size_t nnz = (size_t)p.row_ptr[U], IK = (size_t)I * h->Kp;
  CHK(h->d_row_ptr.alloc(U + 1));
  CHK(h->d_col.alloc(nnz));
  HIPCHK(hipMemcpy(h->d_row_ptr, p.row_ptr, (U + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->d_col, p.col, nnz * sizeof(uint32_t), hipMemcpyHostToDevice));
  CHK(dev_upload(h->d_item_order, p.order.data(), (size_t)I));
  CHK(dev_upload(h->d_rank_of, p.rank_of.data(), (size_t)I));
  if (h->late_rows) {
    CHK(dev_upload(h->d_late_bits, p.split.late_bits.data(), (size_t)h->late_words));
    const size_t nB = (size_t)std::max<uint64_t>(std::min<uint64_t>(h->B, U), 1) * cdae::LATE_MAX;
    CHK(h->d_Ghot.alloc(nB)); CHK(h->d_hotdup.alloc(nB));
    HIPCHK(hipMemset(h->d_Ghot, 0, nB * sizeof(float)));
    HIPCHK(hipMemset(h->d_hotdup, 0xFF, nB * sizeof(uint32_t)));
  }
  if (!h->h_err) CHK(err_slot_acquire(h->device, &h->h_err, &h->d_fused_err, &h->err_slot));
  *(volatile uint32_t*)h->h_err = 0u;
  // The fused launch: needs late rows (else the gather would wait for the longest chains); hot rows take a CU per four of them, so
  // at most half the chip's; the row matrices are addressed through 32-bit buffer offsets.
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, h->device));
  h->num_cus = (uint32_t)std::max(prop.multiProcessorCount, 16);
  h->fused_possible = h->late_rows && h->hot_rows <= 2u * h->num_cus && !h->item_shard && (uint64_t)I * h->Kp * 4u < (1ull << 31) &&
                      !DEV_ENV("CDAE_DECODE_UNFUSED");
#ifdef CDAE_DECODE_TIMING
  h->fused_possible = false;
#endif
  h->fused_decode = h->fused_possible && h->allow_fused;

  // parameters
  CHK(h->d_shared.alloc(h->n_shared));
  HIPCHK(hipMemset(h->d_shared, 0, h->n_shared * sizeof(float)));
  const size_t WR = (size_t)h->wu_rows();                   // private rows held here: every user, or an item shard's own user range
  const bool fism = h->mf == 5u;     // FISM: no user table (CDAE_P_WU stays unallocated), no hidden bias, no example lists
  if (fism) {
    h->cnt[CDAE_P_B] = h->cnt[CDAE_P_B_AG] = 0;
  } else {
    h->cnt[CDAE_P_WU] = h->cnt[CDAE_P_WU_AG] = WR * h->Kp;
    CHK(h->d_Wu.alloc(WR * h->Kp));
    CHK(h->d_Wu_ag.alloc(WR * h->Kp));
    HIPCHK(hipMemset(h->d_Wu, 0, std::max<size_t>(WR * h->Kp, 1) * sizeof(float)));
    HIPCHK(hipMemset(h->d_Wu_ag, 0, std::max<size_t>(WR * h->Kp, 1) * sizeof(float)));
  }
  if (h->cfg.linear_function) {
    h->cnt[CDAE_P_UU] = h->cnt[CDAE_P_UU_AG] = WR * h->Kp;
    CHK(h->d_Uu.alloc(WR * h->Kp));
    CHK(h->d_Uu_ag.alloc(WR * h->Kp));
  }

  const bool als = h->mf == 3u;      // WRMF: no example lists, no batch workspace — the item-major CSR of its item half-step instead
  const bool lists = !als && !fism;
  if (lists) {
    if (h->shard_sampled()) {
      const size_t gnnz = (size_t)grp[U];
      CHK(h->d_grow_ptr.alloc(U + 1)); CHK(h->d_gcol.alloc(gnnz));
      HIPCHK(hipMemcpy(h->d_grow_ptr, grp, (U + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(h->d_gcol, gcl, gnnz * sizeof(uint32_t), hipMemcpyHostToDevice));
      CHK(dev_upload(h->d_gunit_ptr, h->h_gunit_ptr.data(), (size_t)U + 1));
      CHK(dev_upload(h->d_gunit_user, p.gunit_user.data(), p.gunit_user.size()));
    }
    if (h->bucket_sort) {
      CHK(dev_upload(h->d_bucket_cut, p.bucket.cut.data(), p.bucket.cut.size()));
      if (!p.bucket.range_of.empty()) CHK(dev_upload(h->d_range_of, p.bucket.range_of.data(), (size_t)I));
    }
    CHK(dev_upload(h->d_unit_ptr, h->h_unit_ptr.data(), (size_t)U + 1));
    CHK(dev_upload(h->d_unit_user, p.unit_user.data(), p.unit_user.size()));
    CHK(h->d_Hpart.alloc((size_t)h->unit_cap * h->Kp));
    CHK(h->d_uptr_tmp.alloc((size_t)B + 1));
    {
      const uint32_t one_unit[2] = {0u, 1u};          // explicit-input step: one user, one unit
      HIPCHK(hipMemcpy(h->d_uptr_tmp, one_unit, sizeof one_unit, hipMemcpyHostToDevice));
    }
    for (auto& b : h->ex) {
      CHK(b.item.alloc(h->Ecap)); CHK(b.val.alloc(h->Ecap));
      CHK(b.sorted_item.alloc(h->Ecap)); CHK(b.sorted_val.alloc(h->Ecap));
      CHK(b.seg.alloc(4 * (size_t)I));                   // first | one-past-last position by item, then the same by popularity rank
      CHK(b.dup_of_pos.alloc(h->Ecap)); CHK(b.dup_of_ex.alloc(h->Ecap)); CHK(b.dup_count.alloc(cdae::DUP_STRIPES));
      if (packs_rows(h)) CHK(b.pack.alloc(((size_t)I + 3) & ~(size_t)3));   // whole wavefronts of the rows [hot_rows, I)
      if (h->counting_sort) {
        CHK(b.item_count.alloc((size_t)I)); CHK(b.prefix.alloc((size_t)I + 1));
        CHK(b.rank.alloc((size_t)I)); CHK(b.bucketed.alloc(h->Ecap));
        CHK(b.tile_hist.alloc((size_t)((h->Ecap + cdae::TILE_EX - 1) / cdae::TILE_EX + 1) * I));
        CHK(b.block_total.alloc(128));
      } else if (h->mf == 4u) {
        // WARP: warp_user_kernel writes 32-bit keys only (its lists are ordered by the library sort on x.item, VOID = I included)
      } else if (I + (h->shard_sampled() ? 1u : 0u) <= 65536) { CHK(b.key16.alloc(h->Ecap + 8)); CHK(b.sorted_key16.alloc(h->Ecap)); }   // (a sampled item shard sorts one more key: VOID = I)
      if (h->bucket_sort) { CHK(b.bucketed.alloc(h->Ecap)); }
      b.cell_tag = 0;
      if (h->bucket_sort && h->d_range_of) {
        // [ranges][units of the largest batch][BKC_SLOTS] words; beyond 256 MiB per set (or 16 384 units) the sort scans instead
        const size_t words = (size_t)h->bucket_ranges * h->unit_cap * cdae::BKC_SLOTS;
        if (h->unit_cap <= cdae::BK_CELL_UNITS_MAX && words * sizeof(uint32_t) <= (256ull << 20)) {
          CHK(b.cells.alloc(words));
          CHK(b.cell_flag.alloc(1));
          HIPCHK(hipMemset(b.cell_flag, 0, sizeof(uint32_t)));
          h->cell_units = h->unit_cap;
        }
      }
      CHK(b.wg_state.alloc(cdae::BK_MAX_RANGES));
      HIPCHK(hipMemset(b.wg_state, 0, cdae::BK_MAX_RANGES * sizeof(uint32_t)));
      if (!b.ready) { HIPCHK(hipEventCreateWithFlags(&b.ready, sync_event_flags())); HIPCHK(hipEventCreateWithFlags(&b.released, sync_event_flags())); }
      HIPCHK(hipEventRecord(b.released, h->stream));
    }
    CHK(h->d_D0.alloc(IK));
    {
      // one correction row per duplicate negative of a batch (~2 % of the examples at ML-10M shape); beyond the
      // capacity decode falls back to atomics.  Zero-filled once: decode's 16-lane path leaves elements >= 64 NV + 16 NT
      // of a row untouched and the gather reads whole rows.
      const char* ev = DEV_ENV("CDAE_DUP_CAP");
      const uint64_t want = h->mf ? 1 : (ev ? std::strtoull(ev, nullptr, 10) : std::max<uint64_t>(65536, h->Ecap / 4));   // small problems: every example (IMF / BPR have no correction rows)
      h->dup_cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(want, 1), std::max<uint64_t>(h->Ecap, 1));
      h->dup_stripes = std::max<uint32_t>(1u, std::min<uint32_t>(cdae::DUP_STRIPES, h->dup_cap / 4096u));
      // Few workgroups draw (bucket_sort_kernel: one per range): one counter's chain is under 2 us, and stripes only strand capacity —
      // a dense small problem (400 users x 200 items, num_neg = 12: 56 000 duplicates among a batch's 86 000 examples) overflowed its
      // 16 stripes of 4096 rows with 65 536 rows allocated, and the atomics fallback made training differ from run to run.
      if (h->bucket_sort && h->bucket_ranges <= 32u) h->dup_stripes = 1u;
      if ((uint64_t)h->dup_cap * h->Kp * 4u >= (1ull << 31)) h->fused_possible = h->fused_decode = false;     // (32-bit buffer offsets in the fused launch)
      CHK(h->d_dup_corr.alloc((size_t)h->dup_cap * h->Kp));
      HIPCHK(hipMemset(h->d_dup_corr, 0, (size_t)h->dup_cap * h->Kp * sizeof(float)));
    }
    CHK(h->d_G.alloc(h->Ecap));
  }
  if (h->mf) {                                              // IMF / BPR / WRMF: the bias arrays (WRMF: the ones IMF's serving reads)
    const uint64_t inst_cap = p.emax * (h->mf == 2 || h->mf == 4 ? h->hp.num_neg : 1u + h->hp.num_neg);
    if (lists) CHK(h->d_UVpre.alloc((size_t)inst_cap * h->Kp));
    if (h->fism_pair) {                                     // FISMauc: bu cancels in every difference; CDAE_P_UB / _UB_AG are not allocated
      h->cnt[CDAE_P_UB] = h->cnt[CDAE_P_UB_AG] = 0;
    } else {
      CHK(h->d_ub.alloc((size_t)U)); CHK(h->d_ub_ag.alloc((size_t)U));
      h->cnt[CDAE_P_UB] = h->cnt[CDAE_P_UB_AG] = (size_t)U;
      HIPCHK(hipMemset(h->d_ub, 0, (size_t)U * sizeof(float)));
    }
  }
  if (h->mf == 4u) {                                        // WARP: the rank weights (warp.hpp:57-60)
    const std::vector<float> l = cdae::warp_rank_weights(I);
    CHK(dev_upload(h->d_warp_l, l.data(), l.size()));
  }
  if (als) {
    CHK(h->d_tptr.alloc(I + 1));
    CHK(h->d_tcol.alloc(nnz));
    HIPCHK(hipMemcpy(h->d_tptr, p.item_major.ptr.data(), (I + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    if (nnz) HIPCHK(hipMemcpy(h->d_tcol, p.item_major.col.data(), nnz * sizeof(uint32_t), hipMemcpyHostToDevice));
  } else if (fism) {                                        // FISM: the scale table (cdae_fism_host.h)
    const std::vector<float> sc = cdae::fism_scale_table(I, h->fism_alpha);
    CHK(dev_upload(h->d_fism_scale, sc.data(), sc.size()));
  } else {
    h->sort_tmp_bytes = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, h->sort_tmp_bytes, h->ex[0].item.p, h->ex[0].sorted_item.p, h->ex[0].val.p,
                                     h->ex[0].sorted_val.p, (size_t)std::max<uint64_t>(h->Ecap, 1), 0u, (unsigned)h->sort_bits, h->stream));
    if (h->ex[0].key16) {
      size_t bytes16 = 0;
      HIPCHK(rocprim::radix_sort_pairs(nullptr, bytes16, h->ex[0].key16.p, h->ex[0].sorted_key16.p, h->ex[0].val.p, h->ex[0].sorted_val.p,
                                       (size_t)std::max<uint64_t>(h->Ecap, 1), 0u, (unsigned)h->sort_bits, h->stream));
      h->sort_tmp_bytes = std::max(h->sort_tmp_bytes, bytes16);
    }
    h->sort_tmp_stride = (h->sort_tmp_bytes + 255) & ~(size_t)255;
    CHK(h->d_sort_tmp.alloc(2 * h->sort_tmp_stride));
    const size_t BK = (size_t)B * h->Kp;
    CHK(h->d_Z.alloc(BK)); CHK(h->d_Dz.alloc(BK)); CHK(h->d_HG.alloc(BK));
    if (h->cfg.linear_function) { CHK(h->d_Ssum.alloc(BK)); CHK(h->d_delta_rows.alloc(BK)); }
    if (h->cfg.full_output) {
      h->Bp = (B + 127u) & ~127u;
      // big item spaces and K > 256: 256-row GEMM tiles (the K > 256 launches — gemm1_loss_duo_kernel, gemm_tn_bf16_kernel — want them)
      h->Ip = (I >= 32768 || h->Kp > 256) ? (((uint32_t)I + 255u) & ~255u) : (((uint32_t)I + 127u) & ~127u);
      CHK(h->d_Zb.alloc((size_t)h->Bp * h->Kp)); CHK(h->d_ZTb.alloc((size_t)h->Kp * h->Bp));
      CHK(h->d_Db.alloc((size_t)h->Ip * h->Kp)); CHK(h->d_DTb.alloc((size_t)h->Kp * h->Ip));
      // G [Bp x Ip] only where a launch reads it: the NT form of GEMM 2 (K > 256 without gemm_tn_bf16_kernel, or CDAE_FULL_UNFUSED);
      // the fused K <= 256 kernel and the TN form read G^T alone (2 GB less per handle at 1 M items x 1024 users)
      if ((h->Kp > 256 || h->full_unfused) && !gemm2_tn_path(h)) CHK(h->d_Gb.alloc((size_t)h->Bp * h->Ip));
      CHK(h->d_GTb.alloc((size_t)h->Ip * h->Bp));
      CHK(h->d_dD.alloc((size_t)h->Ip * h->Kp));
      CHK(h->d_has_in.alloc((size_t)h->Ip));
      HIPCHK(hipMemsetAsync(h->d_has_in, 0, (size_t)h->Ip, h->stream));
      {
        // the rated-items bitmap is read by the fused K <= 256 decode only (the K = 512 launches patch their positives in place:
        // full_positive_fixup_kernel) — round 5: no longer built where nothing reads it (128 MB and ~1 ms of prep stream per
        // 1024-user block at 1 M items)
        if (h->Kp <= 256 && !h->full_unfused) {
          h->bits_stride = (size_t)B * ((I + 31) / 32);
          CHK(h->d_bits_train.alloc(cdae_hip::NSETS * h->bits_stride));     // one per example-buffer set
        }
        // item slices of the fused decode: slices x Bp/128 workgroups ~ one per CU (measured best at B = 2048: 16 slices; every
        // slice adds a [B x Kp] partial of hg)
        const uint32_t tiles = h->Ip / (32 * cdae::FUSED_SUB), ublocks = h->Bp / 128;
        h->full_slices = std::max<uint32_t>(1, std::min<uint32_t>({32u, tiles, (256u + ublocks - 1) / ublocks}));
      }
    }
    if (h->cfg.full_output || h->item_shard) {
      std::vector<uint32_t> iota((size_t)std::max<uint32_t>(B, h->item_shard ? EVAL_CHUNK : 0u) + 1);
      std::iota(iota.begin(), iota.end(), 0u);
      CHK(h->d_iota.alloc(iota.size()));
      HIPCHK(hipMemcpy(h->d_iota, iota.data(), iota.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
      // item shard: [input sums | gathered Wu rows | gathered Uu rows] of a batch, one all-reduce buffer
      if (h->item_shard) CHK(h->d_Hsum.alloc((size_t)SHARD_BLOCKS * B * h->Kp));
    }
    {
      size_t rows = 8 * (size_t)h->unit_cap;
      if (h->cfg.full_output) {
        rows = std::max(rows, (size_t)h->full_slices * B);
        const uint32_t kps = gemm2_k_per_split(h);                                 // unfused path: one [Bp x Kp] slab per contraction split
        rows = std::max(rows, (size_t)((h->Ip + kps - 1) / kps) * h->Bp);
      }
      CHK(h->d_HGpart.alloc(rows * h->Kp));
    }
  }
  CHK(h->d_touched.alloc((size_t)I));                 // (nothing touches an item of a WRMF handle; the delta entry points read the array)
  HIPCHK(hipMemset(h->d_touched, 0, (size_t)I * sizeof(uint32_t)));
  if (lists) CHK(h->d_uids.alloc((size_t)B));
  // weights 0, accumulators 1e-4 (cdae.hpp:114,...), accumulator pad lanes 1: a well-defined state even
  // before init_params / set_param (a zero accumulator pad would make beta == 0 divide 0 by 0)
  auto fillm = [&](float* M, size_t rows, uint32_t K, uint32_t Kp, float v, float pad) {
    if (M && rows) hipLaunchKernelGGL(cdae::fill_matrix_kernel, dim3((uint32_t)((rows * Kp + 255) / 256)), dim3(256), 0, h->stream, M, rows,
                                      K, Kp, v, pad);
  };
  fillm(h->P(CDAE_P_W_AG), I, h->K, h->Kp, 1e-4f, 1.f);
  fillm(h->P(CDAE_P_V_AG), I, h->K, h->Kp, 1e-4f, 1.f);
  fillm(h->d_Wu_ag, WR, h->K, h->Kp, 1e-4f, 1.f);
  fillm(h->d_Uu, WR, h->K, h->Kp, 1.f, 0.f);                // cdae.hpp:131-132
  fillm(h->d_Uu_ag, WR, h->K, h->Kp, 1e-4f, 1.f);
  fillm(h->P(CDAE_P_B_AG), 1, h->K, h->Kp, 1e-4f, 1.f);
  fillm(h->P(CDAE_P_BP_AG), I, 1, 1, 1e-4f, 1.f);
  fillm(h->d_ub_ag, U, 1, 1, 1e-4f, 1.f);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

}  // namespace

int cdae_hip_init_params(cdae_hip_t* h, uint64_t seed) {
  if (h) h->db_valid = h->db_rows_valid = false;      // the bf16 images of the decoder no longer match it (full-output path, compute_batch_full)
  if (!h || !h->d_shared) return fail("set_interactions must be called first");
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  using namespace cdae;
  const double init_scale = 4. * std::sqrt(6. / (double)((h->item_shard ? h->I_global : h->I) + h->K));          // cdae.hpp:112 (an item shard: the whole item space)
  auto blocks = [](size_t n) { return dim3((uint32_t)((n + 255) / 256)); };
  auto init = [&](float* M, size_t rows, uint32_t id, uint64_t row0 = 0) {
    hipLaunchKernelGGL(init_matrix_kernel, blocks(rows * h->Kp), dim3(256), 0, h->stream, M, rows, h->K, h->Kp,
                       cdae_rng_key(seed, 0, id, CDAE_STREAM_INIT), init_scale, row0);
  };
  auto fill = [&](float* M, size_t rows, uint32_t K, uint32_t Kp, float v) {     // accumulator pads are 1, others 0
    hipLaunchKernelGGL(fill_matrix_kernel, blocks(rows * Kp), dim3(256), 0, h->stream, M, rows, K, Kp, v, v == 0.f ? 0.f : 1.f);
  };
  if (h->mf) {                                             // imf.hpp:57-69: Random() * 0.01, accumulators 1e-4, biases 0; wrmf.hpp:47-48, fism.hpp:66-68: Random() * 0.001
    const double mf_scale = h->mf == 3u || h->mf == 5u ? 0.001 : 0.01;
    auto init01 = [&](float* M, size_t rows, uint32_t id, uint64_t row0) {
      hipLaunchKernelGGL(init_matrix_kernel, blocks(rows * h->Kp), dim3(256), 0, h->stream, M, rows, h->K, h->Kp,
                         cdae_rng_key(seed, 0, id, CDAE_STREAM_INIT), mf_scale, row0);
    };
    if (h->mf == 5u) { init01(h->P(CDAE_P_V), h->I, CDAE_P_V, 0); fill(h->P(CDAE_P_V_AG), h->I, h->K, h->Kp, 1e-4f); }   // FISM: Q, and no user table
    else { init01(h->d_Wu, h->U, CDAE_P_WU, h->uid_offset); fill(h->d_Wu_ag, h->U, h->K, h->Kp, 1e-4f); }
    init01(h->P(CDAE_P_W), h->I, CDAE_P_W, 0); fill(h->P(CDAE_P_W_AG), h->I, h->K, h->Kp, 1e-4f);
    if (h->d_ub) { fill(h->d_ub, h->U, 1, 1, 0.f); fill(h->d_ub_ag, h->U, 1, 1, 1e-4f); }
    fill(h->P(CDAE_P_BP), h->I, 1, 1, 0.f); fill(h->P(CDAE_P_BP_AG), h->I, 1, 1, 1e-4f);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
  }
  init(h->P(CDAE_P_W), h->I, CDAE_P_W, h->item0); fill(h->P(CDAE_P_W_AG), h->I, h->K, h->Kp, 1e-4f);     // :113-114
  if (h->cfg.asymmetric) { init(h->P(CDAE_P_V), h->I, CDAE_P_V, h->item0); fill(h->P(CDAE_P_V_AG), h->I, h->K, h->Kp, 1e-4f); }   // :115-118
  const size_t WR = (size_t)h->wu_rows();                   // (an item shard: its own user range, rows keyed by global user id)
  const uint64_t wu_row0 = h->uid_offset + (h->item_shard ? h->own_u0 : 0);
  if (h->cfg.user_factor && WR) { init(h->d_Wu, WR, CDAE_P_WU, wu_row0); fill(h->d_Wu_ag, WR, h->K, h->Kp, 1e-4f); }   // :119-122
  else if (WR) { fill(h->d_Wu, WR, h->K, h->Kp, 0.f); fill(h->d_Wu_ag, WR, h->K, h->Kp, 1e-4f); }
  fill(h->P(CDAE_P_B), 1, h->K, h->Kp, 0.f); fill(h->P(CDAE_P_B_AG), 1, h->K, h->Kp, 1e-4f);    // :123-124
  fill(h->P(CDAE_P_BP), h->I, 1, 1, 0.f); fill(h->P(CDAE_P_BP_AG), h->I, 1, 1, 1e-4f);          // :125-126
  if (h->cfg.linear_function && WR) {                                                           // :130-133
    hipLaunchKernelGGL(fill_matrix_kernel, blocks(WR * h->Kp), dim3(256), 0, h->stream, h->d_Uu, WR, h->K, h->Kp, 1.f, 0.f);
    fill(h->d_Uu_ag, WR, h->K, h->Kp, 1e-4f);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int cdae_hip_set_param(cdae_hip_t* h, uint32_t which, const float* host, size_t count) {
  if (h) h->db_valid = h->db_rows_valid = false;      // the bf16 images of the decoder no longer match it (full-output path, compute_batch_full)
  if (!h || !h->d_shared) return fail("set_interactions must be called first");
  if (which >= CDAE_P_COUNT || !host) return fail("bad argument");
  std::vector<float> by_pos;
  if (!h->user_perm.empty() && is_user_indexed(which) && count % h->U == 0) {   // by user id -> by training position
    by_pos.resize(count);
    const size_t w = count / h->U;
    for (uint64_t pos = 0; pos < h->U; ++pos) std::copy(host + (size_t)h->user_perm[pos] * w, host + ((size_t)h->user_perm[pos] + 1) * w, by_pos.begin() + pos * w);
    host = by_pos.data();
  }
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  float* d = h->P(which);
  if (!d) return fail("parameter %u is not allocated in this configuration", which);
  if (which == CDAE_P_BP || which == CDAE_P_BP_AG || which == CDAE_P_UB || which == CDAE_P_UB_AG) {
    const size_t want = (which == CDAE_P_UB || which == CDAE_P_UB_AG) ? h->U : h->I;
    if (count != want) return fail("parameter %u has %llu elements, got %zu", which, (unsigned long long)want, count);
    HIPCHK(hipMemcpy(d, host, count * sizeof(float), hipMemcpyHostToDevice));
    return 0;
  }
  const size_t rows = (which == CDAE_P_WU || which == CDAE_P_WU_AG || which == CDAE_P_UU || which == CDAE_P_UU_AG) ? (size_t)h->wu_rows() : ((which == CDAE_P_B || which == CDAE_P_B_AG) ? 1 : h->I);
  if (count != rows * h->K) return fail("parameter %u has %zu elements, got %zu", which, rows * h->K, count);
  if (rows == 0) return 0;
  const bool is_acc = (which & 1u) != 0u;                 // odd ids are the *_AG accumulators: pad lanes stay 1
  hipLaunchKernelGGL(cdae::fill_matrix_kernel, dim3((uint32_t)((rows * h->Kp + 255) / 256)), dim3(256), 0, h->stream, d, rows,
                     h->K, h->Kp, 0.f, is_acc ? 1.f : 0.f);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy2D(d, h->Kp * sizeof(float), host, h->K * sizeof(float), h->K * sizeof(float), rows, hipMemcpyHostToDevice));
  return 0;
}

int cdae_hip_get_param(cdae_hip_t* h, uint32_t which, float* host, size_t count) {
  if (!h || !h->d_shared) return fail("set_interactions must be called first");
  if (which >= CDAE_P_COUNT || !host) return fail("bad argument");
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  if (!h->user_perm.empty() && is_user_indexed(which)) {    // device rows are in training order: hand them out by user id
    std::vector<float> tmp(count);
    CHK(copy_param_out(h, which, tmp.data(), count));
    const size_t w = count / h->U;
    for (uint64_t pos = 0; pos < h->U; ++pos) std::copy(tmp.begin() + pos * w, tmp.begin() + (pos + 1) * w, host + (size_t)h->user_perm[pos] * w);
    return 0;
  }
  return copy_param_out(h, which, host, count);
}

int cdae_hip_param_device_ptr(cdae_hip_t* h, uint32_t which, void** device_ptr, size_t* padded_count) {
  if (!h || !h->d_shared || which >= CDAE_P_COUNT || !device_ptr) return fail("bad argument");
  const bool user_indexed = which == CDAE_P_WU || which == CDAE_P_WU_AG || which == CDAE_P_UU || which == CDAE_P_UU_AG || which == CDAE_P_UB || which == CDAE_P_UB_AG;
  if (user_indexed && !h->user_perm.empty())
    return fail("cdae_hip_param_device_ptr: the user-indexed arrays of an IMF / BPR block-schedule handle are stored in TRAINING order "
                "(cdae_hip_user_order), not by user id: use cdae_hip_get_param / cdae_hip_set_param");
  // the pointer is writable: whoever writes the parameters through it must find the full-output path re-imaging the decoder
  h->db_valid = h->db_rows_valid = false;
  *device_ptr = h->P(which);
  if (padded_count) *padded_count = h->cnt[which];
  return 0;
}

int cdae_hip_set_profiling(cdae_hip_t* h, int enabled) {
  if (!h) return fail("null handle");
  h->profiling = enabled < 0 ? 0 : enabled;
  return 0;
}

int cdae_hip_set_profiling_families(cdae_hip_t* h, uint32_t mask) {
  if (!h) return fail("null handle");
  h->prof_mask = mask;
  return 0;
}

int cdae_hip_synchronize(cdae_hip_t* h) {
  if (!h) return fail("null handle");
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  HIPCHK(hipStreamSynchronize(h->stream));
  return fused_check(h);
}

}  // extern "C"

namespace {

constexpr const char* ALS_EVERY_ROW = "a WRMF handle trains by whole half-steps, and a half-step needs every row "
                                      "(cdae_hip_train_epoch, cdae_hip_als_half_step)";
int als_half_step(cdae_hip* h, uint32_t side);              // (below, beside cdae_hip_als_solve_rows)
constexpr const char* WARP_NO_LIST = "a WARP handle has no example list before the step: its negatives are searched for in the training "
                                     "launch (cdae_hip_warp_search returns them)";

constexpr const char* FISM_NO_LIST = "a FISM handle has no example list and no batch workspace: its instances are drawn in the training "
                                     "launch (cdae_hip_train_users runs the loop)";
constexpr const char* FISM_NO_NODE = "a FISM handle has no user node: its hidden row is a sum over the rated set it is given";

// FISM: the loop over users [u_begin, u_end) (cdae_fism_kernels.hpp; a pairwise handle: cdae_fism_pair_kernels.hpp,
// §8n) — one launch of ONE workgroup per window of users (cdae_fism_host.h fism_windows), all on the training stream
int fism_enqueue(cdae_hip* h, uint64_t seed, uint32_t epoch, uint64_t u_begin, uint64_t u_end) {
  using namespace cdae;
  if (u_begin > u_end || u_end > h->U) return fail("bad user range [%llu, %llu)", (unsigned long long)u_begin, (unsigned long long)u_end);
  CHK(join_aux(h));
  const bool pair = h->fism_pair;    // FISMauc: the pair loop (cdae_fism_pair_kernels.hpp, §8n); a window holds FISM_WINDOW_INSTANCES pairs
  const uint64_t steps = fism_steps_per_interaction(pair, h->hp.num_neg);
  const std::vector<uint64_t> cuts = fism_windows(h->h_row_ptr.data(), u_begin, u_end, steps, FISM_WINDOW_INSTANCES);
  const uint32_t res_rows = fism_resident_rows(h->NI, h->fism_resident);
  for (size_t t = 0; t + 1 < cuts.size(); ++t) {
    const uint64_t s0 = cuts[t];
    const uint32_t nb = (uint32_t)(cuts[t + 1] - s0);
    Prof pr;
    h->prof_q = h->seq;
    CHK(pr.begin(h, F_DECODE, h->stream));
    dispatch_ni(h->NI, [&](auto ni) {
      constexpr int NI = decltype(ni)::value;
      // the two loops take the same arguments (a pairwise handle allocates no user bias: its kernel ignores the two null pointers)
      const auto kernel = pair ? (h->hp.adagrad ? fism_pair_user_kernel<NI, true> : fism_pair_user_kernel<NI, false>)
                               : (h->hp.adagrad ? fism_user_kernel<NI, true> : fism_user_kernel<NI, false>);
      hipLaunchKernelGGL(kernel, dim3(1), dim3(FISM_WAVES * WAVE), 0, h->stream, h->hp, h->mf_bias, res_rows, (const int64_t*)h->d_row_ptr,
                         (const uint32_t*)h->d_col, s0, nb, seed, epoch, (const float*)h->d_fism_scale, h->P(CDAE_P_W), h->P(CDAE_P_W_AG),
                         h->P(CDAE_P_V), h->P(CDAE_P_V_AG), h->P(CDAE_P_BP), h->P(CDAE_P_BP_AG), h->d_ub.p, h->d_ub_ag.p);
    });
    CHK(pr.end());
    HIPCHK(hipGetLastError());
    h->seq++;
    h->acc_examples += fism_step_count(h->h_row_ptr.data(), s0, s0 + nb, steps);
    h->acc_batches += 1u; h->acc_users += nb;
  }
  return 0;
}

// FISM: z of rows [c0, c0 + nu) of a device CSR into h->d_zeval (nu rows of Kp floats, allocated by the caller)
int fism_encode(cdae_hip* h, const int64_t* d_ptr, const uint32_t* d_col, uint64_t c0, uint32_t nu) {
  DISPATCH_NI(h->NI, cdae::fism_encode_rows_kernel, dim3((nu + 3) / 4), dim3(256), 0, h->stream, d_ptr, d_col, c0, nu,
              (const float*)h->d_fism_scale, (const float*)h->P(CDAE_P_W), h->d_zeval.p);
  HIPCHK(hipGetLastError());
  return 0;
}

int make_plan(cdae_hip* h, uint64_t u_begin, uint64_t u_end, std::vector<Batch>& plan) {
  if (u_begin > u_end || u_end > h->U) return fail("bad user range [%llu, %llu)", (unsigned long long)u_begin, (unsigned long long)u_end);
  const uint32_t B = (uint32_t)std::min<uint64_t>(h->B, h->U);
  for (uint64_t s0 = u_begin; s0 < u_end; s0 += B) {
    const uint32_t nb = (uint32_t)std::min<uint64_t>(B, u_end - s0);
    const uint64_t E = (uint64_t)(h->h_row_ptr[s0 + nb] - h->h_row_ptr[s0]) * h->ex_per_pos;
    if (E > h->Ecap || E > 0xFFFFFFF0ull) return fail("batch has %llu examples, capacity %llu", (unsigned long long)E, (unsigned long long)h->Ecap);
    for (uint32_t c = 0; c < h->cfg.num_corruptions; ++c) plan.push_back(Batch{s0, nb, c, E});       // cdae.hpp:141
  }
  return 0;
}

inline int set_of(uint64_t q) { return (int)(q % cdae_hip::NSETS); }
// two lanes only where the second one is free: the sampled CDAE path (the full-output path runs its b recurrence on aux, an
// item shard trains in phases)
constexpr uint64_t PREP2_AUTO_MAX_USERS = 384;
inline size_t prep_depth(const cdae_hip* h) {
  if (!h->prep2 || h->mf || h->cfg.full_output || h->item_shard) return 1;
  if (h->prep2_auto && std::min<uint64_t>(h->B, h->U) > PREP2_AUTO_MAX_USERS) return 1;
  // an exchange runs its collective on the aux stream too, issued by the caller's thread while the worker issues lane 1: whichever
  // is queued first decides whether the next batch's lists wait behind an all-reduce (measured one-rank: 0.115 -> 0.151 ms)
  if (h->prep2 == h->aux && h->xchg) return 1;
  return 2;
}
inline int prep_lane(const cdae_hip* h, uint64_t q) { return prep_depth(h) == 2 ? (int)(q & 1) : 0; }
// ---- prep worker ---------------------------------------------------------------------------------------------------
// The caller's thread hands a batch's sampling + sorting to the worker (submit_prep) and, before it issues the training
// kernels that wait on the set's `ready` event, makes sure the worker has ISSUED that record (await_prep: host-side order
// of hipEventRecord before hipStreamWaitEvent).  The other direction needs no handshake: a set's `released` record is issued
// by the caller before it submits the job that reuses the set (NSETS > look-ahead depth).
void prep_worker_main(cdae_hip* h) {
  (void)hipSetDevice(h->device);
  for (;;) {
    cdae_hip::PrepJob j;
    {
      std::unique_lock<std::mutex> lk(h->job_mu);
      h->job_cv.wait(lk, [&] { return h->worker_stop || !h->jobs.empty(); });
      if (h->jobs.empty()) return;                           // stop requested and nothing left
      j = h->jobs.front();
      h->jobs.pop_front();
    }
    if (!h->worker_failed.load(std::memory_order_relaxed)) {
      const int rc = prep_batch(h, j.set, Batch{j.s0, j.nb, j.cidx, j.E}, j.seed, j.epoch, j.lane, j.prof_q);
      if (rc) {
        h->worker_error = cdae_hip_last_error();             // (thread-local on the worker; published by the release store below)
        h->worker_failed.store(1, std::memory_order_release);
      }
    }
    {
      // (under the mutex so that a caller between its predicate check and its wait cannot miss the wake-up)
      std::lock_guard<std::mutex> lk(h->job_mu);
      h->jobs_issued.fetch_add(1, std::memory_order_release);
    }
    h->issued_cv.notify_all();
  }
}

int submit_prep(cdae_hip* h, int set, const Batch& bt, uint64_t seed, uint32_t epoch, int lane, uint64_t prof_q) {
  if (!h->prep_threaded) return prep_batch(h, set, bt, seed, epoch, lane, prof_q);
  if (!h->worker.joinable()) h->worker = std::thread(prep_worker_main, h);
  {
    std::lock_guard<std::mutex> lk(h->job_mu);
    h->jobs.push_back(cdae_hip::PrepJob{set, bt.s0, bt.nb, bt.cidx, bt.E, seed, epoch, lane, prof_q});
  }
  h->jobs_submitted++;
  h->job_cv.notify_one();
  return 0;
}

// jobs 1..id have been issued (their launches and their `ready` records are in the prep stream)
// A failed job is reported ONCE, to the call that was waiting for it: the jobs queued behind it were skipped (their example sets were
// never written), so the queue is drained, whatever was prefetched is forgotten and the flag is cleared — the next call starts
// clean instead of finding the handle bricked by one transient launch error.
int await_prep_upto(cdae_hip* h, uint64_t id) {
  if (!h->prep_threaded) return 0;
  auto wait_for = [&](uint64_t n) {
    for (uint32_t spins = 0; spins < 4096; ++spins) {        // the worker is normally a few microseconds behind at most
      if (h->jobs_issued.load(std::memory_order_acquire) >= n) return;
      __builtin_ia32_pause();
    }
    std::unique_lock<std::mutex> lk(h->job_mu);
    h->issued_cv.wait(lk, [&] { return h->jobs_issued.load(std::memory_order_acquire) >= n; });
  };
  wait_for(id);
  if (h->worker_failed.load(std::memory_order_acquire)) {
    wait_for(h->jobs_submitted);
    const std::string msg = h->worker_error;
    h->pre_n = 0;
    h->worker_failed.store(0, std::memory_order_release);
    return fail("prep worker: %s", msg.c_str());
  }
  return 0;
}
int await_prep(cdae_hip* h) { return await_prep_upto(h, h->jobs_submitted); }

void stop_prep_worker(cdae_hip* h) {
  if (!h->worker.joinable()) return;
  {
    std::lock_guard<std::mutex> lk(h->job_mu);
    h->worker_stop = true;
  }
  h->job_cv.notify_one();
  h->worker.join();
}

int sync_prep(cdae_hip* h) {
  CHK(await_prep(h));
  HIPCHK(hipStreamSynchronize(h->prep));
  if (h->prep2) HIPCHK(hipStreamSynchronize(h->prep2));
  return 0;
}

bool is_prefetched(const cdae_hip* h, size_t t, const Batch& b, uint64_t seed, uint32_t epoch) {
  if (t >= h->pre_n) return false;
  const cdae_hip::PreBatch& p = h->pre[t];
  return p.s0 == b.s0 && p.nb == b.nb && p.cidx == b.cidx && p.seed == seed && p.epoch == epoch;
}
// leading batches of `plan` that are already prepared, at most the look-ahead depth
size_t prefetched_prefix(const cdae_hip* h, const std::vector<Batch>& plan, uint64_t seed, uint32_t epoch) {
  size_t k = 0;
  while (k < prep_depth(h) && k < plan.size() && is_prefetched(h, k, plan[k], seed, epoch)) ++k;
  return k;
}
// Prepared batches nobody will train on are dropped.  Their launches may still be in flight, and the batch that takes their
// set over may be prepared from the other lane: wait for them (a rare path: a caller that prefetches one range and trains another)
int drop_prefetched(cdae_hip* h, size_t keep) {
  if (h->pre_n <= keep) return 0;
  h->pre_n = (uint32_t)keep;
  return sync_prep(h);
}

// Enqueue (no synchronisation with the MAIN stream; the caller's thread may look for up to host_pace_us per batch at the prep chain's
// event, see below) one pass over users [u_begin, u_end): a software pipeline in which the
// sampling + sorting of batch t+1 (prep stream) overlaps the training of batch t (main stream).
int enqueue_users(cdae_hip* h, uint64_t seed, uint32_t epoch, uint64_t u_begin, uint64_t u_end) {
  if (h->mf == 3u) return fail("%s", ALS_EVERY_ROW);
  if (h->mf == 5u) return fism_enqueue(h, seed, epoch, u_begin, u_end);
  if (h->item_shard) return fail("an item shard trains in phases under cdae_hip_multi_train_epoch, not on its own");
  std::vector<Batch> plan;
  CHK(make_plan(h, u_begin, u_end, plan));
  if (plan.empty()) return 0;
  // look-ahead: batch t + depth is prepared while batch t trains; with two prep lanes consecutive batches alternate between them
  const size_t depth = prep_depth(h);
  const uint64_t q0 = h->seq;
  std::vector<uint64_t> job_of(plan.size(), h->jobs_submitted);   // the job (count) that must be issued before batch t may train
  auto prep = [&](size_t t) -> int {
    const uint64_t q = q0 + t;
    if (!(h->debug_skip_prep && q >= 2 * cdae_hip::NSETS)) CHK(submit_prep(h, set_of(q), plan[t], seed, epoch, prep_lane(h, q), q));
    job_of[t] = h->jobs_submitted;
    return 0;
  };
  const size_t have = prefetched_prefix(h, plan, seed, epoch);
  // what was prepared beyond this call's batches stays for the next call (one-batch calls with two batches of look-ahead)
  const bool carry = have == plan.size() && h->pre_n > have;
  if (carry) {
    for (uint32_t t = (uint32_t)have; t < h->pre_n; ++t) h->pre[t - have] = h->pre[t];
    h->pre_n -= (uint32_t)have;
  } else {
    CHK(drop_prefetched(h, have));       // (prepared for a range the caller did not come back to)
    h->pre_n = 0;
  }
  for (size_t t = have; t < depth && t < plan.size(); ++t) CHK(prep(t));
  for (size_t t = 0; t < plan.size(); ++t) {
    if (t + depth < plan.size()) CHK(prep(t + depth));
    CHK(await_prep_upto(h, job_of[t]));                          // the set's `ready` record is in the prep stream
    h->prof_q = h->seq;
    const int set = set_of(h->seq);
    if (h->host_pace_us && !h->mf && !h->cfg.full_output) {
      // Host pacing (round 6): a wait for `ready` is a barrier packet between the encode and the decode launch, ~2-3 us of idle main
      // stream per batch (HISTORY.md "What the two event packets of a step cost").  When the lists are complete by the time the batch is
      // enqueued there is nothing to wait for on the device: the caller's thread looks (for at most host_pace_us — the prep chain
      // of a batch is ~90 us), and only a batch whose lists are late leaves the wait to the device as before.  Measured 0.0906 ->
      // 0.0879 ms per 256-user step at ML-10M shape (the thread is then ~2 batches ahead of the device instead of a whole call).
      const auto t_in = std::chrono::steady_clock::now();
      for (;;) {
        const hipError_t e = hipEventQuery(h->ex[set].ready);
        if (e == hipSuccess) { h->skip_ready_wait = true; break; }
        (void)hipGetLastError();                                  // (hipErrorNotReady is not an error)
        if (e != hipErrorNotReady) return fail("hipEventQuery: %s", hipGetErrorString(e));
        if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_in).count() >= (long)h->host_pace_us) break;
        for (int i = 0; i < 32; ++i) __builtin_ia32_pause();
      }
    }
    int rc = 0;
    if (h->mf == 4u) rc = compute_batch_warp(h, set, plan[t], seed, epoch);
    else if (h->mf) rc = compute_batch_mf(h, set, plan[t]);
    else if (h->cfg.full_output) rc = compute_batch_full(h, set, plan[t], seed, epoch);
    else rc = compute_batch(h, set, plan[t], seed, epoch);
    h->skip_ready_wait = false;
    if (rc) return rc;
    h->seq++;
    h->acc_examples += plan[t].E; h->acc_batches += h->mf_seq ? plan[t].nb : 1u; h->acc_users += plan[t].nb;     // (mf_seq: a block is one user)
  }
  return 0;
}

int fill_stats(cdae_hip* h, cdae_hip_stats* stats) {
  if (stats) {
    std::memset(stats, 0, sizeof *stats);
    stats->users = h->acc_users; stats->examples = h->acc_examples; stats->batches = h->acc_batches;
  }
  h->acc_users = h->acc_examples = h->acc_batches = 0;
  if (h->profiling) CHK(collect_profile(h, stats));
  return 0;
}

}  // namespace

// ---- top-k lists: one sweep behind every entry point that returns them -------------------------------------------------
// Per chunk an entry point produces hidden rows z and names a mask; TopkSweep::run leaves the chunk's lists in h->d_rec, an optional
// hook scores them there, copy_lists_out hands them to the caller.  A new list-producing entry point is a z-producer and a mask.
namespace {
// The per-chunk hook of the TOPN entry points: the lists of rows [r0, r0 + nu) sit in h->d_rec — score them against rows of the target
// CSR (same stream, no host round trip): per-row terms to pu, hit counts to out16[8, 11)
struct TopnHook { const int64_t* ptr; const uint32_t* col; double rows_with_targets; double* pu; double* out16; };
int topn_chunk(cdae_hip* h, const TopnHook& t, uint32_t topk, uint64_t r0, uint32_t nu) {
  hipLaunchKernelGGL(cdae::topn_user_kernel, dim3((nu + 255) / 256), dim3(256), 0, h->stream, (const uint32_t*)h->d_rec, topk, r0, nu,
                     t.ptr, t.col, t.rows_with_targets, t.pu, reinterpret_cast<unsigned long long*>(t.out16 + 8));
  HIPCHK(hipGetLastError());
  return 0;
}
// The tail of both TOPN entry points: the per-row terms `pu` of n rows summed in row order into out16[0, 8) (its hit counts are already
// in [8, 11)), then the sixteen doubles to the host.
int topn_finish(cdae_hip* h, const double* pu, uint64_t n, double* out16, double* rets8, uint64_t* hits3) {
  hipLaunchKernelGGL(cdae::topn_sum_kernel, dim3(1), dim3(64), 0, h->stream, pu, n, out16);
  HIPCHK(hipGetLastError());
  double host[16];
  HIPCHK(hipMemcpyAsync(host, out16, sizeof host, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int c = 0; c < 8; ++c) rets8[c] = host[c];
  if (hits3) std::memcpy(hits3, host + 8, 3 * sizeof(uint64_t));
  return 0;
}
// The n places of a chunk's lists in d_rec (and their scores in d_rec_score) to the caller's arrays, either of which may be null, then
// one synchronisation: the two buffers are the next chunk's too.
int copy_lists_out(cdae_hip* h, size_t n, uint32_t* ids, float* scores) {
  if (ids) HIPCHK(hipMemcpyAsync(ids, h->d_rec, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  if (scores) HIPCHK(hipMemcpyAsync(scores, h->d_rec_score, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (ids || scores) HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}
// Where the general-path kernels (recommend_kernel, full_rank_general_kernel) keep a row's `items` scores: in LDS where that many
// floats fit; otherwise the scores of a launch go to a global workspace of <= 256 MiB, which bounds the rows of one launch.
struct ScorePlace { bool in_lds; size_t shmem; uint32_t rows; };
ScorePlace score_place(uint64_t items, uint32_t rows) {
  const size_t lds_scores = (size_t)items * sizeof(float) + 64;
  if (lds_scores <= 160 * 1024) return {true, lds_scores, rows};
  return {false, 64, (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(rows, (256ull << 20) / (items * sizeof(float))))};
}
// What the rows of a chunk may not return.
//   CSR:    rows [c0, c0 + nu) of the CSR (ptr, col), as it is: rated_bits_kernel in front of the matrix cores, recommend_kernel's own
//           CSR mask on the general path.
//   FILTER: filter_bits_kernel's inputs — rows of the "rated" CSR (ptr, col) or null | rows of the excl CSR (eptr, ecol) or null, at
//           the places `pos` gives the items (null: their ids).  Both paths mask from the bit table it builds.
//   LIST:   ONE row (general path only) masked by the sorted list (list, n) instead of its row of (ptr, col).
struct Mask {
  enum Kind { CSR, FILTER, LIST } kind;
  const int64_t* ptr; const uint32_t* col;
  const int64_t* eptr = nullptr; const uint32_t* ecol = nullptr; const uint32_t* pos = nullptr;
  const uint32_t* list = nullptr; uint32_t n = 0;
};
// The top-k sweep of hidden rows over a decoder image.  Matrix cores (topk <= REC_TOPK_MAX, num_dim <= 256, where the entry point
// may take them): recommend_mfma_kernel, all rows of a chunk in one launch, masked from bit rows in h->d_bits, the contraction length
// by dispatch_nch.  General path: recommend_kernel, any num_dim / topk / item count, one workgroup per row, a row's scores where
// score_place puts them.  The lists land in h->d_rec and, with_scores, their scores in h->d_rec_score.
struct TopkSweep {
  cdae::HyperParams hp; const float* D; const float* bp;   // the swept image: hp.num_items rows of (D, bp), the index space of the lists
  uint32_t topk; bool with_scores;
  const uint32_t* allow;        // non-null: the image's rows are these items of the catalogue, and the lists' places are mapped back to ids
  bool mfma;
  bool in_lds = false; size_t shmem = 0; uint32_t chunk = 0, words = 0;      // prepare()'s
  TopkSweep(const cdae_hip* h, const cdae::HyperParams& hp_, const float* D_, const float* bp_, uint32_t topk_, bool with_scores_,
            const uint32_t* allow_ = nullptr, bool may_mfma = true)
      : hp(hp_), D(D_), bp(bp_), topk(topk_), with_scores(with_scores_), allow(allow_),
        mfma(may_mfma && topk_ <= (uint32_t)cdae::REC_TOPK_MAX && h->K <= 256) {}
  // Once per call, for launches of at most `rows` rows: the chunk (the general path's global score workspace may bound it further),
  // the grow-only workspaces of the path taken, the dynamic-LDS attribute of the kernel it launches.
  int prepare(cdae_hip* h, uint32_t rows, Mask::Kind kind) {
    const uint64_t items = hp.num_items;
    const bool bits_form = kind == Mask::FILTER;
    const void* kernel;
    words = (uint32_t)((items + 31) / 32);
    chunk = rows;
    if (mfma) {
      kernel = dispatch_nch(h->K, [&](auto nch) {
        constexpr int NCH = decltype(nch)::value;
        shmem = cdae::recommend_mfma_lds_bytes(NCH);
        return with_scores ? (const void*)cdae::recommend_mfma_kernel<NCH, true> : (const void*)cdae::recommend_mfma_kernel<NCH, false>;
      });
    } else {
      const ScorePlace sp = score_place(items, rows);
      in_lds = sp.in_lds; shmem = sp.shmem; chunk = sp.rows;
      if (!in_lds) CHK(h->d_score.ensure((size_t)chunk * items));
      kernel = dispatch_ni(h->NI, [&](auto ni) {
        constexpr int NI = decltype(ni)::value;
        return bits_form ? (const void*)cdae::recommend_kernel<NI, true> : (const void*)cdae::recommend_kernel<NI, false>;
      });
    }
    CHK(h->d_rec.ensure((size_t)chunk * topk));
    if (with_scores) CHK(h->d_rec_score.ensure((size_t)chunk * topk));
    if (mfma || bits_form) CHK(h->d_bits.ensure((size_t)chunk * words));
    HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    return 0;
  }
  // nu <= chunk hidden rows z, rows [c0, c0 + nu) of the mask: the bit rows where the path needs them, the sweep, the way back to ids
  int run(cdae_hip* h, const float* z, uint64_t c0, uint32_t nu, const Mask& m) const {
    const dim3 blk(256);
    float* const rec_score = with_scores ? h->d_rec_score.p : nullptr;
    if (m.kind == Mask::FILTER)
      hipLaunchKernelGGL(cdae::filter_bits_kernel, dim3((nu + 3) / 4), blk, 0, h->stream, m.ptr, m.col, m.eptr, m.ecol, m.pos, c0, nu, words,
                         h->d_bits.p);
    else if (mfma)
      hipLaunchKernelGGL(cdae::rated_bits_kernel, dim3((nu + 3) / 4), blk, 0, h->stream, m.ptr, m.col, c0, nu, words, h->d_bits.p);
    if (mfma) {
      const dim3 grid((nu + cdae::REC_USERS_PER_BLOCK - 1) / cdae::REC_USERS_PER_BLOCK);
      dispatch_nch(h->K, [&](auto nch) {
        constexpr int NCH = decltype(nch)::value;
        const auto launch = [&](auto kernel) {
          hipLaunchKernelGGL(kernel, grid, blk, shmem, h->stream, hp, z, nu, D, bp, (const uint32_t*)h->d_bits, words, topk, h->d_rec.p, rec_score);
        };
        if (with_scores) launch(cdae::recommend_mfma_kernel<NCH, true>);
        else launch(cdae::recommend_mfma_kernel<NCH, false>);
      });
    } else {
      float* const score_ws = in_lds ? nullptr : h->d_score.p;
      dispatch_ni(h->NI, [&](auto ni) {
        constexpr int NI = decltype(ni)::value;
        if (m.kind == Mask::FILTER)
          hipLaunchKernelGGL((cdae::recommend_kernel<NI, true>), dim3(nu), blk, shmem, h->stream, hp, (const int64_t*)nullptr,
                             (const uint32_t*)nullptr, (uint64_t)0, z, D, bp, topk, h->d_rec.p, score_ws, (const uint32_t*)h->d_bits, words, rec_score);
        else
          hipLaunchKernelGGL((cdae::recommend_kernel<NI, false>), dim3(nu), blk, shmem, h->stream, hp, m.ptr, m.col, c0, z, D, bp, topk,
                             h->d_rec.p, score_ws, m.list, m.n, rec_score);
      });
    }
    if (allow)
      hipLaunchKernelGGL(cdae::remap_ids_kernel, dim3((uint32_t)(((size_t)nu * topk + 255) / 256)), blk, 0, h->stream, allow, (size_t)nu * topk,
                         h->d_rec.p);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail("recommend: %s", hipGetErrorString(e));
  }
};

// cdae_hip_recommend_all and cdae_hip_eval_topn (hook != nullptr: every chunk's lists are scored on the device, and out may be null);
// rated != nullptr (cdae_hip_recommend_user): ONE user whose input set and mask are the caller's list (sorted, unique) instead of the
// train row, on the general path whatever num_dim is.
int recommend_run(cdae_hip* h, uint64_t u_begin, uint64_t u_end, uint32_t topk, uint32_t* out, const TopnHook* hook,
                  const uint32_t* rated = nullptr, uint32_t n_rated = 0) {
  TopkSweep sweep(h, h->hp, h->dec(), h->P(CDAE_P_BP), topk, false, nullptr, !rated);
  // users per launch: a chunk of the EVALUATION workspace, not of the training batch (through round 3 it was batch_users: a handle
  // with one user per block — the reference schedule — evaluated 16 384 users in 16 384 launches + host round trips, 75 s)
  const uint64_t rows = sweep.mfma ? std::min<uint64_t>(std::max<uint64_t>(u_end - u_begin, 1), EVAL_CHUNK)
                        : rated    ? 1 : std::min<uint64_t>(h->mf ? EVAL_CHUNK : 4096u, std::max<uint64_t>(h->U, 1));
  CHK(sweep.prepare(h, (uint32_t)rows, rated ? Mask::LIST : Mask::CSR));
  DevBuf<uint32_t> d_rated;                       // (freed on every way out)
  if (rated) {
    CHK(d_rated.alloc(n_rated));
    if (n_rated) HIPCHK(hipMemcpyAsync(d_rated, rated, n_rated * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    const uint32_t one_unit[2] = {0u, 1u};
    HIPCHK(hipMemcpyAsync(h->d_uptr_tmp, one_unit, sizeof one_unit, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  Mask mask{rated ? Mask::LIST : Mask::CSR, h->d_row_ptr, h->d_col};
  mask.list = d_rated; mask.n = n_rated;
  for (uint64_t c0 = u_begin; c0 < u_end; c0 += sweep.chunk) {
    const uint32_t nu = (uint32_t)std::min<uint64_t>(sweep.chunk, u_end - c0);
    const float* z;
    if (rated) {
      // get_hidden_values(uid, rated_items) with the default scale 1 (cdae.hpp:169; q == 1 -> empty input, :168-172)
      const bool none = h->hp.keep_thr == 0x100000000ull;
      DISPATCH_NI(h->NI, cdae::encode_partial_kernel, dim3(1), dim3(256), 0, h->stream, h->hp, h->d_row_ptr, h->d_col, h->P(CDAE_P_W),
                  (const uint32_t*)h->d_uptr_tmp, 1u, (const uint32_t*)nullptr, c0, 1u, 0, CDAE_STREAM_CORRUPT, 0u, (uint64_t)0, 0u, h->d_Hpart,
                  (const uint32_t*)d_rated, none ? 0u : n_rated, (const uint32_t*)nullptr);
      DISPATCH_NI(h->NI, cdae::encode_finish_kernel, dim3(1), dim3(256), 0, h->stream, h->hp, h->d_Hpart, (const uint32_t*)h->d_uptr_tmp, h->d_Wu,
                  h->P(CDAE_P_B), (const uint32_t*)nullptr, c0, 1u, 0, h->d_Z, (float*)nullptr, (float*)nullptr, h->d_Uu, (float*)nullptr);
      z = h->d_Z;
    } else if (h->mf == 5u) {
      CHK(h->d_zeval.ensure(sweep.chunk, h->Kp));           // FISM: z = n^-alpha * the sum of the train row's rows of P
      CHK(fism_encode(h, h->d_row_ptr, h->d_col, c0, nu));
      z = h->d_zeval;
    } else if (h->mf) {
      z = h->d_Wu + (size_t)c0 * h->Kp;           // IMF / BPR: score = ub + ib + uv . iv (imf.hpp:117-119); ub does not rank
    } else {
      CHK(ensure_eval_ws(h, nu, h->h_unit_ptr[c0 + nu] - h->h_unit_ptr[c0]));
      CHK(encode_chunk(h, nullptr, c0, nu, 0, CDAE_STREAM_CORRUPT, 0, 0, 0, 0, h->d_zeval, h->d_hpart_eval, (uint32_t)h->d_hpart_eval.cap));   // cdae.hpp:167-172, full rows
      z = h->d_zeval;
    }
    CHK(sweep.run(h, z, c0, nu, mask));
    if (hook) CHK(topn_chunk(h, *hook, topk, c0, nu));
    if (out) CHK(copy_lists_out(h, (size_t)nu * topk, out + (c0 - u_begin) * topk, nullptr));
  }
  return 0;
}
// cdae_hip_recommend_all (hook == nullptr) and the run of cdae_hip_eval_topn behind the same argument checks
int recommend_all(cdae_hip* h, uint64_t u_begin, uint64_t u_end, uint32_t topk, uint32_t* out, const TopnHook* hook) {
  if (!h || !h->d_shared || (!out && !hook)) return fail("bad argument");
  if (u_begin > u_end || u_end > h->U) return fail("bad user range");
  if (topk == 0 || topk > h->I) return fail("topk must be in [1, num_items]");
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  if (!h->user_perm.empty()) {
    // device rows are in training order: rank every position, hand the lists out by user id
    std::vector<uint32_t> perm, inv;
    perm.swap(h->user_perm); inv.swap(h->user_inv);          // (the recursive call sees an identity order)
    std::vector<uint32_t> all((size_t)h->U * topk);
    const int rc = recommend_all(h, 0, h->U, topk, all.data(), nullptr);
    h->user_perm.swap(perm); h->user_inv.swap(inv);
    if (rc) return rc;
    for (uint64_t u = u_begin; u < u_end; ++u)
      std::copy(all.begin() + (size_t)h->user_inv[u] * topk, all.begin() + ((size_t)h->user_inv[u] + 1) * topk, out + (u - u_begin) * topk);
    return 0;
  }
  return recommend_run(h, u_begin, u_end, topk, out, hook);
}
}  // namespace

// geometry and launch of the pipelined-exchange kernels (delta_pipe_kernel)
namespace {
struct PipeGeom { uint32_t Kc; size_t n_tail, n_compact, threads; };
PipeGeom pipe_geom(const cdae_hip* h) {
  PipeGeom g;
  g.Kc = (h->K + 3u) & ~3u;
  g.n_tail = h->n_shared - h->n_matrix;
  const size_t n_rows = h->n_matrix / h->Kp;
  g.n_compact = n_rows * g.Kc + g.n_tail;
  g.threads = n_rows * (g.Kc / 4) + g.n_tail / 4 + g.n_tail % 4;
  return g;
}
// SYNC: the synchronous exchange's forms of STAGE / MERGE (cdae_kernels.hpp delta_pipe_kernel: no snap, no send copy)
template <int MODE, bool SYNC = false>
int launch_pipe(cdae_hip* h) {
  const PipeGeom g = pipe_geom(h);
  if (h->delta_combine == CDAE_COMBINE_GLOBAL_ACC && h->cfg.using_adagrad) {
    // (parameter, accumulator) pairs: same compact buffers, half the threads of the element-wise pass each moving two elements
    const size_t n_rows = h->n_matrix / h->Kp, threads = (n_rows / 2) * (g.Kc / 4) + h->I + h->Kp;
    hipLaunchKernelGGL((cdae::delta_pipe_pair_kernel<MODE, SYNC>), dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, h->stream, h->d_shared,
                       h->d_base, h->d_snap, h->d_delta, h->d_recv, h->n_matrix, h->Kp, g.Kc, (uint32_t)h->I, (float)h->cfg.beta);
    HIPCHK(hipGetLastError());
    return 0;
  }
  hipLaunchKernelGGL((cdae::delta_pipe_kernel<MODE, SYNC>), dim3((uint32_t)((g.threads + 255) / 256)), dim3(256), 0, h->stream, h->d_shared,
                     h->d_base, h->d_snap, h->d_delta, h->d_recv, h->n_matrix, h->Kp, g.Kc, g.n_tail);
  HIPCHK(hipGetLastError());
  return 0;
}
}  // namespace

extern "C" {

int cdae_hip_train_users(cdae_hip_t* h, uint64_t seed, uint32_t epoch, uint64_t u_begin, uint64_t u_end, cdae_hip_stats* stats) {
  if (!h || !h->d_shared) return fail("set_interactions must be called first");
  HIPCHK(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  if (h->mf == 3u) {                                        // WRMF: the user half-step, then the item half-step (wrmf.hpp:102-109)
    if (u_begin != 0 || u_end != h->U) return fail("%s", ALS_EVERY_ROW);
    CHK(als_half_step(h, CDAE_ALS_USERS));
    CHK(als_half_step(h, CDAE_ALS_ITEMS));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->acc_users = h->U; h->acc_examples = 0; h->acc_batches = 2;
    CHK(fill_stats(h, stats));
    if (stats) stats->wall_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return 0;
  }
  CHK(enqueue_users(h, seed, epoch, u_begin, u_end));
  CHK(join_aux(h));
  HIPCHK(hipStreamSynchronize(h->stream));
  CHK(fused_check(h));
#ifdef CDAE_DECODE_TIMING
  {   // developer aid: cycle stamps of row `debug_rank` in the last decode launch (see decode_rows_kernel)
    unsigned long long t[64];
    HIPCHK(hipMemcpy(t, h->d_touched, sizeof t, hipMemcpyDeviceToHost));
    const int n = (int)(t[63] & 0xffffffffu);
    fprintf(stderr, "[decode timing] rank %u: %llu examples, %d stamps (cycles since first):", h->hp.debug_rank, t[63] >> 32, n);
    for (int i = 1; i < n; ++i) fprintf(stderr, " %llu", t[i] - t[0]);
    fprintf(stderr, "\n");
  }
#endif
  CHK(fill_stats(h, stats));
  if (stats) stats->wall_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

int cdae_hip_enqueue_users(cdae_hip_t* h, uint64_t seed, uint32_t epoch, uint64_t u_begin, uint64_t u_end) {
  if (!h || !h->d_shared) return fail("set_interactions must be called first");
  HIPCHK(hipSetDevice(h->device));
  return enqueue_users(h, seed, epoch, u_begin, u_end);
}

int cdae_hip_prefetch_users(cdae_hip_t* h, uint64_t seed, uint32_t epoch, uint64_t u_begin, uint64_t u_end) {
  if (!h || !h->d_shared) return fail("set_interactions must be called first");
  if (h->mf == 3u) return fail("%s", ALS_EVERY_ROW);
  if (h->mf == 5u) return 0;                               // FISM: nothing is prepared ahead of the loop
  HIPCHK(hipSetDevice(h->device));
  std::vector<Batch> plan;
  CHK(make_plan(h, u_begin, u_end, plan));
  if (plan.empty()) return 0;
  // up to the look-ahead depth: with two prep lanes the second batch is prepared ahead as well
  const size_t n = std::min(plan.size(), prep_depth(h));
  const size_t have = prefetched_prefix(h, plan, seed, epoch);
  if (have >= n) return 0;
  CHK(drop_prefetched(h, have));
  for (size_t t = have; t < n; ++t) {
    const uint64_t q = h->seq + t;
    if (!(h->debug_skip_prep && q >= 2 * cdae_hip::NSETS)) CHK(submit_prep(h, set_of(q), plan[t], seed, epoch, prep_lane(h, q), q));
    h->pre[t] = cdae_hip::PreBatch{plan[t].s0, seed, plan[t].nb, plan[t].cidx, epoch};
    h->pre_n = (uint32_t)t + 1;
  }
  return 0;
}

int cdae_hip_collect_stats(cdae_hip_t* h, cdae_hip_stats* stats) {
  if (!h) return fail("null handle");
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  HIPCHK(hipStreamSynchronize(h->stream));
  return fill_stats(h, stats);
}

int cdae_hip_debug_row_pack(cdae_hip_t* h, uint64_t seed, uint32_t epoch, uint64_t u_begin, uint32_t n_users, uint32_t cidx,
                            uint32_t* out_records, uint64_t* n_records) {
  if (!n_records) return fail("null argument");
  if (!h || !h->d_shared) return fail("set_interactions must be called first");
  if (h->mf == 3u) return fail("%s", ALS_EVERY_ROW);
  if (h->mf == 4u) return fail("%s", WARP_NO_LIST);
  if (h->mf == 5u) return fail("%s", FISM_NO_LIST);
  const uint32_t hot = decode_hot_rows(h);
  const uint64_t want = packs_rows(h) ? (((uint64_t)h->I - hot + 3) & ~3ull) : 0;
  if (want > *n_records) return fail("the pack has %llu records, the caller's array holds %llu", (unsigned long long)want, (unsigned long long)*n_records);
  // the batch prepared as training would: sampling, sort, pack (cdae_hip_debug_sample_batch checks the arguments)
  uint64_t E = h->Ecap;
  CHK(cdae_hip_debug_sample_batch(h, seed, epoch, u_begin, n_users, cidx, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &E));
  const cdae::RowRecord* pack = pack_of(h, h->ex[h->seq % cdae_hip::NSETS], E);
  *n_records = pack ? want : 0;
  if (pack && out_records && want) HIPCHK(hipMemcpy(out_records, pack, want * sizeof(cdae::RowRecord), hipMemcpyDeviceToHost));
  return 0;
}

int cdae_hip_debug_sample_batch(cdae_hip_t* h, uint64_t seed, uint32_t epoch, uint64_t u_begin, uint32_t n_users,
                                uint32_t cidx, uint32_t* ex_item, uint64_t* ex_val, uint32_t* sorted_item,
                                uint64_t* sorted_val, uint32_t* seg_begin, uint32_t* seg_end, uint32_t* dup_of_pos,
                                uint32_t* dup_of_ex, uint64_t* n_examples) {
  if (!h || !h->d_shared) return fail("set_interactions must be called first");
  if (h->mf == 3u) return fail("%s", ALS_EVERY_ROW);
  if (h->mf == 4u) return fail("%s", WARP_NO_LIST);
  if (h->mf == 5u) return fail("%s", FISM_NO_LIST);
  if (!n_examples) return fail("null argument");
  if (n_users == 0 || u_begin + n_users > h->U) return fail("bad user range [%llu, +%u)", (unsigned long long)u_begin, n_users);
  if (n_users > std::min<uint64_t>(h->B, h->U)) return fail("%u users exceed batch_users %u", n_users, h->B);
  if (cidx >= h->cfg.num_corruptions) return fail("corruption index %u out of range", cidx);
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  const uint64_t E = (uint64_t)(h->h_row_ptr[u_begin + n_users] - h->h_row_ptr[u_begin]) * h->ex_per_pos;
  if (E > h->Ecap) return fail("batch has %llu examples, capacity %llu", (unsigned long long)E, (unsigned long long)h->Ecap);
  if (E > *n_examples) return fail("batch has %llu examples, the caller's arrays hold %llu", (unsigned long long)E, (unsigned long long)*n_examples);
  *n_examples = E;
  HIPCHK(hipStreamSynchronize(h->stream));
  CHK(sync_prep(h));
  h->pre_n = 0;                                           // the set is overwritten: a prefetched batch is gone
  const int set = set_of(h->seq);
  const int prof = h->profiling;
  h->profiling = 0;
  h->prep_force_sort = true;
  const int rc = prep_batch(h, set, Batch{u_begin, n_users, cidx, E}, seed, epoch);
  h->prep_force_sort = false;
  h->profiling = prof;
  if (rc) return rc;
  CHK(sync_prep(h));
  cdae_hip::ExBuf& x = h->ex[set];
  const size_t I = (size_t)h->I;
  auto out = [&](void* dst, const void* src, size_t bytes) -> int {
    if (dst && bytes) HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return 0;
  };
  CHK(out(ex_item, x.item, E * sizeof(uint32_t)));
  CHK(out(ex_val, x.val, E * sizeof(uint64_t)));
  CHK(out(sorted_val, x.sorted_val, E * sizeof(uint64_t)));
  CHK(out(seg_begin, x.seg, I * sizeof(uint32_t)));
  CHK(out(seg_end, x.seg + I, I * sizeof(uint32_t)));
  CHK(out(dup_of_pos, x.dup_of_pos, E * sizeof(uint32_t)));
  CHK(out(dup_of_ex, x.dup_of_ex, E * sizeof(uint32_t)));
  if (sorted_item && E) {
    if (h->counting_sort || (h->bucket_sort && x.key16)) {   // the counting / bucket sorts write no sorted key array: the segments say the same
      std::vector<uint32_t> sb(I), se(I);
      HIPCHK(hipMemcpy(sb.data(), x.seg, I * sizeof(uint32_t), hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(se.data(), x.seg + I, I * sizeof(uint32_t), hipMemcpyDeviceToHost));
      for (size_t it = 0; it < I; ++it)
        for (uint32_t q = sb[it]; q < se[it]; ++q) sorted_item[q] = (uint32_t)it;
    } else if (x.key16) {                                        // I <= 65536: the sort ran on 16-bit copies of the item ids
      std::vector<uint16_t> k16(E);
      HIPCHK(hipMemcpy(k16.data(), x.sorted_key16, E * sizeof(uint16_t), hipMemcpyDeviceToHost));
      for (uint64_t i = 0; i < E; ++i) sorted_item[i] = k16[i];
    } else {
      CHK(out(sorted_item, x.sorted_item, E * sizeof(uint32_t)));
    }
  }
  // dup_of_pos is only written at the positions segment_kernel numbered: report DUP_NONE everywhere else
  if (dup_of_pos && sorted_val) {
    for (uint64_t p = 0; p < E; ++p)
      if (!((uint32_t)sorted_val[p] & cdae::DUP_PREV_BIT)) dup_of_pos[p] = cdae::DUP_NONE;
  } else if (dup_of_pos) {
    std::vector<uint64_t> sv(E);
    if (E) HIPCHK(hipMemcpy(sv.data(), x.sorted_val, E * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (uint64_t p = 0; p < E; ++p)
      if (!((uint32_t)sv[p] & cdae::DUP_PREV_BIT)) dup_of_pos[p] = cdae::DUP_NONE;
  }
  HIPCHK(hipEventRecord(x.released, h->stream));          // nothing trains on this set: hand it back
  return 0;
}

int cdae_hip_train_epoch(cdae_hip_t* h, uint64_t seed, uint32_t epoch, cdae_hip_stats* stats) {
  if (!h) return fail("null handle");
  return cdae_hip_train_users(h, seed, epoch, 0, h->U, stats);
}

int cdae_hip_encode(cdae_hip_t* h, uint64_t seed, uint32_t epoch, int mode, const uint32_t* uids, size_t n, float* Z) {
  if (!h || !h->d_shared) return fail("set_interactions must be called first");
  if (h->mf == 5u) return fail("cdae_hip_encode: %s (cdae_hip_score_rows and cdae_hip_recommend_rows serve it)", FISM_NO_NODE);
  if (h->mf) return fail("cdae_hip_encode does not apply to an IMF / BPR handle");
  if ((!uids || !Z) && n) return fail("null argument");
  if (mode != 0 && mode != 1) return fail("mode must be 0 or 1");
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  const uint32_t B = (uint32_t)std::min<uint64_t>(h->B, h->U);
  for (size_t i = 0; i < n; ++i) if (uids[i] >= h->U) return fail("user id %u out of range", uids[i]);
  std::vector<uint32_t> prefix;
  for (size_t c0 = 0, nb = 0; c0 < n; c0 += nb) {
    // a chunk: at most B users, and no more work units than the partial-sum rows hold — a list may name its heaviest user any
    // number of times, which outweighs every batch of distinct users (one user always fits)
    prefix.assign(1, 0u);
    for (nb = 0; nb < B && c0 + nb < n; ++nb) {
      const uint32_t units = h->h_unit_ptr[uids[c0 + nb] + 1] - h->h_unit_ptr[uids[c0 + nb]];
      if (nb && prefix.back() + units > h->unit_cap) break;
      prefix.push_back(prefix.back() + units);
    }
    HIPCHK(hipMemcpyAsync(h->d_uids, uids + c0, nb * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_uptr_tmp, prefix.data(), (nb + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));                     // `prefix` is rewritten for the next chunk
    CHK(encode_chunk(h, h->d_uids, 0, (uint32_t)nb, mode, CDAE_STREAM_CORRUPT, 0, seed, epoch, prefix[nb]));
    HIPCHK(hipMemcpy2DAsync(Z + c0 * h->K, h->K * sizeof(float), h->d_Z, h->Kp * sizeof(float), h->K * sizeof(float), nb,
                            hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

int cdae_hip_data_loss(cdae_hip_t* h, uint64_t seed, uint32_t epoch, double* out) {
  if (!h || !h->d_shared || !out) return fail("bad argument");
  if (h->mf) { *out = 0.; return 0; }                      // IMF / BPR do not override ModelBase::data_loss (model_base.hpp:36-40)
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  HIPCHK(hipMemsetAsync(h->d_scalar, 0, sizeof(double), h->stream));
  for (uint64_t s0 = 0; s0 < h->U; s0 += EVAL_CHUNK) {
    const uint32_t nb = (uint32_t)std::min<uint64_t>(EVAL_CHUNK, h->U - s0);
    const uint32_t n_units = h->h_unit_ptr[s0 + nb] - h->h_unit_ptr[s0];
    CHK(ensure_eval_ws(h, nb, n_units));
    for (uint32_t c = 0; c < h->cfg.num_corruptions; ++c) {       // cdae.hpp:86
      CHK(encode_chunk(h, nullptr, s0, nb, 1, CDAE_STREAM_LOSS_CORRUPT, c, seed, epoch, 0, h->d_zeval, h->d_hpart_eval, (uint32_t)h->d_hpart_eval.cap));
      DISPATCH_NI(h->NI, cdae::data_loss_kernel, dim3((n_units + 3) / 4), dim3(256), 0, h->stream, h->hp, h->d_row_ptr, h->d_col,
                  h->d_unit_ptr + s0, n_units, (const uint32_t*)h->d_unit_user, s0, nb, h->d_zeval, h->dec(), h->P(CDAE_P_BP), h->d_scalar);
    }
  }
  HIPCHK(hipGetLastError());
  double v = 0;
  HIPCHK(hipMemcpyAsync(&v, h->d_scalar, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  *out = v / (double)h->cfg.num_corruptions;                      // cdae.hpp:98
  return 0;
}

int cdae_hip_penalty_loss(cdae_hip_t* h, double* out) {
  if (!h || !h->d_shared || !out) return fail("bad argument");
  if (h->mf) { *out = 0.; return 0; }                      // ModelBase::penalty_loss default (model_base.hpp:43-45)
  double a = 0, b = 0;
  CHK(cdae_internal::shared_penalty(h, &a));
  CHK(cdae_internal::private_penalty(h, &b));
  *out = a + b;
  return 0;
}

int cdae_hip_recommend_all(cdae_hip_t* h, uint64_t u_begin, uint64_t u_end, uint32_t topk, uint32_t* out) {
  return recommend_all(h, u_begin, u_end, topk, out, nullptr);
}

// The validation rows TOPN_Evaluation scores against (evaluation.hpp:118-120 builds them as a hashtable on every call): CSR over
// the handle's users, items ascending and unique inside a row; copied to the device once per data set.
int cdae_hip_set_test_rows(cdae_hip_t* h, const int64_t* test_row_ptr, const uint32_t* test_col) {
  if (!h || !h->d_shared || !test_row_ptr) return fail("bad argument (cdae_hip_set_interactions first)");
  HIPCHK(hipSetDevice(h->device));
  const uint64_t U = h->U;
  uint64_t with_rows = 0;
  CHK(cdae_internal::validate_test_rows(test_row_ptr, test_col, U, h->item_shard ? h->I_global : h->I, &with_rows));
  const uint64_t nnz = (uint64_t)test_row_ptr[U];
  CHK(quiesce(h));
  CHK(h->d_test_ptr.alloc(U + 1));
  CHK(h->d_test_col.alloc(nnz));
  CHK(h->d_topn_pu.alloc(U * 8));
  CHK(h->d_topn_out.alloc(16));
  HIPCHK(hipMemcpy(h->d_test_ptr, test_row_ptr, (U + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  if (nnz) HIPCHK(hipMemcpy(h->d_test_col, test_col, nnz * sizeof(uint32_t), hipMemcpyHostToDevice));
  h->test_users_with_rows = with_rows;
  return 0;
}

// TOPN_Evaluation::evaluate (evaluation.hpp:113-181): every user's top-`topk` list over the unrated items (cdae_hip_recommend_all)
// scored against the test rows on the device; rets = P@1 P@5 P@10 R@1 R@5 R@10 MAP@5 MAP@10 averaged over the users with test
// items, summed in user order (the bits of a sequential host loop); hits = summed hit counts in the first 1 / 5 / 10 places.
int cdae_hip_eval_topn(cdae_hip_t* h, uint32_t topk, double* rets8, uint64_t* hits3, uint32_t* ids_out) {
  if (!h || !h->d_shared || !rets8) return fail("bad argument");
  if (!h->d_test_ptr) return fail("cdae_hip_eval_topn: cdae_hip_set_test_rows first");
  if (h->item_shard) return fail("cdae_hip_eval_topn applies to a whole model (item shards: cdae_hip_multi_eval_topn)");
  if (h->test_users_with_rows == 0) return fail("no user has test items");
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  const TopnHook hook{h->d_test_ptr, h->d_test_col, (double)h->test_users_with_rows, h->d_topn_pu, h->d_topn_out};
  HIPCHK(hipMemsetAsync(h->d_topn_out, 0, 16 * sizeof(double), h->stream));
  if (!h->user_perm.empty()) {
    // IMF / BPR block schedules keep their rows in training order: take the lists by user id, score them from a staged copy
    std::vector<uint32_t> all((size_t)h->U * topk);
    CHK(cdae_hip_recommend_all(h, 0, h->U, topk, all.data()));
    if (ids_out) std::copy(all.begin(), all.end(), ids_out);
    const uint32_t UC = (uint32_t)std::min<uint64_t>(h->U, EVAL_CHUNK);
    CHK(h->d_rec.ensure((size_t)UC * topk));
    for (uint64_t c0 = 0; c0 < h->U; c0 += UC) {
      const uint32_t nu = (uint32_t)std::min<uint64_t>(UC, h->U - c0);
      HIPCHK(hipMemcpyAsync(h->d_rec, all.data() + c0 * topk, (size_t)nu * topk * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
      CHK(topn_chunk(h, hook, topk, c0, nu));
      HIPCHK(hipStreamSynchronize(h->stream));
    }
  } else {
    CHK(recommend_all(h, 0, h->U, topk, ids_out, &hook));
  }
  return topn_finish(h, h->d_topn_pu, h->U, h->d_topn_out, rets8, hits3);
}

int cdae_hip_recommend_user(cdae_hip_t* h, uint64_t uid, const uint32_t* rated_items, size_t n_rated, uint32_t topk, uint32_t* out) {
  if (!h || !h->d_shared || !out) return fail("bad argument");
  if (uid >= h->U) return fail("user id %llu out of range", (unsigned long long)uid);
  if (topk == 0 || topk > h->I) return fail("topk must be in [1, num_items]");
  if (n_rated && !rated_items) return fail("null argument");
  if (n_rated + topk > h->I) return fail("%zu rated items leave fewer than topk = %u candidates", n_rated, topk);
  if (h->mf == 5u) return fail("cdae_hip_recommend_user is not built for a FISM handle: cdae_hip_recommend_rows ranks any rated set as it stands");
  if (h->mf) return fail("cdae_hip_recommend_user does not apply to an IMF / BPR handle (its score does not depend on the rated set)");
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  std::vector<uint32_t> rated(rated_items, rated_items + n_rated);
  std::sort(rated.begin(), rated.end());                         // encode sums in ascending item order like the train row
  for (size_t i = 0; i < n_rated; ++i) {
    if (rated[i] >= h->I) return fail("rated item %u out of range", rated[i]);
    if (i && rated[i] == rated[i - 1]) return fail("duplicate rated item %u", rated[i]);
  }
  return recommend_run(h, uid, uid + 1, topk, out, nullptr, rated.data(), (uint32_t)n_rated);
}

}  // extern "C"

// ---- top-k and TOPN for caller-supplied rated sets (cdae_hip_recommend_rows, cdae_hip_eval_topn_rows) -------------------------------
namespace {
struct RowsArgs {
  uint64_t n_rows; const uint32_t* uids; const int64_t* row_ptr; const uint32_t* col;
  const int64_t* t_ptr; const uint32_t* t_col; uint64_t with_targets;      // eval_topn_rows only (t_ptr == nullptr: no scoring)
  uint32_t topk; uint32_t* out_ids; float* out_scores;
};
// a host CSR over n rows: row_ptr from 0 and non-decreasing, items below I, ascending and unique inside a row
int validate_rows_csr(const char* what, const int64_t* row_ptr, const uint32_t* col, uint64_t n, uint64_t I) {
  if (!row_ptr) return fail("null %s row_ptr", what);
  if (row_ptr[0] != 0) return fail("%s row_ptr[0] must be 0", what);
  for (uint64_t r = 0; r < n; ++r)
    if (row_ptr[r + 1] < row_ptr[r]) return fail("%s row_ptr decreases at row %llu", what, (unsigned long long)r);
  if (row_ptr[n] > 0 && !col) return fail("null %s col with %lld items", what, (long long)row_ptr[n]);
  for (uint64_t r = 0; r < n; ++r)
    for (int64_t p = row_ptr[r]; p < row_ptr[r + 1]; ++p) {
      if (col[p] >= I) return fail("%s row %llu: item %u out of range", what, (unsigned long long)r, col[p]);
      if (p > row_ptr[r] && col[p] <= col[p - 1])
        return fail("%s row %llu is not ascending and unique (item %u after %u)", what, (unsigned long long)r, col[p], col[p - 1]);
    }
  return 0;
}
// uids[r]: CDAE_NO_USER, a local user, or — top bit set on a handle that can hold a guest table — a row of that table
constexpr uint64_t GUEST_USERS_MAX = 0x7FFFFFFFull;     // with more users than this a user id may carry the top bit: no guest table
int rows_check_uids(cdae_hip* h, const char* fn, const uint32_t* uids, uint64_t n_rows) {
  if (!uids) return 0;
  for (uint64_t r = 0; r < n_rows; ++r) {
    const uint32_t u = uids[r];
    if (u == cdae::ROW_NO_USER) continue;
    if ((u & cdae::ROW_GUEST) && h->U <= GUEST_USERS_MAX) {
      const uint32_t g = u & ~cdae::ROW_GUEST;
      if (h->n_guests == 0) return fail("%s: row %llu names guest %u, but the handle has no guest table", fn, (unsigned long long)r, g);
      if (g >= h->n_guests) return fail("%s: row %llu names guest %u of %llu", fn, (unsigned long long)r, g, (unsigned long long)h->n_guests);
    } else if (u >= h->U) {
      return fail("%s: row %llu names user %u of %llu", fn, (unsigned long long)r, u, (unsigned long long)h->U);
    }
  }
  return 0;
}
int rows_check(cdae_hip* h, const char* fn, const RowsArgs& a) {
  if (!h) return fail("%s: null handle", fn);
  if (h->mf && h->mf != 5u) return fail("%s does not apply to an IMF / BPR handle (its score does not depend on the rated set)", fn);
  if (h->item_shard) return fail("%s applies to a whole model, not to an item shard", fn);
  if (!h->d_shared) return fail("%s: cdae_hip_set_interactions first", fn);
  if (a.topk == 0 || a.topk > h->I) return fail("%s: topk must be in [1, num_items]", fn);
  if (a.n_rows == 0) return 0;
  CHK(validate_rows_csr("rated", a.row_ptr, a.col, a.n_rows, h->I));
  return rows_check_uids(h, fn, a.uids, a.n_rows);
}
// a host CSR over R rows to a pair of grow-only buffers, on h->stream; one with no items still gets a col buffer, and nothing is copied to it
int upload_csr(cdae_hip* h, DevBuf<int64_t>& ptr, DevBuf<uint32_t>& col, const int64_t* host_ptr, const uint32_t* host_col, uint64_t R) {
  const size_t nnz = (size_t)host_ptr[R];
  CHK(ptr.ensure(R + 1));
  CHK(col.ensure(std::max<size_t>(nnz, 1)));
  HIPCHK(hipMemcpyAsync(ptr, host_ptr, (R + 1) * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
  if (nnz) HIPCHK(hipMemcpyAsync(col, host_col, nnz * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  return 0;
}
// the part every rows entry point shares: the rated-set CSR and the uids to the handle's grow-only buffers (on h->stream) ...
int rows_upload(cdae_hip* h, uint64_t R, const uint32_t* uids, const int64_t* row_ptr, const uint32_t* col) {
  CHK(upload_csr(h, h->d_rows_ptr, h->d_rows_col, row_ptr, col, R));
  CHK(h->d_rows_uid.ensure(R));
  if (uids) HIPCHK(hipMemcpyAsync(h->d_rows_uid, uids, R * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  else HIPCHK(hipMemsetAsync(h->d_rows_uid, 0xFF, R * sizeof(uint32_t), h->stream));          // every row: no user node
  return 0;
}
inline uint32_t rows_empty_input(const cdae_hip* h) { return h->hp.keep_thr == 0x100000000ull ? 1u : 0u; }   // cdae.hpp:168-172 (q == 1)
// ... and z of rows [c0, c0 + nu) of that CSR to h->d_zeval (nu rows of Kp floats, allocated by the caller)
int rows_encode_chunk(cdae_hip* h, const int64_t* row_ptr, uint64_t c0, uint32_t nu) {
  if (h->mf == 5u) return fism_encode(h, h->d_rows_ptr, h->d_rows_col, c0, nu);     // FISM: no node, no hidden bias, rows of any length
  const uint32_t empty_input = rows_empty_input(h);
  const float* Gwu = h->n_guests ? h->d_guest[0].p : nullptr;   // the guest table's Wu / Uu rows (uids with the top bit), if there is one
  const float* Guu = h->n_guests ? h->d_guest[2].p : nullptr;
  // rows of at most one summation group: a wavefront each; longer ones (if the chunk has any): a workgroup each
  bool any_long = false;
  for (uint64_t r = c0; r < c0 + nu && !any_long && !empty_input; ++r) any_long = row_ptr[r + 1] - row_ptr[r] > (int64_t)h->hp.unit_pos;
  DISPATCH_NI(h->NI, cdae::encode_rows_kernel, dim3((nu + cdae::ENC_ROWS_WAVES - 1) / cdae::ENC_ROWS_WAVES), dim3(cdae::ENC_ROWS_WAVES * cdae::WAVE),
              0, h->stream, h->hp, (const int64_t*)h->d_rows_ptr, (const uint32_t*)h->d_rows_col, (const uint32_t*)h->d_rows_uid, c0, nu, empty_input,
              (const float*)h->P(CDAE_P_W), (const float*)h->d_Wu, (const float*)h->d_Uu, (const float*)h->P(CDAE_P_B), h->d_zeval, Gwu, Guu);
  if (any_long)
    DISPATCH_NI(h->NI, cdae::encode_rows_long_kernel, dim3(nu), dim3(cdae::ENC_ROWS_WAVES * cdae::WAVE), 0, h->stream, h->hp,
                (const int64_t*)h->d_rows_ptr, (const uint32_t*)h->d_rows_col, (const uint32_t*)h->d_rows_uid, c0, empty_input,
                (const float*)h->P(CDAE_P_W), (const float*)h->d_Wu, (const float*)h->d_Uu, (const float*)h->P(CDAE_P_B), h->d_zeval, Gwu, Guu);
  return 0;
}
// ---- the top-k run of every rows entry point (cdae_hip_recommend_rows, cdae_hip_eval_topn_rows, cdae_hip_recommend_rows_filtered) ------
// The z-producer is rows_encode_chunk.  The mask is Mask::FILTER — filter_bits_kernel builds a chunk's exclusion rows (rated rows if the
// call excludes them | excl rows) as a bit table and both top-k paths mask from it; the unfiltered entry points are the run with
// "exclude rated, no excl rows, no allow list".  A run with exactly that filter takes Mask::CSR over the rated CSR as it is, the
// kernels those entry points have always launched: through the bit table the general path took
// 0.7 % longer, outside the spread of two runs of the old code (profiles/rows_refactor_ab.txt).  The lists are the same bits either way
// (tests/test_gpu_rows_filtered.py::test_no_filter_is_recommend_rows).
// With an allow list the call first packs the allowed decoder rows (once, not per chunk; rebuilt by every call: the decoder can change
// behind the library's back through cdae_hip_param_device_ptr), the sweep runs over the pack with a by-value copy of hp whose
// num_items is n_allow, and the lists' places are mapped back to ids.  With targets every chunk's lists are scored by the TOPN hook.
struct FilterArgs {
  const int64_t* excl_ptr = nullptr; const uint32_t* excl_col = nullptr; bool exclude_rated = true;
  const uint32_t* allow = nullptr; uint64_t n_allow = 0;
};
int validate_allow(const char* fn, const uint32_t* allow, uint64_t n_allow, uint64_t I) {
  if (!allow) return n_allow ? fail("%s: null allow_items with n_allow = %llu", fn, (unsigned long long)n_allow) : 0;
  if (n_allow == 0) return fail("%s: an allow list with n_allow = 0 (pass allow_items = NULL for the whole catalogue)", fn);
  for (uint64_t p = 0; p < n_allow; ++p) {
    if (allow[p] >= I) return fail("%s: allow_items[%llu] = %u is out of range", fn, (unsigned long long)p, allow[p]);
    if (p && allow[p] <= allow[p - 1])
      return fail("%s: allow_items is not ascending and unique at position %llu (item %u after %u)", fn, (unsigned long long)p, allow[p], allow[p - 1]);
  }
  return 0;
}
// A call's filter to the device (on h->stream): the excl CSR over R rows; the allow list (d_flt_allow) and its inverse, item -> place
// with 0xFFFFFFFF elsewhere (d_flt_pos) ...
int filter_upload(cdae_hip* h, const FilterArgs& f, uint64_t R) {
  if (f.excl_ptr) CHK(upload_csr(h, h->d_flt_eptr, h->d_flt_ecol, f.excl_ptr, f.excl_col, R));
  if (!f.allow) return 0;
  const uint32_t na = (uint32_t)f.n_allow;
  CHK(h->d_flt_allow.ensure(na));
  CHK(h->d_flt_pos.ensure(h->I));
  HIPCHK(hipMemcpyAsync(h->d_flt_allow, f.allow, na * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(h->d_flt_pos, 0xFF, h->I * sizeof(uint32_t), h->stream));
  hipLaunchKernelGGL(cdae::allow_pos_kernel, dim3((na + 255) / 256), dim3(256), 0, h->stream, (const uint32_t*)h->d_flt_allow, na, h->d_flt_pos.p);
  HIPCHK(hipGetLastError());
  return 0;
}
// ... and the mask it makes with the "rated" CSR (ptr, col), which is null where the call does not exclude those rows
Mask filter_mask(const cdae_hip* h, const FilterArgs& f, const int64_t* ptr, const uint32_t* col) {
  return Mask{Mask::FILTER, ptr, col, f.excl_ptr ? h->d_flt_eptr.p : nullptr, h->d_flt_ecol, f.allow ? h->d_flt_pos.p : nullptr};
}
int rows_run(cdae_hip* h, const RowsArgs& a, const FilterArgs& f = FilterArgs{}) {
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  const uint64_t R = a.n_rows;
  CHK(rows_upload(h, R, a.uids, a.row_ptr, a.col));
  if (a.t_ptr) {
    CHK(upload_csr(h, h->d_rows_tptr, h->d_rows_tcol, a.t_ptr, a.t_col, R));
    CHK(h->d_rows_pu.ensure(R, 8));
    if (!h->d_rows_out) CHK(h->d_rows_out.alloc(16));
    HIPCHK(hipMemsetAsync(h->d_rows_out, 0, 16 * sizeof(double), h->stream));
  }
  const TopnHook hook{h->d_rows_tptr, h->d_rows_tcol, (double)a.with_targets, h->d_rows_pu, h->d_rows_out};
  CHK(filter_upload(h, f, R));
  TopkSweep sweep(h, h->hp, h->dec(), h->P(CDAE_P_BP), a.topk, a.out_scores != nullptr, f.allow ? h->d_flt_allow.p : nullptr);
  if (f.allow) {
    const uint32_t na = (uint32_t)f.n_allow;
    CHK(h->d_flt_D.ensure(na, h->Kp));
    CHK(h->d_flt_bp.ensure(na));
    DISPATCH_NI(h->NI, cdae::pack_decoder_kernel, dim3((na + cdae::PACK_WAVES - 1) / cdae::PACK_WAVES), dim3(cdae::PACK_WAVES * cdae::WAVE), 0,
                h->stream, (const uint32_t*)h->d_flt_allow, na, h->Kp, sweep.D, sweep.bp, h->d_flt_D.p, h->d_flt_bp.p);
    HIPCHK(hipGetLastError());
    sweep.hp.num_items = na; sweep.D = h->d_flt_D; sweep.bp = h->d_flt_bp;
  }
  const bool csr_mask = f.exclude_rated && !f.excl_ptr && !f.allow;     // the mask is the rated CSR and nothing else
  CHK(sweep.prepare(h, (uint32_t)std::min<uint64_t>(R, sweep.mfma ? EVAL_CHUNK : 4096u), csr_mask ? Mask::CSR : Mask::FILTER));
  CHK(h->d_zeval.ensure(sweep.chunk, h->Kp));
  const Mask mask = csr_mask ? Mask{Mask::CSR, h->d_rows_ptr, h->d_rows_col}
                             : filter_mask(h, f, f.exclude_rated ? h->d_rows_ptr.p : nullptr, h->d_rows_col);
  for (uint64_t c0 = 0; c0 < R; c0 += sweep.chunk) {
    const uint32_t nu = (uint32_t)std::min<uint64_t>(sweep.chunk, R - c0);
    CHK(rows_encode_chunk(h, a.row_ptr, c0, nu));
    CHK(sweep.run(h, h->d_zeval, c0, nu, mask));
    if (a.t_ptr) CHK(topn_chunk(h, hook, a.topk, c0, nu));
    CHK(copy_lists_out(h, (size_t)nu * a.topk, a.out_ids ? a.out_ids + c0 * a.topk : nullptr, a.out_scores ? a.out_scores + c0 * a.topk : nullptr));
  }
  return 0;
}

// ---- top-k item neighbours (cdae_hip_similar_items) -----------------------------------------------------------------------------------
// The z-producer is a gather: the hidden row of query q is row q of the item table T (COSINE: divided by its norm),
// the swept image is T itself (DOT without an allow list: in place), or the allowed and / or normalised rows gathered once per call
// (rebuilt by every call: the parameters can change behind the library's back through cdae_hip_param_device_ptr), the bias is a buffer
// of +0.0.  The mask is Mask::FILTER: its "rated" CSR is (0, 1, 2, ... ; query_items) when the query itself is excluded, its
// excl CSR the caller's, its pos the allow list's inverse.  One host synchronisation per chunk.
struct SimilarArgs {
  uint64_t n_queries; const uint32_t* query_items; const float* T; bool cosine, exclude_self;
  uint32_t topk; uint32_t* out_ids; float* out_scores;
};
// out[p] = row ids[p] (ids == nullptr: row p) of T for p < n, normalised when `cosine`
void gather_rows(cdae_hip* h, bool cosine, const uint32_t* ids, uint32_t n, const float* T, float* out) {
  const dim3 grid((n + cdae::PACK_WAVES - 1) / cdae::PACK_WAVES), block(cdae::PACK_WAVES * cdae::WAVE);
  dispatch_ni(h->NI, [&](auto ni) {
    constexpr int NI = decltype(ni)::value;
    if (cosine) hipLaunchKernelGGL((cdae::gather_rows_kernel<NI, true>), grid, block, 0, h->stream, ids, n, h->Kp, T, out);
    else hipLaunchKernelGGL((cdae::gather_rows_kernel<NI, false>), grid, block, 0, h->stream, ids, n, h->Kp, T, out);
  });
}
int similar_run(cdae_hip* h, const SimilarArgs& a, const FilterArgs& f) {
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  const uint64_t Q = a.n_queries;
  CHK(h->d_sim_q.ensure(Q));
  HIPCHK(hipMemcpyAsync(h->d_sim_q, a.query_items, Q * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  if (a.exclude_self) {
    CHK(h->d_sim_iota.ensure(Q + 1));
    hipLaunchKernelGGL(cdae::iota_ptr_kernel, dim3((uint32_t)((Q + 1 + 255) / 256)), dim3(256), 0, h->stream, (size_t)(Q + 1), h->d_sim_iota.p);
  }
  CHK(filter_upload(h, f, Q));
  const uint32_t n = (uint32_t)(f.allow ? f.n_allow : h->I);           // the index space of the sweep
  const bool grew = h->d_sim_zero.cap < n;
  CHK(h->d_sim_zero.ensure(n));
  if (grew) HIPCHK(hipMemsetAsync(h->d_sim_zero, 0, h->d_sim_zero.cap * sizeof(float), h->stream));
  TopkSweep sweep(h, h->hp, a.T, h->d_sim_zero, a.topk, a.out_scores != nullptr, f.allow ? h->d_flt_allow.p : nullptr);
  sweep.hp.num_items = n;
  if (a.cosine || f.allow) {                                           // the table image of this call
    CHK(h->d_sim_T.ensure(n, h->Kp));
    gather_rows(h, a.cosine, sweep.allow, n, a.T, h->d_sim_T.p);
    sweep.D = h->d_sim_T;
  }
  HIPCHK(hipGetLastError());
  CHK(sweep.prepare(h, (uint32_t)std::min<uint64_t>(Q, sweep.mfma ? EVAL_CHUNK : 4096u), Mask::FILTER));
  CHK(h->d_zeval.ensure(sweep.chunk, h->Kp));
  const Mask mask = filter_mask(h, f, a.exclude_self ? h->d_sim_iota.p : nullptr, h->d_sim_q);
  for (uint64_t c0 = 0; c0 < Q; c0 += sweep.chunk) {
    const uint32_t nu = (uint32_t)std::min<uint64_t>(sweep.chunk, Q - c0);
    gather_rows(h, a.cosine, (const uint32_t*)h->d_sim_q + c0, nu, a.T, h->d_zeval.p);
    CHK(sweep.run(h, h->d_zeval, c0, nu, mask));
    CHK(copy_lists_out(h, (size_t)nu * a.topk, a.out_ids + c0 * a.topk, a.out_scores ? a.out_scores + c0 * a.topk : nullptr));
  }
  return 0;
}

// ---- scores and ranks of caller-supplied candidates (cdae_hip_score_rows) ------------------------------------------------------------
// Candidates per chunk: a chunk takes whole candidate rows while they fit; a row of more candidates than this (scores only: ranks stop
// at CDAE_RANK_CANDIDATES_MAX) is cut into chunks of exactly this many, so a row of num_items candidates fits whatever num_items is.
constexpr int64_t SCORE_CAND_CHUNK = 65536;
static_assert(SCORE_CAND_CHUNK % cdae::SCORE_TILE == 0 && SCORE_CAND_CHUNK >= CDAE_RANK_CANDIDATES_MAX, "a ranked row lies inside one chunk");
static_assert(cdae::RANK_CANDIDATES_MAX == CDAE_RANK_CANDIDATES_MAX, "rank_rows_kernel's LDS row");
static_assert(EVAL_CHUNK <= 65536, "a tile names its row's slot in 16 bits");
struct ScoreChunk {
  uint64_t c0; uint32_t nu; bool encode;        // the rows whose z the chunk reads: [c0, c0 + nu), encoded by the first chunk over them
  int64_t p0, p1;                               // its candidates: positions [p0, p1) of the candidate CSR
  size_t t0, t1;                                // its tiles in the call's tile table
  uint64_t ra, rb;                              // the rows that have candidates in it (ranks: each of them wholly)
};
// Host side of the tile map: one walk over the candidate CSR (validated before) cuts the call into chunks and the chunks into tiles.
void score_plan(uint64_t R, const int64_t* cp, std::vector<uint2>& tiles, std::vector<ScoreChunk>& chunks) {
  tiles.clear(); chunks.clear();
  for (uint64_t c0 = 0; c0 < R; c0 += EVAL_CHUNK) {
    const uint32_t nu = (uint32_t)std::min<uint64_t>(EVAL_CHUNK, R - c0);
    bool first = true;
    int64_t pb = cp[c0]; size_t tb = tiles.size(); uint64_t ra = c0;          // the open chunk
    auto close = [&](int64_t pe, uint64_t rb) {
      if (pe > pb) { chunks.push_back(ScoreChunk{c0, nu, first, pb, pe, tb, tiles.size(), ra, rb}); first = false; }
      pb = pe; tb = tiles.size(); ra = rb;
    };
    for (uint64_t r = c0; r < c0 + nu; ++r) {
      int64_t q = cp[r];
      const int64_t qe = cp[r + 1];
      while (q < qe) {
        const int64_t room = SCORE_CAND_CHUNK - (q - pb);
        if (qe - q > room && q > pb) { close(q, q == cp[r] ? r : r + 1); if (q != cp[r]) ra = r; continue; }   // does not fit: the open chunk ends here
        const int64_t take = std::min(qe - q, SCORE_CAND_CHUNK);
        for (int64_t t = q; t < q + take; t += cdae::SCORE_TILE) {
          const uint32_t cnt = (uint32_t)std::min<int64_t>(cdae::SCORE_TILE, q + take - t);
          tiles.push_back(make_uint2((uint32_t)(r - c0) | (cnt - 1u) << 16, (uint32_t)(t - pb)));
        }
        q += take;
      }
    }
    close(cp[c0 + nu], c0 + nu);
  }
}
int score_run(cdae_hip* h, uint64_t R, const uint32_t* uids, const int64_t* row_ptr, const uint32_t* col, const int64_t* cp,
              const uint32_t* cc, float* out_scores, uint32_t* out_ranks) {
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  CHK(rows_upload(h, R, uids, row_ptr, col));
  const size_t total = (size_t)cp[R];
  std::vector<ScoreChunk> chunks;
  score_plan(R, cp, h->h_cand_tiles, chunks);
  const size_t per_chunk = std::min<size_t>(total, (size_t)SCORE_CAND_CHUNK);
  CHK(upload_csr(h, h->d_cand_ptr, h->d_cand_col, cp, cc, R));
  CHK(h->d_cand_tiles.ensure(h->h_cand_tiles.size()));
  CHK(h->d_cand_score.ensure(per_chunk));
  if (out_ranks) CHK(h->d_cand_rank.ensure(per_chunk));
  CHK(h->d_zeval.ensure((size_t)std::min<uint64_t>(R, EVAL_CHUNK), h->Kp));
  HIPCHK(hipMemcpyAsync(h->d_cand_tiles, h->h_cand_tiles.data(), h->h_cand_tiles.size() * sizeof(uint2), hipMemcpyHostToDevice, h->stream));
  for (const ScoreChunk& c : chunks) {
    if (c.encode) CHK(rows_encode_chunk(h, row_ptr, c.c0, c.nu));
    const uint32_t n_tiles = (uint32_t)(c.t1 - c.t0);
    const size_t n_cand = (size_t)(c.p1 - c.p0);
    DISPATCH_NI(h->NI, cdae::score_rows_kernel, dim3((n_tiles + cdae::SCORE_WAVES - 1) / cdae::SCORE_WAVES), dim3(cdae::SCORE_WAVES * cdae::WAVE), 0,
                h->stream, h->hp, (const uint2*)(h->d_cand_tiles + c.t0), n_tiles, (const uint32_t*)(h->d_cand_col + c.p0), (const float*)h->d_zeval,
                (const float*)h->dec(), (const float*)h->P(CDAE_P_BP), h->d_cand_score);
    if (out_ranks)
      hipLaunchKernelGGL(cdae::rank_rows_kernel, dim3((uint32_t)(c.rb - c.ra)), dim3(256), 0, h->stream, (const int64_t*)h->d_cand_ptr, c.ra, c.p0,
                         (int64_t)n_cand, (const float*)h->d_cand_score, h->d_cand_rank);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_scores + c.p0, h->d_cand_score, n_cand * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (out_ranks) HIPCHK(hipMemcpyAsync(out_ranks + c.p0, h->d_cand_rank, n_cand * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));                                                 // one per chunk: the buffers are the next chunk's too
  }
  return 0;
}
}  // namespace

// ---- exact full-catalogue ranks of named items (cdae_hip_full_rank_rows) -----------------------------------------------------------
namespace {
// Chunks: real rows as for the other rows entry points (EVAL_CHUNK on the matrix cores, score_place's bound on the general path), and
// closed early once they hold FR_TARGET_CHUNK targets, which bounds the per-chunk score / rank buffers (one row may still name every
// unrated item: a chunk always takes at least one row).  Matrix-core path: a row with n targets is ceil(n / FR_WINDOW) virtual rows in
// the call's table, and one counting launch takes at most FR_COLS_MAX of them — a row with more is cut across launches that share its z.
constexpr int64_t FR_TARGET_CHUNK = 1 << 22;
constexpr uint32_t FR_COLS_MAX = EVAL_CHUNK;
static_assert(EVAL_CHUNK <= 65536, "a virtual row names its row's slot in 16 bits");
struct FrChunk { uint64_t c0; uint32_t nu; int64_t p0, p1; size_t v0, v1; };

void full_rank_plan(uint64_t R, const int64_t* tp, uint32_t rows_max, bool mfma, std::vector<uint2>& vrows, std::vector<FrChunk>& chunks) {
  vrows.clear(); chunks.clear();
  uint64_t c0 = 0;
  while (c0 < R) {
    FrChunk c{c0, 0, tp[c0], tp[c0], vrows.size(), vrows.size()};
    while (c.c0 + c.nu < R && c.nu < rows_max) {
      const uint64_t r = c.c0 + c.nu;
      const int64_t n = tp[r + 1] - tp[r];
      if (c.nu && (c.p1 - c.p0) + n > FR_TARGET_CHUNK) break;
      if (mfma)
        for (int64_t w = 0; w < n; w += cdae::FR_WINDOW)
          vrows.push_back(make_uint2(c.nu | (uint32_t)(std::min<int64_t>(cdae::FR_WINDOW, n - w) - 1) << 16, (uint32_t)(tp[r] + w - c.p0)));
      c.p1 = tp[r + 1];
      ++c.nu;
    }
    c.v1 = vrows.size();
    chunks.push_back(c);
    c0 += c.nu;
  }
}

template <int NCH>
int launch_full_rank_mfma_as(cdae_hip* h, const FrChunk& c, uint32_t words) {
  const size_t lds = cdae::recommend_mfma_lds_bytes(NCH);
  const float* D = (const float*)h->dec();
  const float* bp = (const float*)h->P(CDAE_P_BP);
  const uint32_t* tcol = h->d_fr_tcol + c.p0;
  HIPCHK(hipFuncSetAttribute((const void*)cdae::full_rank_mfma_kernel<NCH, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  HIPCHK(hipFuncSetAttribute((const void*)cdae::full_rank_mfma_kernel<NCH, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // pass 0: the scores of the targets, a column per row of the chunk
  hipLaunchKernelGGL((cdae::full_rank_mfma_kernel<NCH, 0>), dim3((c.nu + cdae::REC_USERS_PER_BLOCK - 1) / cdae::REC_USERS_PER_BLOCK), dim3(256), lds,
                     h->stream, h->hp, (const float*)h->d_zeval, c.nu, (const uint2*)nullptr, D, bp, (const uint32_t*)h->d_fr_tbits, words,
                     (const int64_t*)h->d_fr_tptr, c.c0, c.p0, tcol, h->d_fr_tscore, (uint32_t*)nullptr);
  // pass 1: the counts, a column per virtual row
  for (size_t v = c.v0; v < c.v1; v += FR_COLS_MAX) {
    const uint32_t ncol = (uint32_t)std::min<size_t>(FR_COLS_MAX, c.v1 - v);
    hipLaunchKernelGGL((cdae::full_rank_mfma_kernel<NCH, 1>), dim3((ncol + cdae::REC_USERS_PER_BLOCK - 1) / cdae::REC_USERS_PER_BLOCK), dim3(256), lds,
                       h->stream, h->hp, (const float*)h->d_zeval, ncol, (const uint2*)(h->d_fr_vrows + v), D, bp, (const uint32_t*)h->d_bits, words,
                       (const int64_t*)nullptr, c.c0, c.p0, tcol, h->d_fr_tscore, h->d_fr_rank);
  }
  return 0;
}
int launch_full_rank_mfma(cdae_hip* h, const FrChunk& c, uint32_t words) {
  return dispatch_nch(h->K, [&](auto nch) { return launch_full_rank_mfma_as<decltype(nch)::value>(h, c, words); });
}

int full_rank_run(cdae_hip* h, uint64_t R, const uint32_t* uids, const int64_t* row_ptr, const uint32_t* col, const int64_t* tp,
                  const uint32_t* tc, uint32_t* out_ranks, float* out_scores) {
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  CHK(rows_upload(h, R, uids, row_ptr, col));
  const bool mfma = h->K <= 256;
  const uint32_t words = (uint32_t)((h->I + 31) / 32);
  const ScorePlace sp = score_place(h->I, 4096u);                  // general path: recommend_kernel's placement of a row's scores
  std::vector<FrChunk> chunks;
  full_rank_plan(R, tp, mfma ? EVAL_CHUNK : sp.rows, mfma, h->h_fr_vrows, chunks);
  size_t rows_cap = 0, targets_cap = 0;
  for (const FrChunk& c : chunks)
    if (c.p1 > c.p0) { rows_cap = std::max<size_t>(rows_cap, c.nu); targets_cap = std::max<size_t>(targets_cap, (size_t)(c.p1 - c.p0)); }
  CHK(upload_csr(h, h->d_fr_tptr, h->d_fr_tcol, tp, tc, R));
  CHK(h->d_fr_tscore.ensure(targets_cap));
  CHK(h->d_fr_rank.ensure(targets_cap));
  CHK(h->d_zeval.ensure(rows_cap, h->Kp));
  if (mfma) {
    CHK(h->d_bits.ensure(rows_cap * words));
    CHK(h->d_fr_tbits.ensure(rows_cap * words));
    CHK(h->d_fr_vrows.ensure(h->h_fr_vrows.size()));
    HIPCHK(hipMemcpyAsync(h->d_fr_vrows, h->h_fr_vrows.data(), h->h_fr_vrows.size() * sizeof(uint2), hipMemcpyHostToDevice, h->stream));
  } else {
    if (!sp.in_lds) CHK(h->d_score.ensure(rows_cap * h->I));
    const void* kernel = dispatch_ni(h->NI, [](auto ni) { return (const void*)cdae::full_rank_general_kernel<decltype(ni)::value>; });
    HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sp.shmem));
  }
  for (const FrChunk& c : chunks) {
    if (c.p1 == c.p0) continue;                                    // no row of the chunk has targets: nothing to launch, nothing to write
    const size_t nt = (size_t)(c.p1 - c.p0);
    CHK(rows_encode_chunk(h, row_ptr, c.c0, c.nu));
    if (mfma) {
      hipLaunchKernelGGL(cdae::rated_bits_kernel, dim3((c.nu + 3) / 4), dim3(256), 0, h->stream, (const int64_t*)h->d_rows_ptr,
                         (const uint32_t*)h->d_rows_col, c.c0, c.nu, words, h->d_bits);
      hipLaunchKernelGGL(cdae::rated_bits_kernel, dim3((c.nu + 3) / 4), dim3(256), 0, h->stream, (const int64_t*)h->d_fr_tptr,
                         (const uint32_t*)h->d_fr_tcol, c.c0, c.nu, words, h->d_fr_tbits);
      CHK(launch_full_rank_mfma(h, c, words));
    } else {
      DISPATCH_NI(h->NI, cdae::full_rank_general_kernel, dim3(c.nu), dim3(256), sp.shmem, h->stream, h->hp, (const int64_t*)h->d_rows_ptr,
                  (const uint32_t*)h->d_rows_col, (const int64_t*)h->d_fr_tptr, (const uint32_t*)h->d_fr_tcol, c.c0, c.p0, (const float*)h->d_zeval,
                  (const float*)h->dec(), (const float*)h->P(CDAE_P_BP), sp.in_lds ? (float*)nullptr : h->d_score.p, h->d_fr_tscore, h->d_fr_rank);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_ranks + c.p0, h->d_fr_rank, nt * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (out_scores) HIPCHK(hipMemcpyAsync(out_scores + c.p0, h->d_fr_tscore, nt * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));                                                 // one per chunk: the buffers are the next chunk's too
  }
  return 0;
}
}  // namespace

// ---- fold-in of user nodes for rows outside the training set (cdae_hip_fold_in_rows) and the guest table ------------------------------
namespace {
constexpr float NODE_INIT[4] = {0.f, cdae::FOLD_AG_INIT, 1.f, cdae::FOLD_AG_INIT};     // wu | wu_ag | uu | uu_ag of a row without a node
int fold_check(cdae_hip* h, const char* fn) {
  if (!h) return fail("%s: null handle", fn);
  if (h->mf == 5u) return fail("%s: %s; there is nothing to fit", fn, FISM_NO_NODE);
  if (h->mf) return fail("%s does not apply to an IMF / BPR handle (its users are trained rows, not input nodes)", fn);
  if (h->item_shard) return fail("%s applies to a whole model, not to an item shard", fn);
  if (!h->d_shared) return fail("%s: cdae_hip_set_interactions first", fn);
  if (h->cfg.full_output) return fail("%s: a full_output handle decodes densely; a dense fold-in is not implemented", fn);
  if (!h->cfg.user_factor && !h->cfg.linear_function)
    return fail("%s: the handle has neither user_factor nor linear_function: there is no user node to fit", fn);
  return 0;
}
int guest_table_check(cdae_hip* h, const char* fn, uint64_t n) {
  if (h->U > GUEST_USERS_MAX) return fail("%s: a handle with %llu users has no room for guest ids (at most %llu users)", fn, (unsigned long long)h->U, (unsigned long long)GUEST_USERS_MAX);
  if (n > GUEST_USERS_MAX) return fail("%s: at most %llu guest nodes, got %llu", fn, (unsigned long long)GUEST_USERS_MAX, (unsigned long long)n);
  return 0;
}
int ensure_nodes(cdae_hip* h, DevBuf<float> (&b)[4], size_t rows) {
  for (int k = 0; k < 4; ++k) CHK(b[k].ensure(rows, h->Kp));
  return 0;
}
void install_staged(cdae_hip* h, uint64_t n) {       // the staging rows become the table (and the old table the next call's staging rows)
  std::swap(h->d_guest, h->d_fold);
  h->n_guests = n;
}
struct FoldCall {
  uint64_t seed; uint32_t epoch_begin, n_epochs; uint64_t stream_id_base; bool install;
  float* out[4];
};
int fold_run(cdae_hip* h, uint64_t R, const uint32_t* uids, const int64_t* row_ptr, const uint32_t* col, const FoldCall& f) {
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  CHK(rows_upload(h, R, uids, row_ptr, col));
  const uint32_t UC = (uint32_t)std::min<uint64_t>(R, EVAL_CHUNK);
  CHK(ensure_nodes(h, h->d_fold, f.install ? (size_t)R : (size_t)UC));
  // the long rows of every chunk, as slots inside their chunk: they take the leading workgroups of the chunk's launch
  std::vector<size_t>& long_off = h->h_fold_long_off;
  long_off.clear();
  h->h_fold_long.clear();
  for (uint64_t c0 = 0; c0 < R; c0 += UC) {
    long_off.push_back(h->h_fold_long.size());
    for (uint64_t r = c0; r < std::min<uint64_t>(R, c0 + UC); ++r)
      if (cdae::fold_row_is_long((uint64_t)(row_ptr[r + 1] - row_ptr[r]), h->hp.num_neg)) h->h_fold_long.push_back((uint32_t)(r - c0));
  }
  long_off.push_back(h->h_fold_long.size());
  CHK(h->d_fold_long.ensure(std::max<size_t>(h->h_fold_long.size(), 1)));
  if (!h->h_fold_long.empty())
    HIPCHK(hipMemcpyAsync(h->d_fold_long, h->h_fold_long.data(), h->h_fold_long.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  const cdae::FoldArgs a{f.seed, f.stream_id_base, f.epoch_begin, f.n_epochs, h->cfg.num_corruptions};
  const bool g = h->n_guests != 0;
  const cdae::FoldNodes nd{h->d_Wu, h->d_Wu_ag, h->d_Uu, h->d_Uu_ag, g ? h->d_guest[0].p : nullptr, g ? h->d_guest[1].p : nullptr,
                           g ? h->d_guest[2].p : nullptr, g ? h->d_guest[3].p : nullptr};
  size_t chunk = 0;
  for (uint64_t c0 = 0; c0 < R; c0 += UC, ++chunk) {
    const uint32_t nu = (uint32_t)std::min<uint64_t>(UC, R - c0);
    const uint32_t n_long = (uint32_t)(long_off[chunk + 1] - long_off[chunk]);
    const size_t so = f.install ? (size_t)c0 * h->Kp : 0;          // an installing call keeps every chunk: the table changes after the last one
    const cdae::FoldOut out{h->d_fold[0] + so, h->d_fold[1] + so, h->d_fold[2] + so, h->d_fold[3] + so};
    DISPATCH_NI(h->NI, cdae::fold_in_rows_kernel, dim3(n_long + (nu + cdae::FOLD_WAVES - 1) / cdae::FOLD_WAVES), dim3(cdae::FOLD_WAVES * cdae::WAVE), 0,
                h->stream, h->hp, a, (const int64_t*)h->d_rows_ptr, (const uint32_t*)h->d_rows_col, (const uint32_t*)h->d_rows_uid, c0, nu,
                (const uint32_t*)(h->d_fold_long + long_off[chunk]), n_long, (const float*)h->P(CDAE_P_W), (const float*)h->dec(),
                (const float*)h->P(CDAE_P_B), (const float*)h->P(CDAE_P_BP), nd, out);
    HIPCHK(hipGetLastError());
    const float* src[4] = {out.wu, out.wu_ag, out.uu, out.uu_ag};
    for (int k = 0; k < 4; ++k)
      if (f.out[k])
        HIPCHK(hipMemcpy2DAsync(f.out[k] + (size_t)c0 * h->K, h->K * sizeof(float), src[k], h->Kp * sizeof(float), h->K * sizeof(float), nu,
                                hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));                         // one per chunk: the staging rows are the next chunk's too
  }
  if (f.install) install_staged(h, R);
  return 0;
}
}  // namespace

extern "C" {

int cdae_hip_fold_in_rows(cdae_hip_t* h, uint64_t n_rows, const uint32_t* uids, const int64_t* row_ptr, const uint32_t* col, uint64_t seed,
                          uint32_t epoch_begin, uint32_t n_epochs, uint64_t stream_id_base, int install, float* out_wu, float* out_wu_ag,
                          float* out_uu, float* out_uu_ag) {
  const char* fn = "cdae_hip_fold_in_rows";
  CHK(fold_check(h, fn));
  if (install) CHK(guest_table_check(h, fn, n_rows));
  if (n_rows == 0) {
    if (install) h->n_guests = 0;
    return 0;
  }
  CHK(validate_rows_csr("fold-in", row_ptr, col, n_rows, h->I));
  CHK(rows_check_uids(h, fn, uids, n_rows));
  for (uint64_t r = 0; r < n_rows; ++r)
    if ((uint64_t)(row_ptr[r + 1] - row_ptr[r]) >= h->I)
      return fail("%s: row %llu holds all %llu items: the negative sampler needs an unrated one", fn, (unsigned long long)r, (unsigned long long)h->I);
  const FoldCall f{seed, epoch_begin, n_epochs, stream_id_base, install != 0, {out_wu, out_wu_ag, out_uu, out_uu_ag}};
  return fold_run(h, n_rows, uids, row_ptr, col, f);
}

int cdae_hip_set_guest_nodes(cdae_hip_t* h, uint64_t n_guests, const float* wu, const float* wu_ag, const float* uu, const float* uu_ag) {
  const char* fn = "cdae_hip_set_guest_nodes";
  CHK(fold_check(h, fn));
  CHK(guest_table_check(h, fn, n_guests));
  if (n_guests == 0) { h->n_guests = 0; return 0; }
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  CHK(ensure_nodes(h, h->d_fold, (size_t)n_guests));
  const float* host[4] = {wu, wu_ag, uu, uu_ag};
  const size_t count = (size_t)n_guests * h->Kp;
  for (int k = 0; k < 4; ++k) {
    hipLaunchKernelGGL(cdae::fold_fill_kernel, dim3((uint32_t)std::min<size_t>((count + 255) / 256, 4096)), dim3(256), 0, h->stream, h->d_fold[k], count,
                       NODE_INIT[k]);
    HIPCHK(hipGetLastError());
    if (host[k])
      HIPCHK(hipMemcpy2DAsync(h->d_fold[k], h->Kp * sizeof(float), host[k], h->K * sizeof(float), h->K * sizeof(float), n_guests,
                              hipMemcpyHostToDevice, h->stream));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  install_staged(h, n_guests);
  return 0;
}

uint64_t cdae_hip_guest_nodes(const cdae_hip_t* h) { return h ? h->n_guests : 0; }

}  // extern "C"

extern "C" {

int cdae_hip_score_rows(cdae_hip_t* h, uint64_t n_rows, const uint32_t* uids, const int64_t* row_ptr, const uint32_t* col,
                        const int64_t* cand_row_ptr, const uint32_t* cand_col, float* out_scores, uint32_t* out_ranks) {
  const RowsArgs a{n_rows, uids, row_ptr, col, nullptr, nullptr, 0, 1, nullptr, nullptr};
  CHK(rows_check(h, "cdae_hip_score_rows", a));
  if (n_rows == 0) return 0;
  CHK(validate_rows_csr("candidate", cand_row_ptr, cand_col, n_rows, h->I));
  if (cand_row_ptr[n_rows] == 0) return 0;
  if (!out_scores) return fail("cdae_hip_score_rows: null out_scores with %lld candidates", (long long)cand_row_ptr[n_rows]);
  if (out_ranks)
    for (uint64_t r = 0; r < n_rows; ++r)
      if (cand_row_ptr[r + 1] - cand_row_ptr[r] > (int64_t)CDAE_RANK_CANDIDATES_MAX)
        return fail("cdae_hip_score_rows: candidate row %llu has %lld candidates, ranks are computed for rows of at most %u", (unsigned long long)r,
                    (long long)(cand_row_ptr[r + 1] - cand_row_ptr[r]), CDAE_RANK_CANDIDATES_MAX);
  return score_run(h, n_rows, uids, row_ptr, col, cand_row_ptr, cand_col, out_scores, out_ranks);
}

int cdae_hip_full_rank_rows(cdae_hip_t* h, uint64_t n_rows, const uint32_t* uids, const int64_t* row_ptr, const uint32_t* col,
                            const int64_t* target_row_ptr, const uint32_t* target_col, uint32_t* out_ranks, float* out_scores) {
  const RowsArgs a{n_rows, uids, row_ptr, col, nullptr, nullptr, 0, 1, nullptr, nullptr};
  CHK(rows_check(h, "cdae_hip_full_rank_rows", a));
  if (n_rows == 0) return 0;
  CHK(validate_rows_csr("target", target_row_ptr, target_col, n_rows, h->I));
  if (target_row_ptr[n_rows] == 0) return 0;
  if (!out_ranks) return fail("cdae_hip_full_rank_rows: null out_ranks with %lld targets", (long long)target_row_ptr[n_rows]);
  for (uint64_t r = 0; r < n_rows; ++r) {                          // a rated item has no place in the list (both rows ascend: one merge walk)
    int64_t p = row_ptr[r];
    const int64_t pe = row_ptr[r + 1];
    for (int64_t q = target_row_ptr[r]; q < target_row_ptr[r + 1] && p < pe; ++q) {
      while (p < pe && col[p] < target_col[q]) ++p;
      if (p < pe && col[p] == target_col[q])
        return fail("cdae_hip_full_rank_rows: target row %llu names item %u, which is one of the row's rated items", (unsigned long long)r, target_col[q]);
    }
  }
  return full_rank_run(h, n_rows, uids, row_ptr, col, target_row_ptr, target_col, out_ranks, out_scores);
}

int cdae_hip_recommend_rows(cdae_hip_t* h, uint64_t n_rows, const uint32_t* uids, const int64_t* row_ptr, const uint32_t* col,
                            uint32_t topk, uint32_t* out_ids, float* out_scores) {
  const RowsArgs a{n_rows, uids, row_ptr, col, nullptr, nullptr, 0, topk, out_ids, out_scores};
  CHK(rows_check(h, "cdae_hip_recommend_rows", a));
  if (n_rows == 0) return 0;
  if (!out_ids) return fail("cdae_hip_recommend_rows: null out_ids");
  return rows_run(h, a);
}

int cdae_hip_recommend_rows_filtered(cdae_hip_t* h, uint64_t n_rows, const uint32_t* uids, const int64_t* row_ptr, const uint32_t* col,
                                     const int64_t* excl_row_ptr, const uint32_t* excl_col, int exclude_rated,
                                     const uint32_t* allow_items, uint64_t n_allow, uint32_t topk, uint32_t* out_ids, float* out_scores) {
  const char* fn = "cdae_hip_recommend_rows_filtered";
  const RowsArgs a{n_rows, uids, row_ptr, col, nullptr, nullptr, 0, topk, out_ids, out_scores};
  CHK(rows_check(h, fn, a));
  CHK(validate_allow(fn, allow_items, n_allow, h->I));
  if (n_rows == 0) return 0;
  if (excl_row_ptr) CHK(validate_rows_csr("excl", excl_row_ptr, excl_col, n_rows, h->I));
  if (!out_ids) return fail("%s: null out_ids", fn);
  return rows_run(h, a, FilterArgs{excl_row_ptr, excl_col, exclude_rated != 0, allow_items, n_allow});
}

int cdae_hip_similar_items(cdae_hip_t* h, uint64_t n_queries, const uint32_t* query_items, uint32_t table, uint32_t metric, int exclude_self,
                           const int64_t* excl_row_ptr, const uint32_t* excl_col, const uint32_t* allow_items, uint64_t n_allow,
                           uint32_t topk, uint32_t* out_ids, float* out_scores) {
  const char* fn = "cdae_hip_similar_items";
  if (!h) return fail("%s: null handle", fn);
  if (h->item_shard) return fail("%s applies to a whole model, not to an item shard", fn);
  if (!h->d_shared) return fail("%s: cdae_hip_set_interactions first", fn);
  if (table != CDAE_ITEMS_OUTPUT && table != CDAE_ITEMS_INPUT) return fail("%s: unknown table %u", fn, table);
  if (metric != CDAE_SIM_DOT && metric != CDAE_SIM_COSINE) return fail("%s: unknown metric %u", fn, metric);
  if (topk == 0 || topk > h->I) return fail("%s: topk must be in [1, num_items]", fn);
  CHK(validate_allow(fn, allow_items, n_allow, h->I));
  if (n_queries == 0) return 0;
  if (!query_items) return fail("%s: null query_items", fn);
  for (uint64_t q = 0; q < n_queries; ++q)
    if (query_items[q] >= h->I) return fail("%s: query_items[%llu] = %u is out of range", fn, (unsigned long long)q, query_items[q]);
  if (excl_row_ptr) CHK(validate_rows_csr("excl", excl_row_ptr, excl_col, n_queries, h->I));
  if (!out_ids) return fail("%s: null out_ids", fn);
  // on an IMF / BPR handle the item factors are the one item table (CDAE_P_W); dec() is that table there
  const float* T = table == CDAE_ITEMS_INPUT ? h->P(CDAE_P_W) : h->dec();
  const SimilarArgs a{n_queries, query_items, T, metric == CDAE_SIM_COSINE, exclude_self != 0, topk, out_ids, out_scores};
  return similar_run(h, a, FilterArgs{excl_row_ptr, excl_col, false, allow_items, n_allow});
}

}  // extern "C"

// ---- WRMF by alternating least squares (cdae_als_kernels.hpp) ------------------------------------------------------
namespace {
// G = T^T T of `rows` rows into G (h->d_als_G; cdae_hip_als_objective's second Gram: h->d_als_G2): per-slice partials, then the fold
// in slice order
int als_gram(cdae_hip* h, const float* T, uint64_t rows, DevBuf<float>& G) {
  const uint32_t Kp = h->Kp, slices = cdae::als_gram_slices(rows), tiles = Kp / 32u;
  CHK(G.ensure((size_t)Kp * Kp));
  CHK(h->d_als_part.ensure((size_t)cdae::ALS_GRAM_SLICES_MAX * Kp * Kp));
  hipLaunchKernelGGL(cdae::als_gram_kernel, dim3(tiles * tiles, slices), dim3(64), 0, h->stream, T, rows, Kp, (float*)h->d_als_part);
  hipLaunchKernelGGL(cdae::als_gram_fold_kernel, dim3((Kp * Kp + 255u) / 256u), dim3(256), 0, h->stream, (const float*)h->d_als_part, slices,
                     Kp * Kp, (float*)G);
  HIPCHK(hipGetLastError());
  return 0;
}
int als_gram(cdae_hip* h, const float* T, uint64_t rows) { return als_gram(h, T, rows, h->d_als_G); }
// n rows of the CSR (ptr, col) solved against the table Y and h->d_als_G, 32 rows per workgroup; w: one confidence weight per entry
// of col, or null for the binary kernel
int als_solve(cdae_hip* h, const int64_t* ptr, const uint32_t* col, const float* w, uint64_t n, const float* Y, const float* x0, float* dst,
              uint32_t steps) {
  return dispatch_ni(h->NI, [&](auto ni) {
    constexpr int NI = decltype(ni)::value;
    constexpr size_t lds = cdae::als_solve_lds_bytes<NI>();
    const dim3 grid((uint32_t)((n + cdae::ALS_BLOCK_ROWS - 1) / cdae::ALS_BLOCK_ROWS)), block(cdae::als_waves<NI>() * 64);
    const void* const kernel = w ? (const void*)cdae::als_solve_kernel<NI, true> : (const void*)cdae::als_solve_kernel<NI, false>;
    HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (w) hipLaunchKernelGGL((cdae::als_solve_kernel<NI, true>), grid, block, lds, h->stream, ptr, col, n, Y, (const float*)h->d_als_G, x0, dst,
                              h->als_alpha, h->als_lambda, steps, w);
    else hipLaunchKernelGGL((cdae::als_solve_kernel<NI, false>), grid, block, lds, h->stream, ptr, col, n, Y, (const float*)h->d_als_G, x0, dst,
                            h->als_alpha, h->als_lambda, steps, (const float*)nullptr);
    HIPCHK(hipGetLastError());
    return 0;
  });
}
int als_check(cdae_hip* h, const char* fn) {
  if (!h) return fail("%s: null handle", fn);
  if (h->mf != 3u) return fail("%s applies to a WRMF handle (cdae_hip_create_als)", fn);
  if (!h->d_shared) return fail("%s: cdae_hip_set_interactions first", fn);
  return 0;
}
// one half-step, enqueued on h->stream: the side's rows in place against the other side's table
int als_half_step(cdae_hip* h, uint32_t side) {
  float* X = h->d_Wu; float* Y = h->P(CDAE_P_W);
  if (side == CDAE_ALS_USERS) {
    CHK(als_gram(h, Y, h->I));
    return als_solve(h, h->d_row_ptr, h->d_col, h->d_als_w, h->U, Y, X, X, h->als_steps);
  }
  CHK(als_gram(h, X, h->U));
  return als_solve(h, h->d_tptr, h->d_tcol, h->d_als_tw, h->I, X, Y, Y, h->als_steps);
}
constexpr uint64_t ALS_ROWS_CHUNK = 32768;
}  // namespace

extern "C" {

int cdae_hip_als_half_step(cdae_hip_t* h, uint32_t side) {
  CHK(als_check(h, "cdae_hip_als_half_step"));
  if (side != CDAE_ALS_USERS && side != CDAE_ALS_ITEMS) return fail("cdae_hip_als_half_step: side must be CDAE_ALS_USERS or CDAE_ALS_ITEMS");
  HIPCHK(hipSetDevice(h->device));
  CHK(als_half_step(h, side));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// ---- WARP (cdae_warp_kernels.hpp) ---------------------------------------------------------------------------------------
constexpr uint32_t WARP_SEARCH_CHUNK = 8192;      // users (one wavefront each) per launch of cdae_hip_warp_search
static int warp_check(cdae_hip* h, const char* fn) {
  if (!h || !h->d_shared) return fail("set_interactions must be called first");
  if (h->mf != 4u) return fail("%s applies to a WARP handle (cdae_hip_create_warp)", fn);
  return 0;
}

int cdae_hip_warp_search(cdae_hip_t* h, uint64_t seed, uint32_t epoch, uint64_t pos_begin, uint64_t pos_end, uint32_t* out_item,
                         uint32_t* out_cnt, float* out_margin, size_t count) {
  const char* fn = "cdae_hip_warp_search";
  CHK(warp_check(h, fn));
  if (pos_begin > pos_end || pos_end > h->U) return fail("%s: bad range of positions [%llu, %llu)", fn, (unsigned long long)pos_begin, (unsigned long long)pos_end);
  const uint64_t pairs = cdae::warp_pair_count(h->h_row_ptr.data(), pos_begin, pos_end, h->hp.num_neg);
  if (count != pairs) return fail("%s: the range holds %llu pairs, the caller's arrays %zu", fn, (unsigned long long)pairs, count);
  if (pairs && (!out_item || !out_cnt)) return fail("%s: null argument", fn);
  if (pairs == 0) return 0;
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  // the outputs of the largest chunk
  uint64_t chunk_pairs = 0;
  for (uint64_t c0 = pos_begin; c0 < pos_end; c0 += WARP_SEARCH_CHUNK)
    chunk_pairs = std::max(chunk_pairs, cdae::warp_pair_count(h->h_row_ptr.data(), c0, std::min<uint64_t>(c0 + WARP_SEARCH_CHUNK, pos_end), h->hp.num_neg));
  CHK(h->d_warp_out_item.ensure(chunk_pairs)); CHK(h->d_warp_out_cnt.ensure(chunk_pairs));
  if (out_margin) CHK(h->d_warp_out_margin.ensure(chunk_pairs));
  for (uint64_t c0 = pos_begin; c0 < pos_end; c0 += WARP_SEARCH_CHUNK) {
    const uint32_t nu = (uint32_t)std::min<uint64_t>(WARP_SEARCH_CHUNK, pos_end - c0);
    const uint64_t np = cdae::warp_pair_count(h->h_row_ptr.data(), c0, c0 + nu, h->hp.num_neg);
    if (np == 0) continue;
    const uint64_t q0 = cdae::warp_pair_count(h->h_row_ptr.data(), pos_begin, c0, h->hp.num_neg);
    DISPATCH_NI(h->NI, cdae::warp_search_kernel, dim3((nu + 3) / 4), dim3(256), 0, h->stream, h->hp, (const int64_t*)h->d_row_ptr,
                (const uint32_t*)h->d_col, c0, nu, (int64_t)h->h_row_ptr[c0], seed, epoch, (const float*)h->d_Wu, (const float*)h->P(CDAE_P_W),
                (const float*)h->P(CDAE_P_BP), h->d_warp_out_item.p, h->d_warp_out_cnt.p, out_margin ? h->d_warp_out_margin.p : (float*)nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_item + q0, h->d_warp_out_item, np * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(out_cnt + q0, h->d_warp_out_cnt, np * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (out_margin) HIPCHK(hipMemcpyAsync(out_margin + q0, h->d_warp_out_margin, np * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));            // the next chunk writes the same buffers
  }
  return 0;
}

int cdae_hip_warp_record_choices(cdae_hip_t* h, uint32_t on) {
  CHK(warp_check(h, "cdae_hip_warp_record_choices"));
  HIPCHK(hipSetDevice(h->device));
  if (on && !h->d_warp_rec_item) {
    const size_t n = (size_t)cdae::warp_pair_count(h->h_row_ptr.data(), 0, h->U, h->hp.num_neg);
    CHK(h->d_warp_rec_item.alloc(n)); CHK(h->d_warp_rec_cnt.alloc(n));
    HIPCHK(hipMemsetAsync(h->d_warp_rec_item, 0xFF, std::max<size_t>(n, 1) * sizeof(uint32_t), h->stream));
    HIPCHK(hipMemsetAsync(h->d_warp_rec_cnt, 0, std::max<size_t>(n, 1) * sizeof(uint32_t), h->stream));
  }
  h->warp_record = on != 0;
  return 0;
}

int cdae_hip_warp_choices(cdae_hip_t* h, uint32_t* out_item, uint32_t* out_cnt, size_t count) {
  const char* fn = "cdae_hip_warp_choices";
  CHK(warp_check(h, fn));
  if (!h->d_warp_rec_item) return fail("%s: nothing has been recorded (cdae_hip_warp_record_choices)", fn);
  const size_t n = (size_t)cdae::warp_pair_count(h->h_row_ptr.data(), 0, h->U, h->hp.num_neg);
  if (count != n) return fail("%s: the record holds %zu pairs, the caller's arrays %zu", fn, n, count);
  if (n && (!out_item || !out_cnt)) return fail("%s: null argument", fn);
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpyAsync(out_item, h->d_warp_rec_item, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(out_cnt, h->d_warp_rec_cnt, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// ---- FISM (cdae_fism_kernels.hpp) ---------------------------------------------------------------------------------------
int cdae_hip_fism_plan(const cdae_hip_t* h, uint32_t* resident_rows, uint64_t* window_instances) {
  if (!h) return fail("null handle");
  if (h->mf != 5u) return fail("cdae_hip_fism_plan applies to a FISM handle (cdae_hip_create_fism)");
  if (resident_rows) *resident_rows = h->d_shared ? cdae::fism_resident_rows(h->NI, h->fism_resident) : 0u;
  if (window_instances) *window_instances = cdae::FISM_WINDOW_INSTANCES;
  return 0;
}

int cdae_hip_fism_set_resident(cdae_hip_t* h, int allow) {
  if (!h) return fail("null handle");
  if (h->mf != 5u) return fail("cdae_hip_fism_set_resident applies to a FISM handle (cdae_hip_create_fism)");
  h->fism_resident = allow != 0;
  return 0;
}

int cdae_hip_als_gram(cdae_hip_t* h, uint32_t side, float* out, size_t count) {
  CHK(als_check(h, "cdae_hip_als_gram"));
  if (side != CDAE_ALS_USERS && side != CDAE_ALS_ITEMS) return fail("cdae_hip_als_gram: side must be CDAE_ALS_USERS or CDAE_ALS_ITEMS");
  if (!out || count != (size_t)h->K * h->K) return fail("cdae_hip_als_gram: out must hold num_dim x num_dim = %zu floats, got %zu", (size_t)h->K * h->K, count);
  HIPCHK(hipSetDevice(h->device));
  CHK(side == CDAE_ALS_USERS ? als_gram(h, h->d_Wu, h->U) : als_gram(h, h->P(CDAE_P_W), h->I));
  HIPCHK(hipMemcpy2DAsync(out, h->K * sizeof(float), h->d_als_G, h->Kp * sizeof(float), h->K * sizeof(float), h->K, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

static int als_solve_rows(cdae_hip* h, const char* fn, uint64_t n_rows, const int64_t* row_ptr, const uint32_t* col, const float* w,
                          const float* x0, uint32_t cg_steps, float* out_x) {
  CHK(als_check(h, fn));
  if (n_rows == 0) return 0;
  CHK(validate_rows_csr("rated", row_ptr, col, n_rows, h->I));
  if (!out_x) return fail("%s: null out_x", fn);
  const size_t nnz = (size_t)row_ptr[n_rows];
  if (w) {
    const std::string refusal = cdae::plan::check_weights(w, nnz);
    if (!refusal.empty()) return fail("%s: %s", fn, refusal.c_str());
  }
  HIPCHK(hipSetDevice(h->device));
  const uint32_t steps = cg_steps ? cg_steps : h->als_steps;
  const size_t chunk = (size_t)std::min<uint64_t>(n_rows, ALS_ROWS_CHUNK);
  CHK(upload_csr(h, h->d_rows_ptr, h->d_rows_col, row_ptr, col, n_rows));
  if (w) {
    CHK(h->d_als_rw.ensure(std::max<size_t>(nnz, 1)));
    if (nnz) HIPCHK(hipMemcpyAsync(h->d_als_rw, w, nnz * sizeof(float), hipMemcpyHostToDevice, h->stream));
  }
  CHK(h->d_als_out.ensure(chunk * h->Kp));
  if (x0) CHK(h->d_als_x.ensure(chunk * h->Kp));
  const float* Y = h->P(CDAE_P_W);
  CHK(als_gram(h, Y, h->I));
  const size_t wK = h->K * sizeof(float), wKp = h->Kp * sizeof(float);
  for (uint64_t c0 = 0; c0 < n_rows; c0 += ALS_ROWS_CHUNK) {
    const uint64_t nu = std::min<uint64_t>(ALS_ROWS_CHUNK, n_rows - c0);
    if (x0) {                                               // (pad lanes zero: the kernel relies on it)
      HIPCHK(hipMemsetAsync(h->d_als_x, 0, nu * wKp, h->stream));
      HIPCHK(hipMemcpy2DAsync(h->d_als_x, wKp, x0 + c0 * h->K, wK, wK, nu, hipMemcpyHostToDevice, h->stream));
    }
    CHK(als_solve(h, h->d_rows_ptr.p + c0, h->d_rows_col.p, w ? (const float*)h->d_als_rw.p : nullptr, nu, Y,
                  x0 ? (const float*)h->d_als_x.p : nullptr, h->d_als_out.p, steps));
    HIPCHK(hipMemcpy2DAsync(out_x + c0 * h->K, wK, h->d_als_out, wKp, wK, nu, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));                // the two chunk buffers are the next chunk's too
  }
  return 0;
}

int cdae_hip_als_solve_rows(cdae_hip_t* h, uint64_t n_rows, const int64_t* row_ptr, const uint32_t* col, const float* x0,
                            uint32_t cg_steps, float* out_x) {
  return als_solve_rows(h, "cdae_hip_als_solve_rows", n_rows, row_ptr, col, nullptr, x0, cg_steps, out_x);
}

int cdae_hip_als_solve_rows_weighted(cdae_hip_t* h, uint64_t n_rows, const int64_t* row_ptr, const uint32_t* col, const float* w,
                                     const float* x0, uint32_t cg_steps, float* out_x) {
  return als_solve_rows(h, "cdae_hip_als_solve_rows_weighted", n_rows, row_ptr, col, w, x0, cg_steps, out_x);
}

int cdae_hip_als_set_confidence(cdae_hip_t* h, const float* w, size_t count) {
  const char* fn = "cdae_hip_als_set_confidence";
  CHK(als_check(h, fn));
  const size_t nnz = (size_t)h->h_row_ptr[h->U];
  if (!w && count == 0) {                                   // back to binary
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    CHK(h->d_als_w.drop());
    return h->d_als_tw.drop();
  }
  if (!w) return fail("%s: null weights with count %zu", fn, count);
  if (count != nnz) return fail("%s: the data set holds %zu interactions, the caller's array %zu weights", fn, nnz, count);
  const std::string refusal = cdae::plan::check_weights(w, count);
  if (!refusal.empty()) return fail("%s: %s", fn, refusal.c_str());
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));                  // no half-step is still reading the weights this call replaces
  std::vector<uint32_t> col(std::max<size_t>(nnz, 1));
  if (nnz) HIPCHK(hipMemcpy(col.data(), h->d_col, nnz * sizeof(uint32_t), hipMemcpyDeviceToHost));
  const std::vector<float> tw = cdae::plan::item_major_weights(h->U, h->I, h->h_row_ptr.data(), col.data(), w);
  // both buffers exist before either is written: a failed allocation leaves the weights the handle had
  DevBuf<float> uw, iw;
  CHK(uw.alloc(nnz)); CHK(iw.alloc(nnz));
  if (nnz) {
    HIPCHK(hipMemcpy(uw.p, w, nnz * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(iw.p, tw.data(), nnz * sizeof(float), hipMemcpyHostToDevice));
  }
  h->d_als_w = std::move(uw); h->d_als_tw = std::move(iw);
  return 0;
}

int cdae_hip_als_objective(cdae_hip_t* h, double* out2) {
  const char* fn = "cdae_hip_als_objective";
  CHK(als_check(h, fn));
  if (!out2) return fail("%s: null out2", fn);
  HIPCHK(hipSetDevice(h->device));
  const float* X = h->d_Wu; const float* Y = h->P(CDAE_P_W);
  const uint64_t U = h->U;
  CHK(als_gram(h, X, U, h->d_als_G));
  CHK(als_gram(h, Y, h->I, h->d_als_G2));
  CHK(h->d_als_obj.ensure((size_t)U + 3));
  CHK(dispatch_ni(h->NI, [&](auto ni) {
    constexpr int NI = decltype(ni)::value;
    hipLaunchKernelGGL((cdae::als_objective_kernel<NI>), dim3((uint32_t)((U + 3) / 4)), dim3(256), 0, h->stream, (const int64_t*)h->d_row_ptr,
                       (const uint32_t*)h->d_col, (const float*)h->d_als_w, U, X, Y, h->als_alpha, h->d_als_obj.p);
    HIPCHK(hipGetLastError());
    return 0;
  }));
  hipLaunchKernelGGL(cdae::als_objective_gram_kernel, dim3(1), dim3(256), 0, h->stream, (const float*)h->d_als_G, (const float*)h->d_als_G2, h->Kp,
                     h->d_als_obj.p + U);
  HIPCHK(hipGetLastError());
  std::vector<double> host((size_t)U + 3);
  HIPCHK(hipMemcpyAsync(host.data(), h->d_als_obj, host.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  double sparse = 0.0;
  for (uint64_t u = 0; u < U; ++u) sparse += host[u];       // in row order
  out2[0] = host[U] + sparse;
  out2[1] = h->als_lambda_cfg * (host[U + 1] + host[U + 2]);
  return 0;
}

int cdae_hip_eval_topn_rows(cdae_hip_t* h, uint64_t n_rows, const uint32_t* uids, const int64_t* row_ptr, const uint32_t* col,
                            const int64_t* target_row_ptr, const uint32_t* target_col, uint32_t topk, double* rets8, uint64_t* hits3,
                            uint32_t* ids_out) {
  RowsArgs a{n_rows, uids, row_ptr, col, target_row_ptr, target_col, 0, topk, ids_out, nullptr};
  CHK(rows_check(h, "cdae_hip_eval_topn_rows", a));
  if (!rets8) return fail("cdae_hip_eval_topn_rows: null rets8");
  if (n_rows) CHK(validate_rows_csr("target", target_row_ptr, target_col, n_rows, h->I));
  for (uint64_t r = 0; r < n_rows; ++r) a.with_targets += target_row_ptr[r + 1] > target_row_ptr[r];
  if (a.with_targets == 0) return fail("cdae_hip_eval_topn_rows: no row has target items");
  CHK(rows_run(h, a));
  return topn_finish(h, h->d_rows_pu, n_rows, h->d_rows_out, rets8, hits3);
}

int cdae_hip_train_one_user_corruption(cdae_hip_t* h, uint64_t uid, const uint32_t* input_items, size_t n_in,
                                       const uint32_t* negative_items, size_t n_neg) {
  if (h) h->db_valid = h->db_rows_valid = false;      // the bf16 images of the decoder no longer match it (full-output path, compute_batch_full)
  if (!h || !h->d_shared) return fail("set_interactions must be called first");
  if (uid >= h->U) return fail("user id %llu out of range", (unsigned long long)uid);
  if (h->cfg.full_output) return fail("train_one_user_corruption takes an explicit negative list; it is not available in full_output mode");
  if (h->mf == 5u) return fail("train_one_user_corruption: %s", FISM_NO_LIST);
  if (h->mf) return fail("train_one_user_corruption does not apply to an IMF / BPR handle");
  if ((n_in && !input_items) || (n_neg && !negative_items)) return fail("null argument");
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  const int64_t r0 = h->h_row_ptr[uid];
  const size_t n_pos = (size_t)(h->h_row_ptr[uid + 1] - r0);
  const size_t E = n_pos + n_neg;
  if (E > h->Ecap) return fail("%zu examples exceed the batch capacity %llu", E, (unsigned long long)h->Ecap);
  std::vector<uint32_t> pos(n_pos), items(E), in_sorted(input_items, input_items + n_in);
  HIPCHK(hipMemcpy(pos.data(), h->d_col + r0, n_pos * sizeof(uint32_t), hipMemcpyDeviceToHost));
  std::sort(in_sorted.begin(), in_sorted.end());
  for (size_t i = 0; i < n_in; ++i) {
    if (!std::binary_search(pos.begin(), pos.end(), in_sorted[i])) return fail("input item %u is not a training item of user %llu", in_sorted[i], (unsigned long long)uid);
    if (i && in_sorted[i] == in_sorted[i - 1]) return fail("duplicate input item %u", in_sorted[i]);
  }
  std::vector<uint64_t> vals(E);
  for (size_t p = 0; p < n_pos; ++p) {
    const bool kept = std::binary_search(in_sorted.begin(), in_sorted.end(), pos[p]);
    items[p] = pos[p];
    vals[p] = ((uint64_t)p << 32) | (uint64_t)(cdae::TARGET_BIT | (kept ? cdae::INPUT_BIT : 0u));    // slot 0
  }
  for (size_t i = 0; i < n_neg; ++i) {
    if (negative_items[i] >= h->I) return fail("negative item %u out of range", negative_items[i]);
    if (std::binary_search(pos.begin(), pos.end(), negative_items[i])) return fail("negative item %u is a training item", negative_items[i]);
    items[n_pos + i] = negative_items[i];
    vals[n_pos + i] = (uint64_t)(n_pos + i) << 32;
  }
  h->pre_n = 0;
  HIPCHK(hipStreamSynchronize(h->stream));
  CHK(sync_prep(h));
  const int set = set_of(h->seq);
  cdae_hip::ExBuf& x = h->ex[set];
  HIPCHK(hipMemcpyAsync(x.item, items.data(), E * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(x.val, vals.data(), E * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
  HIPCHK(rocprim::radix_sort_pairs(h->d_sort_tmp.p, h->sort_tmp_bytes, x.item.p, x.sorted_item.p, x.val.p, x.sorted_val.p, E, 0u,
                                   (unsigned)h->sort_bits, h->stream));
  HIPCHK(hipMemsetAsync(x.seg, 0, 4 * (size_t)h->I * sizeof(uint32_t), h->stream));
  HIPCHK(hipMemsetAsync(x.dup_count, 0, cdae::DUP_STRIPES * sizeof(uint32_t), h->stream));
  HIPCHK(hipMemsetAsync(x.dup_of_ex, 0xFF, E * sizeof(uint32_t), h->stream));
  hipLaunchKernelGGL(cdae::segment_kernel<uint32_t>, dim3((uint32_t)((E + 256 * cdae::SEG_PER_THREAD - 1) / (256 * cdae::SEG_PER_THREAD))),
                     dim3(256), 0, h->stream, x.sorted_item, x.sorted_val,
                     (uint32_t)E, x.seg, x.seg + h->I, x.dup_count, h->dup_cap, x.dup_of_pos, x.dup_of_ex, h->dup_stripes,
                     (const uint32_t*)h->d_rank_of, x.seg + 2 * (size_t)h->I, x.seg + 3 * (size_t)h->I);
  HIPCHK(hipEventRecord(x.ready, h->stream));
  const uint32_t one_unit[2] = {0u, 1u};                         // one user, one unit
  HIPCHK(hipMemcpyAsync(h->d_uptr_tmp, one_unit, sizeof one_unit, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  uint32_t* d_in = h->d_uids;                     // capacity min(B, U) >= 1; longer input sets get their own buffer
  DevBuf<uint32_t> d_in_owned;                    // (freed on every way out)
  if (n_in > std::min<uint64_t>(h->B, h->U)) { CHK(d_in_owned.alloc(n_in)); d_in = d_in_owned; }
  if (n_in) HIPCHK(hipMemcpyAsync(d_in, in_sorted.data(), n_in * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  h->prof_q = h->seq;
  int rc = compute_batch(h, set, Batch{uid, 1, 0, E}, 0, 0, d_in, (uint32_t)n_in);
  h->seq++;
  hipError_t se = hipStreamSynchronize(h->stream);
  if (rc) return rc;
  if (se != hipSuccess) return fail("stream synchronize failed: %s", hipGetErrorString(se));
  return 0;
}

// ---- data-parallel exchange ---------------------------------------------------------------------
int cdae_hip_delta_begin(cdae_hip_t* h) {
  if (!h || !h->d_shared) return fail("set_interactions must be called first");
  if (h->mf == 5u) return fail("cdae_hip_delta_begin: %s", cdae_internal::exchange_refusal(h));
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  if (!h->d_base) { CHK(h->d_base.alloc(h->n_shared)); CHK(h->d_delta.alloc(h->n_shared + h->I)); }
  HIPCHK(hipMemcpyAsync(h->d_base, h->d_shared, h->n_shared * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemsetAsync(h->d_touched, 0, h->I * sizeof(uint32_t), h->stream));
  return 0;
}

int cdae_hip_stream(cdae_hip_t* h, void** hip_stream) {
  if (!h || !hip_stream) return fail("bad argument");
  *hip_stream = (void*)h->stream;
  return 0;
}

int cdae_hip_delta_compute(cdae_hip_t* h) {
  if (!h || !h->d_base) return fail("delta_begin must be called first");
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  hipLaunchKernelGGL(cdae::delta_kernel, dim3((uint32_t)((h->n_shared + 255) / 256)), dim3(256), 0, h->stream, h->d_shared,
                     h->d_base, h->d_delta, h->n_shared);
  hipLaunchKernelGGL(cdae::touch_to_float_kernel, dim3((uint32_t)((h->I + 255) / 256)), dim3(256), 0, h->stream, h->d_touched,
                     h->d_delta + h->n_shared, (uint32_t)h->I);
  HIPCHK(hipGetLastError());
  return 0;                                  // stream-ordered: callers that read the buffer on another stream synchronise
}

int cdae_hip_delta_device_ptr(cdae_hip_t* h, void** device_ptr, size_t* count_floats) {
  if (!h || !h->d_delta || !device_ptr) return fail("delta_begin must be called first");
  *device_ptr = h->d_delta;
  if (count_floats) *count_floats = h->n_shared + h->I;
  return 0;
}

int cdae_hip_delta_apply(cdae_hip_t* h, uint32_t world_size, uint32_t rule) {
  if (h) h->db_valid = h->db_rows_valid = false;      // the bf16 images of the decoder no longer match it (full-output path, compute_batch_full)
  if (!h || !h->d_delta) return fail("delta_begin must be called first");
  if (world_size == 0) return fail("world_size must be >= 1");
  if (rule > CDAE_DELTA_TOUCH_MEAN) return fail("unknown delta rule %u", rule);
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  hipLaunchKernelGGL(cdae::apply_delta_kernel, dim3((uint32_t)((h->n_shared + 255) / 256)), dim3(256), 0, h->stream, h->d_shared,
                     h->d_base, h->d_delta, h->d_delta + h->n_shared, h->n_matrix, h->Kp, (uint32_t)h->I, h->n_shared, world_size, rule);
  HIPCHK(hipGetLastError());
  return 0;
}

int cdae_hip_delta_set_combine(cdae_hip_t* h, uint32_t combine) {
  if (!h) return fail("null handle");
  if (combine > CDAE_COMBINE_GLOBAL_ACC) return fail("unknown combine rule %u", combine);
  h->delta_combine = combine;      // (takes effect at the next stage: call it between a merge and the following stage)
  return 0;
}

// pipelined variant: see delta_pipe_kernel.  The staged / received buffers are compact (no pad columns).
int cdae_hip_delta_stage(cdae_hip_t* h) {
  if (!h || !h->d_base) return fail("delta_begin must be called first");
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  if (!h->d_recv) {
    CHK(h->d_recv.alloc(h->n_shared + 4096));            // slack: collectives may round the count up
    CHK(h->d_snap.alloc(h->n_shared));
    HIPCHK(hipMemsetAsync(h->d_recv, 0, (h->n_shared + 4096) * sizeof(float), h->stream));
  }
  return launch_pipe<cdae::DELTA_STAGE>(h);
}

int cdae_hip_delta_recv_device_ptr(cdae_hip_t* h, void** device_ptr, size_t* count_floats) {
  if (!h || !h->d_recv || !device_ptr) return fail("delta_stage must be called first");
  *device_ptr = h->d_recv;
  if (count_floats) *count_floats = pipe_geom(h).n_compact;
  return 0;
}

int cdae_hip_delta_merge(cdae_hip_t* h) {
  if (h) h->db_valid = h->db_rows_valid = false;      // the bf16 images of the decoder no longer match it (full-output path, compute_batch_full)
  if (!h || !h->d_recv) return fail("delta_stage must be called first");
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  return launch_pipe<cdae::DELTA_MERGE>(h);
}

int cdae_hip_delta_merge_stage(cdae_hip_t* h) {
  if (h) h->db_valid = h->db_rows_valid = false;      // the bf16 images of the decoder no longer match it (full-output path, compute_batch_full)
  if (!h || !h->d_recv) return fail("delta_stage must be called first");
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  return launch_pipe<cdae::DELTA_MERGE_STAGE>(h);
}

}  // extern "C"

// ---- accessor surface for cdae_multi.hip (cdae_internal.hpp) --------------------------------------------------------
namespace cdae_internal {

int fail(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return 1;
}
int device_of(const cdae_hip_t* h) { return h->device; }
const char* exchange_refusal(const cdae_hip_t* h) {
  return h->mf == 5u ? "a FISM handle trains alone: its loop is one workgroup on one device, and no delta or exchange schedule is built for it" : nullptr;
}
hipStream_t main_stream(cdae_hip_t* h) { return h->stream; }
hipStream_t aux_stream(cdae_hip_t* h) { return h->aux; }
uint64_t num_users(const cdae_hip_t* h) { return h->U; }
uint64_t num_items(const cdae_hip_t* h) { return h->I; }
uint32_t batch_users(const cdae_hip_t* h) { return (uint32_t)std::min<uint64_t>(h->B, h->U); }
bool ready(const cdae_hip_t* h) { return h->d_shared != nullptr; }
float* send_buf(cdae_hip_t* h) { return h->d_delta; }
float* recv_buf(cdae_hip_t* h) { return h->d_recv; }
size_t compact_count(const cdae_hip_t* h) { return pipe_geom(h).n_compact; }
int validate_test_rows(const int64_t* test_row_ptr, const uint32_t* test_col, uint64_t U, uint64_t I, uint64_t* users_with_rows) {
  if (!test_row_ptr) return fail("null test_row_ptr");
  if (test_row_ptr[0] != 0) return fail("test_row_ptr[0] must be 0");
  for (uint64_t u = 0; u < U; ++u)
    if (test_row_ptr[u + 1] < test_row_ptr[u]) return fail("test_row_ptr must be non-decreasing");
  if (test_row_ptr[U] > 0 && !test_col) return fail("null test_col with %lld test interactions", (long long)test_row_ptr[U]);
  uint64_t with_rows = 0;
  for (uint64_t u = 0; u < U; ++u) {
    with_rows += test_row_ptr[u + 1] > test_row_ptr[u];
    for (int64_t p = test_row_ptr[u]; p < test_row_ptr[u + 1]; ++p) {
      if (test_col[p] >= I) return fail("test item id %u of user %llu out of range", test_col[p], (unsigned long long)u);
      if (p > test_row_ptr[u] && test_col[p] <= test_col[p - 1]) return fail("test row %llu is not ascending and unique", (unsigned long long)u);
    }
  }
  if (users_with_rows) *users_with_rows = with_rows;
  return 0;
}
int delta_stage_sync(cdae_hip_t* h) {
  if (!h || !h->d_recv) return fail("delta_stage must have been called once (it allocates the exchange buffers)");
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  return launch_pipe<cdae::DELTA_STAGE, true>(h);
}
int delta_merge_sync(cdae_hip_t* h) {
  if (!h || !h->d_recv) return fail("delta_stage must be called first");
  h->db_valid = h->db_rows_valid = false;
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  return launch_pipe<cdae::DELTA_MERGE, true>(h);
}

int adopt_shared_block(cdae_hip_t* dst, cdae_hip_t* src) {
  if (!dst || !src || !dst->d_shared || !src->d_shared || dst->n_shared != src->n_shared) return fail("adopt_shared_block: the handles do not hold the same model");
  CHK(cdae_hip_synchronize(src));
  HIPCHK(hipSetDevice(dst->device));
  CHK(quiesce(dst));
  dst->db_valid = dst->db_rows_valid = false;      // (full-output path) the bf16 images of the decoder no longer match it
  if (dst->device == src->device)
    HIPCHK(hipMemcpyAsync(dst->d_shared, src->d_shared, dst->n_shared * sizeof(float), hipMemcpyDeviceToDevice, dst->stream));
  else
    HIPCHK(hipMemcpyPeerAsync(dst->d_shared, dst->device, src->d_shared, src->device, dst->n_shared * sizeof(float), dst->stream));
  return 0;
}
void*& exchange_slot(cdae_hip_t* h) { return h->xchg; }
void set_exchange_deleter(cdae_hip_t* h, void (*deleter)(void*)) { h->xchg_free = deleter; }

static int sqnorm_sum(cdae_hip* h, std::initializer_list<std::pair<const float*, size_t>> parts, double* out) {
  HIPCHK(hipSetDevice(h->device));
  CHK(join_aux(h));
  HIPCHK(hipMemsetAsync(h->d_scalar, 0, sizeof(double), h->stream));
  for (auto& pr : parts)
    if (pr.first && pr.second)
      hipLaunchKernelGGL(cdae::sqnorm_kernel, dim3((uint32_t)std::min<size_t>(2048, (pr.second + 255) / 256)), dim3(256), 0, h->stream,
                         pr.first, pr.second, h->d_scalar);
  HIPCHK(hipGetLastError());
  double v = 0;
  HIPCHK(hipMemcpyAsync(&v, h->d_scalar, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  *out = 0.5 * h->cfg.lambda * v;
  return 0;
}
// cdae.hpp:104-106: W, V, Wu, b, b_prime (pad lanes are zero)
int shared_penalty(cdae_hip_t* h, double* out) {
  return sqnorm_sum(h, {{h->P(CDAE_P_W), h->cnt[CDAE_P_W]}, {h->P(CDAE_P_V), h->cnt[CDAE_P_V]}, {h->P(CDAE_P_B), h->cnt[CDAE_P_B]},
                        {h->P(CDAE_P_BP), h->cnt[CDAE_P_BP]}}, out);
}
int item_rows_penalty(cdae_hip_t* h, double* out) {
  return sqnorm_sum(h, {{h->P(CDAE_P_W), h->cnt[CDAE_P_W]}, {h->P(CDAE_P_V), h->cnt[CDAE_P_V]}, {h->P(CDAE_P_BP), h->cnt[CDAE_P_BP]}}, out);
}
int hidden_bias_penalty(cdae_hip_t* h, double* out) { return sqnorm_sum(h, {{h->P(CDAE_P_B), h->cnt[CDAE_P_B]}}, out); }
int private_penalty(cdae_hip_t* h, double* out) {
  if (!h->cfg.user_factor) { *out = 0.; return 0; }
  return sqnorm_sum(h, {{h->d_Wu, h->cnt[CDAE_P_WU]}}, out);
}

// ---- item-sharded layout: phases of a full-output batch and of the evaluation passes (cdae_internal.hpp) ---------------
int set_item_shard(cdae_hip_t* h, uint64_t item0, uint64_t num_items_global) {
  if (!h) return fail("null handle");
  if (h->mf) return fail("the item-sharded layout is CDAE's");
  h->item_shard = true; h->item0 = item0; h->I_global = num_items_global;
  return 0;
}
int set_item_shard_owner(cdae_hip_t* h, uint64_t u_begin, uint64_t u_end) {
  if (!h || !h->item_shard) return fail("set_item_shard must be called first");
  if (u_begin > u_end) return fail("bad owned user range");
  h->own_u0 = u_begin; h->own_u1 = u_end;
  return 0;
}
int set_item_shard_global(cdae_hip_t* h, const int64_t* row_ptr, const uint32_t* col) {
  if (!h || !h->item_shard) return fail("set_item_shard must be called first");
  h->g_row_ptr_src = row_ptr; h->g_col_src = col;
  return 0;
}
uint32_t shard_blocks(const cdae_hip_t* h) { return shard_blocks_of(h); }
int set_item_shard_positions(cdae_hip_t* h, const uint32_t* len_and_first /* [2 U] */) {
  if (!h || !h->d_shared || !h->item_shard || !len_and_first) return fail("set_item_shard and set_interactions must be called first");
  HIPCHK(hipSetDevice(h->device));
  if (!h->d_gpos) CHK(h->d_gpos.alloc(2 * (size_t)h->U));
  HIPCHK(hipMemcpy(h->d_gpos, len_and_first, 2 * (size_t)h->U * sizeof(uint32_t), hipMemcpyHostToDevice));
  return 0;
}
uint32_t row_stride(const cdae_hip_t* h) { return h->Kp; }
float* hsum_buf(cdae_hip_t* h) { return h->d_Hsum; }
float* hg_buf(cdae_hip_t* h) { return h->d_HG; }
float* ev_hsum_buf(cdae_hip_t* h) { return h->d_hsum_eval; }
uint32_t eval_chunk() { return EVAL_CHUNK; }

// block 0 = the users' input sums over this shard's rows; blocks 1.. = the Wu / Uu rows of the users this shard owns (zeros for everybody
// else's: after the all-reduce(sum) every shard holds the owners' rows, bit for bit) — one launch (unit_sum_stage_kernel)
static int sum_and_stage(cdae_hip* h, const float* hpart, const uint32_t* uptr, uint64_t u0, uint32_t n, float* buf) {
  const float* ta = h->cfg.user_factor ? h->d_Wu.p : (h->cfg.linear_function ? h->d_Uu.p : nullptr);
  const float* tb = h->cfg.user_factor && h->cfg.linear_function ? h->d_Uu.p : nullptr;
  DISPATCH_NI(h->NI, cdae::unit_sum_stage_kernel, dim3((n + 3) / 4), dim3(256), 0, h->stream, h->hp, hpart, uptr, n, u0, ta, tb, buf);
  return 0;
}
// the gathered rows inside an all-reduced buffer (nullptr when the configuration has none)
static const float* gathered_wu(const cdae_hip* h, const float* buf, uint32_t n) { return h->cfg.user_factor ? buf + (size_t)n * h->Kp : nullptr; }
static const float* gathered_uu(const cdae_hip* h, const float* buf, uint32_t n) {
  return h->cfg.linear_function ? buf + (size_t)(h->cfg.user_factor ? 2 : 1) * n * h->Kp : nullptr;
}

static int fs_batch(cdae_hip* h, uint64_t s0, uint32_t nb, uint32_t cidx, Batch* bt) {
  if (!h->d_shared || !h->item_shard) return fail("not an item-sharded handle with data");
  if (nb == 0 || s0 + nb > h->U || nb > std::min<uint64_t>(h->B, h->U)) return fail("bad batch [%llu, +%u)", (unsigned long long)s0, nb);
  const uint64_t E = h->shard_sampled() ? (uint64_t)(h->h_grow_ptr[s0 + nb] - h->h_grow_ptr[s0]) * h->ex_per_pos
                                        : (uint64_t)(h->h_row_ptr[s0 + nb] - h->h_row_ptr[s0]);
  if (E > h->Ecap) return fail("batch has %llu examples, capacity %llu", (unsigned long long)E, (unsigned long long)h->Ecap);
  *bt = Batch{s0, nb, cidx, E};
  return 0;
}

int fs_prep(cdae_hip_t* h, uint64_t seed, uint32_t epoch, uint64_t s0, uint32_t nb, uint32_t cidx) {
  HIPCHK(hipSetDevice(h->device));
  Batch bt;
  CHK(fs_batch(h, s0, nb, cidx, &bt));
  h->prof_q = h->seq;
  CHK(prep_batch(h, (int)(h->fs_prepped & 1), bt, seed, epoch));       // fs_prepped counts prepared batches: set = parity
  h->fs_prepped++;
  return 0;
}

int fs_phase0(cdae_hip_t* h, uint64_t seed, uint32_t epoch, uint64_t s0, uint32_t nb, uint32_t cidx) {
  HIPCHK(hipSetDevice(h->device));
  Batch bt;
  CHK(fs_batch(h, s0, nb, cidx, &bt));
  const uint32_t n_units = units_of(h, bt);
  const uint32_t* uptr = h->d_unit_ptr + s0;
  if (!h->encode_two_launches && nb <= ENCODE_USERS_MAX) {
    // one launch (round 4): the training encode's workgroup-per-user kernel, stopped at the raw input sum of the local rows, with the
    // owner's private rows staged behind it — the same sums in the same order as the single handle's encode for every user
    const float* ta = h->cfg.user_factor ? h->d_Wu.p : (h->cfg.linear_function ? h->d_Uu.p : nullptr);
    const float* tb = h->cfg.user_factor && h->cfg.linear_function ? h->d_Uu.p : nullptr;
    DISPATCH_NI(h->NI, cdae::encode_users_kernel, dim3(nb), dim3(cdae::ENC_WAVES * cdae::WAVE), 0, h->stream, h->hp, h->d_row_ptr, h->d_col,
                h->P(CDAE_P_W), uptr, s0, nb, cidx, seed, epoch, (const float*)nullptr, (const float*)nullptr, (float*)nullptr, (float*)nullptr,
                (float*)nullptr, (const float*)nullptr, (float*)nullptr, (cdae::BF16_T*)nullptr, (cdae::BF16_T*)nullptr, 0u, h->d_Hsum, ta, tb,
                (const uint32_t*)h->d_gpos);
    HIPCHK(hipGetLastError());
    return 0;
  }
  if (n_units)
    DISPATCH_NI(h->NI, cdae::encode_partial_kernel, dim3((n_units + 3) / 4), dim3(256), 0, h->stream, h->hp, h->d_row_ptr, h->d_col,
                h->P(CDAE_P_W), uptr, n_units, (const uint32_t*)nullptr, s0, nb, 1, CDAE_STREAM_CORRUPT, cidx, seed, epoch, h->d_Hpart,
                (const uint32_t*)nullptr, 0u, (const uint32_t*)h->d_unit_user, (const uint32_t*)h->d_gpos);
  CHK(sum_and_stage(h, h->d_Hpart, uptr, s0, nb, h->d_Hsum));
  HIPCHK(hipGetLastError());
  return 0;
}

int fs_phase1(cdae_hip_t* h, uint64_t s0, uint32_t nb) {
  using namespace cdae;
  HIPCHK(hipSetDevice(h->device));
  Batch bt;
  CHK(fs_batch(h, s0, nb, 0, &bt));
  const int b = (int)(h->seq & 1);
  cdae_hip::ExBuf& x = h->ex[b];
  hipStream_t st = h->stream;
  const uint32_t I = (uint32_t)h->I, Kp = h->Kp, Bp = h->Bp, Ip = h->Ip;
  const dim3 blk(256), grid_users((nb + 3) / 4);
  // the batch's Wu / Uu rows arrived with the all-reduced input sums (stage_own_rows): encode_finish reads them by slot (uids = iota)
  const float* wu_b = gathered_wu(h, h->d_Hsum, nb);
  const float* uu_b = gathered_uu(h, h->d_Hsum, nb);
  if (!h->cfg.full_output) {
    // ---- sampled decode over the local item rows: the single-GPU step's kernels on this shard's rows / examples ----
    DISPATCH_NI(h->NI, encode_finish_kernel, grid_users, blk, 0, st, h->hp, h->d_Hsum, (const uint32_t*)h->d_iota, wu_b, h->P(CDAE_P_B),
                (const uint32_t*)h->d_iota, s0, nb, 1, h->d_Z, h->d_Dz, h->d_HG, uu_b, h->d_Ssum,
                (BF16_T*)nullptr, (BF16_T*)nullptr, 0u, h->late_rows ? h->d_Ghot : (float*)nullptr, h->d_hotdup);
    HIPCHK(hipStreamWaitEvent(st, x.ready, 0));
    Prof pr;                                                  // (cdae_hip_set_profiling on a shard's handle: the decode launch of this shard's rows)
    CHK(pr.begin(h, F_DECODE, st, h->seq));
    CHK(launch_decode(h, x));
    CHK(pr.end());
    // local hidden gradient: the user's examples on THIS shard's rows (the others are VOID), partial rows per unit of the whole rows
    const uint32_t n_gunits = gunits_of(h, bt);
    const uint32_t* guptr = h->d_gunit_ptr + s0;
    if (n_gunits)
      DISPATCH_NI(h->NI, hidden_gather_kernel, dim3(8 * ((n_gunits + 3) / 4)), blk, 0, st, h->hp, h->d_grow_ptr, guptr, n_gunits, s0, nb,
                  x.item, h->d_G, h->d_D0, h->d_HGpart, 0u, x.dup_of_ex, h->d_dup_corr, (const uint32_t*)h->d_gunit_user,
                  h->late_rows ? (const uint32_t*)h->d_late_bits : (const uint32_t*)nullptr, h->late_words);
    DISPATCH_NI(h->NI, hg_raw_kernel, dim3(nb), blk, 0, st, h->hp, guptr, n_gunits, nb, h->d_HGpart, 8u, h->d_HG, h->late_finish());
    HIPCHK(hipGetLastError());
    return 0;
  }
  // bf16 images of the shard's decoder rows: the fused row step (gemm3_rows_fused_kernel) leaves the row-major one current, and with
  // GEMM 2 reading G^T and D nothing needs D^T — converted only when something else wrote the parameters
  if (!(rows_fused_path(h) && gemm2_tn_path(h) && h->db_rows_valid))
    hipLaunchKernelGGL(to_bf16_transpose_kernel, dim3(Kp / 64, Ip / 64), blk, 0, st, h->dec(), I, Kp, Kp, Ip, h->d_Db, h->d_DTb);
  CHK(join_aux(h));
  // z from the ALL-REDUCED input sums: encode_finish with one "unit" per user (identity prefix)
  DISPATCH_NI(h->NI, encode_finish_kernel, grid_users, blk, 0, st, h->hp, h->d_Hsum, (const uint32_t*)h->d_iota, wu_b, h->P(CDAE_P_B),
              (const uint32_t*)h->d_iota, s0, nb, 1, h->d_Z, h->d_Dz, h->d_HG, uu_b, h->d_Ssum);
  hipLaunchKernelGGL(to_bf16_transpose_kernel, dim3(Kp / 64, Bp / 64), blk, 0, st, h->d_Z, nb, Kp, Kp, Bp, h->d_Zb, h->d_ZTb);
  HIPCHK(hipStreamWaitEvent(st, x.ready, 0));
  uint32_t parts = 0, rows = nb;
  if (Kp <= 256 && !h->full_unfused) {
    CHK(launch_full_fused(h, st, b, nb));
    parts = h->full_slices; rows = nb;
  } else {
    Prof prd;
    CHK(prd.begin(h, F_DECODE, st, h->seq));
    CHK(full_products_k512(h, st, x, bt, nb, &parts, &rows));      // the single handle's launches over this shard's item rows
    CHK(prd.end());
  }
  // local hidden gradient of the batch, raw: the shards' sums are all-reduced before delta is formed
  DISPATCH_NI(h->NI, slab_sum_kernel, grid_users, blk, 0, st, h->hp, h->d_HGpart, parts, rows, nb, h->d_HG);
  HIPCHK(hipGetLastError());
  return 0;
}

int fs_phase2(cdae_hip_t* h, uint64_t s0, uint32_t nb) {
  using namespace cdae;
  HIPCHK(hipSetDevice(h->device));
  Batch bt;
  CHK(fs_batch(h, s0, nb, 0, &bt));
  cdae_hip::ExBuf& x = h->ex[h->seq & 1];
  const float* uu_b = gathered_uu(h, h->d_Hsum, nb);
  // the tail of the single handle's step over the local rows: d_HG holds the all-reduced hg (no slab to add, no late-row terms), delta
  // and the Wu / Uu steps are those of the users this shard owns, the b recurrence is replicated (identical everywhere).  Full
  // output: the row kernels write no bf16 image here — phase 1 converts the decoder — except the fused row step, which always
  // leaves the row-major image current
  if (!h->cfg.full_output) CHK(sampled_tail(h, x, s0, nb, h->d_iota, nb, 0u, uu_b, LateFinish{}, nullptr));
  else CHK(full_tail(h, x, s0, nb, FullTail{0u, nb, uu_b, false, h->seq, nullptr}));
  h->seq++;
  h->acc_examples += bt.E; h->acc_batches++; h->acc_users += nb;
  return 0;
}

int ev_phase0(cdae_hip_t* h, uint64_t u0, uint32_t nu, int mode, uint32_t cidx, uint64_t seed, uint32_t epoch) {
  HIPCHK(hipSetDevice(h->device));
  if (!h->d_shared || !h->item_shard) return fail("not an item-sharded handle with data");
  if (nu == 0 || nu > EVAL_CHUNK || u0 + nu > h->U) return fail("bad evaluation chunk");
  CHK(join_aux(h));
  const uint32_t n_units = h->h_unit_ptr[u0 + nu] - h->h_unit_ptr[u0];
  CHK(ensure_eval_ws(h, nu, std::max<uint32_t>(n_units, 1u)));
  CHK(h->d_hsum_eval.ensure(nu, (size_t)SHARD_BLOCKS * h->Kp));
  const uint32_t* uptr = h->d_unit_ptr + u0;
  if (n_units)
    DISPATCH_NI(h->NI, cdae::encode_partial_kernel, dim3((n_units + 3) / 4), dim3(256), 0, h->stream, h->hp, h->d_row_ptr, h->d_col,
                h->P(CDAE_P_W), uptr, n_units, (const uint32_t*)nullptr, u0, nu, mode, mode ? CDAE_STREAM_LOSS_CORRUPT : CDAE_STREAM_CORRUPT, cidx,
                seed, epoch, h->d_hpart_eval, (const uint32_t*)nullptr, 0u, (const uint32_t*)h->d_unit_user, (const uint32_t*)h->d_gpos);
  CHK(sum_and_stage(h, h->d_hpart_eval, uptr, u0, nu, h->d_hsum_eval));
  HIPCHK(hipGetLastError());
  return 0;
}

int ev_finish(cdae_hip_t* h, uint64_t u0, uint32_t nu, int mode) {
  HIPCHK(hipSetDevice(h->device));
  DISPATCH_NI(h->NI, cdae::encode_finish_kernel, dim3((nu + 3) / 4), dim3(256), 0, h->stream, h->hp, h->d_hsum_eval, (const uint32_t*)h->d_iota,
              gathered_wu(h, h->d_hsum_eval, nu), h->P(CDAE_P_B), (const uint32_t*)h->d_iota, u0, nu, mode, h->d_zeval, (float*)nullptr,
              (float*)nullptr, gathered_uu(h, h->d_hsum_eval, nu), (float*)nullptr);
  HIPCHK(hipGetLastError());
  return 0;
}

int ev_data_loss(cdae_hip_t* h, uint64_t u0, uint32_t nu, double* sum) {
  HIPCHK(hipSetDevice(h->device));
  const uint32_t n_units = h->h_unit_ptr[u0 + nu] - h->h_unit_ptr[u0];
  if (n_units == 0) return 0;
  HIPCHK(hipMemsetAsync(h->d_scalar, 0, sizeof(double), h->stream));
  DISPATCH_NI(h->NI, cdae::data_loss_kernel, dim3((n_units + 3) / 4), dim3(256), 0, h->stream, h->hp, h->d_row_ptr, h->d_col,
              h->d_unit_ptr + u0, n_units, (const uint32_t*)h->d_unit_user, u0, nu, h->d_zeval, h->dec(), h->P(CDAE_P_BP), h->d_scalar);
  HIPCHK(hipGetLastError());
  double v = 0;
  HIPCHK(hipMemcpyAsync(&v, h->d_scalar, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  *sum += v;
  return 0;
}

int ev_recommend(cdae_hip_t* h, uint64_t u0, uint32_t nu, uint32_t topk, uint32_t* ids, float* scores) {
  HIPCHK(hipSetDevice(h->device));
  if (topk == 0 || topk > h->I) return fail("topk %u exceeds the %llu items of this shard", topk, (unsigned long long)h->I);
  TopkSweep sweep(h, h->hp, h->dec(), h->P(CDAE_P_BP), topk, true, nullptr, false);      // (an item shard: the general path)
  CHK(sweep.prepare(h, nu, Mask::CSR));
  const Mask mask{Mask::CSR, h->d_row_ptr, h->d_col};
  for (uint32_t c0 = 0; c0 < nu; c0 += sweep.chunk) {
    const uint32_t nb = std::min(sweep.chunk, nu - c0);
    CHK(sweep.run(h, h->d_zeval + (size_t)c0 * h->Kp, u0 + c0, nb, mask));
    CHK(copy_lists_out(h, (size_t)nb * topk, ids + (size_t)c0 * topk, scores + (size_t)c0 * topk));
  }
  return 0;
}

}  // namespace cdae_internal
