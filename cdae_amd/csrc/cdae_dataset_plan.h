// cdae_dataset_plan.h — what cdae_hip_set_interactions DECIDES from a data set, as plain host arithmetic: no HIP, no handle, no
// environment.  The library compiles it (cdae_hip.hip builds a Plan before it touches the handle, then allocates and uploads what the
// plan says) and so does tests/native/dataset_plan_cpu.cpp, which tests/test_dataset_plan_cpu.py compares with numpy on a CPU.
// Rule (DESIGN.md "Data-set plan"): a new data-dependent decision goes HERE, with its numpy line in tests/plan_ref.py and the smallest
// shape at which it can go wrong in tests/test_dataset_plan_cpu.py.  The limits the plan reads are defined here, once; the kernel
// headers include this file for them.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <functional>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/cdae_hip.h"

namespace cdae {

// Correction rows are numbered by bumping a counter once per workgroup of segment_kernel / segment_sort_kernel.  ONE counter for
// hundreds of workgroups is a chain of same-address returning atomics (~55 ns each: 37 us of a 660-workgroup launch); the index
// space is cut into up to DUP_STRIPES stripes of at least 4096 rows with a counter each (workgroup b draws from stripe b mod
// stripes; a stripe that runs out hands out DUP_NONE and decode falls back to its atomics path for those examples — small
// problems use one stripe: they must not run out where one counter would not).
constexpr uint32_t DUP_STRIPES = 64;
constexpr uint32_t LATE_MAX = 64;               // one lane of hidden_finish_kernel per late row
constexpr uint32_t LATE_BITS_WORDS = 2048;       // LDS copy of the late-row bitmap: item spaces up to 65 536
constexpr uint32_t BKC_ITEM_BITS = 12;        // a cell entry of bucket_sort_kernel: example index << BKC_ITEM_BITS | item - range start
constexpr uint32_t BKC_MAX_RANGES = 256;      // LDS counters per wavefront in sample_kernel
constexpr uint32_t UNIT_POS_MAX = 128;     // HyperParams::unit_pos (set per data set / batch size by the host) never exceeds it
constexpr uint32_t TILE_SORT_MAX_ITEMS = 32768;         // tile_scatter_kernel's cursors: 4 bytes per item of LDS (128 KiB at the limit)
constexpr uint32_t BK_ITEMS = 2048;       // most items of one range (LDS counters: 4 per thread in bk_block_scan)
constexpr uint32_t BK_MAX_RANGES = 1024;  // wg_state words (sample_kernel clears them with the other per-batch counters)
constexpr uint32_t BK_CELL_UNITS_MAX = 16384;   // most units of a batch the cell path takes (their counts, 2 bytes each, fit the `raw` array)

namespace plan {

// a refusal as text (the caller passes it to fail()); the empty string means "accepted"
inline std::string refuse(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return buf;
}

// Rows: monotone row_ptr, ids below I, strictly ascending inside a row; `sampled` handles (every kind but an item shard, which sees
// only its slice of every row, and WRMF, which samples nothing) also refuse a row with every item and, unless `empty_ok`, a row with no
// item.  empty_ok is FISM's: a user without train items takes no step there (include/cdae_hip.h), and is served z = 0.
// pop[i] = users of item i.
inline std::string check_rows(uint64_t U, uint64_t I, const int64_t* row_ptr, const uint32_t* col, bool sampled, bool empty_ok,
                              std::vector<uint64_t>& pop) {
  pop.assign(I, 0);
  for (uint64_t u = 0; u < U; ++u) {
    const int64_t a = row_ptr[u], b = row_ptr[u + 1];
    if (b < a) return refuse("row_ptr is not monotone at user %llu", (unsigned long long)u);
    if (sampled) {
      if (b <= a && !empty_ok) return refuse("user %llu has no training item (the reference CHECK-fails too, cdae.hpp:139)", (unsigned long long)u);
      if ((uint64_t)(b - a) >= I) return refuse("user %llu rated every item: no negative can be sampled", (unsigned long long)u);
    }
    for (int64_t p = a; p < b; ++p) {
      if (col[p] >= I) return refuse("item id %u out of range at position %lld", col[p], (long long)p);
      if (p > a && col[p] <= col[p - 1]) return refuse("row %llu is not strictly ascending at position %lld", (unsigned long long)u, (long long)p);
      pop[col[p]]++;
    }
  }
  return {};
}

// IMF / BPR block schedule: the activity-grouped training order (see cdae_hip::user_perm) and the CSR permuted into it
struct ActivityOrder {
  std::vector<uint32_t> user_perm, user_inv;      // user of a position, position of a user
  std::vector<int64_t> row_ptr;                   // rows by POSITION
  std::vector<uint32_t> col;
};
inline std::string activity_order(uint64_t U, uint32_t B, const int64_t* row_ptr, const uint32_t* col, ActivityOrder& o) {
  for (uint64_t u = 0; u < U; ++u)
    if (row_ptr[u + 1] < row_ptr[u]) return refuse("row_ptr is not monotone at user %llu", (unsigned long long)u);
  std::vector<uint32_t> by_len(U);
  std::iota(by_len.begin(), by_len.end(), 0u);
  std::stable_sort(by_len.begin(), by_len.end(), [&](uint32_t a, uint32_t b) { return row_ptr[a + 1] - row_ptr[a] > row_ptr[b + 1] - row_ptr[b]; });
  const uint64_t nblk = (U + B - 1) / B;
  std::vector<uint32_t> blk(nblk);
  std::iota(blk.begin(), blk.end(), 0u);
  // the short last group (U % B users, the least active) stays LAST: make_plan cuts batches at multiples of B from position 0, so
  // a short group in the middle made every later batch straddle two unrelated activity groups and last as long as the heavier one
  const uint64_t shuffled = (U % B) ? nblk - 1 : nblk;
  std::stable_sort(blk.begin(), blk.begin() + shuffled, [](uint32_t a, uint32_t b) { return (uint32_t)(a * 2654435761u) < (uint32_t)(b * 2654435761u); });
  o.user_perm.clear();
  o.user_perm.reserve(U);
  for (uint32_t k : blk)
    for (uint64_t t = (uint64_t)k * B; t < std::min<uint64_t>(U, (uint64_t)(k + 1) * B); ++t) o.user_perm.push_back(by_len[t]);
  o.user_inv.resize(U);
  for (uint64_t pos = 0; pos < U; ++pos) o.user_inv[o.user_perm[pos]] = (uint32_t)pos;
  o.row_ptr.assign(U + 1, 0);
  o.col.resize((size_t)row_ptr[U]);
  for (uint64_t pos = 0; pos < U; ++pos) {
    const uint32_t u = o.user_perm[pos];
    std::copy(col + row_ptr[u], col + row_ptr[u + 1], o.col.begin() + o.row_ptr[pos]);
    o.row_ptr[pos + 1] = o.row_ptr[pos] + (row_ptr[u + 1] - row_ptr[u]);
  }
  return {};
}

// decode launch order: most popular rows first (their example chains are the longest); ties keep item order
inline std::vector<uint32_t> popularity_order(const std::vector<uint64_t>& pop) {
  std::vector<uint32_t> order(pop.size());
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return pop[a] > pop[b]; });
  return order;
}
inline std::vector<uint32_t> inverse_order(const std::vector<uint32_t>& order) {
  std::vector<uint32_t> rank_of(order.size());
  for (uint32_t r = 0; r < order.size(); ++r) rank_of[order[r]] = r;
  return rank_of;
}

// The decode split by popularity rank.  share = the part of the users one batch holds.
struct DecodeSplit {
  uint32_t hot_rows = 0, late_rows = 0;
  std::vector<float> rank_len;        // [I] expected examples per batch of the row of rank r
  std::vector<uint32_t> late_bits;    // [(I + 31) / 32] bitmap over the items of the late rows; empty without late rows
};
inline DecodeSplit decode_split(uint64_t U, uint64_t I, uint32_t B, uint64_t nnz, uint32_t num_neg, const std::vector<uint64_t>& pop,
                                const std::vector<uint32_t>& order, double hot_pos, double late_pos, bool late_allowed) {
  DecodeSplit d;
  const double share = (double)std::min<uint64_t>(B, U) / (double)U;
  // hot rows: expected positives per batch (popularity x batch share) of at least hot_pos (CDAE_DECODE_HOT_POS, default 48);
  // every row also receives ~ B * mean(n_u) * num_neg / I uniformly spread negatives
  uint32_t hot = 0;
  while (hot < I && (double)pop[order[hot]] * share >= hot_pos) ++hot;
  d.hot_rows = std::min<uint32_t>((hot + 3u) & ~3u, (uint32_t)I);
  // Late rows: the most popular of the hot rows (at most one lane of hidden_finish_kernel each).  Their terms of the hidden gradient are
  // added by hidden_finish_kernel / hg_raw_kernel from Ghot, not gathered — in EVERY launch order (so that the fused launch, the
  // separate launches and an item shard of one agree bit for bit); the gather tells them by a bitmap it stages in LDS (item spaces up
  // to 65 536).
  if (late_allowed && I <= 32u * LATE_BITS_WORDS) {
    // late: at least late_pos (CDAE_DECODE_LATE_POS, default 48, i.e. the hot rows: measured 16 / 24 / 32 / 48 -> 0.0915 / 0.0918 / 0.0907 / 0.0898 ms per step) expected positives per batch, at most LATE_MAX rows; all of them take a
    // wavefront of their own (a late row in the four-rows-per-wavefront format would need its own Ghot bookkeeping there)
    uint32_t late = 0;
    while (late < I && late < LATE_MAX && (double)pop[order[late]] * share >= late_pos) ++late;
    // (a batch must have examples enough to make the split worth its bookkeeping: none for tiny batches)
    d.late_rows = d.hot_rows ? std::min<uint32_t>(std::min<uint32_t>((late + 3u) & ~3u, LATE_MAX), (uint32_t)I) : 0u;
    d.hot_rows = std::max(d.hot_rows, d.late_rows);
  }
  // expected examples per batch of every row, by popularity rank: positives (popularity x batch share) + the uniformly drawn negatives
  const double neg_per_item = share * (double)nnz * (double)num_neg / (double)std::max<uint64_t>(I, 1);
  d.rank_len.resize(I);
  for (uint32_t r = 0; r < I; ++r) d.rank_len[r] = (float)((double)pop[order[r]] * share + neg_per_item);
  if (d.late_rows) {
    d.late_bits.assign((I + 31) / 32, 0u);
    for (uint32_t r = 0; r < d.late_rows; ++r) d.late_bits[order[r] >> 5] |= 1u << (order[r] & 31u);
  }
  return d;
}

// the largest prefix[min(U, s0 + B)] - prefix[s0] over every s0 < U: any window of B consecutive users may be asked for (train_users)
template <class T> uint64_t window_max(const T* prefix, uint64_t U, uint64_t B) {
  uint64_t m = 0;
  for (uint64_t s0 = 0; s0 < U; ++s0) m = std::max<uint64_t>(m, (uint64_t)(prefix[std::min<uint64_t>(U, s0 + B)] - prefix[s0]));
  return m;
}

// Work units (cdae_kernels.hpp): prefix of the units (at most unit_pos positives each) per user, and the user of every unit
inline std::vector<uint32_t> unit_prefix(const int64_t* row_ptr, uint64_t U, uint32_t unit_pos) {
  std::vector<uint32_t> ptr(U + 1, 0u);
  for (uint64_t u = 0; u < U; ++u) ptr[u + 1] = ptr[u] + (uint32_t)((row_ptr[u + 1] - row_ptr[u] + unit_pos - 1) / unit_pos);
  return ptr;
}
inline std::vector<uint32_t> unit_owners(const std::vector<uint32_t>& unit_ptr) {
  const uint64_t U = unit_ptr.size() - 1;
  std::vector<uint32_t> user(unit_ptr[U]);
  for (uint64_t u = 0; u < U; ++u)
    for (uint32_t g = unit_ptr[u]; g < unit_ptr[u + 1]; ++g) user[g] = (uint32_t)u;
  return user;
}
// cdae_hip_encode takes arbitrary user lists of up to B users: the heaviest B (<= U) users bound its unit count
inline uint64_t encode_unit_bound(const std::vector<uint32_t>& unit_ptr, uint32_t B) {
  const uint64_t U = unit_ptr.size() - 1;
  std::vector<uint32_t> per(U);
  for (uint64_t u = 0; u < U; ++u) per[u] = unit_ptr[u + 1] - unit_ptr[u];
  std::partial_sort(per.begin(), per.begin() + B, per.end(), std::greater<uint32_t>());
  uint64_t top = 0;
  for (uint32_t i = 0; i < B; ++i) top += per[i];
  return top;
}

// bucket_sort_kernel — one narrow launch, every workgroup owns a range of item ids cut HERE so that the ranges expect equal numbers
// of examples per batch: B * pop[i] / U positives + the uniformly drawn negatives.  It scans the batch's whole 16-bit key list once
// per range and pass, so it is for batches up to `max_examples` examples (256-512 users at the BASELINE shapes) over at most 65536
// keys; beyond that the library sort stays.
struct BucketCuts {
  bool on = false;                    // the bucket sort orders this handle's batches
  std::vector<uint32_t> cut;          // [ranges + 1] item ids
  std::vector<uint16_t> range_of;     // [I] item -> range: the cell path; empty: the sort scans the batch's key list
};
// full-output blocks list their positives only and are long (thousands of users).  There the one narrow launch is the wrong shape: its
// workgroups (1024 threads, 90 KB of LDS: a CU each) run ~130 us beside a fused decode whose grid wants every CU (ML-10M shape, 2048
// users per block: full_decode_fused_kernel 57 -> 93 us, step 0.203 -> 0.24 ms), and from ~300 K examples on it is longer than the
// block it prepares (4096 users: 0.43 ms against a 0.33 ms step).  Blocks above 100 K examples keep the library sort's short launches.
inline uint64_t bucket_max_examples(bool full_output) { return full_output ? 100000 : 600000; }
// B: users of a batch (<= U); keys: item ids the sort tells apart (a sampled item shard sorts one more: VOID); draw_items, whole_nnz:
// the item space negatives are drawn from and the interactions of the whole rows (an item shard's differ from its own); negs: negatives
// per positive; allowed / cells_allowed: what the handle's kind and switches leave open
inline BucketCuts bucket_cuts(uint64_t U, uint64_t I, uint32_t B, uint64_t keys, uint64_t Ecap, uint64_t max_examples, double draw_items,
                              double whole_nnz, uint32_t negs, const std::vector<uint64_t>& pop, bool allowed, bool cells_allowed) {
  BucketCuts k;
  if (!(keys <= 65536 && allowed && Ecap <= max_examples && Ecap > 0)) return k;
  const double b_share = (double)B / (double)U;
  const double neg_per_item = b_share * whole_nnz * (double)negs / draw_items;
  std::vector<double> wgt(I);
  double total = 0.0;
  for (uint64_t i = 0; i < I; ++i) { wgt[i] = b_share * (double)pop[i] + neg_per_item; total += wgt[i]; }
  const double per_range = std::max(total / 256.0, std::min(2730.0, total / 8.0));   // ~2.7 K examples per range: half the LDS window
  std::vector<uint32_t> cut{0u};
  double acc = 0.0;
  for (uint64_t i = 0; i < I; ++i) {
    acc += wgt[i];
    if (i + 1 < I && (acc >= per_range || (i + 1) - cut.back() == BK_ITEMS)) { cut.push_back((uint32_t)(i + 1)); acc = 0.0; }
  }
  cut.push_back((uint32_t)I);
  if (cut.size() - 1 > BK_MAX_RANGES) return k;
  k.on = true;
  k.cut = std::move(cut);
  // cells: sample_kernel routes every example into the cell of (its item's range, its unit), so that the sort reads its range's cells
  // instead of scanning the batch's key list.  The CDAE sampler only; <= 256 ranges (LDS counters per wavefront); example indices must
  // fit the entry's 20 bits (Ecap <= 600 000 does)
  if (cells_allowed && k.cut.size() - 1 <= BKC_MAX_RANGES && Ecap < (1ull << (32 - BKC_ITEM_BITS))) {
    k.range_of.resize(I);
    for (uint32_t r = 0; r + 1 < k.cut.size(); ++r)
      for (uint32_t i = k.cut[r]; i < k.cut[r + 1]; ++i) k.range_of[i] = (uint16_t)r;
  }
  return k;
}

// WRMF: the item-major CSR of the item half-step — a counting sort, users ascending inside a column
struct ItemMajor {
  std::vector<int64_t> ptr;           // [I + 1]
  std::vector<uint32_t> col;          // [max(nnz, 1)] users
};
inline ItemMajor item_major_csr(uint64_t U, uint64_t I, const int64_t* row_ptr, const uint32_t* col, const std::vector<uint64_t>& pop) {
  ItemMajor t;
  t.ptr.assign(I + 1, 0);
  for (uint64_t i = 0; i < I; ++i) t.ptr[i + 1] = t.ptr[i] + (int64_t)pop[i];
  t.col.resize(std::max<size_t>((size_t)row_ptr[U], 1));
  std::vector<int64_t> cursor(t.ptr.begin(), t.ptr.end() - 1);
  for (uint64_t u = 0; u < U; ++u)
    for (int64_t p = row_ptr[u]; p < row_ptr[u + 1]; ++p) t.col[(size_t)cursor[col[p]]++] = (uint32_t)u;
  return t;
}

// WRMF with per-pair confidence weights (cdae_hip_als_set_confidence): w holds one weight per entry of col; the result holds the same
// weights in the order of item_major_csr's col — the same counting sort, so entry k of the result belongs to entry k of ItemMajor::col.
// The column starts are rebuilt from col (the caller need not have kept the plan).
inline std::vector<float> item_major_weights(uint64_t U, uint64_t I, const int64_t* row_ptr, const uint32_t* col, const float* w) {
  std::vector<int64_t> cursor(I + 1, 0);
  for (int64_t p = row_ptr[0]; p < row_ptr[U]; ++p) cursor[col[p] + 1]++;
  for (uint64_t i = 0; i < I; ++i) cursor[i + 1] += cursor[i];
  std::vector<float> t(std::max<size_t>((size_t)(row_ptr[U] - row_ptr[0]), 1), 0.f);
  for (uint64_t u = 0; u < U; ++u)
    for (int64_t p = row_ptr[u]; p < row_ptr[u + 1]; ++p) t[(size_t)cursor[col[p]]++] = w[p];
  return t;
}
// a weight array as cdae_hip_als_set_confidence accepts it: every value finite and >= 0
inline std::string check_weights(const float* w, size_t count) {
  for (size_t p = 0; p < count; ++p)
    if (!(w[p] >= 0.f) || !(w[p] <= 3.402823466e38f)) return refuse("weight %g at position %zu: a confidence weight must be finite and >= 0", (double)w[p], p);
  return {};
}

// the shared (item-side) parameter block: [W | W_ag | (V | V_ag) | bp | bp_ag | b | b_ag], padded element counts
struct ParamLayout {
  size_t off[CDAE_P_COUNT] = {0}, cnt[CDAE_P_COUNT] = {0};
  size_t n_matrix = 0, n_shared = 0;
};
inline ParamLayout param_layout(uint64_t I, uint32_t Kp, bool asymmetric) {
  ParamLayout l;
  const size_t IK = (size_t)I * Kp;
  size_t o = 0;
  auto place = [&](uint32_t id, size_t n) { l.off[id] = o; l.cnt[id] = n; o += n; };
  place(CDAE_P_W, IK); place(CDAE_P_W_AG, IK);
  if (asymmetric) { place(CDAE_P_V, IK); place(CDAE_P_V_AG, IK); }
  l.n_matrix = o;
  place(CDAE_P_BP, I); place(CDAE_P_BP_AG, I);
  place(CDAE_P_B, Kp); place(CDAE_P_B_AG, Kp);
  l.n_shared = o;
  return l;
}

// ---- the whole plan of one cdae_hip_set_interactions call ----
struct Args {
  uint64_t U = 0, I = 0;
  const int64_t* row_ptr = nullptr; const uint32_t* col = nullptr;
  const int64_t* whole_row_ptr = nullptr;   // sampled item shard: row_ptr of the WHOLE rows (else unused)
  uint32_t kind = 0;                        // cdae_hip::mf: 0 CDAE, 1 IMF, 2 BPR, 3 WRMF, 4 WARP (sized as BPR with one more sort key: VOID = I),
                                            // 5 FISM (rows checked as for the SGD handles, but a row may be empty; no example lists, no batch workspace)
  bool mf_seq = false, full_output = false, asymmetric = false, item_shard = false;
  uint32_t batch_users = 0;                 // cdae_hip::B, the default already resolved
  uint32_t K = 0, Kp = 0, num_neg = 0;      // num_neg: HyperParams::num_neg (0 for full output)
  uint64_t I_global = 0, own_u0 = 0, own_u1 = ~0ull;   // item shard: the whole item space, the users whose private rows live here
  double hot_pos = 48.0, late_pos = 48.0;   // CDAE_DECODE_HOT_POS, CDAE_DECODE_LATE_POS
  bool no_late_rows = false, sort_tile = false, sort_library = false, sort_scan = false;   // developer switches (false in the shipped library)
};
struct Plan {
  ActivityOrder act;                        // empty: identity
  const int64_t* row_ptr = nullptr; const uint32_t* col = nullptr;   // the rows as the device gets them: Args' or act's
  uint64_t own_u0 = 0, own_u1 = ~0ull;
  uint32_t B = 0, unit_pos = 0;             // users of the largest batch, min(batch_users, U)
  std::vector<uint64_t> pop;
  std::vector<uint32_t> order, rank_of;
  DecodeSplit split;
  ParamLayout params;
  ItemMajor item_major;                     // WRMF only
  // batch workspace (every kind but WRMF)
  uint32_t ex_per_pos = 1;                  // examples of the batch's item-sorted list per train interaction
  uint64_t emax = 0, Ecap = 0;              // most interactions / examples of any window of B users
  std::vector<uint32_t> unit_ptr, unit_user, gunit_ptr, gunit_user;   // g*: units of a sampled item shard's WHOLE rows
  uint32_t unit_cap = 0;                    // most units of any window of B users, or of any B users (cdae_hip_encode)
  bool counting_sort = false;
  BucketCuts bucket;
  int sort_bits = 1;
};

inline std::string build(const Args& a, Plan& p) {
  const uint64_t U = a.U, I = a.I;
  const bool shard_sampled = a.item_shard && !a.full_output;
  p.row_ptr = a.row_ptr; p.col = a.col;
  if (a.kind && !a.mf_seq && a.batch_users > 1 && U > a.batch_users) {
    std::string e = activity_order(U, a.batch_users, a.row_ptr, a.col, p.act);
    if (!e.empty()) return e;
    p.row_ptr = p.act.row_ptr.data(); p.col = p.act.col.data();       // from here on: rows by POSITION
  }
  std::string e = check_rows(U, I, p.row_ptr, p.col, !a.item_shard && a.kind != 3u, a.kind == 5u, p.pop);
  if (!e.empty()) return e;
  p.own_u0 = a.own_u0; p.own_u1 = a.own_u1;
  if (a.item_shard) {
    if (p.own_u1 == ~0ull) { p.own_u0 = 0; p.own_u1 = U; }
    if (p.own_u0 > p.own_u1 || p.own_u1 > U) return refuse("owned user range [%llu, %llu) outside the %llu users", (unsigned long long)p.own_u0, (unsigned long long)p.own_u1, (unsigned long long)U);
  }
  if (shard_sampled && a.whole_row_ptr[0] != 0) return refuse("whole-row row_ptr[0] must be 0");
  // Work-unit size of the user-parallel kernels (sample, encode, hidden gather, data_loss: one wavefront per unit).  Those
  // launches are latency-bound per wavefront — a unit's rows are gathered a few at a time — so a batch should offer the chip
  // (256 CUs x 4 SIMDs) several thousand wavefronts: small batches take small units.
  const uint32_t B = p.B = (uint32_t)std::min<uint64_t>(a.batch_users, U);
  p.unit_pos = B <= 1024 ? 64u : UNIT_POS_MAX;       // measured at ML-10M shape, batch_users 256 / 512: 64 best (profiles/r02_unit_size.txt)
  if ((uint64_t)B * a.Kp * sizeof(float) > 0x7FFFFFFFull && a.kind != 3u && a.kind != 5u)      // decode addresses z rows with 31-bit byte offsets (buffer loads, cdae_kernels.hpp)
    return refuse("batch_users %u x row stride %u floats exceeds the 2 GiB the batch's Z may occupy; lower batch_users", B, a.Kp);
  const uint64_t nnz = (uint64_t)p.row_ptr[U];
  p.order = popularity_order(p.pop);
  p.rank_of = inverse_order(p.order);
  p.split = decode_split(U, I, a.batch_users, nnz, a.num_neg, p.pop, p.order, a.hot_pos, a.late_pos,
                         a.K <= 256 && !a.kind && !a.full_output && !a.no_late_rows);
  p.params = param_layout(I, a.Kp, a.asymmetric);
  if (a.kind == 3u) {                       // WRMF: no example lists, no batch workspace
    p.item_major = item_major_csr(U, I, p.row_ptr, p.col, p.pop);
    p.unit_ptr.assign(U + 1, 0u);
    return {};
  }
  if (a.kind == 5u) {                       // FISM: its loop draws inside the launch and its encode takes whole rows: no lists, no units
    p.unit_ptr.assign(U + 1, 0u);
    return {};
  }
  // batch workspace sized for the largest batch of B consecutive users
  p.emax = window_max(p.row_ptr, U, B);
  const bool pairs = a.kind == 2u || a.kind == 4u;      // two examples per (positive, k)
  p.ex_per_pos = pairs ? 2u * a.num_neg : 1u + a.num_neg;
  p.Ecap = p.emax * p.ex_per_pos;
  if (shard_sampled) {
    // the example list of a batch is the single-GPU one (every position of the WHOLE rows, every negative draw), entries of other
    // shards' rows VOID: capacity, units and offsets come from the whole rows
    p.Ecap = window_max(a.whole_row_ptr, U, B) * p.ex_per_pos;
    p.gunit_ptr = unit_prefix(a.whole_row_ptr, U, p.unit_pos);
    p.gunit_user = unit_owners(p.gunit_ptr);
  }
  if (p.Ecap > 0xFFFFFFF0ull) return refuse("batch of %u users holds %llu examples (> 2^32); lower batch_users", B, (unsigned long long)p.Ecap);
  const uint64_t keys = I + (shard_sampled || a.kind == 4u ? 1u : 0u);     // (WARP: a skipped pair's two examples carry the VOID key I)
  p.counting_sort = I <= TILE_SORT_MAX_ITEMS && a.sort_tile && a.kind != 4u;
  p.bucket = bucket_cuts(U, I, B, keys, p.Ecap, bucket_max_examples(a.full_output), (double)(shard_sampled ? a.I_global : I),
                         shard_sampled ? (double)a.whole_row_ptr[U] : (double)nnz,
                         pairs ? 2u * a.num_neg : a.num_neg,      // (BPR lists the positive once per pair too: weights only balance, any estimate is legal)
                         p.pop, !p.counting_sort && !a.mf_seq && !a.sort_library && a.kind != 4u /* WARP orders its lists after phase U: the library sort */,
                         !a.kind && !a.sort_scan);
  p.unit_ptr = unit_prefix(p.row_ptr, U, p.unit_pos);
  p.unit_user = unit_owners(p.unit_ptr);
  p.unit_cap = (uint32_t)std::max(window_max(p.unit_ptr.data(), U, B), encode_unit_bound(p.unit_ptr, B));
  if (shard_sampled) p.unit_cap = std::max(p.unit_cap, (uint32_t)window_max(p.gunit_ptr.data(), U, B));   // hidden_gather's partial rows are per unit of the WHOLE rows
  while ((1ull << p.sort_bits) < keys) p.sort_bits++;
  return {};
}

}  // namespace plan
}  // namespace cdae
