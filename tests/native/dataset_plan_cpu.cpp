// CPU slice of cdae_hip_set_interactions' data-set plan for tests/test_dataset_plan_cpu.py and tests/test_gpu_dataset_plan.py: the SAME
// header cdae_hip.hip compiles (cdae_amd/csrc/cdae_dataset_plan.h) behind a C ABI for ctypes.  Test infrastructure.
#include <cstring>

#include "../../cdae_amd/csrc/cdae_dataset_plan.h"

using namespace cdae;

extern "C" {

// the limits the plan reads, by the order of dp_limit_names() (so that no test hard-codes one)
const char* dp_limit_names() {
  return "LATE_MAX LATE_BITS_WORDS UNIT_POS_MAX BKC_MAX_RANGES BKC_ITEM_BITS BK_ITEMS BK_MAX_RANGES BK_CELL_UNITS_MAX TILE_SORT_MAX_ITEMS DUP_STRIPES "
         "BUCKET_MAX_EXAMPLES_SAMPLED BUCKET_MAX_EXAMPLES_FULL";
}
void dp_limits(uint64_t* out) {
  const uint64_t v[] = {LATE_MAX, LATE_BITS_WORDS, UNIT_POS_MAX, BKC_MAX_RANGES, BKC_ITEM_BITS, BK_ITEMS, BK_MAX_RANGES, BK_CELL_UNITS_MAX,
                        TILE_SORT_MAX_ITEMS, DUP_STRIPES, plan::bucket_max_examples(false), plan::bucket_max_examples(true)};
  std::memcpy(out, v, sizeof v);
}

// plan::Args, flattened (the order tests/plan_ref.py ARGS lists)
struct dp_args {
  uint64_t U, I;
  const int64_t* row_ptr; const uint32_t* col; const int64_t* whole_row_ptr;
  uint32_t kind, mf_seq, full_output, asymmetric, item_shard, batch_users, K, Kp, num_neg;
  uint64_t I_global, own_u0, own_u1;
  double hot_pos, late_pos;
  uint32_t no_late_rows, sort_tile, sort_library, sort_scan;
};

// the whole plan: nullptr and the refusal's text in err, or a plan to read with dp_scalars / dp_field and to give back to dp_free
void* dp_build(const dp_args* d, char* err, size_t err_cap) {
  plan::Args a;
  a.U = d->U; a.I = d->I; a.row_ptr = d->row_ptr; a.col = d->col; a.whole_row_ptr = d->whole_row_ptr;
  a.kind = d->kind; a.mf_seq = d->mf_seq; a.full_output = d->full_output; a.asymmetric = d->asymmetric; a.item_shard = d->item_shard;
  a.batch_users = d->batch_users; a.K = d->K; a.Kp = d->Kp; a.num_neg = d->num_neg;
  a.I_global = d->I_global; a.own_u0 = d->own_u0; a.own_u1 = d->own_u1;
  a.hot_pos = d->hot_pos; a.late_pos = d->late_pos;
  a.no_late_rows = d->no_late_rows; a.sort_tile = d->sort_tile; a.sort_library = d->sort_library; a.sort_scan = d->sort_scan;
  plan::Plan* p = new plan::Plan;
  const std::string e = plan::build(a, *p);
  std::snprintf(err, err_cap, "%s", e.c_str());
  if (e.empty()) return p;
  delete p;
  return nullptr;
}
void dp_free(void* p) { delete (plan::Plan*)p; }

void dp_scalars(const void* vp, uint64_t* out /* [16], the order tests/plan_ref.py SCALARS lists */) {
  const plan::Plan& p = *(const plan::Plan*)vp;
  const uint64_t v[16] = {p.own_u0, p.own_u1, p.B, p.unit_pos, p.split.hot_rows, p.split.late_rows, p.ex_per_pos, p.emax, p.Ecap, p.unit_cap,
                          p.counting_sort, p.bucket.on, (uint64_t)p.sort_bits, p.params.n_matrix, p.params.n_shared, !p.act.user_perm.empty()};
  std::memcpy(out, v, sizeof v);
}

// array f of the plan (the order tests/plan_ref.py FIELDS lists): its size in bytes; copied to out when out is not null
size_t dp_field(const void* vp, int f, void* out) {
  const plan::Plan& p = *(const plan::Plan*)vp;
  auto give = [&](const void* src, size_t bytes) { if (out && bytes) std::memcpy(out, src, bytes); return bytes; };
  auto vec = [&](const auto& v) { return give(v.data(), v.size() * sizeof(v[0])); };
  switch (f) {
    case 0: return vec(p.act.user_perm);
    case 1: return vec(p.act.user_inv);
    case 2: return vec(p.act.row_ptr);
    case 3: return vec(p.act.col);
    case 4: return vec(p.pop);
    case 5: return vec(p.order);
    case 6: return vec(p.rank_of);
    case 7: return vec(p.split.rank_len);
    case 8: return vec(p.split.late_bits);
    case 9: return vec(p.unit_ptr);
    case 10: return vec(p.unit_user);
    case 11: return vec(p.gunit_ptr);
    case 12: return vec(p.gunit_user);
    case 13: return vec(p.bucket.cut);
    case 14: return vec(p.bucket.range_of);
    case 15: return vec(p.item_major.ptr);
    case 16: return vec(p.item_major.col);
    case 17: { uint64_t v[CDAE_P_COUNT]; for (uint32_t i = 0; i < CDAE_P_COUNT; ++i) v[i] = p.params.off[i]; return give(v, sizeof v); }
    case 18: { uint64_t v[CDAE_P_COUNT]; for (uint32_t i = 0; i < CDAE_P_COUNT; ++i) v[i] = p.params.cnt[i]; return give(v, sizeof v); }
  }
  return 0;
}

// single rules, for inputs no data set reaches through dp_build
uint64_t dp_window_max_i64(const int64_t* prefix, uint64_t U, uint64_t B) { return plan::window_max(prefix, U, B); }
uint64_t dp_window_max_u32(const uint32_t* prefix, uint64_t U, uint64_t B) { return plan::window_max(prefix, U, B); }

// bucket_cuts over a popularity array: returns on | cells << 1, the number of ranges in *ranges, the cuts in cut (room for I + 1), the table in range_of (room for I)
uint32_t dp_bucket_cuts(uint64_t U, uint64_t I, uint32_t B, uint64_t keys, uint64_t Ecap, uint64_t max_examples, double draw_items, double whole_nnz,
                        uint32_t negs, const uint64_t* pop, uint32_t allowed, uint32_t cells_allowed, uint32_t* ranges, uint32_t* cut, uint16_t* range_of) {
  const plan::BucketCuts k = plan::bucket_cuts(U, I, B, keys, Ecap, max_examples, draw_items, whole_nnz, negs, std::vector<uint64_t>(pop, pop + I),
                                               allowed != 0, cells_allowed != 0);
  *ranges = k.on ? (uint32_t)k.cut.size() - 1 : 0u;
  if (!k.cut.empty()) std::memcpy(cut, k.cut.data(), k.cut.size() * sizeof(uint32_t));
  if (!k.range_of.empty()) std::memcpy(range_of, k.range_of.data(), k.range_of.size() * sizeof(uint16_t));
  return (k.on ? 1u : 0u) | (k.range_of.empty() ? 0u : 2u);
}

}
