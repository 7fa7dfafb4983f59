// libcf::FISM (factored item similarity, Kabbur / Ning / Karypis KDD'13) on MI355X: the reference's config struct and class
// (src/model/recsys/fism.hpp:8-20, 29-239) forwarding to libcdae_hip.so (cdae_hip_create_fism; kernels in
// cdae_amd/csrc/cdae_fism_kernels.hpp; include/cdae_hip.h has the definition and the one deliberate difference from the reference:
// x is the sum of the CURRENT rows at the start of every visit, not a per-user table that goes stale).  Solver<FISM> works as
// Solver<WARP> does: TOPN_Evaluation runs on the device over the train rows.
//
//   method (reference lines)             -> C ABI
//   reset (55-89)                         cdae_hip_create_fism, _set_interactions (fills the scale table), _init_params
//   train_one_iteration (91-166)          cdae_hip_train_epoch: the loop, one workgroup
//   recommend (170-199)                   the train row: cdae_hip_recommend_all's table; any other rated set: cdae_hip_recommend_rows
//   predict (201-218)                     cdae_hip_score_rows over the user's row without the item (leave-one-out for a rated item) + bu
// alpha is a real number here (the reference's is an int).  using_factor_term = false and using_global_mean (which predict never
// reads) are refused.  There is no user table: get_user_vecs has nothing to return and CHECK-fails; get_item_vecs is Q, get_input_vecs P.
#ifndef CDAE_HOST_MODEL_RECSYS_FISM_HPP_
#define CDAE_HOST_MODEL_RECSYS_FISM_HPP_

#include <model/recsys/imf.hpp>

namespace libcf {

struct FISMConfig {
  FISMConfig() = default;
  double learn_rate = 0.1;       // (SGDConfig's, which the reference's solver hands to update_one_sgd_step)
  double lambda = 0.01;
  LossType lt = SQUARE;
  PenaltyType pt = L2;
  size_t num_dim = 10;
  size_t num_neg = 5;
  double alpha = 1.;
  bool using_bias_term = true;
  bool using_factor_term = true;
  bool using_global_mean = false;
  bool using_adagrad = true;
};

class FISM : public IMF {
 public:
  FISM(const FISMConfig& mcfg) : alpha_(mcfg.alpha) {
    CHECK(mcfg.using_factor_term) << "FISM without its factor term is not built";
    CHECK(!mcfg.using_global_mean) << "using_global_mean is not taken over (the reference's predict never reads it)";
    IMFConfig c;
    c.learn_rate = mcfg.learn_rate; c.beta = 0.; c.lambda = mcfg.lambda; c.lt = mcfg.lt; c.pt = mcfg.pt;
    c.num_dim = mcfg.num_dim; c.num_neg = mcfg.num_neg; c.using_bias_term = mcfg.using_bias_term; c.using_adagrad = mcfg.using_adagrad;
    configure(c, false, "FISM");
  }

  virtual void reset(const Data& data_set) {
    ModelBase::reset(data_set);
    num_users_ = data_->feature_group_total_dimension(0);
    num_items_ = data_->feature_group_total_dimension(1);
    cdae_fism_config c = cdae_fism_config();
    c.struct_size = sizeof(c);
    c.num_dim = static_cast<uint32_t>(num_dim_); c.num_neg = static_cast<uint32_t>(num_neg_);
    c.loss_type = static_cast<uint32_t>(lt_);
    c.using_adagrad = using_adagrad_; c.using_bias_term = using_bias_term_;
    c.batch_users = 1;
    c.lambda = lambda_; c.learn_rate = learn_rate_; c.alpha = alpha_;
    cdae_hip_t* raw = nullptr;
    CDAE_HIP_CHECK(create_handle(&c, static_cast<int>(mf_env_u64("CDAE_DEVICE", 0)), &raw));
    dev_.reset(raw, [](cdae_hip_t* h) { cdae_hip_destroy(h); });
    auto csr = std::make_shared<Csr>();
    data_->to_csr(0, 1, csr->row_ptr, csr->col);
    CDAE_HIP_CHECK(cdae_hip_set_interactions(raw, num_users_, num_items_, csr->row_ptr.data(), csr->col.data()));
    csr_ = csr;
    train_generation_ = data_->generation();
    test_generation_ = std::make_shared<uint64_t>(0);
    seed_ = std::getenv("CDAE_SEED") ? mf_env_u64("CDAE_SEED", 0) : Random::next_u64();
    CDAE_HIP_CHECK(cdae_hip_init_params(raw, seed_));
    epoch_ = 0;
    invalidate();
  }

  virtual void train_one_iteration(const Data&) {
    CHECK(dev_ != nullptr) << "reset() must be called first";
    cdae_hip_stats st;
    CDAE_HIP_CHECK(cdae_hip_train_epoch(dev_.get(), seed_, epoch_++, &st));
    LOG(INFO) << "FISM epoch " << epoch_ << ": " << st.users << " users, " << st.examples << " instances in " << st.wall_seconds << " s ("
              << static_cast<double>(st.examples) / st.wall_seconds << " instances/s, " << st.batches << " launches)";
    invalidate();
  }

  // fism.hpp:170-199 for any rated set; bu is constant within the list and takes no part
  std::vector<size_t> recommend(size_t uid, size_t topk, const std::unordered_map<size_t, double>& rated) const {
    CHECK_LT(uid, num_users_);
    if (is_train_row(uid, rated)) return recommend_train_row(uid, topk);
    std::vector<uint32_t> col;
    for (const auto& kv : rated) col.push_back(static_cast<uint32_t>(kv.first));
    std::sort(col.begin(), col.end());
    const int64_t ptr[2] = {0, static_cast<int64_t>(col.size())};
    std::vector<uint32_t> ids(topk);
    std::lock_guard<std::mutex> lk(*mu_);
    CHECK(dev_ != nullptr) << "reset() must be called first";
    CDAE_HIP_CHECK(cdae_hip_recommend_rows(dev_.get(), 1, nullptr, ptr, col.data(), static_cast<uint32_t>(topk), ids.data(), nullptr));
    return std::vector<size_t>(ids.begin(), ids.end());
  }

  // fism.hpp:201-218: a rated item is scored leave-one-out, from the (n - 1) other rows
  double predict_user_item_rating(size_t uid, size_t iid) const {
    CHECK(dev_ != nullptr);
    CHECK_LT(uid, num_users_); CHECK_LT(iid, num_items_);
    std::vector<uint32_t> col;
    for (int64_t p = csr_->row_ptr[uid]; p < csr_->row_ptr[uid + 1]; ++p)
      if (csr_->col[p] != iid) col.push_back(csr_->col[p]);
    const int64_t ptr[2] = {0, static_cast<int64_t>(col.size())}, cptr[2] = {0, 1};
    const uint32_t cand = static_cast<uint32_t>(iid);
    float score = 0.f;
    std::vector<float> bu(num_users_);
    std::lock_guard<std::mutex> lk(*mu_);
    CDAE_HIP_CHECK(cdae_hip_score_rows(dev_.get(), 1, nullptr, ptr, col.data(), cptr, &cand, &score, nullptr));
    fetch(CDAE_P_UB, bu);
    return static_cast<double>(score) + bu[uid];
  }
  DMatrix get_user_vecs() { CHECK(false) << "a FISM model has no user table: a user is the sum of the input rows of their items"; return DMatrix(); }
  DMatrix get_item_vecs() { return matrix(CDAE_P_V, num_items_); }        // q_
  DMatrix get_input_vecs() { return matrix(CDAE_P_W, num_items_); }       // p_

 protected:
  // which entry point makes the handle (libcf::FISMP, fism_pair.hpp: cdae_hip_create_fism_pair)
  virtual int create_handle(const cdae_fism_config* c, int device, cdae_hip_t** out) const { return cdae_hip_create_fism(c, device, out); }
  double alpha_ = 1.;
};

}  // namespace libcf
#endif
