// libcf::WARP (rank-weighted pairwise matrix factorisation) on MI355X: the reference's config struct and class
// (src/model/recsys/warp.hpp:12-23, 25-122) — an IMF whose training loop searches, per (positive, k), for a negative that violates the
// margin and weights the step by the harmonic number of items_left / draws — forwarding to libcdae_hip.so (cdae_hip_create_warp;
// kernels in cdae_amd/csrc/cdae_warp_kernels.hpp; include/cdae_hip.h has the definition).  Everything IMF serves — recommend,
// TOPN_Evaluation on the device, similar_items, get_user_vecs / get_item_vecs — is inherited, and Solver<WARP> works as Solver<IMF> does.
//
//   method (reference lines)             -> C ABI
//   reset (53-61)                         cdae_hip_create_warp, _set_interactions (fills the rank weights), _init_params (IMF's)
//   train_one_iteration (63-117)          cdae_hip_train_epoch; batch_users = 1, the reference loop, unless CDAE_BATCH_USERS says otherwise
//   search                                cdae_hip_warp_search: the negative every pair would train on now (hard-negative mining)
// beta and using_bias_term are accepted as the reference accepts them and change nothing: warp.hpp never reads beta in its AdaGrad step
// and its bias steps are comments.
#ifndef CDAE_HOST_MODEL_RECSYS_WARP_HPP_
#define CDAE_HOST_MODEL_RECSYS_WARP_HPP_

#include <model/recsys/imf.hpp>

namespace libcf {

struct WARPConfig {
  WARPConfig() = default;
  double learn_rate = 0.1;
  double beta = 0.;
  double lambda = 0.1;
  LossType lt = HINGE;
  PenaltyType pt = L2;
  size_t num_dim = 10;
  size_t num_neg = 5;
  bool using_bias_term = true;
  bool using_adagrad = true;
};

class WARP : public IMF {
 public:
  WARP(const WARPConfig& mcfg) {
    IMFConfig c;
    c.learn_rate = mcfg.learn_rate; c.beta = mcfg.beta; c.lambda = mcfg.lambda; c.lt = mcfg.lt; c.pt = mcfg.pt;
    c.num_dim = mcfg.num_dim; c.num_neg = mcfg.num_neg; c.using_bias_term = mcfg.using_bias_term; c.using_adagrad = mcfg.using_adagrad;
    configure(c, true, "WARP");
  }

  virtual void reset(const Data& data_set) {
    ModelBase::reset(data_set);
    num_users_ = data_->feature_group_total_dimension(0);
    num_items_ = data_->feature_group_total_dimension(1);
    cdae_warp_config c = cdae_warp_config();
    c.struct_size = sizeof(c);
    c.num_dim = static_cast<uint32_t>(num_dim_); c.num_neg = static_cast<uint32_t>(num_neg_);
    c.loss_type = static_cast<uint32_t>(lt_);
    c.using_adagrad = using_adagrad_;
    c.batch_users = static_cast<uint32_t>(mf_env_u64("CDAE_BATCH_USERS", 1));   // the drop-in default is the reference loop, as for IMF / BPR
    c.lambda = lambda_; c.learn_rate = learn_rate_;
    cdae_hip_t* raw = nullptr;
    CDAE_HIP_CHECK(cdae_hip_create_warp(&c, static_cast<int>(mf_env_u64("CDAE_DEVICE", 0)), &raw));
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
    LOG(INFO) << "WARP epoch " << epoch_ << ": " << st.users << " users in " << st.wall_seconds << " s ("
              << static_cast<double>(st.users) / st.wall_seconds << " users/s, " << st.batches << " blocks)";
    invalidate();
  }

  // The negative every (user, positive, k) would train on with the draws of the NEXT epoch, against the current parameters: items[q] and
  // draws[q] with q = (index of the positive in the train rows) * num_neg + k; draws == CDAE_WARP_MAX_TRY: no violator among the draws
  // (items 0xFFFFFFFF).  Positions are user ids while batch_users is 1 (cdae_hip_user_order otherwise).
  void search(std::vector<uint32_t>& items, std::vector<uint32_t>& draws) const {
    std::lock_guard<std::mutex> lk(*mu_);
    CHECK(dev_ != nullptr) << "reset() must be called first";
    const size_t n = static_cast<size_t>(csr_->row_ptr[num_users_]) * num_neg_;
    items.resize(n); draws.resize(n);
    CDAE_HIP_CHECK(cdae_hip_warp_search(dev_.get(), seed_, epoch_, 0, num_users_, items.data(), draws.data(), nullptr, n));
  }
};

}  // namespace libcf
#endif
