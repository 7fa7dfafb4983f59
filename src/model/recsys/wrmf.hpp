// libcf::WRMF (weighted-regularised matrix factorisation by alternating least squares) on MI355X: the reference's config struct
// (src/model/recsys/wrmf.hpp:9-16) plus cg_steps, and a class with its constructor and public methods that forwards to
// libcdae_hip.so (cdae_hip_create_als; kernels in cdae_amd/csrc/cdae_als_kernels.hpp; include/cdae_hip.h has the definition).
// It is an IMF whose handle is fitted by half-steps instead of the sampled loop, so everything IMF serves — recommend,
// TOPN_Evaluation on the device, similar_items, get_user_vecs / get_item_vecs — is inherited, and Solver<WRMF> works as Solver<IMF> does.
//
//   method (reference lines)             -> C ABI
//   reset (41-52)                         cdae_hip_create_als, _set_interactions, _init_params (Random() * 0.001)
//   train_one_iteration (102-109)         cdae_hip_train_epoch: the user half-step, then the item half-step
//   half_step                             cdae_hip_als_half_step
//   solve_rows                            cdae_hip_als_solve_rows: factors of rows outside the training set
// The system solved per row is the paper's, G + alpha sum y y^T + lambda I with G = Y^T Y, by cg_steps iterations of conjugate
// gradients.  The reference's literal train_one_index (66-100) omits the Y^T Y term and is deliberately not offered (cdae_hip.h).
#ifndef CDAE_HOST_MODEL_RECSYS_WRMF_HPP_
#define CDAE_HOST_MODEL_RECSYS_WRMF_HPP_

#include <model/recsys/imf.hpp>

namespace libcf {

struct WRMFConfig {
  WRMFConfig() = default;
  double lambda = 0.01;
  double scalar = 40;        // alpha: confidence 1 + scalar on a stored pair
  LossType lt = SQUARE;
  PenaltyType pt = L2;
  size_t num_dim = 10;
  size_t cg_steps = 3;       // not in the reference: conjugate-gradient iterations per row and half-step
};

class WRMF : public IMF {
 public:
  explicit WRMF(const WRMFConfig& mcfg) : scalar_(mcfg.scalar), cg_steps_(mcfg.cg_steps) {
    lambda_ = mcfg.lambda; num_dim_ = mcfg.num_dim; lt_ = mcfg.lt;
    loss_ = Loss::create(mcfg.lt);
    penalty_ = Penalty::create(mcfg.pt);
    LOG(INFO) << "WRMF Configure (MI355X / HIP): \n"
              << "\t{lambda: " << lambda_ << "}, {Loss: " << loss_->loss_type() << "}, {Penalty: " << penalty_->penalty_type() << "}\n"
              << "\t{Dim: " << num_dim_ << "}, {Scalar: " << scalar_ << "}, {CG steps: " << cg_steps_ << "}";
  }
  WRMF() : WRMF(WRMFConfig()) {}

  virtual void reset(const Data& data_set) {
    ModelBase::reset(data_set);
    num_users_ = data_->feature_group_total_dimension(0);
    num_items_ = data_->feature_group_total_dimension(1);
    cdae_als_config c = cdae_als_config();
    c.struct_size = sizeof(c);
    c.num_dim = static_cast<uint32_t>(num_dim_); c.cg_steps = static_cast<uint32_t>(cg_steps_);
    c.lambda = lambda_; c.alpha = scalar_;
    cdae_hip_t* raw = nullptr;
    CDAE_HIP_CHECK(cdae_hip_create_als(&c, static_cast<int>(mf_env_u64("CDAE_DEVICE", 0)), &raw));
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
    CDAE_HIP_CHECK(cdae_hip_train_epoch(dev_.get(), 0, epoch_++, &st));
    LOG(INFO) << "WRMF epoch " << epoch_ << ": " << st.users << " users, " << st.batches << " half-steps in " << st.wall_seconds << " s";
    invalidate();
  }

  // one half-step: CDAE_ALS_USERS or CDAE_ALS_ITEMS
  void half_step(uint32_t side) {
    CHECK(dev_ != nullptr) << "reset() must be called first";
    CDAE_HIP_CHECK(cdae_hip_als_half_step(dev_.get(), side));
    invalidate();
  }

  // Factors of rows outside the training set against the frozen item table, in ONE device call: rows[r] the items of row r (any
  // order, no duplicates), start empty (zeros) or one num_dim vector per row -> one num_dim vector per row.  cg_steps 0: the model's.
  std::vector<std::vector<float>> solve_rows(const std::vector<std::vector<size_t>>& rows,
                                            const std::vector<std::vector<float>>& start = std::vector<std::vector<float>>(),
                                            size_t cg_steps = 0) const {
    std::lock_guard<std::mutex> lk(*mu_);
    CHECK(dev_ != nullptr) << "reset() must be called first";
    CHECK(start.empty() || start.size() == rows.size());
    std::vector<int64_t> ptr(rows.size() + 1, 0);
    std::vector<uint32_t> col;
    for (size_t r = 0; r < rows.size(); ++r) {
      std::vector<uint32_t> s(rows[r].begin(), rows[r].end());
      std::sort(s.begin(), s.end());
      col.insert(col.end(), s.begin(), s.end());
      ptr[r + 1] = static_cast<int64_t>(col.size());
    }
    std::vector<float> x0, out(rows.size() * num_dim_);
    for (const std::vector<float>& v : start) {
      CHECK_EQ(v.size(), num_dim_);
      x0.insert(x0.end(), v.begin(), v.end());
    }
    CDAE_HIP_CHECK(cdae_hip_als_solve_rows(dev_.get(), rows.size(), ptr.data(), col.data(), start.empty() ? nullptr : x0.data(),
                                           static_cast<uint32_t>(cg_steps), out.data()));
    std::vector<std::vector<float>> ret(rows.size());
    for (size_t r = 0; r < rows.size(); ++r) ret[r].assign(out.begin() + r * num_dim_, out.begin() + (r + 1) * num_dim_);
    return ret;
  }

 protected:
  double scalar_ = 40.;
  size_t cg_steps_ = 3;
};

}  // namespace libcf
#endif
