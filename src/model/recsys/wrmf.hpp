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
//   solve_rows (with weights)             cdae_hip_als_solve_rows_weighted: the same with one confidence weight per item
//   objective                             cdae_hip_als_objective: the data term and the penalty the half-steps minimise
// WRMFConfig::use_ratings (not in the reference's struct; wrmf.hpp:76-96 multiplies by rating * scalar_): reset passes the Data labels,
// in the order of to_csr, to cdae_hip_als_set_confidence — confidence 1 + scalar * label on a stored pair.  The default is binary.
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
  bool use_ratings = false;  // not in the reference's struct: the labels are per-pair confidence weights (1 + scalar * label)
};

class WRMF : public IMF {
 public:
  explicit WRMF(const WRMFConfig& mcfg) : scalar_(mcfg.scalar), cg_steps_(mcfg.cg_steps), use_ratings_(mcfg.use_ratings) {
    lambda_ = mcfg.lambda; num_dim_ = mcfg.num_dim; lt_ = mcfg.lt;
    loss_ = Loss::create(mcfg.lt);
    penalty_ = Penalty::create(mcfg.pt);
    LOG(INFO) << "WRMF Configure (MI355X / HIP): \n"
              << "\t{lambda: " << lambda_ << "}, {Loss: " << loss_->loss_type() << "}, {Penalty: " << penalty_->penalty_type() << "}\n"
              << "\t{Dim: " << num_dim_ << "}, {Scalar: " << scalar_ << "}, {CG steps: " << cg_steps_ << "}, {Ratings: " << use_ratings_ << "}";
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
    if (use_ratings_) {                                       // the labels in the order of to_csr (a repeated pair: its first label)
      const auto labels = data_->get_feature_pair_label_hashtable(0, 1);
      std::vector<float> w(csr->col.size());
      for (size_t u = 0; u < num_users_; ++u) {
        if (csr->row_ptr[u + 1] == csr->row_ptr[u]) continue;
        const auto& row = labels.at(u);
        for (int64_t p = csr->row_ptr[u]; p < csr->row_ptr[u + 1]; ++p) w[p] = static_cast<float>(row.at(csr->col[p]));
      }
      CDAE_HIP_CHECK(cdae_hip_als_set_confidence(raw, w.data(), w.size()));
    }
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
    return solve_rows_impl(rows, nullptr, start, cg_steps);
  }
  // ... with per-pair confidence weights: weights[r][k] belongs to rows[r][k] (the caller's weights, not the model's)
  std::vector<std::vector<float>> solve_rows(const std::vector<std::vector<size_t>>& rows, const std::vector<std::vector<float>>& weights,
                                            const std::vector<std::vector<float>>& start, size_t cg_steps) const {
    CHECK_EQ(weights.size(), rows.size());
    return solve_rows_impl(rows, &weights, start, cg_steps);
  }

  // {data term, penalty term} of the objective the half-steps minimise, under the model's confidences (cdae_hip_als_objective)
  std::pair<double, double> objective() const {
    std::lock_guard<std::mutex> lk(*mu_);
    CHECK(dev_ != nullptr) << "reset() must be called first";
    double out[2] = {0., 0.};
    CDAE_HIP_CHECK(cdae_hip_als_objective(dev_.get(), out));
    return std::make_pair(out[0], out[1]);
  }

 protected:
  std::vector<std::vector<float>> solve_rows_impl(const std::vector<std::vector<size_t>>& rows, const std::vector<std::vector<float>>* weights,
                                                 const std::vector<std::vector<float>>& start, size_t cg_steps) const {
    std::lock_guard<std::mutex> lk(*mu_);
    CHECK(dev_ != nullptr) << "reset() must be called first";
    CHECK(start.empty() || start.size() == rows.size());
    std::vector<int64_t> ptr(rows.size() + 1, 0);
    std::vector<uint32_t> col;
    std::vector<float> w;
    for (size_t r = 0; r < rows.size(); ++r) {
      std::vector<std::pair<uint32_t, float>> s(rows[r].size());
      if (weights) CHECK_EQ((*weights)[r].size(), rows[r].size());
      for (size_t k = 0; k < s.size(); ++k) s[k] = std::make_pair(static_cast<uint32_t>(rows[r][k]), weights ? (*weights)[r][k] : 1.f);
      std::sort(s.begin(), s.end());
      for (const auto& e : s) { col.push_back(e.first); w.push_back(e.second); }
      ptr[r + 1] = static_cast<int64_t>(col.size());
    }
    std::vector<float> x0, out(rows.size() * num_dim_);
    for (const std::vector<float>& v : start) {
      CHECK_EQ(v.size(), num_dim_);
      x0.insert(x0.end(), v.begin(), v.end());
    }
    if (weights)
      CDAE_HIP_CHECK(cdae_hip_als_solve_rows_weighted(dev_.get(), rows.size(), ptr.data(), col.data(), w.data(), start.empty() ? nullptr : x0.data(),
                                                      static_cast<uint32_t>(cg_steps), out.data()));
    else
      CDAE_HIP_CHECK(cdae_hip_als_solve_rows(dev_.get(), rows.size(), ptr.data(), col.data(), start.empty() ? nullptr : x0.data(),
                                             static_cast<uint32_t>(cg_steps), out.data()));
    std::vector<std::vector<float>> ret(rows.size());
    for (size_t r = 0; r < rows.size(); ++r) ret[r].assign(out.begin() + r * num_dim_, out.begin() + (r + 1) * num_dim_);
    return ret;
  }

  double scalar_ = 40.;
  size_t cg_steps_ = 3;
  bool use_ratings_ = false;
};

}  // namespace libcf
#endif
