// libcf::FISMP (FISMauc, the pairwise form of FISM: Kabbur / Ning / Karypis KDD'13) on MI355X: the reference's config struct and
// class names (src/model/recsys/fism_pair.hpp) forwarding to libcdae_hip.so (cdae_hip_create_fism_pair; kernel in
// cdae_amd/csrc/cdae_fism_pair_kernels.hpp; include/cdae_hip.h has the definition and what differs from the reference file, which does
// not compile as it stands).  Everything but the training loop is libcf::FISM's (fism.hpp): reset, recommend over any rated set, the
// tables.  A pair handle has no user bias, so predict_user_item_rating is the served score alone.
#ifndef CDAE_HOST_MODEL_RECSYS_FISM_PAIR_HPP_
#define CDAE_HOST_MODEL_RECSYS_FISM_PAIR_HPP_

#include <model/recsys/fism.hpp>

namespace libcf {

struct FISMPConfig : public FISMConfig {     // the reference's defaults: lambda 0.01, SQUARE, 10 dimensions, 5 negatives, alpha 1, AdaGrad, bias
  FISMPConfig() = default;
};

class FISMP : public FISM {
 public:
  FISMP(const FISMPConfig& mcfg) : FISM(mcfg) {}

  virtual void train_one_iteration(const Data&) {
    CHECK(dev_ != nullptr) << "reset() must be called first";
    cdae_hip_stats st;
    CDAE_HIP_CHECK(cdae_hip_train_epoch(dev_.get(), seed_, epoch_++, &st));
    LOG(INFO) << "FISMP epoch " << epoch_ << ": " << st.users << " users, " << st.examples << " pairs in " << st.wall_seconds << " s ("
              << static_cast<double>(st.examples) / st.wall_seconds << " pairs/s, " << st.batches << " launches)";
    invalidate();
  }

  // a rated item is scored leave-one-out, from the (n - 1) other rows; there is no bu to add
  double predict_user_item_rating(size_t uid, size_t iid) const {
    CHECK(dev_ != nullptr);
    CHECK_LT(uid, num_users_); CHECK_LT(iid, num_items_);
    std::vector<uint32_t> col;
    for (int64_t p = csr_->row_ptr[uid]; p < csr_->row_ptr[uid + 1]; ++p)
      if (csr_->col[p] != iid) col.push_back(csr_->col[p]);
    const int64_t ptr[2] = {0, static_cast<int64_t>(col.size())}, cptr[2] = {0, 1};
    const uint32_t cand = static_cast<uint32_t>(iid);
    float score = 0.f;
    std::lock_guard<std::mutex> lk(*mu_);
    CDAE_HIP_CHECK(cdae_hip_score_rows(dev_.get(), 1, nullptr, ptr, col.data(), cptr, &cand, &score, nullptr));
    return static_cast<double>(score);
  }

 protected:
  virtual int create_handle(const cdae_fism_config* c, int device, cdae_hip_t** out) const { return cdae_hip_create_fism_pair(c, device, out); }
};

}  // namespace libcf
#endif
