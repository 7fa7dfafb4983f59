// Compile-and-link check of libcf::WRMF's confidence weights and objective, and a small end-to-end driver of them:
//   wrmf_weighted_check                                              -> the additions compile and link (no device is touched)
//   wrmf_weighted_check --run=true --input_file=<file> --dump=<file> -> fits WRMF with use_ratings on a GPU through Solver<WRMF>,
//                                                                       prints the objective after every epoch and dumps what a second
//                                                                       implementation needs to repeat the fit: the train CSR, its
//                                                                       weights and the fitted factors
#include <algorithm>
#include <fstream>
#include <iomanip>
#include <utility>

#include <glog/logging.h>
#include <gflags/gflags.h>

#include <base/data.hpp>
#include <model/recsys/wrmf.hpp>
#include <solver/solver.hpp>

DEFINE_string(input_file, "", "user item rating text file (header line skipped)");
DEFINE_string(dump, "", "binary file: U, I, nnz, K (uint64), row_ptr (int64), col (uint32), weights (float), X, Y (float)");
DEFINE_bool(run, false, "fit WRMF on the GPU and check it");
DEFINE_int32(num_dim, 16, "latent dimensions");
DEFINE_int32(iters, 4, "epochs");

namespace {
using namespace libcf;
struct ObjectiveSolver : public Solver<WRMF> {
  ObjectiveSolver(WRMF& m, size_t iters) : Solver<WRMF>(m, iters) {}
  void train_one_iteration(const Data& train) override {
    model_->train_one_iteration(train);
    const std::pair<double, double> o = model_->objective();
    objective.push_back(o.first + o.second);
    LOG(INFO) << "objective after epoch " << objective.size() << ": " << std::setprecision(12) << o.first + o.second << " = data " << o.first
              << " + penalty " << o.second;
  }
  std::vector<double> objective;
};
template <class T> void put(std::ofstream& f, const std::vector<T>& v) { f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T))); }
}  // namespace

int main(int argc, char* argv[]) {
  gflags::ParseCommandLineFlags(&argc, &argv, true);
  typedef std::vector<std::vector<float>> Vecs;
  // the signatures the documents give
  std::pair<double, double> (WRMF::*objective)() const = &WRMF::objective;
  Vecs (WRMF::*solve)(const std::vector<std::vector<size_t>>&, const Vecs&, size_t) const = &WRMF::solve_rows;
  Vecs (WRMF::*solve_w)(const std::vector<std::vector<size_t>>&, const Vecs&, const Vecs&, size_t) const = &WRMF::solve_rows;
  CHECK(objective != nullptr && solve != nullptr && solve_w != nullptr);
  WRMFConfig cfg;
  CHECK(!cfg.use_ratings);
  CHECK_EQ(cfg.lambda, 0.01); CHECK_EQ(cfg.scalar, 40.); CHECK_EQ(cfg.num_dim, size_t(10)); CHECK_EQ(cfg.cg_steps, size_t(3));
  if (!FLAGS_run) { LOG(INFO) << "wrmf weighted check OK (compiled)"; return 0; }

  auto parser = [&](const std::string& line) {
    auto f = split_line(line, " ");
    CHECK_EQ(f.size(), size_t(3));
    return std::vector<std::string>{f[0], f[1], f[2]};
  };
  Data data;
  data.load(FLAGS_input_file, RECSYS, parser, true);
  Random::seed(20141119);
  Data train, test;
  data.random_split_by_feature_group(train, test, 0, 0.2);
  cfg.num_dim = FLAGS_num_dim;
  cfg.lambda = 1.0;
  cfg.scalar = 5.0;
  cfg.use_ratings = true;
  WRMF model(cfg);
  ObjectiveSolver solver(model, FLAGS_iters);
  solver.train(train, test, {TOPN});
  std::shared_ptr<WRMF> trained = solver.get_model();
  CHECK_EQ(solver.objective.size(), static_cast<size_t>(FLAGS_iters));
  for (size_t e = 1; e < solver.objective.size(); ++e) CHECK_LT(solver.objective[e], solver.objective[e - 1]) << "epoch " << e + 1;

  // the train rows and their labels as reset hands them to the device
  const size_t num_users = train.feature_group_total_dimension(0), num_items = train.feature_group_total_dimension(1);
  std::vector<int64_t> ptr; std::vector<uint32_t> col;
  train.to_csr(0, 1, ptr, col);
  const auto labels = train.get_feature_pair_label_hashtable(0, 1);
  std::vector<float> w(col.size());
  float lo = 1e30f, hi = -1e30f;
  for (size_t u = 0; u < num_users; ++u)
    for (int64_t p = ptr[u]; p < ptr[u + 1]; ++p) { w[p] = static_cast<float>(labels.at(u).at(col[p])); lo = std::min(lo, w[p]); hi = std::max(hi, w[p]); }
  CHECK_LT(lo, hi) << "the labels must differ between pairs";

  // a new user with the first user's items AND weights, started from that user's factors, gets that user's next half-step
  const DMatrix X = trained->get_user_vecs(), Y = trained->get_item_vecs();
  std::vector<size_t> items(col.begin() + ptr[0], col.begin() + ptr[1]);
  std::vector<float> wrow(w.begin() + ptr[0], w.begin() + ptr[1]);
  CHECK(!items.empty());
  std::reverse(items.begin(), items.end());                        // any order, the weights with their items
  std::reverse(wrow.begin(), wrow.end());
  Vecs start(1, std::vector<float>(cfg.num_dim));
  for (size_t k = 0; k < cfg.num_dim; ++k) start[0][k] = static_cast<float>(X(0, k));
  const Vecs fitted = trained->solve_rows({items}, Vecs{wrow}, start, 0);
  const Vecs binary = trained->solve_rows({items}, start);

  if (!FLAGS_dump.empty()) {                                       // (before the half-step below moves the user factors)
    std::ofstream f(FLAGS_dump, std::ios::binary);
    put(f, std::vector<uint64_t>{num_users, num_items, col.size(), cfg.num_dim});
    put(f, ptr); put(f, col); put(f, w);
    std::vector<float> xf(num_users * cfg.num_dim), yf(num_items * cfg.num_dim);
    for (size_t u = 0; u < num_users; ++u) for (size_t k = 0; k < cfg.num_dim; ++k) xf[u * cfg.num_dim + k] = static_cast<float>(X(u, k));
    for (size_t i = 0; i < num_items; ++i) for (size_t k = 0; k < cfg.num_dim; ++k) yf[i * cfg.num_dim + k] = static_cast<float>(Y(i, k));
    put(f, xf); put(f, yf);
    CHECK(f.good());
  }

  trained->half_step(CDAE_ALS_USERS);
  const DMatrix X2 = trained->get_user_vecs();
  bool differs = false;
  for (size_t k = 0; k < cfg.num_dim; ++k) {
    CHECK_EQ(fitted[0][k], static_cast<float>(X2(0, k))) << "dimension " << k;
    differs = differs || binary[0][k] != fitted[0][k];
  }
  CHECK(differs) << "the weights changed nothing";
  LOG(INFO) << "wrmf weighted OK (" << num_users << " users, " << num_items << " items, labels " << lo << " .. " << hi << ")";
  return 0;
}
