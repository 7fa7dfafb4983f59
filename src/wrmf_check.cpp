// Compile-and-link check of libcf::WRMF, and a small end-to-end driver of it:
//   wrmf_check                                  -> the class compiles and links (no device is touched)
//   wrmf_check --run=true --input_file=<file>   -> fits WRMF on a GPU through Solver<WRMF> with TOPN and checks the INTEGRATION.md recipe
#include <algorithm>
#include <set>

#include <glog/logging.h>
#include <gflags/gflags.h>

#include <base/data.hpp>
#include <model/recsys/wrmf.hpp>
#include <solver/solver.hpp>

DEFINE_string(input_file, "", "user item text file (header line skipped)");
DEFINE_bool(run, false, "fit WRMF on the GPU and check it");
DEFINE_int32(num_dim, 16, "latent dimensions");
DEFINE_int32(iters, 3, "epochs");

int main(int argc, char* argv[]) {
  using namespace libcf;
  gflags::ParseCommandLineFlags(&argc, &argv, true);
  typedef std::vector<std::vector<float>> Vecs;
  // the signatures the documents give
  void (WRMF::*half)(uint32_t) = &WRMF::half_step;
  Vecs (WRMF::*solve)(const std::vector<std::vector<size_t>>&, const Vecs&, size_t) const = &WRMF::solve_rows;
  CHECK(half != nullptr && solve != nullptr);
  WRMFConfig cfg;
  CHECK_EQ(cfg.lambda, 0.01); CHECK_EQ(cfg.scalar, 40.); CHECK_EQ(cfg.num_dim, size_t(10)); CHECK_EQ(cfg.cg_steps, size_t(3));
  CHECK_EQ(sizeof(cdae_als_config), size_t(32));
  if (!FLAGS_run) { LOG(INFO) << "wrmf check OK (compiled)"; return 0; }

  auto parser = [&](const std::string& line) {
    auto f = split_line(line, " ");
    CHECK_EQ(f.size(), size_t(2));
    return std::vector<std::string>{f[0], f[1], "1"};
  };
  Data data;
  data.load(FLAGS_input_file, RECSYS, parser, true);
  Random::seed(20141119);
  Data train, test;
  data.random_split_by_feature_group(train, test, 0, 0.2);
  cfg.num_dim = FLAGS_num_dim;
  cfg.lambda = 1.0;
  WRMF model(cfg);
  Solver<WRMF> solver(model, FLAGS_iters);
  solver.train(train, test, {TOPN});
  std::shared_ptr<WRMF> trained = solver.get_model();
  const size_t num_users = train.feature_group_total_dimension(0), num_items = train.feature_group_total_dimension(1), topk = 10;

  // a fitted model: the users' lists hold topk distinct items, none of them from the train row
  const DMatrix X = trained->get_user_vecs(), Y = trained->get_item_vecs();
  CHECK_EQ(static_cast<size_t>(X.rows()), num_users); CHECK_EQ(static_cast<size_t>(Y.rows()), num_items);
  double norm = 0.;
  for (size_t i = 0; i < num_users * cfg.num_dim; ++i) norm += X.data()[i] * X.data()[i];
  CHECK_GT(norm, 1e-3) << "the user factors are still the initial ones";
  for (size_t u = 0; u < num_users; u += 7) {
    const std::vector<size_t> list = trained->recommend_train_row(u, topk);
    CHECK_EQ(std::set<size_t>(list.begin(), list.end()).size(), topk);
  }
  // a half-step moves the side it solves and nothing else
  trained->half_step(CDAE_ALS_USERS);
  const DMatrix X2 = trained->get_user_vecs(), Y2 = trained->get_item_vecs();
  bool x_moved = false, y_moved = false;
  for (size_t i = 0; i < num_users * cfg.num_dim; ++i) x_moved = x_moved || X.data()[i] != X2.data()[i];
  for (size_t i = 0; i < num_items * cfg.num_dim; ++i) y_moved = y_moved || Y.data()[i] != Y2.data()[i];
  CHECK(x_moved && !y_moved);
  // a new user with the first user's items, started from that user's factors, gets that user's next half-step
  std::vector<size_t> items;
  const auto rated = train.get_feature_pair_label_hashtable(0, 1);
  for (size_t i = 0; i < num_items; ++i) if (rated.at(0).count(i)) items.push_back(i);
  CHECK(!items.empty());
  std::reverse(items.begin(), items.end());                        // any order
  Vecs start(1, std::vector<float>(cfg.num_dim));
  for (size_t k = 0; k < cfg.num_dim; ++k) start[0][k] = static_cast<float>(X2(0, k));
  const Vecs fitted = trained->solve_rows({items}, start);
  trained->half_step(CDAE_ALS_USERS);
  const DMatrix X3 = trained->get_user_vecs();
  for (size_t k = 0; k < cfg.num_dim; ++k) CHECK_EQ(fitted[0][k], static_cast<float>(X3(0, k))) << "dimension " << k;
  const Vecs cold = trained->solve_rows({items, std::vector<size_t>()});
  CHECK_EQ(cold.size(), size_t(2));
  for (size_t k = 0; k < cfg.num_dim; ++k) CHECK_EQ(cold[1][k], 0.f);   // a row without items returns its start vector
  LOG(INFO) << "wrmf OK (" << num_users << " users, " << num_items << " items)";
  return 0;
}
