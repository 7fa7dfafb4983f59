// Compile-and-link check of libcf::FISM and libcf::FISMP, the host arithmetic of a FISM handle of either kind under the host sanitizers,
// and a small end-to-end driver:
//   fism_check                                  -> the classes compile and link; the scale table, the residency plan, and the step count
//                                                  and launch windows of cdae_amd/csrc/cdae_fism_host.h at both step counts (FISM's
//                                                  1 + num_neg instances, the pairwise handle's num_neg pairs) are checked against their
//                                                  definitions (no device); the refusals a pairwise handle decides without a device
//   fism_check --run=true --input_file=<file>   -> fits FISM on a GPU through Solver<FISM> with TOPN and checks what it serves
// `make sanitize` builds the same program without the library (-DFISM_CHECK_HOST_ONLY) with -fsanitize=address,undefined and runs it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../cdae_amd/csrc/cdae_fism_host.h"

namespace {
int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "fism_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// the one count and the one window function, at the step count of either handle kind
uint64_t instance_count(const int64_t* ptr, uint64_t a, uint64_t b, uint32_t nn) { return cdae::fism_step_count(ptr, a, b, cdae::fism_steps_per_interaction(false, nn)); }
uint64_t pair_count(const int64_t* ptr, uint64_t a, uint64_t b, uint32_t nn) { return cdae::fism_step_count(ptr, a, b, cdae::fism_steps_per_interaction(true, nn)); }
std::vector<uint64_t> windows(bool pair, const int64_t* ptr, uint64_t b, uint64_t e, uint32_t nn, uint64_t cap) {
  return cdae::fism_windows(ptr, b, e, cdae::fism_steps_per_interaction(pair, nn), cap);
}

const int64_t ptr[] = {0, 3, 3, 10, 11, 411, 412};

// the launch windows of every range of ptr: consecutive, covering, within the cap unless a single user exceeds it, greedy
void check_windows(bool pair, uint32_t nn, const std::vector<uint64_t>& caps) {
  for (uint64_t cap : caps)
    for (uint64_t b = 0; b <= 6; ++b)
      for (uint64_t e = b; e <= 6; ++e) {
        const std::vector<uint64_t> cuts = windows(pair, ptr, b, e, nn, cap);
        EXPECT(cuts.front() == b && cuts.back() == e);
        EXPECT(cuts.size() == 1 || b < e);
        for (size_t t = 0; t + 1 < cuts.size(); ++t) {
          EXPECT(cuts[t] < cuts[t + 1]);
          const uint64_t steps = pair ? pair_count(ptr, cuts[t], cuts[t + 1], nn) : instance_count(ptr, cuts[t], cuts[t + 1], nn);
          EXPECT(steps <= cap || cuts[t + 1] == cuts[t] + 1);
          // greedy: the next user would not have fitted
          if (cuts[t + 1] < e) EXPECT((pair ? pair_count(ptr, cuts[t], cuts[t + 1] + 1, nn) : instance_count(ptr, cuts[t], cuts[t + 1] + 1, nn)) > cap);
        }
      }
}

void check_host_arithmetic() {
  // the scale table: n^-alpha by fp64 pow, rounded once; scale[0] = 0
  const double alphas[] = {0., 0.5, 1., 1.7, 2.};
  const uint64_t sizes[] = {0, 1, 2, 45, 1468, uint64_t(1) << 17};
  for (double alpha : alphas)
    for (uint64_t n_max : sizes) {
      const std::vector<float> s = cdae::fism_scale_table(n_max, alpha);
      EXPECT(s.size() == n_max + 1);
      EXPECT(s[0] == 0.f);
      for (uint64_t n = 1; n <= n_max; ++n)
        if (s[n] != (float)std::pow((double)n, -alpha)) { EXPECT(s[n] == (float)std::pow((double)n, -alpha)); break; }
      if (n_max >= 1) EXPECT(s[1] == 1.f);
      if (n_max >= 2 && alpha == 0.) EXPECT(s[2] == 1.f);
      if (n_max >= 45 && alpha == 1.) { EXPECT(s[2] == 0.5f); EXPECT(s[4] == 0.25f); EXPECT(s[8] == 0.125f); EXPECT(s[45] == (float)(1. / 45.)); }
      if (n_max >= 45 && alpha == 0.5) { EXPECT(s[4] == 0.5f); EXPECT(s[16] == 0.25f); }
      for (uint64_t n = 2; n <= n_max && alpha > 0.; n += 97) EXPECT(s[n] < s[n - 1]);
    }
  // the residency plan: W wavefronts x min(FISM_RESIDENT_FLOATS / NI, FISM_RESIDENT_SLOTS) rows each; nothing when it is switched off
  EXPECT(cdae::FISM_WAVES == 8u && cdae::FISM_RESIDENT_FLOATS == 64u && cdae::FISM_RESIDENT_SLOTS == 32u);
  EXPECT(cdae::fism_resident_rows(1, true) == 256u);
  EXPECT(cdae::fism_resident_rows(2, true) == 256u);
  EXPECT(cdae::fism_resident_rows(4, true) == 128u);
  EXPECT(cdae::fism_resident_rows(8, true) == 64u);
  for (uint32_t ni : {1u, 2u, 4u, 8u}) {
    EXPECT(cdae::fism_resident_rows(ni, false) == 0u);
    EXPECT(cdae::fism_resident_rows(ni, true) % cdae::FISM_WAVES == 0u);       // the kernel's first streamed position of wavefront w is C + w
  }
  EXPECT(cdae::fism_resident_rows(0, true) == 0u);
  // the instance count: (1 + num_neg) per stored interaction
  EXPECT(instance_count(ptr, 0, 6, 5) == 412u * 6u);
  EXPECT(instance_count(ptr, 1, 2, 5) == 0u);
  EXPECT(instance_count(ptr, 2, 4, 12) == 8u * 13u);
  EXPECT(instance_count(ptr, 3, 3, 12) == 0u);
  // the launch windows in instances
  check_windows(false, 5, {1, 6, 18, 60, 66, 2048, 2400, 2472, uint64_t(1) << 40});
  const std::vector<uint64_t> w = windows(false, ptr, 0, 6, 5, 66);            // 18 + 0 + 42 + 6 | 2400 (a window of its own) | 6
  EXPECT(w.size() == 4 && w[0] == 0 && w[1] == 4 && w[2] == 5 && w[3] == 6);
  const std::vector<uint64_t> w2 = windows(false, ptr, 0, 6, 5, 65);           // 18 + 0 + 42 | 6 | 2400 | 6
  EXPECT(w2.size() == 5 && w2[1] == 3 && w2[2] == 4 && w2[3] == 5 && w2[4] == 6);
  EXPECT(cdae::FISM_WINDOW_INSTANCES == 2048u);
}

void check_pair_arithmetic() {
  // the pair count: num_neg per stored interaction
  EXPECT(pair_count(ptr, 0, 6, 5) == 412u * 5u);
  EXPECT(pair_count(ptr, 1, 2, 5) == 0u);
  EXPECT(pair_count(ptr, 2, 4, 12) == 8u * 12u);
  EXPECT(pair_count(ptr, 3, 3, 12) == 0u);
  EXPECT(pair_count(ptr, 0, 6, 1) == 412u);
  const int64_t big[] = {0, int64_t(1) << 33};                                 // no 32-bit product anywhere
  EXPECT(pair_count(big, 0, 1, 0xFFFFFFFFu) == (uint64_t(1) << 33) * 0xFFFFFFFFull);
  EXPECT(cdae::fism_steps_per_interaction(false, 0xFFFFFFFFu) == uint64_t(1) << 32);    // ... nor a 32-bit 1 + num_neg
  for (uint32_t nn : {1u, 5u, 12u, 65u})                                       // always num_nnz fewer than FISM's instances
    EXPECT(instance_count(ptr, 0, 6, nn) - pair_count(ptr, 0, 6, nn) == 412u);
  // the launch windows in pairs
  for (uint32_t nn : {1u, 5u, 12u}) check_windows(true, nn, {1, 5, 15, 50, 55, 2000, 2048, 2060, uint64_t(1) << 40});
  const std::vector<uint64_t> w = windows(true, ptr, 0, 6, 5, 55);             // 15 + 0 + 35 + 5 | 2000 (a window of its own) | 5
  EXPECT(w.size() == 4 && w[0] == 0 && w[1] == 4 && w[2] == 5 && w[3] == 6);
  const std::vector<uint64_t> w2 = windows(true, ptr, 0, 6, 5, 54);            // 15 + 0 + 35 | 5 | 2000 | 5
  EXPECT(w2.size() == 5 && w2[1] == 3 && w2[2] == 4 && w2[3] == 5 && w2[4] == 6);
  const std::vector<uint64_t> w3 = windows(true, ptr, 0, 6, 5, 2005);          // 55 | 2000 + 5: pairs fit where FISM's 2406 instances would not
  EXPECT(w3.size() == 3 && w3[1] == 4 && w3[2] == 6);
  EXPECT(windows(false, ptr, 4, 6, 5, 2005).size() == 3);
  // what FISM's step count gives is untouched
  EXPECT(instance_count(ptr, 0, 6, 5) == 412u * 6u);
  EXPECT(cdae::FISM_WINDOW_INSTANCES == 2048u && cdae::FISM_WAVES == 8u);
}
}  // namespace

#ifdef FISM_CHECK_HOST_ONLY
int main() {
  check_host_arithmetic();
  if (failures) return 1;
  std::printf("fism check OK (host arithmetic)\n");
  check_pair_arithmetic();
  if (failures) return 1;
  std::printf("fism pair check OK (host arithmetic)\n");
  return 0;
}
#else
#include <set>

#include <glog/logging.h>
#include <gflags/gflags.h>

#include <base/data.hpp>
#include <model/recsys/fism.hpp>
#include <model/recsys/fism_pair.hpp>
#include <solver/solver.hpp>

DEFINE_string(input_file, "", "user item text file (header line skipped)");
DEFINE_bool(run, false, "fit FISM on the GPU and check it");
DEFINE_int32(num_dim, 16, "latent dimensions");
DEFINE_int32(iters, 3, "epochs");

// libcf::FISMP: the reference's defaults (fism_pair.hpp), the structure the library takes, which is FISM's, and the refusals the library
// decides without a device
void check_pair_class() {
  using namespace libcf;
  FISMPConfig cfg;
  CHECK_EQ(cfg.lambda, 0.01); CHECK_EQ(cfg.lt, SQUARE); CHECK_EQ(cfg.num_dim, size_t(10)); CHECK_EQ(cfg.num_neg, size_t(5));
  CHECK_EQ(cfg.alpha, 1.); CHECK_EQ(cfg.learn_rate, 0.1);
  CHECK(cfg.using_bias_term && cfg.using_adagrad);
  CHECK_EQ(sizeof(cdae_fism_config), size_t(56));
  FISMP model(cfg);                                          // (no device is touched before reset)
  Solver<FISMP>* solver = nullptr;                           // the solver template accepts the class
  (void)solver;
  cdae_fism_config c = cdae_fism_config();
  cdae_hip_t* h = nullptr;
  c.struct_size = sizeof(c); c.num_dim = 10; c.num_neg = 5; c.using_adagrad = 1; c.using_bias_term = 1; c.lambda = 0.01; c.learn_rate = 0.1; c.alpha = 1.;
  c.loss_type = 5;
  CHECK_NE(cdae_hip_create_fism_pair(&c, 0, &h), 0);
  CHECK(std::string(cdae_hip_last_error()).find("CROSS_ENTROPY") != std::string::npos);
  CHECK_NE(cdae_hip_create_fism_pair(nullptr, 0, &h), 0);
}

int main(int argc, char* argv[]) {
  using namespace libcf;
  gflags::ParseCommandLineFlags(&argc, &argv, true);
  check_host_arithmetic();
  check_pair_arithmetic();
  CHECK_EQ(failures, 0);
  // the reference's defaults (fism.hpp:8-20) and the structure the library takes
  FISMConfig cfg;
  CHECK_EQ(cfg.lambda, 0.01); CHECK_EQ(cfg.lt, SQUARE); CHECK_EQ(cfg.num_dim, size_t(10)); CHECK_EQ(cfg.num_neg, size_t(5));
  CHECK_EQ(cfg.alpha, 1.); CHECK_EQ(cfg.learn_rate, 0.1);
  CHECK(cfg.using_bias_term && cfg.using_factor_term && !cfg.using_global_mean && cfg.using_adagrad);
  CHECK_EQ(sizeof(cdae_fism_config), size_t(56));
  check_pair_class();
  if (!FLAGS_run) { LOG(INFO) << "fism check OK (compiled)"; LOG(INFO) << "fism pair check OK (compiled)"; return 0; }

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
  cfg.learn_rate = 0.01;
  FISM model(cfg);
  Solver<FISM> solver(model, FLAGS_iters);
  solver.train(train, test, {TOPN});
  std::shared_ptr<FISM> trained = solver.get_model();
  const size_t num_users = train.feature_group_total_dimension(0), num_items = train.feature_group_total_dimension(1), topk = 10;
  const DMatrix P = trained->get_input_vecs(), Q = trained->get_item_vecs();
  CHECK_EQ(static_cast<size_t>(P.rows()), num_items); CHECK_EQ(static_cast<size_t>(Q.rows()), num_items);
  const auto rated = train.get_feature_pair_label_hashtable(0, 1);
  for (size_t u = 0; u < num_users; u += 7) {
    const std::vector<size_t> list = trained->recommend_train_row(u, topk);
    CHECK_EQ(std::set<size_t>(list.begin(), list.end()).size(), topk);
    if (!rated.count(u)) continue;
    CHECK(trained->recommend(u, topk, rated.at(u)) == list);                       // the train row through the generic entry
    std::unordered_map<size_t, double> fewer(rated.at(u));
    fewer.erase(fewer.begin());                                                    // ... and a rated set that is no train row
    const std::vector<size_t> other = trained->recommend(u, topk, fewer);
    for (size_t item : other) CHECK(!fewer.count(item));
    CHECK(std::isfinite(trained->predict_user_item_rating(u, list[0])));
  }
  LOG(INFO) << "fism OK (" << num_users << " users, " << num_items << " items)";
  return 0;
}
#endif
