// Compile-and-link check of libcf::FISMP and the host arithmetic of a pairwise FISM handle under the host sanitizers:
//   fism_pair_check   -> the class compiles and links; the pair count and the launch windows in pairs of
//                        cdae_amd/csrc/cdae_fism_host.h are checked against their definitions (no device)
// `make sanitize` builds the same program without the library (-DFISM_PAIR_CHECK_HOST_ONLY) with -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../cdae_amd/csrc/cdae_fism_host.h"

namespace {
int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "fism_pair_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

void check_host_arithmetic() {
  // the pair count: num_neg per stored interaction
  const int64_t ptr[] = {0, 3, 3, 10, 11, 411, 412};
  EXPECT(cdae::fism_pair_count(ptr, 0, 6, 5) == 412u * 5u);
  EXPECT(cdae::fism_pair_count(ptr, 1, 2, 5) == 0u);
  EXPECT(cdae::fism_pair_count(ptr, 2, 4, 12) == 8u * 12u);
  EXPECT(cdae::fism_pair_count(ptr, 3, 3, 12) == 0u);
  EXPECT(cdae::fism_pair_count(ptr, 0, 6, 1) == 412u);
  const int64_t big[] = {0, int64_t(1) << 33};                                 // no 32-bit product anywhere
  EXPECT(cdae::fism_pair_count(big, 0, 1, 0xFFFFFFFFu) == (uint64_t(1) << 33) * 0xFFFFFFFFull);
  for (uint32_t nn : {1u, 5u, 12u, 65u})                                       // always num_nnz fewer than FISM's instances
    EXPECT(cdae::fism_instance_count(ptr, 0, 6, nn) - cdae::fism_pair_count(ptr, 0, 6, nn) == 412u);
  // the launch windows in pairs: consecutive, covering, within the cap unless a single user exceeds it, greedy
  const uint64_t caps[] = {1, 5, 15, 50, 55, 2000, 2048, 2060, uint64_t(1) << 40};
  for (uint32_t nn : {1u, 5u, 12u})
    for (uint64_t cap : caps)
      for (uint64_t b = 0; b <= 6; ++b)
        for (uint64_t e = b; e <= 6; ++e) {
          const std::vector<uint64_t> cuts = cdae::fism_pair_windows(ptr, b, e, nn, cap);
          EXPECT(cuts.front() == b && cuts.back() == e);
          EXPECT(cuts.size() == 1 || b < e);
          for (size_t t = 0; t + 1 < cuts.size(); ++t) {
            EXPECT(cuts[t] < cuts[t + 1]);
            const uint64_t pairs = cdae::fism_pair_count(ptr, cuts[t], cuts[t + 1], nn);
            EXPECT(pairs <= cap || cuts[t + 1] == cuts[t] + 1);
            if (cuts[t + 1] < e) EXPECT(cdae::fism_pair_count(ptr, cuts[t], cuts[t + 1] + 1, nn) > cap);
          }
        }
  const std::vector<uint64_t> w = cdae::fism_pair_windows(ptr, 0, 6, 5, 55);   // 15 + 0 + 35 + 5 | 2000 (a window of its own) | 5
  EXPECT(w.size() == 4 && w[0] == 0 && w[1] == 4 && w[2] == 5 && w[3] == 6);
  const std::vector<uint64_t> w2 = cdae::fism_pair_windows(ptr, 0, 6, 5, 54);  // 15 + 0 + 35 | 5 | 2000 | 5
  EXPECT(w2.size() == 5 && w2[1] == 3 && w2[2] == 4 && w2[3] == 5 && w2[4] == 6);
  const std::vector<uint64_t> w3 = cdae::fism_pair_windows(ptr, 0, 6, 5, 2005); // 55 | 2000 + 5: pairs fit where FISM's 2406 instances would not
  EXPECT(w3.size() == 3 && w3[1] == 4 && w3[2] == 6);
  EXPECT(cdae::fism_windows(ptr, 4, 6, 5, 2005).size() == 3);
  // what FISM's functions give is untouched
  EXPECT(cdae::fism_instance_count(ptr, 0, 6, 5) == 412u * 6u);
  EXPECT(cdae::FISM_WINDOW_INSTANCES == 2048u && cdae::FISM_WAVES == 8u);
}
}  // namespace

#ifdef FISM_PAIR_CHECK_HOST_ONLY
int main() {
  check_host_arithmetic();
  if (failures) return 1;
  std::printf("fism pair check OK (host arithmetic)\n");
  return 0;
}
#else
#include <glog/logging.h>
#include <gflags/gflags.h>

#include <base/data.hpp>
#include <model/recsys/fism_pair.hpp>
#include <solver/solver.hpp>

int main(int argc, char* argv[]) {
  using namespace libcf;
  gflags::ParseCommandLineFlags(&argc, &argv, true);
  check_host_arithmetic();
  CHECK_EQ(failures, 0);
  // the reference's defaults (fism_pair.hpp) and the structure the library takes, which is FISM's
  FISMPConfig cfg;
  CHECK_EQ(cfg.lambda, 0.01); CHECK_EQ(cfg.lt, SQUARE); CHECK_EQ(cfg.num_dim, size_t(10)); CHECK_EQ(cfg.num_neg, size_t(5));
  CHECK_EQ(cfg.alpha, 1.); CHECK_EQ(cfg.learn_rate, 0.1);
  CHECK(cfg.using_bias_term && cfg.using_adagrad);
  CHECK_EQ(sizeof(cdae_fism_config), size_t(56));
  FISMP model(cfg);                                          // (no device is touched before reset)
  Solver<FISMP>* solver = nullptr;                           // the solver template accepts the class
  (void)solver;
  // refusals the library decides without a device
  cdae_fism_config c = cdae_fism_config();
  cdae_hip_t* h = nullptr;
  c.struct_size = sizeof(c); c.num_dim = 10; c.num_neg = 5; c.using_adagrad = 1; c.using_bias_term = 1; c.lambda = 0.01; c.learn_rate = 0.1; c.alpha = 1.;
  c.loss_type = 5;
  CHECK_NE(cdae_hip_create_fism_pair(&c, 0, &h), 0);
  CHECK(std::string(cdae_hip_last_error()).find("CROSS_ENTROPY") != std::string::npos);
  CHECK_NE(cdae_hip_create_fism_pair(nullptr, 0, &h), 0);
  LOG(INFO) << "fism pair check OK (compiled)";
  return 0;
}
#endif
