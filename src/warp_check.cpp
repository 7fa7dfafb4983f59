// Compile-and-link check of libcf::WARP, the host arithmetic of a WARP handle under the host sanitizers, and a small end-to-end driver:
//   warp_check                                  -> the class compiles and links; the rank table, the draw index and the pair count of
//                                                  cdae_amd/csrc/cdae_warp_host.h are checked against their definitions (no device)
//   warp_check --run=true --input_file=<file>   -> fits WARP on a GPU through Solver<WARP> with TOPN and checks what it serves
// `make sanitize` builds the same program without the library (-DWARP_CHECK_HOST_ONLY) with -fsanitize=address,undefined and runs it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <cdae_rng.h>
#include "../cdae_amd/csrc/cdae_warp_host.h"

namespace {
int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "warp_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

void check_host_arithmetic() {
  // the rank weights: H_{idx + 1}, the fp64 recurrence rounded once
  for (uint64_t n : {uint64_t(0), uint64_t(1), uint64_t(2), uint64_t(40), uint64_t(10600), uint64_t(1) << 20}) {
    const std::vector<float> l = cdae::warp_rank_weights(n);
    EXPECT(l.size() == n);
    double h = 0.;
    for (uint64_t idx = 0; idx < n; ++idx) {
      h += 1. / (double)(idx + 1);
      if (l[idx] != (float)h) { EXPECT(l[idx] == (float)h); break; }
    }
    if (n) { EXPECT(l[0] == 1.f); EXPECT(std::fabs(l[n - 1] - (std::log((double)n) + 0.5772156649 + 0.5 / (double)n)) < 1e-3 + 0.1 / (double)n); }
  }
  // the draw index: pairs in (p, k) order, CDAE_WARP_MAX_TRY candidates each, no two alike
  EXPECT(cdae::WARP_MAX_TRY == 500u);
  EXPECT(cdae::warp_draw_index(0, 5, 0, 0) == 0u);
  EXPECT(cdae::warp_draw_index(0, 5, 0, 499) == 499u);
  EXPECT(cdae::warp_draw_index(0, 5, 1, 0) == 500u);
  EXPECT(cdae::warp_draw_index(3, 5, 4, 7) == (3u * 5u + 4u) * 500u + 7u);
  EXPECT(cdae::warp_draw_index(7, 12, 0, 0) == cdae::warp_draw_index(6, 12, 11, 499) + 1u);
  const uint64_t big = cdae::warp_draw_index((uint64_t(1) << 30) - 1, 4096u, 4095u, 499);            // the longest legal row, num_neg 4 096
  EXPECT(big / 500u == ((uint64_t(1) << 30) - 1) * 4096u + 4095u);
  EXPECT(big <= 0xFFFFFFFFFFFFFFFFull / CDAE_NEG_MAX_TRY);          // cdae_sample_negative multiplies it by CDAE_NEG_MAX_TRY
  // ... and what it indexes: a candidate is never one of the row's items, for a row with every item but one it is that item
  const uint32_t row[] = {0, 1, 2, 3, 5, 6, 7};
  const uint64_t key = cdae_rng_key(7, 3, 11, CDAE_STREAM_NEGATIVE);
  for (uint32_t t = 0; t < cdae::WARP_MAX_TRY; ++t) EXPECT(cdae_sample_negative(key, cdae::warp_draw_index(6, 3, 2, t), row, 7, 8) == 4u);
  for (uint32_t t = 0; t < cdae::WARP_MAX_TRY; ++t) {
    const uint32_t c = cdae_sample_negative(key, cdae::warp_draw_index(1, 3, 0, t), row, 4, 40);
    EXPECT(c < 40u && c > 3u);
  }
  // the pair count of a range of rows
  const int64_t ptr[] = {0, 3, 3, 10, 11};
  EXPECT(cdae::warp_pair_count(ptr, 0, 4, 5) == 55u);
  EXPECT(cdae::warp_pair_count(ptr, 1, 2, 5) == 0u);
  EXPECT(cdae::warp_pair_count(ptr, 2, 4, 12) == 96u);
  EXPECT(cdae::warp_pair_count(ptr, 3, 3, 12) == 0u);
}
}  // namespace

#ifdef WARP_CHECK_HOST_ONLY
int main() {
  check_host_arithmetic();
  if (failures) return 1;
  std::printf("warp check OK (host arithmetic)\n");
  return 0;
}
#else
#include <set>

#include <glog/logging.h>
#include <gflags/gflags.h>

#include <base/data.hpp>
#include <model/recsys/warp.hpp>
#include <solver/solver.hpp>

DEFINE_string(input_file, "", "user item text file (header line skipped)");
DEFINE_bool(run, false, "fit WARP on the GPU and check it");
DEFINE_int32(num_dim, 16, "latent dimensions");
DEFINE_int32(iters, 3, "epochs");

int main(int argc, char* argv[]) {
  using namespace libcf;
  gflags::ParseCommandLineFlags(&argc, &argv, true);
  check_host_arithmetic();
  CHECK_EQ(failures, 0);
  // the reference's defaults (warp.hpp:12-23) and the structure the library takes
  WARPConfig cfg;
  CHECK_EQ(cfg.learn_rate, 0.1); CHECK_EQ(cfg.beta, 0.); CHECK_EQ(cfg.lambda, 0.1); CHECK_EQ(cfg.lt, HINGE);
  CHECK_EQ(cfg.num_dim, size_t(10)); CHECK_EQ(cfg.num_neg, size_t(5)); CHECK(cfg.using_bias_term && cfg.using_adagrad);
  CHECK_EQ(sizeof(cdae_warp_config), size_t(40));
  CHECK_EQ(CDAE_WARP_MAX_TRY, cdae::WARP_MAX_TRY);
  void (WARP::*search)(std::vector<uint32_t>&, std::vector<uint32_t>&) const = &WARP::search;
  CHECK(search != nullptr);
  if (!FLAGS_run) { LOG(INFO) << "warp check OK (compiled)"; return 0; }

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
  WARP model(cfg);
  Solver<WARP> solver(model, FLAGS_iters);
  solver.train(train, test, {TOPN});
  std::shared_ptr<WARP> trained = solver.get_model();
  const size_t num_users = train.feature_group_total_dimension(0), num_items = train.feature_group_total_dimension(1), topk = 10;
  const DMatrix X = trained->get_user_vecs(), Y = trained->get_item_vecs();
  CHECK_EQ(static_cast<size_t>(X.rows()), num_users); CHECK_EQ(static_cast<size_t>(Y.rows()), num_items);
  double norm = 0.;
  for (size_t i = 0; i < num_users * cfg.num_dim; ++i) norm += X.data()[i] * X.data()[i];
  CHECK_GT(norm, 1e-2 * num_users * cfg.num_dim * 1e-4) << "the user factors are still the initial ones";
  for (size_t u = 0; u < num_users; u += 7) {
    const std::vector<size_t> list = trained->recommend_train_row(u, topk);
    CHECK_EQ(std::set<size_t>(list.begin(), list.end()).size(), topk);
  }
  // the search: a chosen negative is never one of the user's items, and its draw count says whether there is one
  std::vector<uint32_t> items, draws;
  trained->search(items, draws);
  const auto rated = train.get_feature_pair_label_hashtable(0, 1);
  size_t q = 0, found = 0;
  for (size_t u = 0; u < num_users; ++u) {
    const size_t n_u = rated.count(u) ? rated.at(u).size() : 0;
    for (size_t e = 0; e < n_u * cfg.num_neg; ++e, ++q) {
      CHECK(draws[q] >= 1 && draws[q] <= CDAE_WARP_MAX_TRY);
      CHECK_EQ(draws[q] == CDAE_WARP_MAX_TRY, items[q] == 0xFFFFFFFFu);
      if (draws[q] < CDAE_WARP_MAX_TRY) { CHECK_LT(items[q], num_items); CHECK(!rated.at(u).count(items[q])); ++found; }
    }
  }
  CHECK_EQ(q, items.size());
  CHECK_GT(found, size_t(0));
  LOG(INFO) << "warp OK (" << num_users << " users, " << num_items << " items, " << found << " of " << q << " searches found a violator)";
  return 0;
}
#endif
