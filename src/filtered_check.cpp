// Compile-and-link check of libcf::CDAE::recommend_rows_filtered, and a small end-to-end driver of it:
//   filtered_check                                  -> the method compiles and links (no device is touched)
//   filtered_check --run=true --input_file=<file>   -> trains CDAE on a GPU and checks the filtered lists against recommend_rows
#include <algorithm>
#include <set>

#include <glog/logging.h>
#include <gflags/gflags.h>

#include <base/data.hpp>
#include <model/recsys/cdae.hpp>
#include <solver/solver.hpp>

DEFINE_string(input_file, "", "user item text file (header line skipped)");
DEFINE_bool(run, false, "train CDAE on the GPU and check recommend_rows_filtered");
DEFINE_int32(num_dim, 16, "latent dimensions");
DEFINE_int32(iters, 2, "epochs");

int main(int argc, char* argv[]) {
  using namespace libcf;
  gflags::ParseCommandLineFlags(&argc, &argv, true);
  typedef std::vector<std::vector<size_t>> Lists;
  // the signature the documents give: (uids, rated_sets, excluded_sets, allow, topk, exclude_rated)
  Lists (CDAE::*method)(const std::vector<size_t>&, const Lists&, const Lists&, const std::vector<size_t>&, size_t, bool) const =
      &CDAE::recommend_rows_filtered;
  CHECK(method != nullptr);
  if (!FLAGS_run) { LOG(INFO) << "filtered check OK (compiled)"; return 0; }

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
  CDAEConfig cfg;
  cfg.num_dim = FLAGS_num_dim;
  cfg.beta = 1.;
  cfg.lt = CROSS_ENTROPY;
  CDAE model(cfg);
  Solver<CDAE> solver(model, FLAGS_iters);
  solver.train(train, test, {TOPN});
  std::shared_ptr<CDAE> trained = solver.get_model();
  const size_t num_items = train.feature_group_total_dimension(1);
  auto train_sets = train.get_feature_pair_label_hashtable(0, 1);
  std::vector<size_t> uids;
  Lists sets;
  for (auto& ur : train_sets) {
    uids.push_back(ur.first);
    sets.emplace_back();
    for (auto& p : ur.second) sets.back().push_back(p.first);
  }
  const size_t n = sets.size(), topk = 10;
  const Lists plain = trained->recommend_rows(uids, sets, topk);
  // no filter: recommend_rows' lists
  CHECK(trained->recommend_rows_filtered(uids, sets, Lists(), std::vector<size_t>(), topk) == plain);
  // the rated sets handed over as exclusions instead: the same lists again
  CHECK(trained->recommend_rows_filtered(uids, sets, sets, std::vector<size_t>(), topk, false) == plain);
  // "hide what was shown": the head of every list is excluded, the list moves up by one
  Lists shown(n);
  for (size_t r = 0; r < n; ++r) shown[r].push_back(plain[r][0]);
  const Lists hidden = trained->recommend_rows_filtered(uids, sets, shown, std::vector<size_t>(), topk);
  for (size_t r = 0; r < n; ++r) {
    CHECK_EQ(hidden[r].size(), topk);
    CHECK(std::equal(plain[r].begin() + 1, plain[r].end(), hidden[r].begin())) << "row " << r << " does not move up by one";
  }
  // "category page": every third item, handed over in descending order (the method sorts it)
  std::vector<size_t> allow;
  for (size_t i = num_items; i-- > 0;) if (i % 3 == 0) allow.push_back(i);
  const Lists page = trained->recommend_rows_filtered(uids, sets, Lists(), allow, topk);
  for (size_t r = 0; r < n; ++r) {
    const std::set<size_t> rated(sets[r].begin(), sets[r].end());
    for (size_t iid : page[r]) CHECK(iid % 3 == 0 && !rated.count(iid)) << "row " << r << " lists item " << iid;
    std::vector<size_t> kept;                                      // the allowed items of the unfiltered list keep their order
    for (size_t iid : plain[r]) if (iid % 3 == 0) kept.push_back(iid);
    CHECK(std::equal(kept.begin(), kept.end(), page[r].begin())) << "row " << r;
  }
  // "buy it again": rated items are candidates; a list may name them, and never an excluded one
  const Lists again = trained->recommend_rows_filtered(uids, sets, shown, std::vector<size_t>(), topk, false);
  size_t rated_listed = 0;
  for (size_t r = 0; r < n; ++r) {
    const std::set<size_t> rated(sets[r].begin(), sets[r].end());
    for (size_t iid : again[r]) { CHECK_NE(iid, shown[r][0]); rated_listed += rated.count(iid); }
  }
  CHECK_GT(rated_listed, size_t(0));
  LOG(INFO) << "recommend_rows_filtered OK (" << n << " rows, " << rated_listed << " rated items listed again)";
  return 0;
}
