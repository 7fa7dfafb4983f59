// Compile-and-link check of libcf::CDAE::similar_items and libcf::IMF::similar_items, and a small end-to-end driver of them:
//   similar_check                                  -> the methods compile and link (no device is touched)
//   similar_check --run=true --input_file=<file>   -> trains CDAE on a GPU and checks the item-page recipes of INTEGRATION.md
#include <algorithm>
#include <set>

#include <glog/logging.h>
#include <gflags/gflags.h>

#include <base/data.hpp>
#include <model/recsys/cdae.hpp>
#include <model/recsys/imf.hpp>
#include <solver/solver.hpp>

DEFINE_string(input_file, "", "user item text file (header line skipped)");
DEFINE_bool(run, false, "train CDAE on the GPU and check similar_items");
DEFINE_int32(num_dim, 16, "latent dimensions");
DEFINE_int32(iters, 2, "epochs");

int main(int argc, char* argv[]) {
  using namespace libcf;
  gflags::ParseCommandLineFlags(&argc, &argv, true);
  typedef std::vector<std::vector<size_t>> Lists;
  // the signature the documents give: (items, topk, metric, table, exclude_self, excluded_sets, allow)
  Lists (CDAE::*method)(const std::vector<size_t>&, size_t, uint32_t, uint32_t, bool, const Lists&, const std::vector<size_t>&) const =
      &CDAE::similar_items;
  Lists (IMF::*mf_method)(const std::vector<size_t>&, size_t, uint32_t, uint32_t, bool, const Lists&, const std::vector<size_t>&) const =
      &IMF::similar_items;
  CHECK(method != nullptr && mf_method != nullptr);
  if (!FLAGS_run) { LOG(INFO) << "similar check OK (compiled)"; return 0; }

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
  const size_t num_items = train.feature_group_total_dimension(1), topk = 10;
  std::vector<size_t> items;
  for (size_t i = 0; i < num_items; i += 3) items.push_back(i);
  items.push_back(items[0]);                                       // any item any number of times
  const size_t n = items.size();

  // an item page: ten neighbours by cosine, never the item itself
  const Lists page = trained->similar_items(items, topk);
  for (size_t r = 0; r < n; ++r) {
    CHECK_EQ(page[r].size(), topk);
    CHECK(std::find(page[r].begin(), page[r].end(), items[r]) == page[r].end()) << "item " << items[r] << " lists itself";
    CHECK_EQ(std::set<size_t>(page[r].begin(), page[r].end()).size(), topk);
  }
  CHECK(page[n - 1] == page[0]);
  // with the item itself as a candidate it heads its own list (a trained row is not zero), and the rest moves down by one
  const Lists own = trained->similar_items(items, topk, CDAE_SIM_COSINE, CDAE_ITEMS_OUTPUT, false);
  for (size_t r = 0; r < n; ++r) {
    CHECK_EQ(own[r][0], items[r]);
    CHECK(std::equal(own[r].begin() + 1, own[r].end(), page[r].begin())) << "item " << items[r];
  }
  // the head of every list excluded: the list moves up by one
  Lists shown(n);
  for (size_t r = 0; r < n; ++r) shown[r].push_back(page[r][0]);
  const Lists hidden = trained->similar_items(items, topk, CDAE_SIM_COSINE, CDAE_ITEMS_OUTPUT, true, shown);
  for (size_t r = 0; r < n; ++r) CHECK(std::equal(page[r].begin() + 1, page[r].end(), hidden[r].begin())) << "item " << items[r];
  // "more like this within a category": every fourth item, handed over in descending order (the method sorts it); the allowed items
  // of the whole list keep their order
  std::vector<size_t> allow;
  for (size_t i = num_items; i-- > 0;) if (i % 4 == 1) allow.push_back(i);
  const Lists whole = trained->similar_items(items, num_items);
  const Lists cat = trained->similar_items(items, topk, CDAE_SIM_COSINE, CDAE_ITEMS_OUTPUT, true, Lists(), allow);
  for (size_t r = 0; r < n; ++r) {
    CHECK_EQ(whole[r].size(), num_items - 1);
    std::vector<size_t> kept;
    for (size_t iid : whole[r]) if (iid % 4 == 1 && kept.size() < topk) kept.push_back(iid);
    CHECK(kept == cat[r]) << "item " << items[r];
  }
  // the dot product and the input table answer too (a tied model has one table)
  const Lists dot = trained->similar_items(items, topk, CDAE_SIM_DOT, CDAE_ITEMS_INPUT);
  CHECK(dot == trained->similar_items(items, topk, CDAE_SIM_DOT, CDAE_ITEMS_OUTPUT));
  for (size_t r = 0; r < n; ++r) CHECK_EQ(dot[r].size(), topk);
  LOG(INFO) << "similar_items OK (" << n << " queries over " << num_items << " items)";
  return 0;
}
