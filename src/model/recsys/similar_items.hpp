// The host side of cdae_hip_similar_items, shared by libcf::CDAE and libcf::IMF / BPR (which wrap a device handle the same way): the
// caller's sets become the device call's ascending arrays, the lists come back without their sentinel places.
#ifndef _LIBCF_SIMILAR_ITEMS_HPP_
#define _LIBCF_SIMILAR_ITEMS_HPP_

#include <algorithm>
#include <vector>

#include <glog/logging.h>

#include <cdae_hip.h>

namespace libcf {

// The topk items closest to each of `items` in ONE device call, on a handle the caller has locked: metric CDAE_SIM_COSINE /
// CDAE_SIM_DOT, table CDAE_ITEMS_OUTPUT / CDAE_ITEMS_INPUT; excluded_sets[r] must not be listed for items[r] (empty vector of sets:
// none anywhere); allow, when not empty, is ONE item list for the whole call — the only items that may be listed.  A list is shorter
// than topk when fewer candidates are left.
inline std::vector<std::vector<size_t>> similar_items_on(cdae_hip_t* h, size_t num_items, const std::vector<size_t>& items, size_t topk,
                                                         uint32_t metric, uint32_t table, bool exclude_self,
                                                         const std::vector<std::vector<size_t>>& excluded_sets,
                                                         const std::vector<size_t>& allow) {
  CHECK(excluded_sets.empty() || excluded_sets.size() == items.size());
  const size_t n = items.size();
  std::vector<uint32_t> q(n), ecol, al;
  std::vector<int64_t> eptr(n + 1, 0);
  for (size_t r = 0; r < n; ++r) {
    CHECK_LT(items[r], num_items);
    q[r] = static_cast<uint32_t>(items[r]);
    if (!excluded_sets.empty()) {
      const size_t eat = ecol.size();
      for (size_t i : excluded_sets[r]) { CHECK_LT(i, num_items); ecol.push_back(static_cast<uint32_t>(i)); }
      std::sort(ecol.begin() + eat, ecol.end());                   // the device CSR is ascending inside a row (duplicates: its error)
      eptr[r + 1] = static_cast<int64_t>(ecol.size());
    }
  }
  for (size_t i : allow) { CHECK_LT(i, num_items); al.push_back(static_cast<uint32_t>(i)); }
  std::sort(al.begin(), al.end());                                 // one ascending list (duplicates: the device call's error)
  std::vector<uint32_t> ids(n * topk);
  CHECK_EQ(cdae_hip_similar_items(h, n, q.data(), table, metric, exclude_self ? 1 : 0, excluded_sets.empty() ? nullptr : eptr.data(),
                                  ecol.data(), al.empty() ? nullptr : al.data(), al.size(), static_cast<uint32_t>(topk), ids.data(),
                                  nullptr), 0) << "libcdae_hip: " << cdae_hip_last_error() << " ";
  std::vector<std::vector<size_t>> out(n);
  for (size_t r = 0; r < n; ++r)
    for (size_t i = 0; i < topk && ids[r * topk + i] != 0xFFFFFFFFu; ++i) out[r].push_back(ids[r * topk + i]);
  return out;
}

}  // namespace libcf

#endif  // _LIBCF_SIMILAR_ITEMS_HPP_
