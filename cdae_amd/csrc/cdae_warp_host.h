// cdae_warp_host.h — the arithmetic of a WARP handle (cdae_warp_kernels.hpp) that runs on the host or on both sides:
// the rank-weight table, the index of a candidate in the negative stream, the pair count of a range of rows.  Plain C++ with no HIP
// header, so src/warp_check.cpp compiles it with the host sanitizers.
#pragma once
#include <stdint.h>

#include <cstddef>
#include <vector>

#ifndef CDAE_WARP_FN
#if defined(__HIPCC__)
#define CDAE_WARP_FN static __host__ __device__ __forceinline__
#else
#define CDAE_WARP_FN static inline
#endif
#endif

namespace cdae {

constexpr uint32_t WARP_MAX_TRY = 500u;        // CDAE_WARP_MAX_TRY (include/cdae_hip.h)

// draw index of candidate t of pair (p, k) of a user: what cdae_sample_negative takes (include/cdae_rng.h)
CDAE_WARP_FN uint64_t warp_draw_index(uint64_t p, uint32_t num_neg, uint32_t k, uint32_t t) {
  return (p * num_neg + k) * WARP_MAX_TRY + t;
}

// l[idx] = H_{idx + 1} for idx < num_items (warp.hpp:57-60): the fp64 recurrence, rounded once to fp32
inline std::vector<float> warp_rank_weights(uint64_t num_items) {
  std::vector<float> l((size_t)num_items);
  double h = 0.;
  for (uint64_t idx = 0; idx < num_items; ++idx) {
    h += 1. / (double)(idx + 1);
    l[(size_t)idx] = (float)h;
  }
  return l;
}

// pairs of rows [r_begin, r_end) of a CSR: (positives of the range) * num_neg
inline uint64_t warp_pair_count(const int64_t* row_ptr, uint64_t r_begin, uint64_t r_end, uint32_t num_neg) {
  return (uint64_t)(row_ptr[r_end] - row_ptr[r_begin]) * num_neg;
}

}  // namespace cdae
