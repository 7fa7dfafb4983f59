// cdae_fism_host.h — the arithmetic of a FISM handle (cdae_fism_kernels.hpp) that runs on the host or on both sides:
// the scale table, the residency plan, and the step count and launch windows of either loop (FISM's instances, §8n's pairs).
// Plain C++ with no HIP header, so src/fism_check.cpp compiles it with the host sanitizers.
#pragma once
#include <stdint.h>

#include <cmath>
#include <cstddef>
#include <vector>

namespace cdae {

constexpr uint32_t FISM_WAVES = 8u;                 // W: wavefronts of the one workgroup; row position q of a user belongs to wavefront q % W
constexpr uint32_t FISM_RESIDENT_FLOATS = 64u;      // floats per lane a wavefront keeps for resident row values (as many again for accumulators)
constexpr uint32_t FISM_RESIDENT_SLOTS = 32u;       // ... in at most this many rows (NI = 1: half the floats; the unrolled slot loops stay short)
constexpr uint64_t FISM_WINDOW_INSTANCES = 2048u;   // instances one launch holds at most (a user is never cut: a longer one has a launch of its own)

// scale[n] = n^-alpha for 1 <= n <= max_n, scale[0] = 0: fp64 pow, rounded once to fp32.  A user with n items takes s_pos = scale[n - 1]
// (0 for a lone positive: the empty neighbourhood) and s_neg = scale[n]; serving takes scale[size of the rated set].
inline std::vector<float> fism_scale_table(uint64_t max_n, double alpha) {
  std::vector<float> s((size_t)max_n + 1);
  s[0] = 0.f;
  for (uint64_t n = 1; n <= max_n; ++n) s[(size_t)n] = (float)std::pow((double)n, -alpha);
  return s;
}

// resident rows per wavefront at NI floats per lane and row
constexpr uint32_t fism_resident_slots(uint32_t ni) {
  return ni >= 1u && ni <= FISM_RESIDENT_FLOATS ? (FISM_RESIDENT_FLOATS / ni < FISM_RESIDENT_SLOTS ? FISM_RESIDENT_FLOATS / ni : FISM_RESIDENT_SLOTS) : 0u;
}
// rows of a user that stay on chip for a whole visit (0: every row streams through memory)
inline uint32_t fism_resident_rows(uint32_t ni, bool allow) { return allow ? FISM_WAVES * fism_resident_slots(ni) : 0u; }

// steps (sweeps of the user's rows) per stored interaction: FISM's instances, the rated one and num_neg negatives; the pairwise handle's
// (cdae_hip_create_fism_pair) num_neg pairs.  64 bits: 1 + 0xFFFFFFFF does not wrap.
inline uint64_t fism_steps_per_interaction(bool pair, uint32_t num_neg) { return pair ? (uint64_t)num_neg : 1ull + num_neg; }

// steps of rows [r_begin, r_end) of a CSR
inline uint64_t fism_step_count(const int64_t* row_ptr, uint64_t r_begin, uint64_t r_end, uint64_t steps) {
  return (uint64_t)(row_ptr[r_end] - row_ptr[r_begin]) * steps;
}

// The launch windows of users [u_begin, u_end): cuts[0] = u_begin < cuts[1] < ... < cuts.back() = u_end (u_begin alone for an empty
// range).  A window takes users while its steps stay within `cap`, and always at least one (a user is never cut).
inline std::vector<uint64_t> fism_windows(const int64_t* row_ptr, uint64_t u_begin, uint64_t u_end, uint64_t steps, uint64_t cap) {
  std::vector<uint64_t> cuts{u_begin};
  uint64_t u = u_begin;
  while (u < u_end) {
    uint64_t e = u + 1;
    while (e < u_end && fism_step_count(row_ptr, u, e + 1, steps) <= cap) ++e;
    cuts.push_back(e);
    u = e;
  }
  return cuts;
}

}  // namespace cdae
