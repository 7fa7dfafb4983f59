// Fold-in of user nodes for rows outside the training set (cdae_hip_fold_in_rows).
//
// train_one_user_corruption (cdae.hpp:198-358) with every update of a shared parameter removed: W, V, b, b' are frozen, and all that
// moves is the row's own node — (wu, wu_ag), and (uu, uu_ag) under linear_function.  The rows are then independent of each other and
// inside a row every example of a step is independent given z: no sort, no segment list, no duplicate correction, no hand-over between
// workgroups and no atomics.  A node is one private recurrence that lives in registers, so ONE launch runs all epochs of a chunk.
//
// Per row r (ascending unique items R, n = |R|, stream id s = stream_id_base + r), for every epoch e and corruption c:
//   kept   = {R[pos] : cdae_keep(cdae_rng_draw(key(seed, e, s, CDAE_STREAM_CORRUPT), c n + pos), thr)}
//   S      = sum_{j in kept} W[j]                                      (unscaled)
//   h      = scale S ((.) uu) + b (+ wu),  z = act(h),  z' = act'(z)
//   N_i    = cdae_sample_negative(key(seed, e, s, CDAE_STREAM_NEGATIVE), c m + i, R, n, num_items),  i < m = n num_neg
//   hg     = sum_{j in R} loss'(D[j].z + b'[j], 1) D[j] + sum_i loss'(D[N_i].z + b'[N_i], 0) D[N_i]        (a duplicate counts per occurrence)
//   delta  = hg (.) z'
//   wu, wu_ag  <- ada_step with gradient lambda wu + delta              (user_factor; cdae.hpp:317-331)
//   uu, uu_ag  <- ada_step with gradient lambda uu + delta (.) S        (linear_function; cdae.hpp:295-299, :340, :351-357)
// These are the draws, the sums and the steps the training step makes for a user with id s and train row R.
//
// Work split.  Lane l owns elements [l NI, (l + 1) NI) of every K-vector.  A step's n kept-mask draws and its n (1 + num_neg) examples
// are cut into chunks of 64 (one lane per draw / per example: the mask is a ballot, a negative is drawn and rejected against the row by
// its own lane); the item ids of a chunk are then broadcast with readlane and the W / D rows stream as whole-row wave loads, UN in
// flight (8; 4 at NI = 8).  One kernel, two roles:
//   short rows  n (1 + num_neg) <= FOLD_LONG_EXAMPLES: one wavefront per row, FOLD_WAVES rows to a workgroup, no LDS and no barrier;
//   long rows   one workgroup per row (the leading workgroups of the grid, named by a slot list the host builds): chunk q goes to
//               wavefront q mod FOLD_WAVES, the partial S and hg meet in LDS, EVERY wavefront adds them from 0 in wavefront order and
//               takes the same step, so all of them hold the same node and no z has to be handed round.  Two barriers per step.
// Threshold: FOLD_LONG_EXAMPLES = FOLD_WAVES x 64 — a row is long once every wavefront of its workgroup has a full chunk of examples
// per step.  Below that the split has less than one chunk per wavefront to win and still pays the two barriers and LDS round trips.
// (num_neg = 5: rows of more than 42 items.)
//
// Summation order (fixed: the result is a function of the row alone).  Short: S over the kept items in ascending position, hg over the
// positives in ascending position, then the negatives in draw order.  Long: the same inside a wavefront's chunks, then the FOLD_WAVES
// partials from 0 in wavefront order.  Which of the two a row takes depends on n and num_neg only.
//
// Registers (NI = 8): node 32, b 8, z 8, S 8, hg 8, UN x NI = 32 in flight: 140 VGPRs, and no scratch at any NI (the build's
// kernel-resource-usage report: 37 / 57 / 104 / 140 VGPRs at NI = 1 / 2 / 4 / 8; the scalar registers that do not fit go to VGPR lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cdae_kernels.hpp"
#include "cdae_recommend_kernels.hpp"

namespace cdae {

constexpr int FOLD_WAVES = 4;
constexpr uint32_t FOLD_LONG_EXAMPLES = FOLD_WAVES * WAVE;
constexpr float FOLD_AG_INIT = 1e-4f;                    // reset()'s accumulator value (cdae.hpp:109-134)

__host__ __device__ __forceinline__ bool fold_row_is_long(uint64_t n, uint32_t num_neg) {
  return n * (1ull + num_neg) > (uint64_t)FOLD_LONG_EXAMPLES;
}

struct FoldArgs {
  uint64_t seed, stream_id_base;
  uint32_t epoch_begin, n_epochs, num_corruptions;
};
// where a start node comes from: the handle's users, or (top bit of the uid, table present) the guest table
struct FoldNodes {
  const float *Wu, *Wu_ag, *Uu, *Uu_ag;
  const float *Gwu, *Gwu_ag, *Guu, *Guu_ag;
};
struct FoldOut { float *wu, *wu_ag, *uu, *uu_ag; };      // [rows][Kp] each, indexed by the row's slot in the launch

// all epochs of one row on NW wavefronts (NW == 1: no LDS, no barrier).  Every wavefront ends with the fitted node.
template <int NI, int NW>
__device__ __forceinline__ void fold_in_row(const HyperParams& hp, const FoldArgs& a, const uint32_t* __restrict__ items, uint32_t n, uint64_t s,
                                            const float* __restrict__ W, const float* __restrict__ D, const float* __restrict__ bp,
                                            const float (&bb)[NI], float (&wu)[NI], float (&wa)[NI], float (&uu)[NI], float (&ua)[NI],
                                            uint32_t wid, uint32_t lane, float* __restrict__ lds_s, float* __restrict__ lds_hg) {
  constexpr int UN = NI >= 8 ? 4 : 8;
  const uint32_t lo = lane * NI;
  const uint64_t m = (uint64_t)n * hp.num_neg;
  for (uint32_t e = 0; e < a.n_epochs; ++e) {
    const uint32_t epoch = a.epoch_begin + e;
    const uint64_t key_c = cdae_rng_key(a.seed, epoch, s, CDAE_STREAM_CORRUPT);
    const uint64_t key_n = cdae_rng_key(a.seed, epoch, s, CDAE_STREAM_NEGATIVE);
    for (uint32_t c = 0; c < a.num_corruptions; ++c) {
      // ---- S: the kept rows of W, chunk by chunk, in ascending position ----
      float S[NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) S[i] = 0.f;
      uint32_t chunk = 0;
      for (uint32_t q0 = 0; q0 < n; q0 += WAVE, ++chunk) {
        if (NW > 1 && chunk % NW != wid) continue;                   // (wave-uniform)
        const uint32_t p = q0 + lane;
        uint32_t item = 0;
        int keep = 0;
        if (p < n) {
          item = items[p];
          keep = cdae_keep(cdae_rng_draw(key_c, (uint64_t)c * n + p), hp.keep_thr);
        }
        unsigned long long mask = __ballot(keep);
        while (mask) {
          float v[UN][NI];
#pragma unroll
          for (int j = 0; j < UN; ++j) {
            if (mask) {                                              // wave-uniform
              const int src = __ffsll((long long)mask) - 1;
              mask &= mask - 1;
              const uint32_t it = (uint32_t)__builtin_amdgcn_readlane((int)item, src);
              vload<NI>(v[j], W + (size_t)it * hp.Kp + lo);
            } else {
#pragma unroll
              for (int i = 0; i < NI; ++i) v[j][i] = 0.f;
            }
          }
#pragma unroll
          for (int j = 0; j < UN; ++j)
#pragma unroll
            for (int i = 0; i < NI; ++i) S[i] += v[j][i];
        }
      }
      if (NW > 1) {
#pragma unroll
        for (int i = 0; i < NI; ++i) { lds_s[wid * (64 * NI) + lo + i] = S[i]; S[i] = 0.f; }
        __syncthreads();
        for (int w = 0; w < NW; ++w)
#pragma unroll
          for (int i = 0; i < NI; ++i) S[i] += lds_s[w * (64 * NI) + lo + i];
      }
      // ---- z = act(scale S ((.) uu) + b (+ wu)), pad elements 0 (encode_finish_kernel's expression) ----
      float z[NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        float x = S[i];
        if (hp.linear_function) x *= uu[i];
        float hh = fmaf(x, hp.scale, bb[i]);
        if (hp.user_factor) hh += wu[i];
        z[i] = lo + i < hp.K ? activate(hp, hh) : 0.f;
      }
      // ---- hg: the n positives (target 1), then the m negatives (target 0), chunk by chunk ----
      float hg[NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) hg[i] = 0.f;
      const uint64_t n_ex = (uint64_t)n + m;
      for (uint64_t x0 = 0; x0 < n_ex; ++chunk) {
        const bool positive = x0 < n;                                // (a chunk never straddles the two lists)
        const uint64_t list_end = positive ? (uint64_t)n : n_ex;
        const uint32_t cnt = (uint32_t)(list_end - x0 < (uint64_t)WAVE ? list_end - x0 : (uint64_t)WAVE);
        const uint64_t x = x0 + lane;
        x0 += cnt;
        if (NW > 1 && chunk % NW != wid) continue;                   // (wave-uniform)
        uint32_t item = 0;
        if (lane < cnt)
          item = positive ? items[x] : cdae_sample_negative(key_n, (uint64_t)c * m + (x - n), items, n, hp.num_items);
        const float bias = lane < cnt ? bp[item] : 0.f;              // requested before the rows
        const float target = positive ? 1.f : 0.f;
        for (uint32_t j0 = 0; j0 < cnt; j0 += UN) {
          float v[UN][NI];
#pragma unroll
          for (int j = 0; j < UN; ++j)
            if (j0 + j < cnt) {                                      // wave-uniform
              const uint32_t it = (uint32_t)__builtin_amdgcn_readlane((int)item, (int)(j0 + j));
              vload<NI>(v[j], D + (size_t)it * hp.Kp + lo);
            }
#pragma unroll
          for (int j = 0; j < UN; ++j)
            if (j0 + j < cnt) {
              float dot = z[0] * v[j][0];
#pragma unroll
              for (int i = 1; i < NI; ++i) dot = fmaf(z[i], v[j][i], dot);
              const float y = wave_sum(dot) + __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, bias), (int)(j0 + j)));
              const float g = loss_grad(hp.loss_type, y, target);
#pragma unroll
              for (int i = 0; i < NI; ++i) hg[i] = fmaf(g, v[j][i], hg[i]);
            }
        }
      }
      if (NW > 1) {
#pragma unroll
        for (int i = 0; i < NI; ++i) { lds_hg[wid * (64 * NI) + lo + i] = hg[i]; hg[i] = 0.f; }
        __syncthreads();
        for (int w = 0; w < NW; ++w)
#pragma unroll
          for (int i = 0; i < NI; ++i) hg[i] += lds_hg[w * (64 * NI) + lo + i];
      }
      // ---- the node's step, both gradients from the pre-step values; pad elements stay as they are ----
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        if (lo + i < hp.K) {
          const float delta = hg[i] * act_deriv(hp, z[i]);
          if (hp.user_factor) ada_step(hp, wu[i], wa[i], fmaf(hp.lambda, wu[i], delta));
          if (hp.linear_function) ada_step(hp, uu[i], ua[i], fmaf(hp.lambda, uu[i], delta * S[i]));
        }
      }
    }
  }
}

// one row of the launch: its start node, its epochs, its fitted node to the staging rows of `slot`
template <int NI, int NW>
__device__ __forceinline__ void fold_in_slot(const HyperParams& hp, const FoldArgs& a, const int64_t* __restrict__ row_ptr,
                                             const uint32_t* __restrict__ col, const uint32_t* __restrict__ uids, uint64_t row, uint32_t slot,
                                             const float* __restrict__ W, const float* __restrict__ D, const float* __restrict__ b,
                                             const float* __restrict__ bp, const FoldNodes& nd, const FoldOut& out, uint32_t wid, uint32_t lane,
                                             float* __restrict__ lds_s, float* __restrict__ lds_hg) {
  const int64_t p0 = row_ptr[row];
  const uint32_t n = (uint32_t)(row_ptr[row + 1] - p0);
  const uint32_t uid = uids[row];
  const uint32_t lo = lane * NI;
  float bb[NI], wu[NI], wa[NI], uu[NI], ua[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) { wu[i] = 0.f; wa[i] = FOLD_AG_INIT; uu[i] = 1.f; ua[i] = FOLD_AG_INIT; }
  vload<NI>(bb, b + lo);
  if (uid != ROW_NO_USER) {
    const bool guest = nd.Gwu != nullptr && (uid & ROW_GUEST) != 0u;
    const size_t o = (size_t)(guest ? uid & ~ROW_GUEST : uid) * hp.Kp + lo;
    if (hp.user_factor) { vload<NI>(wu, (guest ? nd.Gwu : nd.Wu) + o); vload<NI>(wa, (guest ? nd.Gwu_ag : nd.Wu_ag) + o); }
    if (hp.linear_function) { vload<NI>(uu, (guest ? nd.Guu : nd.Uu) + o); vload<NI>(ua, (guest ? nd.Guu_ag : nd.Uu_ag) + o); }
  }
  if (n) fold_in_row<NI, NW>(hp, a, col + p0, n, a.stream_id_base + row, W, D, bp, bb, wu, wa, uu, ua, wid, lane, lds_s, lds_hg);
  if (wid != 0) return;
  const size_t o = (size_t)slot * hp.Kp + lo;
  vstore<NI>(out.wu + o, wu);
  vstore<NI>(out.wu_ag + o, wa);
  vstore<NI>(out.uu + o, uu);
  vstore<NI>(out.uu_ag + o, ua);
}

// rows [r0, r0 + nu) of the device CSR.  grid = n_long + ceil(nu / FOLD_WAVES): workgroup g < n_long takes the long row of slot
// long_slots[g] (every one of them < nu and long by fold_row_is_long: the host's list); the others take FOLD_WAVES slots each, a
// wavefront per row, and leave the long ones alone.
template <int NI>
__global__ void __launch_bounds__(FOLD_WAVES * WAVE)
fold_in_rows_kernel(HyperParams hp, FoldArgs a, const int64_t* __restrict__ row_ptr, const uint32_t* __restrict__ col,
                    const uint32_t* __restrict__ uids, uint64_t r0, uint32_t nu, const uint32_t* __restrict__ long_slots, uint32_t n_long,
                    const float* __restrict__ W, const float* __restrict__ D, const float* __restrict__ b, const float* __restrict__ bp,
                    FoldNodes nd, FoldOut out) {
  // Only the long role uses the LDS; the short-row workgroups of the same launch reserve their 2 NI KiB for nothing.  At 16 KiB (NI = 8)
  // ten workgroups still fit a CU's 160 KiB, more than the three wavefronts per SIMD the registers allow, so it costs no occupancy.
  __shared__ float lds[2][FOLD_WAVES * 64 * NI];
  const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE)), lane = threadIdx.x % WAVE;
  if (blockIdx.x < n_long) {                                         // (workgroup-uniform: the barriers are the long role's alone)
    const uint32_t slot = long_slots[blockIdx.x];
    fold_in_slot<NI, FOLD_WAVES>(hp, a, row_ptr, col, uids, r0 + slot, slot, W, D, b, bp, nd, out, wid, lane, lds[0], lds[1]);
    return;
  }
  const uint32_t slot = (blockIdx.x - n_long) * FOLD_WAVES + wid;
  if (slot >= nu) return;
  const uint64_t row = r0 + slot;
  if (fold_row_is_long((uint64_t)(row_ptr[row + 1] - row_ptr[row]), hp.num_neg)) return;
  fold_in_slot<NI, 1>(hp, a, row_ptr, col, uids, row, slot, W, D, b, bp, nd, out, 0u, lane, nullptr, nullptr);
}

// rows [0, n) of the four node arrays to their "no node" values, before set_guest_nodes copies the caller's columns over them
__global__ void __launch_bounds__(256)
fold_fill_kernel(float* __restrict__ p, size_t count, float value) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) p[i] = value;
}

}  // namespace cdae
