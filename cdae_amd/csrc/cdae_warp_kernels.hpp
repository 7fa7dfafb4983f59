// cdae_warp_kernels.hpp — WARP: rank-weighted pairwise matrix factorisation (Weston, Bengio, Usunier, "WSABIE: scaling up to large
// vocabulary image annotation"; the reference's src/model/recsys/warp.hpp, `class WARP : public IMF`), DESIGN.md §8l.
// Per (user, positive i, k < num_neg) the model SEARCHES for a negative j that violates the margin, s(j) > s(i) - 1, among at most
// CDAE_WARP_MAX_TRY draws; the number of draws cnt sets the step size through the rank weight l[(num_items - n_u) / cnt].  Unlike
// IMF / BPR (cdae_mf_kernels.hpp) nothing is drawn ahead of the step: the items of a pair are chosen on the device, against the
// parameters of the moment.
//   warp_search<NI>                 one wavefront, the user vector in registers: candidates 64 at a time (one per lane: rejection sampling
//                                   and the binary search of cdae_sample_negative run lane-parallel), scored in draw order in groups of
//                                   WARP_GROUP rows whose loads are in flight together; leaves at the first group that holds a violator
//   warp_search_kernel<NI>          cdae_hip_warp_search: the search of every pair of a range of users, nothing trained
//   warp_user_kernel<NI, IN_PLACE>  IN_PLACE: the reference loop — one wavefront walks the launch's users in order and steps uv, iv_i and
//                                   iv_j of every pair at once.  Otherwise phase U of the block schedule: a wavefront per user of the block
//                                   against the block-start item rows; every pair leaves BPR's record (two examples, g, the user vector
//                                   before its step) for mf_item_kernel, a skipped pair two VOID examples.
// Scores: s(x) = ib[x] + uv . iv_x (ub cancels on both sides of the test); biases are read and never stepped (warp.hpp:93-94, 100-103,
// 112-113 are comments).  yui is taken ONCE per positive (warp.hpp:71) and is stale between that positive's pairs in the reference too,
// so the block schedule carries no private copy of the positive's row as BPR's does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cdae_mf_kernels.hpp"
#include "cdae_warp_host.h"

namespace cdae {

constexpr uint32_t WARP_LOOK = WARP_MAX_TRY - 1u;   // draws that can train a pair: a violator found at the 500th draw is skipped too (warp.hpp:79-83)
constexpr uint32_t WARP_NONE = 0xFFFFFFFFu;    // the item of an exhausted search
constexpr int WARP_GROUP = 8;                  // candidate rows in flight together

struct WarpPick { uint32_t item, cnt; float score; };   // cnt == WARP_MAX_TRY: exhausted (item WARP_NONE, score 0)

// x . y over the wavefront's NI floats per lane
template <int NI>
__device__ __forceinline__ float warp_dot(const float (&x)[NI], const float (&y)[NI]) {
  float dot = 0.f;
#pragma unroll
  for (int i = 0; i < NI; ++i) dot = fmaf(x[i], y[i], dot);
  return wave_sum(dot);
}

// The search of pair (p, k) of a user: candidate t is cdae_sample_negative(key_n, warp_draw_index(p, num_neg, k, t), ...); the
// first t < WARP_LOOK with s(cand) > thr wins, cnt = t + 1.  Every candidate of one search is scored against the same state: uv is in
// registers and the caller steps nothing until the search has returned.  COHERENT: the rows may have been stored by this wavefront
// (the in-place loop; the caller has waited for its stores) — read past the L1.  Everything returned is wave-uniform.
template <int NI, bool COHERENT>
__device__ __forceinline__ WarpPick warp_search(const float (&uv)[NI], uint32_t lo, uint32_t Kp, const float* __restrict__ IV,
                                                const float* __restrict__ IB, uint64_t key_n, uint32_t p, uint32_t num_neg, uint32_t k, const uint32_t* __restrict__ row,
                                                uint32_t n, uint32_t num_items, float thr, uint32_t lane) {
  for (uint32_t t0 = 0; t0 < WARP_LOOK; t0 += WAVE) {
    const uint32_t cnt = min((uint32_t)WAVE, WARP_LOOK - t0);              // candidates of this round (wave-uniform)
    uint32_t cand = 0;
    float cb = 0.f;
    if (lane < cnt) {
      cand = cdae_sample_negative(key_n, warp_draw_index(p, num_neg, k, t0 + lane), row, n, num_items);
      cb = IB[cand];                                                       // (item biases are never stepped: a plain load)
    }
    for (uint32_t g0 = 0; g0 < cnt; g0 += WARP_GROUP) {
      float r[WARP_GROUP][NI];
#pragma unroll
      for (int s = 0; s < WARP_GROUP; ++s) {                               // past the end of the round: the last candidate again (never used)
        const uint32_t it = (uint32_t)__builtin_amdgcn_readlane((int)cand, min(g0 + (uint32_t)s, cnt - 1u));
        if (COHERENT) vload_coherent<NI>(r[s], IV + (size_t)it * Kp + lo); else vload<NI>(r[s], IV + (size_t)it * Kp + lo);
      }
      float sc[WARP_GROUP];
#pragma unroll
      for (int s = 0; s < WARP_GROUP; ++s)
        sc[s] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, cb), min(g0 + (uint32_t)s, cnt - 1u))) + warp_dot<NI>(uv, r[s]);
#pragma unroll
      for (int s = 0; s < WARP_GROUP; ++s) {
        if (g0 + (uint32_t)s < cnt && sc[s] > thr)
          return WarpPick{(uint32_t)__builtin_amdgcn_readlane((int)cand, g0 + (uint32_t)s), t0 + g0 + (uint32_t)s + 1u, sc[s]};
      }
    }
  }
  return WarpPick{WARP_NONE, WARP_MAX_TRY, 0.f};
}

// cdae_hip_warp_search: one wavefront per user of [u0, u0 + nb); out index q = (row offset of the positive from row_ptr[base]) * num_neg + k
template <int NI>
__global__ void __launch_bounds__(256)
warp_search_kernel(HyperParams hp, const int64_t* __restrict__ row_ptr, const uint32_t* __restrict__ col, uint64_t u0, uint32_t nb,
                   int64_t base /* row_ptr[u0]: outputs are relative to this chunk */, uint64_t seed, uint32_t epoch,
                   const float* __restrict__ UV, const float* __restrict__ IV, const float* __restrict__ IB,
                   uint32_t* __restrict__ out_item, uint32_t* __restrict__ out_cnt, float* __restrict__ out_margin) {
  const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE));
  const uint32_t lane = threadIdx.x % WAVE;
  if (slot >= nb) return;
  const uint64_t uid = u0 + slot;
  const int64_t r0 = row_ptr[uid];
  const uint32_t n = (uint32_t)(row_ptr[uid + 1] - r0);
  const uint32_t* row = col + r0;
  const uint32_t lo = lane * NI;
  const uint64_t key_n = cdae_rng_key(seed, epoch, uid + hp.uid_offset, CDAE_STREAM_NEGATIVE);
  float uv[NI];
  vload<NI>(uv, UV + (size_t)uid * hp.Kp + lo);
  for (uint32_t p = 0; p < n; ++p) {
    const uint32_t it = row[p];
    float ri[NI];
    vload<NI>(ri, IV + (size_t)it * hp.Kp + lo);
    const float thr = IB[it] + warp_dot<NI>(uv, ri) - 1.f;
    for (uint32_t k = 0; k < hp.num_neg; ++k) {
      const WarpPick w = warp_search<NI, false>(uv, lo, hp.Kp, IV, IB, key_n, p, hp.num_neg, k, row, n, hp.num_items, thr, lane);
      const uint64_t q = (uint64_t)(r0 - base + p) * hp.num_neg + k;
      if (lane == 0) {
        out_item[q] = w.item; out_cnt[q] = w.cnt;
        if (out_margin) out_margin[q] = w.cnt >= WARP_MAX_TRY ? 0.f : w.score - thr;
      }
    }
  }
}

// the reference loop (IN_PLACE) / phase U of the block schedule
template <int NI, bool IN_PLACE>
__global__ void __launch_bounds__(256)
warp_user_kernel(HyperParams hp, const int64_t* __restrict__ row_ptr, const uint32_t* __restrict__ col, uint64_t u0, uint32_t nb,
                 uint64_t seed, uint32_t epoch, const float* __restrict__ rank_w /* [num_items]: H_{idx + 1} */, float* __restrict__ UV,
                 float* __restrict__ UV_ag, float* __restrict__ IV, float* __restrict__ IV_ag, const float* __restrict__ IB,
                 uint32_t* __restrict__ ex_item, uint64_t* __restrict__ ex_val, float* __restrict__ UVpre, float* __restrict__ G,
                 uint32_t* __restrict__ rec_item /* cdae_hip_warp_record_choices: [nnz * num_neg] by position, or nullptr */,
                 uint32_t* __restrict__ rec_cnt) {
  const uint32_t wave_slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE));
  const uint32_t lane = threadIdx.x % WAVE;
  if (wave_slot >= (IN_PLACE ? 1u : nb)) return;
  const uint32_t slot_first = IN_PLACE ? 0u : wave_slot, slot_end = IN_PLACE ? nb : wave_slot + 1u;
  const uint32_t lo = lane * NI;
  const float lam2 = hp.lambda;                        // the host stores 2 * lambda here (warp.hpp:95-97)
  auto run = [&](auto ada_tag) __attribute__((always_inline)) {
  constexpr bool ADA = decltype(ada_tag)::value;
  for (uint32_t slot = slot_first; slot < slot_end; ++slot) {
    const uint64_t uid = u0 + slot;
    const int64_t r0 = row_ptr[uid];
    const uint32_t n = (uint32_t)(row_ptr[uid + 1] - r0);
    const uint32_t* row = col + r0;
    const uint32_t items_left = hp.num_items - n;      // warp.hpp:68
    const uint64_t key_n = cdae_rng_key(seed, epoch, uid + hp.uid_offset, CDAE_STREAM_NEGATIVE);
    const uint64_t inst0 = (uint64_t)(r0 - row_ptr[u0]) * hp.num_neg;      // first pair of the user in the block
    float uv[NI], ua[NI];
    vload<NI>(uv, UV + (size_t)uid * hp.Kp + lo);
    vload<NI>(ua, UV_ag + (size_t)uid * hp.Kp + lo);
    for (uint32_t p = 0; p < n; ++p) {
      const uint32_t it = row[p];
      float ri[NI];
      // IN_PLACE: this wavefront may have stepped the row (as a negative of an earlier pair, or as a positive of an earlier user)
      if (IN_PLACE) { __builtin_amdgcn_s_waitcnt(WAIT_VM0); vload_coherent<NI>(ri, IV + (size_t)it * hp.Kp + lo); }
      else vload<NI>(ri, IV + (size_t)it * hp.Kp + lo);
      const float yui = IB[it] + warp_dot<NI>(uv, ri);                     // warp.hpp:71: once per positive
      for (uint32_t k = 0; k < hp.num_neg; ++k) {
        const uint64_t pair = (uint64_t)p * hp.num_neg + k;
        if (IN_PLACE) __builtin_amdgcn_s_waitcnt(WAIT_VM0);                // the rows the last pair stepped are in memory
        const WarpPick w = warp_search<NI, IN_PLACE>(uv, lo, hp.Kp, IV, IB, key_n, p, hp.num_neg, k, row, n, hp.num_items, yui - 1.f, lane);
        if (rec_item && lane == 0) { rec_item[(uint64_t)r0 * hp.num_neg + pair] = w.item; rec_cnt[(uint64_t)r0 * hp.num_neg + pair] = w.cnt; }
        const uint64_t q = inst0 + pair;
        if (w.cnt >= WARP_MAX_TRY) {                                       // warp.hpp:83: the pair is skipped
          if (!IN_PLACE && lane == 0) {                                    // two VOID examples (item num_items sorts behind every row)
            ex_item[2u * q] = hp.num_items; ex_item[2u * q + 1u] = hp.num_items;
            ex_val[2u * q] = (q << 32) | (uint64_t)slot; ex_val[2u * q + 1u] = (q << 32) | (uint64_t)(slot | TARGET_BIT);
            G[q] = 0.f;
          }
          continue;
        }
        const uint32_t jt = w.item;
        const float g = mf_loss_grad(hp.loss_type, yui - w.score, 1.f) * rank_w[items_left / w.cnt];     // warp.hpp:84, 91-92
        float rj[NI];
        if (IN_PLACE) {
          // the rows as they are NOW (warp.hpp:95-97 read iv_ at the step; only yui is stale), with their accumulators
          float ai[NI], aj[NI];
          vload_coherent<NI>(ri, IV + (size_t)it * hp.Kp + lo);
          vload_coherent<NI>(rj, IV + (size_t)jt * hp.Kp + lo);
          vload_coherent<NI>(ai, IV_ag + (size_t)it * hp.Kp + lo);
          vload_coherent<NI>(aj, IV_ag + (size_t)jt * hp.Kp + lo);
          float wi[NI], wj[NI];
#pragma unroll
          for (int i = 0; i < NI; ++i) {                                   // all three from the pre-step values (warp.hpp:95-97)
            wi[i] = ri[i]; wj[i] = rj[i];
            ada_step_t<ADA>(hp, wi[i], ai[i], fmaf(g, uv[i], lam2 * ri[i]));
            ada_step_t<ADA>(hp, wj[i], aj[i], fmaf(-g, uv[i], lam2 * rj[i]));
          }
          vstore<NI>(IV + (size_t)it * hp.Kp + lo, wi);
          vstore<NI>(IV_ag + (size_t)it * hp.Kp + lo, ai);
          vstore<NI>(IV + (size_t)jt * hp.Kp + lo, wj);
          vstore<NI>(IV_ag + (size_t)jt * hp.Kp + lo, aj);
        } else {
          vload<NI>(rj, IV + (size_t)jt * hp.Kp + lo);
          vstore<NI>(UVpre + (size_t)q * hp.Kp + lo, uv);
          if (lane == 0) {
            ex_item[2u * q] = it; ex_item[2u * q + 1u] = jt;
            ex_val[2u * q] = (q << 32) | (uint64_t)slot; ex_val[2u * q + 1u] = (q << 32) | (uint64_t)(slot | TARGET_BIT);
            G[q] = g;
          }
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) ada_step_t<ADA>(hp, uv[i], ua[i], fmaf(g, ri[i] - rj[i], lam2 * uv[i]));
      }
    }
    vstore<NI>(UV + (size_t)uid * hp.Kp + lo, uv);
    vstore<NI>(UV_ag + (size_t)uid * hp.Kp + lo, ua);
  }
  };
  if (hp.adagrad) run(std::true_type{}); else run(std::false_type{});
}

}  // namespace cdae
