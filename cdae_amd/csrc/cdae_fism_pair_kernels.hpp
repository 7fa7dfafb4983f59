// cdae_fism_pair_kernels.hpp — FISMauc: the pairwise form of FISM (Kabbur, Ning, Karypis, KDD'13; the reference's
// src/model/recsys/fism_pair.hpp), DESIGN.md §8n.  A pair (i, j) of a rated item and a drawn negative shares ONE neighbourhood vector
// v = x - P[i]; its difference d = [bi[i] - bi[j]] + s v . (Q[i] - Q[j]) takes one sweep of the user's rows with qd = Q[i] - Q[j], so a
// positive costs num_neg sweeps against FISM's 1 + num_neg.
//   fism_pair_user_kernel<NI, ADA>   ONE workgroup of FISM_WAVES wavefronts walks the launch's users on the visit frame of
//                                    cdae_fism_kernels.hpp (row ownership, resident rows, the order of every sum: stated there).
//                                    Per positive: the owner of P[i] publishes it through LDS ONCE for its pairs; every
//                                    wavefront loads Q[i], its accumulator and bi[i] and carries them through the positive's pairs,
//                                    stepping them redundantly (same instructions, same bits: the way fism_user_kernel carries bu);
//                                    the output wavefront stores them once, with the last pair.  Per pair: every wavefront loads Q[j]
//                                    and bi[j], forms qd, d and g; behind the barrier that keeps the output wavefront's stores after
//                                    everybody's loads it sweeps its rows with qd; the output wavefront steps Q[j] and bi[j] in memory.
// The output wavefront is the LAST one: it owns the fewest row positions.
// What is stored and read again is read past the L1 after the storer's vmcnt(0) and a barrier, as in §8m.  A negative that repeats
// inside a positive is loaded again for every pair, so the second pair sees the first one's step.  No atomics on parameters.
#pragma once
#include "cdae_fism_kernels.hpp"

namespace cdae {

template <int NI, bool ADA>
__global__ void __launch_bounds__(FISM_WAVES * WAVE)
fism_pair_user_kernel(HyperParams hp, uint32_t bias_term, uint32_t res_rows /* 0 or FISM_WAVES * fism_resident_slots(NI) */,
                      const int64_t* __restrict__ row_ptr, const uint32_t* __restrict__ col, uint64_t u0, uint32_t nb, uint64_t seed,
                      uint32_t epoch, const float* __restrict__ scale /* [num_items + 1] */, float* P, float* P_ag, float* Q, float* Q_ag,
                      float* BI, float* BI_ag, float* /* BU */, float* /* BU_ag: fism_user_kernel's arguments; bu cancels in a pair */) {
  constexpr uint32_t W = FISM_WAVES;
  constexpr uint32_t OUT = W - 1u;                             // the output wavefront
  constexpr int R = (int)fism_resident_slots(NI);
  constexpr uint32_t KP = WAVE * NI;
  __shared__ float s_pi[KP];                                   // P[i] of the positive (it takes no step while i is the positive)
  __shared__ float s_d[2][W][KP];                              // per-wavefront column sums, two sets in turn
  const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  const uint32_t lane = threadIdx.x % WAVE, lo = lane * NI;
  uint32_t par = 0;
  for (uint32_t slot = 0; slot < nb; ++slot) {
    const uint64_t uid = u0 + slot;
    const int64_t r0 = row_ptr[uid];
    const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(row_ptr[uid + 1] - r0));
    if (n == 0u) continue;                                     // no pair, and scale[n - 1] does not exist; no barrier reached yet
    const uint32_t* row = col + r0;
    const uint32_t n_res = min(n, res_rows);
    const float s = scale[n - 1u];                             // both items of a pair (fism_pair.hpp:137, 147, 148); 0 for a lone positive
    const uint64_t key_n = cdae_rng_key(seed, epoch, uid + hp.uid_offset, CDAE_STREAM_NEGATIVE);
    float pr[R][NI], pa[R][NI];
    {
      float part[NI];
      fism_visit_load<NI, R>(pr, pa, part, row, n, n_res, res_rows, w, lo, P, P_ag);
#pragma unroll
      for (int i = 0; i < NI; ++i) s_d[par][w][lo + i] = part[i];
    }
    __syncthreads();
    float x[NI];
    fism_total<NI>(s_d[par], lo, x);
    par ^= 1u;
    for (uint32_t p = 0; p < n; ++p) {
      const uint32_t item_i = (uint32_t)__builtin_amdgcn_readfirstlane((int)row[p]);
      // the owner of P[i] publishes it, once for the positive's pairs
      fism_publish<NI, R>(s_pi, pr, p, n_res, w, lo, P + (size_t)item_i * KP);
      // every wavefront: Q[i], its accumulator and bi[i], carried through the pairs (nobody has stored them since the last barrier
      // behind a vmcnt(0): a negative of this user is never i)
      float qi[NI], qia[NI];
      fism_load_row<NI>(qi, Q + (size_t)item_i * KP, lo);
      fism_load_row<NI>(qia, Q_ag + (size_t)item_i * KP, lo);
      float bi_i = 0.f, bia_i = 1.f;
      if (bias_term) { bi_i = load_f32_sc1(BI + item_i); bia_i = load_f32_sc1(BI_ag + item_i); }
      __syncthreads();
      uint32_t cand = 0;
      for (uint32_t k = 0; k < hp.num_neg; ++k) {
        if (k % WAVE == 0u) {                                  // the next 64 negatives of this positive, one per lane
          cand = 0;
          if (k + lane < hp.num_neg) cand = cdae_sample_negative(key_n, (uint64_t)p * hp.num_neg + (k + lane), row, n, hp.num_items);
        }
        const uint32_t item_j = (uint32_t)__builtin_amdgcn_readlane((int)cand, (int)(k % WAVE));
        float qj[NI], qd[NI], v[NI];
        fism_load_row<NI>(qj, Q + (size_t)item_j * KP, lo);
        float bj = 0.f;
        if (bias_term) bj = load_f32_sc1(BI + item_j);
        float dot = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          v[i] = x[i] - s_pi[lo + i];                          // the current x
          qd[i] = qi[i] - qj[i];
          dot = fmaf(v[i], qd[i], dot);
        }
        dot = wave_sum(dot);
        const float diff = fmaf(s, dot, bias_term ? bi_i - bj : 0.f);
        const float g = mf_loss_grad(hp.loss_type, diff, 1.f);
        const float gs = g * s;
        // every wavefront holds Q[j] and bi[j] from BEFORE this pair's step before the output wavefront may store the stepped values
        __builtin_amdgcn_s_waitcnt(WAIT_VM0);
        __syncthreads();
        float d[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) d[i] = 0.f;
#pragma unroll
        for (int sl = 0; sl < R; ++sl) {
          const uint32_t qp = w + W * (uint32_t)sl;
          if (qp < n_res && qp != p) fism_row_step<NI, ADA>(hp, pr[sl], pa[sl], qd, gs, d);
        }
        fism_sweep_streamed<NI, ADA>(hp, row, n, res_rows, w, lo, p, P, P_ag, qd, gs, d);
#pragma unroll
        for (int i = 0; i < NI; ++i) s_d[par][w][lo + i] = d[i];
        // the output wavefront: Q[j] on -g s v + lambda Q[j], bi[j] on -g + lambda bi[j]
        if (w == OUT) {
          float qa[NI];
          fism_load_row<NI>(qa, Q_ag + (size_t)item_j * KP, lo);
#pragma unroll
          for (int i = 0; i < NI; ++i) { const float before = qj[i]; ada_step_t<ADA>(hp, qj[i], qa[i], fmaf(-gs, v[i], hp.lambda * before)); }
          vstore<NI>(Q + (size_t)item_j * KP + lo, qj);
          vstore<NI>(Q_ag + (size_t)item_j * KP + lo, qa);
          if (bias_term && lane == 0u) {
            float b = bj, ba = load_f32_sc1(BI_ag + item_j);
            ada_step_t<ADA>(hp, b, ba, fmaf(hp.lambda, b, -g));
            BI[item_j] = b; BI_ag[item_j] = ba;
          }
        }
        // every wavefront: its copy of Q[i] on g s v + lambda Q[i] and of bi[i] on g + lambda bi[i]
#pragma unroll
        for (int i = 0; i < NI; ++i) { const float before = qi[i]; ada_step_t<ADA>(hp, qi[i], qia[i], fmaf(gs, v[i], hp.lambda * before)); }
        if (bias_term) ada_step_t<ADA>(hp, bi_i, bia_i, fmaf(hp.lambda, bi_i, g));
        if (w == OUT && k + 1u == hp.num_neg) {                 // ... stored once, with the positive's last pair
          vstore<NI>(Q + (size_t)item_i * KP + lo, qi);
          vstore<NI>(Q_ag + (size_t)item_i * KP + lo, qia);
          if (bias_term && lane == 0u) { BI[item_i] = bi_i; BI_ag[item_i] = bia_i; }
        }
        __builtin_amdgcn_s_waitcnt(WAIT_VM0);                  // this pair's stores are in memory before anybody reads them again
        __syncthreads();
        float t[NI];
        fism_total<NI>(s_d[par], lo, t);
#pragma unroll
        for (int i = 0; i < NI; ++i) x[i] += t[i];
        par ^= 1u;
      }
    }
    // the resident rows go back; the next visit reads them behind the barrier
    fism_visit_store<NI, R>(pr, pa, row, n_res, w, lo, P, P_ag);
    __builtin_amdgcn_s_waitcnt(WAIT_VM0);
    __syncthreads();
  }
}

}  // namespace cdae
