// cdae_fism_kernels.hpp — FISM: factored item similarity (Kabbur, Ning, Karypis, KDD'13; the reference's src/model/recsys/fism.hpp),
// DESIGN.md §8m.  A user is the sum x of the input rows P[j] of their items; an item is scored against a second table Q.  Every
// instance (u, i) steps ALL n_u rows P[j], j in R_u, so a visit is (1 + num_neg) n_u instances of n_u row steps each.
//   fism_user_kernel<NI, ADA>     the loop: ONE workgroup of FISM_WAVES wavefronts walks the launch's users in order (consecutive visits
//                                 share rows), on the visit frame below.  Per instance every wavefront loads Q[item] and
//                                 forms the prediction and g redundantly (same instructions, same bits: g itself crosses no
//                                 barrier); behind a barrier that keeps wavefront 0's stores after everybody's loads it steps its
//                                 rows and leaves its column sums of (after - before) in LDS; after one more barrier every wavefront
//                                 adds them to its copy of x in wavefront order.  Wavefront 0 steps Q[item] and bi[item]; bu is
//                                 carried by every wavefront and stored by wavefront 0 at the end of the visit.  For k = 0 the owner
//                                 of P[i] publishes it through LDS first.  A user with no items is passed over before the
//                                 visit's first load and barrier.
//   fism_encode_rows_kernel<NI>   serving: z = scale[n] * sum of the rated rows of P, a wavefront per row of a chunk.
//   the visit frame               what this loop shares with the pair loop (cdae_fism_pair_kernels.hpp): which wavefront owns which row
//                                 position, the rows that stay in registers for a visit, the order of every sum; five helpers
//                                 (fism_visit_load, fism_total, fism_publish, fism_sweep_streamed, fism_visit_store) without a barrier
//                                 or a wait in them, so each kernel body shows its own in program order.
// Everything this workgroup has stored and reads again (P, Q, their accumulators, bi) is read past the L1 (sc1 loads) after the storing
// wavefront has waited for its stores and the workgroup has met at a barrier: the discipline of the in-place MF kernels.
// No atomics on parameters; the same state gives the same bits on every run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cdae_mf_kernels.hpp"
#include "cdae_fism_host.h"

namespace cdae {

// NI floats of a row this workgroup may have stored: past the L1, through a descriptor of the row itself (any table size)
template <int NI>
__device__ __forceinline__ void fism_load_row(float (&d)[NI], const float* row_base, uint32_t lo) {
  vload_sc1<NI>(d, rows_rsrc(row_base), lo * (uint32_t)sizeof(float));
}

// one row's step of an instance: P[j] steps on gs * Q[item] + lambda * P[j]; d collects after - before
template <int NI, bool ADA>
__device__ __forceinline__ void fism_row_step(const HyperParams& hp, float (&w)[NI], float (&a)[NI], const float (&q)[NI], float gs, float (&d)[NI]) {
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const float before = w[i];
    ada_step_t<ADA>(hp, w[i], a[i], fmaf(gs, q[i], hp.lambda * before));
    d[i] += w[i] - before;
  }
}

// ---- the visit frame: what fism_user_kernel and fism_pair_user_kernel (cdae_fism_pair_kernels.hpp) do alike -----------------------------
// Row position q of the user belongs to wavefront q % FISM_WAVES; positions [0, n_res), n_res = min(n, res_rows), are resident: slot sl of
// wavefront w holds position w + FISM_WAVES * sl in pr[sl] with its accumulator in pa[sl] for the whole visit (loaded once, stored
// once); later positions are stepped through memory every step (an instance of FISM, a pair of FISMauc).
// Summation order (it does not depend on where a row lives, so res_rows = 0 gives the same bits): a wavefront sums its rows'
// contributions in position order from 0.f; the FISM_WAVES sums are added in wavefront order from 0.f; x at the start of a visit IS that
// total, x after a step is x + that total.
// No helper holds a barrier or a wait: every __syncthreads() and vmcnt(0) stands in the two kernel bodies.

// visit load: the resident rows into pr / pa (an empty slot: 0 and 1), and part = this wavefront's sum of its rows of P
template <int NI, int R>
__device__ __forceinline__ void fism_visit_load(float (&pr)[R][NI], float (&pa)[R][NI], float (&part)[NI], const uint32_t* row, uint32_t n,
                                                uint32_t n_res, uint32_t res_rows, uint32_t w, uint32_t lo, const float* P, const float* P_ag) {
  constexpr uint32_t W = FISM_WAVES, KP = WAVE * NI;
#pragma unroll
  for (int i = 0; i < NI; ++i) part[i] = 0.f;
#pragma unroll
  for (int sl = 0; sl < R; ++sl) {
    const uint32_t qp = w + W * (uint32_t)sl;
    if (qp < n_res) {
      const uint32_t it = (uint32_t)__builtin_amdgcn_readfirstlane((int)row[qp]);
      fism_load_row<NI>(pr[sl], P + (size_t)it * KP, lo);
      fism_load_row<NI>(pa[sl], P_ag + (size_t)it * KP, lo);
#pragma unroll
      for (int i = 0; i < NI; ++i) part[i] += pr[sl][i];
    } else {
#pragma unroll
      for (int i = 0; i < NI; ++i) { pr[sl][i] = 0.f; pa[sl][i] = 1.f; }
    }
  }
  for (uint32_t qp = res_rows + w; qp < n; qp += W) {
    const uint32_t it = (uint32_t)__builtin_amdgcn_readfirstlane((int)row[qp]);
    float t[NI];
    fism_load_row<NI>(t, P + (size_t)it * KP, lo);
#pragma unroll
    for (int i = 0; i < NI; ++i) part[i] += t[i];
  }
}

// total: the FISM_WAVES sums of one set of column sums, in wavefront order from 0.f
template <int NI>
__device__ __forceinline__ void fism_total(const float (&set)[FISM_WAVES][WAVE * NI], uint32_t lo, float (&t)[NI]) {
#pragma unroll
  for (int i = 0; i < NI; ++i) t[i] = 0.f;
  for (uint32_t ww = 0; ww < FISM_WAVES; ++ww)
#pragma unroll
    for (int i = 0; i < NI; ++i) t[i] += set[ww][lo + i];
}

// publish: the owner of position p writes its row (item's) as it is now to s_pi, from its register slot or from memory
template <int NI, int R>
__device__ __forceinline__ void fism_publish(float (&s_pi)[WAVE * NI], const float (&pr)[R][NI], uint32_t p, uint32_t n_res, uint32_t w,
                                             uint32_t lo, const float* P_item) {
  if (w != p % FISM_WAVES) return;
  float t[NI];
  if (p < n_res) {
#pragma unroll
    for (int sl = 0; sl < R; ++sl)
      if ((uint32_t)sl == p / FISM_WAVES) {
#pragma unroll
        for (int i = 0; i < NI; ++i) t[i] = pr[sl][i];
      }
  } else {
    fism_load_row<NI>(t, P_item, lo);
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) s_pi[lo + i] = t[i];
}

// streamed sweep: this wavefront's streamed rows take their step in memory, all but position `skip` (no position: FISM_NO_SKIP)
constexpr uint32_t FISM_NO_SKIP = ~0u;
template <int NI, bool ADA>
__device__ __forceinline__ void fism_sweep_streamed(const HyperParams& hp, const uint32_t* row, uint32_t n, uint32_t res_rows, uint32_t w, uint32_t lo,
                                                    uint32_t skip, float* P, float* P_ag, const float (&q)[NI], float gs, float (&d)[NI]) {
  constexpr uint32_t KP = WAVE * NI;
  for (uint32_t qp = res_rows + w; qp < n; qp += FISM_WAVES) {
    if (qp == skip) continue;
    const uint32_t it = (uint32_t)__builtin_amdgcn_readfirstlane((int)row[qp]);
    float tw[NI], ta[NI];
    fism_load_row<NI>(tw, P + (size_t)it * KP, lo);
    fism_load_row<NI>(ta, P_ag + (size_t)it * KP, lo);
    fism_row_step<NI, ADA>(hp, tw, ta, q, gs, d);
    vstore<NI>(P + (size_t)it * KP + lo, tw);
    vstore<NI>(P_ag + (size_t)it * KP + lo, ta);
  }
}
// (The resident sweep, `for sl < R: if (qp < n_res && qp != skip) fism_row_step(pr[sl], pa[sl], ...)`, stays in each kernel body: behind a
// helper that takes pr / pa by reference the pair kernel spills to scratch; profiles/fism_frame_resources.txt.)

// visit store: the resident rows go back
template <int NI, int R>
__device__ __forceinline__ void fism_visit_store(const float (&pr)[R][NI], const float (&pa)[R][NI], const uint32_t* row, uint32_t n_res,
                                                 uint32_t w, uint32_t lo, float* P, float* P_ag) {
  constexpr uint32_t KP = WAVE * NI;
#pragma unroll
  for (int sl = 0; sl < R; ++sl) {
    const uint32_t qp = w + FISM_WAVES * (uint32_t)sl;
    if (qp < n_res) {
      const uint32_t it = (uint32_t)__builtin_amdgcn_readfirstlane((int)row[qp]);
      vstore<NI>(P + (size_t)it * KP + lo, pr[sl]);
      vstore<NI>(P_ag + (size_t)it * KP + lo, pa[sl]);
    }
  }
}

template <int NI, bool ADA>
__global__ void __launch_bounds__(FISM_WAVES * WAVE)
fism_user_kernel(HyperParams hp, uint32_t bias_term, uint32_t res_rows /* 0 or FISM_WAVES * fism_resident_slots(NI) */,
                 const int64_t* __restrict__ row_ptr, const uint32_t* __restrict__ col, uint64_t u0, uint32_t nb, uint64_t seed, uint32_t epoch,
                 const float* __restrict__ scale /* [num_items + 1] */, float* P, float* P_ag, float* Q, float* Q_ag, float* BI, float* BI_ag,
                 float* BU, float* BU_ag) {
  constexpr uint32_t W = FISM_WAVES;
  constexpr int R = (int)fism_resident_slots(NI);               // resident rows per wavefront
  constexpr uint32_t KP = WAVE * NI;
  __shared__ float s_pi[KP];                                   // P[i] of a rated instance, as it is at that instance
  __shared__ float s_d[2][W][KP];                              // per-wavefront column sums, two sets in turn (see `par`)
  const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  const uint32_t lane = threadIdx.x % WAVE, lo = lane * NI;
  const float neg_label = mf_negative_label(hp.loss_type);
  uint32_t par = 0;
  for (uint32_t slot = 0; slot < nb; ++slot) {
    const uint64_t uid = u0 + slot;
    const int64_t r0 = row_ptr[uid];
    const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(row_ptr[uid + 1] - r0));
    // A user without train items takes no step: no instance, bu[uid] and its accumulator keep their bits, and scale[n - 1] below does
    // not exist.  n is the same in every wavefront and no barrier of this visit has been reached, so all of them leave together.
    if (n == 0u) continue;
    const uint32_t* row = col + r0;
    const uint32_t n_res = min(n, res_rows);                   // positions [0, n_res) are resident
    const float s_pos = scale[n - 1u], s_neg = scale[n];
    const uint64_t key_n = cdae_rng_key(seed, epoch, uid + hp.uid_offset, CDAE_STREAM_NEGATIVE);
    float bu = 0.f, bua = 1.f;
    if (bias_term) { bu = BU[uid]; bua = BU_ag[uid]; }
    float pr[R][NI], pa[R][NI];
    // the visit's rows: resident ones into registers; x = their sum with the streamed ones'
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
      const uint32_t item_pos = (uint32_t)__builtin_amdgcn_readfirstlane((int)row[p]);
      uint32_t cand = 0;
      for (uint32_t k = 0; k <= hp.num_neg; ++k) {
        const bool rated = k == 0u;
        if (!rated && (k - 1u) % WAVE == 0u) {                   // the next 64 negatives of this positive, one per lane
          cand = 0;
          if (k - 1u + lane < hp.num_neg) cand = cdae_sample_negative(key_n, (uint64_t)p * hp.num_neg + (k - 1u + lane), row, n, hp.num_items);
        }
        const uint32_t item = rated ? item_pos : (uint32_t)__builtin_amdgcn_readlane((int)cand, (int)((k - 1u) % WAVE));
        const float s = rated ? s_pos : s_neg;
        const float label = rated ? 1.f : neg_label;
        if (rated) {                                           // the owner of P[i] publishes it
          fism_publish<NI, R>(s_pi, pr, p, n_res, w, lo, P + (size_t)item * KP);
          __syncthreads();
        }
        // every wavefront: Q[item], the prediction and g
        float q[NI], v[NI];
        fism_load_row<NI>(q, Q + (size_t)item * KP, lo);
        float bq = 0.f;
        if (bias_term) bq = load_f32_sc1(BI + item);
#pragma unroll
        for (int i = 0; i < NI; ++i) v[i] = rated ? x[i] - s_pi[lo + i] : x[i];      // fism.hpp:210-216
        float dot = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) dot = fmaf(v[i], q[i], dot);
        dot = wave_sum(dot);
        const float pred = fmaf(s, dot, bias_term ? bu + bq : 0.f);
        const float g = mf_loss_grad(hp.loss_type, pred, label);
        const float gs = g * s;
        // Every wavefront holds Q[item] and bi[item] from BEFORE this instance's step (pred has consumed both loads) before wavefront 0
        // may store the stepped values: the wavefronts do not leave the negative draws above at the same time, and without this
        // barrier a late one read what wavefront 0 had already written (a user with 35 of 40 items, whose draws take long)
        __builtin_amdgcn_s_waitcnt(WAIT_VM0);
        __syncthreads();
        // its rows (fism.hpp:140-149): Q[item] from before its own step
        const uint32_t skip = rated ? p : FISM_NO_SKIP;        // P[i] takes no step in its own rated instance
        float d[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) d[i] = 0.f;
#pragma unroll
        for (int sl = 0; sl < R; ++sl) {
          const uint32_t qp = w + W * (uint32_t)sl;
          if (qp < n_res && qp != skip) fism_row_step<NI, ADA>(hp, pr[sl], pa[sl], q, gs, d);
        }
        fism_sweep_streamed<NI, ADA>(hp, row, n, res_rows, w, lo, skip, P, P_ag, q, gs, d);
#pragma unroll
        for (int i = 0; i < NI; ++i) s_d[par][w][lo + i] = d[i];
        // wavefront 0: Q[item] on g s v + lambda Q[item] (fism.hpp:151-164), bi[item]; every wavefront: its copy of bu (:113-124)
        if (w == 0u) {
          float qa[NI], qn[NI];
          fism_load_row<NI>(qa, Q_ag + (size_t)item * KP, lo);
#pragma unroll
          for (int i = 0; i < NI; ++i) { qn[i] = q[i]; ada_step_t<ADA>(hp, qn[i], qa[i], fmaf(gs, v[i], hp.lambda * q[i])); }
          vstore<NI>(Q + (size_t)item * KP + lo, qn);
          vstore<NI>(Q_ag + (size_t)item * KP + lo, qa);
          if (bias_term && lane == 0u) {
            float b = bq, ba = load_f32_sc1(BI_ag + item);
            ada_step_t<ADA>(hp, b, ba, fmaf(hp.lambda, b, g));
            BI[item] = b; BI_ag[item] = ba;
          }
        }
        if (bias_term) ada_step_t<ADA>(hp, bu, bua, fmaf(hp.lambda, bu, g));
        __builtin_amdgcn_s_waitcnt(WAIT_VM0);                  // this instance's stores are in memory before anybody reads them again
        __syncthreads();
        float t[NI];
        fism_total<NI>(s_d[par], lo, t);
#pragma unroll
        for (int i = 0; i < NI; ++i) x[i] += t[i];             // fism.hpp:148, 165
        par ^= 1u;
      }
    }
    // the resident rows go back; the next visit reads them behind the barrier
    fism_visit_store<NI, R>(pr, pa, row, n_res, w, lo, P, P_ag);
    if (bias_term && w == 0u && lane == 0u) { BU[uid] = bu; BU_ag[uid] = bua; }
    __builtin_amdgcn_s_waitcnt(WAIT_VM0);
    __syncthreads();
  }
}

// serving: z of rows [c0, c0 + nu) of the CSR (ptr, col) into out[slot][Kp], a wavefront per row; rows of any length, eight loads in flight
constexpr int FISM_ENC_GROUP = 8;
template <int NI>
__global__ void __launch_bounds__(256)
fism_encode_rows_kernel(const int64_t* __restrict__ ptr, const uint32_t* __restrict__ col, uint64_t c0, uint32_t nu,
                        const float* __restrict__ scale /* [num_items + 1] */, const float* __restrict__ P, float* __restrict__ out) {
  constexpr uint32_t KP = WAVE * NI;
  const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE));
  const uint32_t lo = (threadIdx.x % WAVE) * NI;
  if (slot >= nu) return;
  const int64_t a = ptr[c0 + slot];
  const uint32_t n = (uint32_t)(ptr[c0 + slot + 1] - a);
  const uint32_t* row = col + a;
  float sum[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) sum[i] = 0.f;
  for (uint32_t j0 = 0; j0 < n; j0 += FISM_ENC_GROUP) {
    float t[FISM_ENC_GROUP][NI];
#pragma unroll
    for (int s = 0; s < FISM_ENC_GROUP; ++s) vload<NI>(t[s], P + (size_t)row[min(j0 + (uint32_t)s, n - 1u)] * KP + lo);   // past the end: the last row again (never used)
#pragma unroll
    for (int s = 0; s < FISM_ENC_GROUP; ++s)
      if (j0 + (uint32_t)s < n) {
#pragma unroll
        for (int i = 0; i < NI; ++i) sum[i] += t[s][i];
      }
  }
  const float sc = scale[n];                                   // scale[0] = 0: an empty rated set gives z = 0
#pragma unroll
  for (int i = 0; i < NI; ++i) sum[i] *= sc;
  vstore<NI>(out + (size_t)slot * KP + lo, sum);
}

}  // namespace cdae
