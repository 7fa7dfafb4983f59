// K7 on the matrix cores: top-k recommendation for many users at once (cdae.hpp:162-196, evaluation.hpp:135-145).
//
// scores[user][item] = z_user . D[item] + b'[item] is a [users x K] x [K x items] product — GEMM-shaped, unlike the
// sampled training path — so it runs on MFMA with fp32 operands (v_mfma_f32_32x32x2_f32, exact fp32 products and
// accumulation: ranking parity with the fp64 oracle needs more than bf16).  A 256-thread workgroup serves 128 users:
// wavefront w keeps the z rows of its 32 users in registers as the MFMA's B operand for the whole launch; the
// workgroup streams the decoder matrix through LDS in tiles of 32 items (double-buffered, rows padded to 8 NCH + 4
// floats so that the ds_read_b128 of 16 consecutive rows hit distinct banks) as the A operand.  After K / 2 MFMAs a
// lane holds 16 item scores of ONE user (C[item][user]: column = lane & 31), adds b', drops the user's training items
// (one bit per (user, item), built by rated_bits_kernel; a tile of 32 items is one 32-bit word) and keeps its own sorted
// top-16; the two lanes of a user merge through LDS at the end.  Ties resolve to the lower item id like the reference's
// heap walk over ascending ids.
//
// Contraction order: the K axis is cut into chunks of 8; lane half h = lane >> 5 owns elements 4h..4h+3 of every chunk,
// so both operands are plain float4 loads (A and B only have to agree on the order in which k is summed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cdae_kernels.hpp"

namespace cdae {

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int REC_TOPK_MAX = 16;       // per-lane list length; larger topk falls back to recommend_kernel
constexpr int REC_USERS_PER_BLOCK = 128;

// bits[(u - u0) * words + item / 32] = OR of 1 << (item % 32) over the training items of users [u0, u0 + nu).  No memset launch in front
// (round 5): the wavefront that owns a user's row of words builds it in LDS and writes every word once (item spaces up to 65 536: 8 KiB
// per wavefront); larger rows are cleared in global memory by their wavefront, which waits for its own stores (s_waitcnt: same-wave order
// is all that is needed — an agent-scope fence here wrote back the L2 under the training kernels of the other stream) before its atomics.
constexpr uint32_t RATED_LDS_WORDS = 2048;
__global__ void __launch_bounds__(256)
rated_bits_kernel(const int64_t* __restrict__ row_ptr, const uint32_t* __restrict__ col, uint64_t u0, uint32_t nu,
                  uint32_t words, uint32_t* __restrict__ bits) {
  __shared__ uint32_t lrow[4][RATED_LDS_WORDS];
  const uint32_t wid = threadIdx.x / WAVE;
  const uint32_t slot = blockIdx.x * (blockDim.x / WAVE) + wid;
  const uint32_t lane = threadIdx.x % WAVE;
  if (slot >= nu) return;
  const int64_t r0 = row_ptr[u0 + slot], r1 = row_ptr[u0 + slot + 1];
  uint32_t* out = bits + (size_t)slot * words;
  if (words <= RATED_LDS_WORDS) {
    uint32_t* w = lrow[wid];
    for (uint32_t i = lane; i < words; i += WAVE) w[i] = 0u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int64_t p = r0 + lane; p < r1; p += WAVE) {
      const uint32_t item = col[p];
      atomicOr(&w[item >> 5], 1u << (item & 31u));                 // LDS
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (uint32_t i = lane; i < words; i += WAVE) out[i] = w[i];
    return;
  }
  {                                                                // 16-byte stores over the aligned middle of the row, words at its ends
    const uint32_t head = min(words, (uint32_t)((16u - ((uintptr_t)out & 15u)) & 15u) / 4u), quads = (words - head) / 4u;
    for (uint32_t i = lane; i < head; i += WAVE) out[i] = 0u;
    uint4* o4 = reinterpret_cast<uint4*>(out + head);
    for (uint32_t i = lane; i < quads; i += WAVE) o4[i] = make_uint4(0u, 0u, 0u, 0u);
    for (uint32_t i = head + 4u * quads + lane; i < words; i += WAVE) out[i] = 0u;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  for (int64_t p = r0 + lane; p < r1; p += WAVE) {
    const uint32_t item = col[p];
    atomicOr(out + (item >> 5), 1u << (item & 31u));
  }
}

// ---- caller-supplied rated sets (cdae_hip_recommend_rows / cdae_hip_eval_topn_rows) ----------------------------------------------
// z of rows [r0, r0 + gridDim.x) of a device CSR that is NOT the handle's train set: get_hidden_values(uid, rated_set) with scale 1
// (cdae.hpp:169, :373-416), z = act(sum_{k in row} W[k] (.) Uu[uid] + b + Wu[uid]).  uids[row] names the user whose private rows the
// row takes — any user any number of times — or ROW_NO_USER: a Wu row of zeros that is still added and a Uu row of ones, i.e. the
// arithmetic of a real user with those rows.  empty_input: corruption_ratio == 1, the sum is over nothing (cdae.hpp:168-172).
//
// Summation order (part of the contract, include/cdae_hip.h): the one encode_partial_kernel + encode_finish_kernel give a train
// row at mode 0 — groups of hp.unit_pos consecutive items, each group summed from 0 in ascending item order, the group sums added
// from 0 in group order — so a row that equals a handle's train row has that handle's inference z bit for bit.  No unit table is
// needed: group g of a row is items [g unit_pos, (g + 1) unit_pos).
//
// Two launches share the rows of a chunk by length.  encode_rows_kernel gives every row of at most one group — the rows fold-in and
// sessions bring, 1 to some tens of items — a wavefront of its own, ENC_ROWS_WAVES rows to a workgroup, with no LDS and no barrier
// (a W row is one 256 NI-byte wave load, UN of them in flight per wavefront).  encode_rows_long_kernel gives every longer row a
// workgroup: its wavefronts take the groups of a round side by side, the sums meet in LDS and wavefront 0 adds them in group order
// before the next round.  Each kernel leaves the other's rows alone; the host launches the second only for a chunk that has a long
// row.  contract(off): h = s * uu + b must round the product as encode_finish_kernel's fmaf(s * uu, 1, b) does.
constexpr uint32_t ROW_NO_USER = 0xFFFFFFFFu;
constexpr int ENC_ROWS_WAVES = 4;

// one wavefront: ua = sum of the W rows of items[p_begin, p_end) (at most hp.unit_pos of them), from 0 in ascending position order
template <int NI>
__device__ __forceinline__ void enc_rows_group_sum(const HyperParams& hp, const float* __restrict__ W, const uint32_t* __restrict__ items,
                                                   uint32_t p_begin, uint32_t p_end, uint32_t lane, float (&ua)[NI]) {
#pragma clang fp contract(off)
  constexpr int UN = 8;
  const uint32_t lo = lane * NI;
#pragma unroll
  for (int i = 0; i < NI; ++i) ua[i] = 0.f;
  for (uint32_t q0 = p_begin; q0 < p_end; q0 += WAVE) {
    const uint32_t cnt = min((uint32_t)WAVE, p_end - q0);
    const uint32_t item = lane < cnt ? items[q0 + lane] : 0u;
    for (uint32_t j0 = 0; j0 < cnt; j0 += UN) {
      float v[UN][NI];
#pragma unroll
      for (int j = 0; j < UN; ++j) {
        if (j0 + j < cnt) {                                        // wave-uniform
          const uint32_t it = (uint32_t)__builtin_amdgcn_readlane((int)item, (int)(j0 + j));
          vload<NI>(v[j], W + (size_t)it * hp.Kp + lo);
        } else {
#pragma unroll
          for (int i = 0; i < NI; ++i) v[j][i] = 0.f;
        }
      }
#pragma unroll
      for (int j = 0; j < UN; ++j)
#pragma unroll
        for (int i = 0; i < NI; ++i) ua[i] += v[j][i];
    }
  }
}

// one wavefront: what the finish of a row needs — b, and the user's private rows (zeros / ones for a row without a user node).  A uid
// with ROW_GUEST set names a row of the handle's guest table (cdae_hip_set_guest_nodes, cdae_hip_fold_in_rows) when there is one
// (Gwu != nullptr; the host has checked the index): only the base pointer and the index change, so every uid without the bit loads
// what it always did.
constexpr uint32_t ROW_GUEST = 0x80000000u;
template <int NI>
__device__ __forceinline__ void enc_rows_user(const HyperParams& hp, uint32_t uid, const float* __restrict__ Wu, const float* __restrict__ Uu,
                                              const float* __restrict__ Gwu, const float* __restrict__ Guu,
                                              const float* __restrict__ b, uint32_t lane, float (&bb)[NI], float (&wu)[NI], float (&uu)[NI]) {
  const uint32_t lo = lane * NI;
#pragma unroll
  for (int i = 0; i < NI; ++i) { wu[i] = 0.f; uu[i] = 1.f; }
  vload<NI>(bb, b + lo);
  const bool guest = Gwu != nullptr && (uid & ROW_GUEST) != 0u;      // (wave-uniform)
  const size_t o = (size_t)(guest ? uid & ~ROW_GUEST : uid) * hp.Kp + lo;
  if (hp.user_factor && uid != ROW_NO_USER) vload<NI>(wu, (guest ? Gwu : Wu) + o);
  if (hp.linear_function && uid != ROW_NO_USER) vload<NI>(uu, (guest ? Guu : Uu) + o);
}

// one wavefront: z = act(acc (.) uu + b + wu) to zrow, pad elements 0
template <int NI>
__device__ __forceinline__ void enc_rows_finish(const HyperParams& hp, const float (&acc)[NI], const float (&bb)[NI], const float (&wu)[NI],
                                                const float (&uu)[NI], uint32_t lane, float* __restrict__ zrow) {
#pragma clang fp contract(off)
  const uint32_t lo = lane * NI;
  float z[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    float s = acc[i];
    if (hp.linear_function) s *= uu[i];                            // h1 = Uu[u] (.) h1   cdae.hpp:382-384
    float h = s + bb[i];
    if (hp.user_factor) h += wu[i];
    z[i] = lo + i < hp.K ? activate(hp, h) : 0.f;                  // pad elements of z must be 0
  }
  vstore<NI>(zrow + lo, z);
}

// rows of at most one group: a wavefront per row, grid = ceil(nu / ENC_ROWS_WAVES)
template <int NI>
__global__ void __launch_bounds__(ENC_ROWS_WAVES * WAVE)
encode_rows_kernel(HyperParams hp, const int64_t* __restrict__ row_ptr, const uint32_t* __restrict__ col,
                   const uint32_t* __restrict__ uids, uint64_t r0, uint32_t nu, uint32_t empty_input, const float* __restrict__ W,
                   const float* __restrict__ Wu, const float* __restrict__ Uu, const float* __restrict__ b,
                   float* __restrict__ Z /* [nu][Kp] */, const float* __restrict__ Gwu /* the guest table's rows, or nullptr */,
                   const float* __restrict__ Guu) {
#pragma clang fp contract(off)
  const uint32_t wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const uint32_t slot = blockIdx.x * ENC_ROWS_WAVES + wid;
  if (slot >= nu) return;                                          // (no barrier in this kernel)
  const uint64_t row = r0 + slot;
  const int64_t p0 = row_ptr[row];
  const uint32_t n = empty_input ? 0u : (uint32_t)(row_ptr[row + 1] - p0);
  if (n > hp.unit_pos) return;                                     // encode_rows_long_kernel's
  float bb[NI], wu[NI], uu[NI], acc[NI], ua[NI];
  enc_rows_user<NI>(hp, uids[row], Wu, Uu, Gwu, Guu, b, lane, bb, wu, uu);  // requested before the sum
#pragma unroll
  for (int i = 0; i < NI; ++i) acc[i] = 0.f;
  if (n) {
    enc_rows_group_sum<NI>(hp, W, col + p0, 0u, n, lane, ua);
#pragma unroll
    for (int i = 0; i < NI; ++i) acc[i] += ua[i];                  // group 0 added to 0, as for any row
  }
  enc_rows_finish<NI>(hp, acc, bb, wu, uu, lane, Z + (size_t)slot * hp.Kp);
}

// rows of several groups: a workgroup per row, grid = nu (a workgroup whose row is short leaves at once)
template <int NI>
__global__ void __launch_bounds__(ENC_ROWS_WAVES * WAVE)
encode_rows_long_kernel(HyperParams hp, const int64_t* __restrict__ row_ptr, const uint32_t* __restrict__ col,
                        const uint32_t* __restrict__ uids, uint64_t r0, uint32_t empty_input, const float* __restrict__ W,
                        const float* __restrict__ Wu, const float* __restrict__ Uu, const float* __restrict__ b,
                        float* __restrict__ Z /* [gridDim.x][Kp] */, const float* __restrict__ Gwu /* the guest table's rows, or nullptr */,
                        const float* __restrict__ Guu) {
#pragma clang fp contract(off)
  __shared__ float part[ENC_ROWS_WAVES][64 * NI];
  const uint32_t slot = blockIdx.x, wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const uint64_t row = r0 + slot;
  const int64_t p0 = row_ptr[row];
  const uint32_t n = empty_input ? 0u : (uint32_t)(row_ptr[row + 1] - p0);
  if (n <= hp.unit_pos) return;                                    // encode_rows_kernel's (workgroup-uniform, before any barrier)
  const uint32_t* items = col + p0;
  const uint32_t n_groups = (n + hp.unit_pos - 1u) / hp.unit_pos;
  const uint32_t lo = lane * NI;
  float bb[NI], wu[NI], uu[NI], acc[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) acc[i] = 0.f;
  if (wid == 0) enc_rows_user<NI>(hp, uids[row], Wu, Uu, Gwu, Guu, b, lane, bb, wu, uu);   // requested before the sums
  for (uint32_t g0 = 0; g0 < n_groups; g0 += ENC_ROWS_WAVES) {     // (workgroup-uniform trip count)
    const uint32_t g = g0 + wid;
    if (g < n_groups) {
      const uint32_t p_begin = g * hp.unit_pos;
      float ua[NI];
      enc_rows_group_sum<NI>(hp, W, items, p_begin, min(p_begin + hp.unit_pos, n), lane, ua);
#pragma unroll
      for (int i = 0; i < NI; ++i) part[wid][lo + i] = ua[i];
    }
    __syncthreads();
    if (wid == 0) {
      const uint32_t nw = min((uint32_t)ENC_ROWS_WAVES, n_groups - g0);
      for (uint32_t w = 0; w < nw; ++w)
#pragma unroll
        for (int i = 0; i < NI; ++i) acc[i] += part[w][lo + i];
    }
    __syncthreads();
  }
  if (wid != 0) return;
  enc_rows_finish<NI>(hp, acc, bb, wu, uu, lane, Z + (size_t)slot * hp.Kp);
}

// ---- scores and ranks of caller-supplied candidates (cdae_hip_score_rows: get_output_values, cdae.hpp:418-426) -------------------
// out[p] = D[cand[p]] . z_row + b'[cand[p]] for the candidates of a chunk.  A gather, not a GEMM: ~100 candidates out of thousands
// of items would leave the matrix-core path streaming 99 % of D for nothing.  Work unit: a TILE of up to SCORE_TILE consecutive
// candidates of one row, one wavefront per tile, SCORE_WAVES tiles to a workgroup, no LDS and no barrier (encode_rows_kernel's
// pattern).  The wavefront keeps z_row in NI registers per lane (lane l owns elements [l NI, (l + 1) NI), pad elements 0 by
// enc_rows_finish), takes the candidate ids one per lane and streams the candidates' D rows as whole-row wave loads, UN in flight.
//
// Contraction order (part of the contract, include/cdae_hip.h) — one per row stride, the same for every candidate wherever it sits:
//   lane l:      p = z[l NI] * D[l NI], then p = p + z[l NI + i] * D[l NI + i] for i = 1 .. NI - 1, every product and every sum
//                rounded on its own (contract(off): no fused multiply-add);
//   across lanes: wave_sum's tree — lanes 1 apart, 2 apart, the two quads of 8, the two eights of a row of 16, then row 0 + row 1
//                and row 2 + row 3, then the two halves;
//   then + b'[item], once.
// So the score of (row, item) is a function of z_row, D[item] and b'[item] alone.
//
// Tile table (built by the host while it validates the candidate CSR, uploaded with it): word x = slot of the row in the encoded
// chunk | (candidates in the tile - 1) << 16, word y = offset of the tile's first candidate from the chunk's first candidate.
constexpr uint32_t SCORE_TILE = 64;
constexpr int SCORE_WAVES = 4;

template <int NI>
__global__ void __launch_bounds__(SCORE_WAVES * WAVE)
score_rows_kernel(HyperParams hp, const uint2* __restrict__ tiles, uint32_t n_tiles, const uint32_t* __restrict__ cand /* the chunk's */,
                  const float* __restrict__ Z /* [rows of the chunk][Kp] */, const float* __restrict__ D, const float* __restrict__ bp,
                  float* __restrict__ out /* the chunk's */) {
#pragma clang fp contract(off)
  constexpr int UN = 8;
  const uint32_t wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const uint32_t t = blockIdx.x * SCORE_WAVES + wid;
  if (t >= n_tiles) return;                                        // (no barrier in this kernel)
  const uint2 tile = tiles[t];
  const uint32_t tx = (uint32_t)__builtin_amdgcn_readfirstlane((int)tile.x), off = (uint32_t)__builtin_amdgcn_readfirstlane((int)tile.y);
  const uint32_t slot = tx & 0xFFFFu, cnt = (tx >> 16) + 1u;
  const uint32_t lo = lane * NI;
  float z[NI];
  vload<NI>(z, Z + (size_t)slot * hp.Kp + lo);
  const uint32_t item = lane < cnt ? cand[off + lane] : 0u;
  const float bias = lane < cnt ? bp[item] : 0.f;                  // requested before the rows
  float s = 0.f;
  for (uint32_t j0 = 0; j0 < cnt; j0 += UN) {
    float v[UN][NI];
#pragma unroll
    for (int j = 0; j < UN; ++j)
      if (j0 + j < cnt) {                                          // wave-uniform
        const uint32_t it = (uint32_t)__builtin_amdgcn_readlane((int)item, (int)(j0 + j));
        vload<NI>(v[j], D + (size_t)it * hp.Kp + lo);
      }
#pragma unroll
    for (int j = 0; j < UN; ++j)
      if (j0 + j < cnt) {
        float p = z[0] * v[j][0];
#pragma unroll
        for (int i = 1; i < NI; ++i) p = p + z[i] * v[j][i];
        const float total = wave_sum(p);
        if (lane == j0 + j) s = total;
      }
  }
  if (lane < cnt) out[off + lane] = s + bias;                      // one coalesced store per tile
}

// ranks[p] = how many candidates of the same row precede p in cdae_hip_recommend_all's total order (a strictly greater score, or an
// equal score and a lower item id), from the very scores score_rows_kernel wrote.  Candidates ascend inside a row, so "a lower item
// id" is "an earlier position" and the ids are not needed.  One workgroup per row of [row0, row0 + gridDim.x); the row's scores in
// LDS (at most RANK_CANDIDATES_MAX of them: the host refuses longer rows before anything is launched).
constexpr uint32_t RANK_CANDIDATES_MAX = 4096;
__global__ void __launch_bounds__(256)
rank_rows_kernel(const int64_t* __restrict__ cand_ptr, uint64_t row0, int64_t p_chunk /* the chunk's first candidate */, int64_t n_chunk,
                 const float* __restrict__ scores /* the chunk's */, uint32_t* __restrict__ ranks /* the chunk's */) {
  __shared__ float sc[RANK_CANDIDATES_MAX];
  const uint64_t row = row0 + blockIdx.x;
  const int64_t p0 = cand_ptr[row];
  const uint32_t n = min((uint32_t)(cand_ptr[row + 1] - p0), RANK_CANDIDATES_MAX);
  if (n == 0 || p0 < p_chunk || p0 + n > p_chunk + n_chunk) return;   // (workgroup-uniform, before the barrier; a row outside the chunk is not this launch's)
  const float* mine = scores + (p0 - p_chunk);
  for (uint32_t i = threadIdx.x; i < n; i += 256) sc[i] = mine[i];
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n; i += 256) {
    const float si = sc[i];
    uint32_t before = 0;
    for (uint32_t q = 0; q < n; ++q) {
      const float sq = sc[q];
      before += (sq > si || (sq == si && q < i)) ? 1u : 0u;
    }
    ranks[(p0 - p_chunk) + i] = before;
  }
}

constexpr size_t recommend_mfma_lds_bytes(int nch) {
  const size_t tiles = 2 * 32 * (size_t)(8 * nch + 4) * sizeof(float), merge = 2 * 4 * 64 * (size_t)REC_TOPK_MAX * sizeof(float);
  return tiles > merge ? tiles : merge;
}

// SCORES (cdae_hip_recommend_rows with out_scores): the merge also writes the fp32 score of every listed item to out_score
// [nu x topk], -INFINITY in the sentinel places; the instantiations without it are the code cdae_hip_recommend_all has always launched.
template <int NCH, bool SCORES = false>
__global__ void __launch_bounds__(256)
recommend_mfma_kernel(HyperParams hp, const float* __restrict__ Z /* [nu x Kp] */, uint32_t nu,
                      const float* __restrict__ D, const float* __restrict__ bp,
                      const uint32_t* __restrict__ bits, uint32_t words, uint32_t topk, uint32_t* __restrict__ out,
                      float* __restrict__ out_score = nullptr) {
  constexpr int KC = 8 * NCH;                     // contraction length (>= K; pad columns are zero in Z and D)
  constexpr int ROW = KC + 4;                     // LDS row stride in floats
  constexpr int TILE = 32;
  extern __shared__ __attribute__((aligned(16))) char rec_smem[];   // max(2 tiles, merge scratch): see recommend_mfma_lds_bytes
  float (*tile)[TILE * ROW] = reinterpret_cast<float (*)[TILE * ROW]>(rec_smem);
  const uint32_t lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
  const uint32_t col_u = lane & 31u, half = lane >> 5;
  const uint32_t user = blockIdx.x * REC_USERS_PER_BLOCK + wave * 32u + col_u;
  const uint32_t user_ld = min(user, nu - 1u);

  // B operand: this lane's user, elements 8c + 4 half .. + 3 of every chunk
  float4 bz[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c)
    bz[c] = *reinterpret_cast<const float4*>(Z + (size_t)user_ld * hp.Kp + 8 * c + 4 * half);

  float tv[REC_TOPK_MAX];
  uint32_t ti[REC_TOPK_MAX];
#pragma unroll
  for (int j = 0; j < REC_TOPK_MAX; ++j) { tv[j] = -INFINITY; ti[j] = 0xFFFFFFFFu; }

  const uint32_t n_tiles = (hp.num_items + TILE - 1) / TILE;
  // cooperative tile load: TILE rows x (KC / 4) float4 = 8 NCH float4 per row; thread t takes float4 t, t + 256, ...
  constexpr int F4_PER_ROW = KC / 4;
  constexpr int F4_PER_TILE = TILE * F4_PER_ROW;
  constexpr int F4_PER_THREAD = (F4_PER_TILE + 255) / 256;
  float4 stage[F4_PER_THREAD];
  auto fetch = [&](uint32_t t) {
#pragma unroll
    for (int q = 0; q < F4_PER_THREAD; ++q) {
      const uint32_t f = threadIdx.x + 256u * q;
      const uint32_t r = f / F4_PER_ROW, c4 = f % F4_PER_ROW;
      const uint32_t item = min(t * TILE + r, hp.num_items - 1u);
      stage[q] = f < (uint32_t)F4_PER_TILE ? *reinterpret_cast<const float4*>(D + (size_t)item * hp.Kp + 4 * c4)
                                           : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int q = 0; q < F4_PER_THREAD; ++q) {
      const uint32_t f = threadIdx.x + 256u * q;
      const uint32_t r = f / F4_PER_ROW, c4 = f % F4_PER_ROW;
      if (f < (uint32_t)F4_PER_TILE) *reinterpret_cast<float4*>(&tile[buf][r * ROW + 4 * c4]) = stage[q];
    }
  };
  fetch(0);
  commit(0);
  __syncthreads();

  for (uint32_t t = 0; t < n_tiles; ++t) {
    const int buf = (int)(t & 1u);
    if (t + 1 < n_tiles) fetch(t + 1);                              // global loads of the next tile fly under the MFMAs
    const uint32_t word = bits[(size_t)user_ld * words + t];        // this user's training items among the tile's 32
    floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* arow = &tile[buf][col_u * ROW + 4 * half];         // A operand: item row (lane & 31) of the tile
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const float4 a = *reinterpret_cast<const float4*>(arow + 8 * c);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bz[c].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bz[c].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bz[c].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bz[c].w, acc, 0, 0, 0);
    }
    // C[item][user]: lane holds items 8 (r / 4) + 4 half + (r % 4), r = 0..15, of user column lane & 31
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t i0 = t * TILE + 8u * q + 4u * half;
      const float4 b4 = i0 + 3u < hp.num_items ? *reinterpret_cast<const float4*>(bp + i0)
                                                : make_float4(i0 < hp.num_items ? bp[i0] : 0.f, i0 + 1u < hp.num_items ? bp[i0 + 1u] : 0.f,
                                                              i0 + 2u < hp.num_items ? bp[i0 + 2u] : 0.f, 0.f);
      const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t item = i0 + (uint32_t)e;
        const float s = acc[4 * q + e] + bb[e];
        const bool ok = item < hp.num_items && !((word >> (8u * q + 4u * half + (uint32_t)e)) & 1u);
        if (ok && s > tv[REC_TOPK_MAX - 1]) {                       // strict: an equal score keeps the earlier (lower) id
          tv[REC_TOPK_MAX - 1] = s; ti[REC_TOPK_MAX - 1] = item;
#pragma unroll
          for (int j = REC_TOPK_MAX - 1; j >= 1; --j) {
            const bool up = tv[j] > tv[j - 1];
            const float fv = tv[j]; const uint32_t fi = ti[j];
            tv[j] = up ? tv[j - 1] : fv; ti[j] = up ? ti[j - 1] : fi;
            tv[j - 1] = up ? fv : tv[j - 1]; ti[j - 1] = up ? fi : ti[j - 1];
          }
        }
      }
    }
    if (t + 1 < n_tiles) commit(buf ^ 1);
    __syncthreads();
  }

  // merge the two lanes of every user (lists are sorted by score desc, id asc within a lane)
  float* mv = &tile[0][0];                                           // [4 waves][64 lanes][16] scores, then ids
  uint32_t* mi = reinterpret_cast<uint32_t*>(mv + 4 * 64 * REC_TOPK_MAX);
#pragma unroll
  for (int j = 0; j < REC_TOPK_MAX; ++j) {
    mv[(wave * 64 + lane) * REC_TOPK_MAX + j] = tv[j];
    mi[(wave * 64 + lane) * REC_TOPK_MAX + j] = ti[j];
  }
  __syncthreads();
  if (half == 0 && user < nu) {
    const float* va = mv + (wave * 64 + lane) * REC_TOPK_MAX;
    const float* vb = mv + (wave * 64 + lane + 32) * REC_TOPK_MAX;
    const uint32_t* ia = mi + (wave * 64 + lane) * REC_TOPK_MAX;
    const uint32_t* ib = mi + (wave * 64 + lane + 32) * REC_TOPK_MAX;
    uint32_t pa = 0, pb = 0;
    for (uint32_t j = 0; j < topk; ++j) {
      const float a = pa < (uint32_t)REC_TOPK_MAX ? va[pa] : -INFINITY, b = pb < (uint32_t)REC_TOPK_MAX ? vb[pb] : -INFINITY;
      const uint32_t xa = pa < (uint32_t)REC_TOPK_MAX ? ia[pa] : 0xFFFFFFFFu, xb = pb < (uint32_t)REC_TOPK_MAX ? ib[pb] : 0xFFFFFFFFu;
      const bool take_a = a > b || (a == b && xa <= xb);
      out[(size_t)user * topk + j] = take_a ? xa : xb;
      if constexpr (SCORES) out_score[(size_t)user * topk + j] = take_a ? a : b;
      if (take_a) ++pa; else ++pb;
    }
  }
}

// ---- TOPN metrics on the device (TOPN_Evaluation::evaluate evaluation.hpp:113-181, evaluate_rec_list :183-219) ------------------
// The reference scores each user's top-10 list against the user's test items on num_thread host threads and averages the eight
// columns P@1 P@5 P@10 R@1 R@5 R@10 MAP@5 MAP@10 over the users that have test items (:160-166).  Here the lists never leave the
// device: topn_user_kernel turns the list of one user (a thread each) into that user's eight fp64 terms r[c] / n_test_users —
// the same expressions in the same order as evaluate_rec_list, membership by binary search in the sorted test row — and
// topn_sum_kernel adds the terms of all users IN USER ORDER, one lane per column, so that the eight means carry the bits of the
// reference's sequential `rets[c] += r[c] / n` loop (users without test items contribute +0.0, which changes no bit of a
// non-negative sum).  The integer hit counts at 1 / 5 / 10 are summed with atomics (order-free).
__global__ void __launch_bounds__(256)
topn_user_kernel(const uint32_t* __restrict__ rec, uint32_t topk, uint64_t u0, uint32_t nu, const int64_t* __restrict__ test_ptr,
                 const uint32_t* __restrict__ test_col, double n_test_users, double* __restrict__ per_user,
                 unsigned long long* __restrict__ hits) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= nu) return;
  const uint64_t u = u0 + slot;
  const int64_t t0 = test_ptr[u], t1 = test_ptr[u + 1];
  double r[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
  if (t1 > t0) {
    const double nt = (double)(t1 - t0);
    const uint32_t top = topk < 20u ? topk : 20u;                       // evaluation.hpp:186,191
    double hit = 0., map5 = 0., map10 = 0.;
    uint32_t h1 = 0, h5 = 0, h10 = 0;
    for (uint32_t i = 0; i < top; ++i) {
      const uint32_t item = rec[(size_t)slot * topk + i];
      int64_t lo = t0, hi = t1;                                         // first position with test_col >= item
      while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (test_col[mid] < item) lo = mid + 1; else hi = mid; }
      if (lo < t1 && test_col[lo] == item) {
        hit += 1.;
        if (i < 5) map5 += hit / (double)(i + 1);
        if (i < 10) map10 += hit / (double)(i + 1);
        h1 += i < 1; h5 += i < 5; h10 += i < 10;
      }
      if (i == 0) { r[0] = hit; r[3] = hit / nt; }
      else if (i == 4) { r[1] = hit / 5.; r[4] = hit / nt; }
      else if (i == 9) { r[2] = hit / 10.; r[5] = hit / nt; }
    }
    r[6] = map5 / (nt < 5. ? nt : 5.);
    r[7] = map10 / (nt < 10. ? nt : 10.);
    if (h1) atomicAdd(hits + 0, (unsigned long long)h1);
    if (h5) atomicAdd(hits + 1, (unsigned long long)h5);
    if (h10) atomicAdd(hits + 2, (unsigned long long)h10);
#pragma unroll
    for (int c = 0; c < 8; ++c) r[c] = r[c] / n_test_users;             // evaluation.hpp:162-166 divides per user, then adds
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) per_user[u * 8 + c] = r[c];
}

// out[c] = ((per_user[0][c] + per_user[1][c]) + per_user[2][c]) + ...  — one wavefront, lane c < 8 owns column c; 16 users'
// terms are requested ahead of the dependent chain of fp64 adds
__global__ void __launch_bounds__(64)
topn_sum_kernel(const double* __restrict__ per_user, uint64_t num_users, double* __restrict__ out) {
  const uint32_t c = threadIdx.x;
  if (c >= 8) return;
  double acc = 0.;
  uint64_t u = 0;
  for (; u + 16 <= num_users; u += 16) {
    double v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = per_user[(u + j) * 8 + c];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc += v[j];
  }
  for (; u < num_users; ++u) acc += per_user[u * 8 + c];
  out[c] = acc;
}

// ---- exact full-catalogue ranks of named items (cdae_hip_full_rank_rows) -----------------------------------------------------------
// Where does a held-out item stand in a row's WHOLE list?  rank = the number of items outside the row's rated set that precede the
// target in cdae_hip_recommend_all's total order (a strictly greater score, or an equal score and a lower item id).  The kernels below
// COUNT where recommend_mfma_kernel / recommend_kernel keep a list, over the very same scores: two sweeps of the catalogue, the first
// to learn the targets' scores, the second to count against them, both by the sweep arithmetic of the top-k kernel of the same
// num_dim — so a target that recommend_rows lists at place j has rank j and the listed score, bit for bit.
//
// Matrix-core path (num_dim <= 256): full_rank_mfma_kernel<NCH, PASS> has recommend_mfma_kernel's shape — 256 threads and 128 columns
// per workgroup, z of the column in bz[NCH], the decoder double-buffered through LDS in 32-item tiles with the 8 NCH + 4 row stride,
// the same acc layout, the same b' float4 epilogue.  The tile loop, the MFMA chain and the epilogue are recommend_mfma_kernel's, copied
// unchanged (that kernel is not edited, and nothing here emulates the chain in scalar code).
//   PASS 0, target scores: a column is a row of the chunk.  A second bit table (rated_bits_kernel over the target CSR) tells the lane
//     which of its 16 scores of a tile belong to targets; each such score goes to tscore[p], p found by a binary search in the row's
//     target list (rare: once per target).  Targets are never rated (the host refuses such a call), so the rated bits are not read.
//   PASS 1, counting: a column is a VIRTUAL row — a row's z slot and rated-bits row plus a window of at most FR_WINDOW of its targets
//     (table built by the host: x = slot | (targets in the window - 1) << 16, y = offset of the window's first target from the chunk's
//     first target).  A row with n targets is ceil(n / 16) virtual rows: there is no cap on targets.  A lane keeps the window as 16
//     64-bit keys and 16 counters in registers.  key(s, item) = ordered(s) << 32 | ~item, ordered() the usual monotone map of fp32 to
//     uint32 after s + 0.0f has turned -0 into +0: key(a) > key(b) exactly when a precedes b in the total order, so one 64-bit compare
//     per (score, target) replaces (s > ts) | (s == ts & item < tid), and the target itself compares equal and adds nothing.  A masked
//     or out-of-range item has key 0, the unused places of the last window the largest key: neither counts anything.  (NaN scores are
//     unordered in the contract; here they sort by their bits.)  The two lane halves of a column add their counters through LDS at the
//     end; lane half 0 stores the window's ranks.
// LDS: at most recommend_mfma_lds_bytes (the counter scratch is 16 KiB).
constexpr int FR_WINDOW = 16;
static_assert(FR_WINDOW == REC_TOPK_MAX, "the counter scratch is laid out like the top-k merge scratch");

__device__ __forceinline__ uint32_t fr_ordered(float s) {
  const uint32_t b = __float_as_uint(s + 0.0f);
  return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ uint64_t fr_key(float s, uint32_t item) { return (uint64_t)fr_ordered(s) << 32 | (uint64_t)(~item); }

template <int NCH, int PASS>
__global__ void __launch_bounds__(256)
full_rank_mfma_kernel(HyperParams hp, const float* __restrict__ Z /* [rows of the chunk x Kp] */, uint32_t ncol,
                      const uint2* __restrict__ vrows /* PASS 1: the launch's virtual rows */, const float* __restrict__ D,
                      const float* __restrict__ bp, const uint32_t* __restrict__ bits /* PASS 0: target bits; PASS 1: rated bits */,
                      uint32_t words, const int64_t* __restrict__ tptr /* PASS 0: target row_ptr of the call */, uint64_t row0,
                      int64_t p0 /* PASS 0: the chunk's first target */, const uint32_t* __restrict__ tcol /* the chunk's */,
                      float* __restrict__ tscore /* the chunk's */, uint32_t* __restrict__ ranks /* PASS 1: the chunk's */) {
  constexpr int KC = 8 * NCH;                     // contraction length (>= K; pad columns are zero in Z and D)
  constexpr int ROW = KC + 4;                     // LDS row stride in floats
  constexpr int TILE = 32;
  extern __shared__ __attribute__((aligned(16))) char rec_smem[];   // max(2 tiles, counter scratch): recommend_mfma_lds_bytes
  float (*tile)[TILE * ROW] = reinterpret_cast<float (*)[TILE * ROW]>(rec_smem);
  const uint32_t lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
  const uint32_t col_u = lane & 31u, half = lane >> 5;
  const uint32_t column = blockIdx.x * REC_USERS_PER_BLOCK + wave * 32u + col_u;
  const uint32_t column_ld = min(column, ncol - 1u);

  uint32_t user_ld = column_ld;                   // the row's slot in Z and in the bit table
  uint32_t win_n = 0, win_off = 0;
  int64_t ta = 0, tb = 0;                         // PASS 0: the row's targets, positions in the chunk's
  uint64_t tkey[FR_WINDOW];
  uint32_t cnt[FR_WINDOW];
  if constexpr (PASS == 1) {
    const uint2 vr = vrows[column_ld];
    user_ld = vr.x & 0xFFFFu; win_n = (vr.x >> 16) + 1u; win_off = vr.y;
#pragma unroll
    for (int j = 0; j < FR_WINDOW; ++j) {
      const bool in = (uint32_t)j < win_n;
      const uint32_t at = win_off + (in ? (uint32_t)j : 0u);
      tkey[j] = in ? fr_key(tscore[at], tcol[at]) : ~0ull;
      cnt[j] = 0u;
    }
  } else {
    ta = tptr[row0 + column_ld] - p0; tb = tptr[row0 + column_ld + 1] - p0;
  }

  // B operand: this lane's row, elements 8c + 4 half .. + 3 of every chunk
  float4 bz[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c)
    bz[c] = *reinterpret_cast<const float4*>(Z + (size_t)user_ld * hp.Kp + 8 * c + 4 * half);

  const uint32_t n_tiles = (hp.num_items + TILE - 1) / TILE;
  // cooperative tile load: TILE rows x (KC / 4) float4 = 8 NCH float4 per row; thread t takes float4 t, t + 256, ...
  constexpr int F4_PER_ROW = KC / 4;
  constexpr int F4_PER_TILE = TILE * F4_PER_ROW;
  constexpr int F4_PER_THREAD = (F4_PER_TILE + 255) / 256;
  float4 stage[F4_PER_THREAD];
  auto fetch = [&](uint32_t t) {
#pragma unroll
    for (int q = 0; q < F4_PER_THREAD; ++q) {
      const uint32_t f = threadIdx.x + 256u * q;
      const uint32_t r = f / F4_PER_ROW, c4 = f % F4_PER_ROW;
      const uint32_t item = min(t * TILE + r, hp.num_items - 1u);
      stage[q] = f < (uint32_t)F4_PER_TILE ? *reinterpret_cast<const float4*>(D + (size_t)item * hp.Kp + 4 * c4)
                                           : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int q = 0; q < F4_PER_THREAD; ++q) {
      const uint32_t f = threadIdx.x + 256u * q;
      const uint32_t r = f / F4_PER_ROW, c4 = f % F4_PER_ROW;
      if (f < (uint32_t)F4_PER_TILE) *reinterpret_cast<float4*>(&tile[buf][r * ROW + 4 * c4]) = stage[q];
    }
  };
  fetch(0);
  commit(0);
  __syncthreads();

  for (uint32_t t = 0; t < n_tiles; ++t) {
    const int buf = (int)(t & 1u);
    if (t + 1 < n_tiles) fetch(t + 1);                              // global loads of the next tile fly under the MFMAs
    const uint32_t word = bits[(size_t)user_ld * words + t];        // PASS 0: the row's targets, PASS 1: its rated items, among the tile's 32
    floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* arow = &tile[buf][col_u * ROW + 4 * half];         // A operand: item row (lane & 31) of the tile
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const float4 a = *reinterpret_cast<const float4*>(arow + 8 * c);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bz[c].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bz[c].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bz[c].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bz[c].w, acc, 0, 0, 0);
    }
    // C[item][column]: lane holds items 8 (r / 4) + 4 half + (r % 4), r = 0..15, of column lane & 31
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t i0 = t * TILE + 8u * q + 4u * half;
      const float4 b4 = i0 + 3u < hp.num_items ? *reinterpret_cast<const float4*>(bp + i0)
                                                : make_float4(i0 < hp.num_items ? bp[i0] : 0.f, i0 + 1u < hp.num_items ? bp[i0 + 1u] : 0.f,
                                                              i0 + 2u < hp.num_items ? bp[i0 + 2u] : 0.f, 0.f);
      const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t item = i0 + (uint32_t)e;
        const float s = acc[4 * q + e] + bb[e];
        const bool bit = (word >> (8u * q + 4u * half + (uint32_t)e)) & 1u;
        if constexpr (PASS == 0) {
          if (bit && column < ncol) {                               // (a set bit is an item below num_items)
            int64_t lo = ta, hi = tb;                               // first position with tcol >= item: the target itself
            while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (tcol[mid] < item) lo = mid + 1; else hi = mid; }
            if (lo < tb) tscore[lo] = s;
          }
        } else {
          const uint64_t key = item < hp.num_items && !bit ? fr_key(s, item) : 0ull;
#pragma unroll
          for (int j = 0; j < FR_WINDOW; ++j) cnt[j] += key > tkey[j] ? 1u : 0u;
          if (e & 1) {                                               // pin the counters every two items: left alone, the compiler gathers
            asm volatile("" : "+v"(cnt[0]), "+v"(cnt[1]), "+v"(cnt[2]), "+v"(cnt[3]), "+v"(cnt[4]), "+v"(cnt[5]), "+v"(cnt[6]), "+v"(cnt[7]));
            asm volatile("" : "+v"(cnt[8]), "+v"(cnt[9]), "+v"(cnt[10]), "+v"(cnt[11]), "+v"(cnt[12]), "+v"(cnt[13]), "+v"(cnt[14]), "+v"(cnt[15]));
          }                                                          // the tile's 256 compare masks first and spills SGPRs by the hundred
        }
      }
    }
    if (t + 1 < n_tiles) commit(buf ^ 1);
    __syncthreads();
  }

  if constexpr (PASS == 1) {
    // add the counters of the two lanes of every column
    uint32_t* mc = reinterpret_cast<uint32_t*>(rec_smem);            // [4 waves][64 lanes][16]
#pragma unroll
    for (int j = 0; j < FR_WINDOW; ++j) mc[(wave * 64 + lane) * FR_WINDOW + j] = cnt[j];
    __syncthreads();
    if (half == 0 && column < ncol) {
      const uint32_t* ca = mc + (wave * 64 + lane) * FR_WINDOW;
      const uint32_t* cb = mc + (wave * 64 + lane + 32) * FR_WINDOW;
      for (uint32_t j = 0; j < win_n; ++j) ranks[win_off + j] = ca[j] + cb[j];
    }
  }
}

// General path (num_dim > 256): recommend_kernel's front half — one workgroup per row of [r0, r0 + gridDim.x), the scores of all items
// (fmaf chain over the lane's NI elements, wave_sum, + b') to LDS or to the row's workspace row, rated items set to -INFINITY — then
// each wavefront takes targets of the row in turn: the target's own score is read from the array, the lanes stride over the array
// counting its predecessors, and the counts are combined with __shfl_xor.  A row without targets leaves at once.
template <int NI>
__global__ void __launch_bounds__(256)
full_rank_general_kernel(HyperParams hp, const int64_t* __restrict__ row_ptr, const uint32_t* __restrict__ col,
                         const int64_t* __restrict__ tptr, const uint32_t* __restrict__ tcol /* the call's */, uint64_t r0,
                         int64_t p0 /* the chunk's first target */, const float* __restrict__ Z, const float* __restrict__ D,
                         const float* __restrict__ bp, float* __restrict__ score_ws /* [gridDim.x][num_items] or nullptr */,
                         float* __restrict__ tscore /* the chunk's */, uint32_t* __restrict__ ranks /* the chunk's */) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const uint32_t slot = blockIdx.x;
  float* score = score_ws ? score_ws + (size_t)slot * hp.num_items : reinterpret_cast<float*>(smem_raw + 64);
  const uint64_t row = r0 + slot;
  const int64_t ta = tptr[row], tb = tptr[row + 1];
  if (ta == tb) return;                                            // (workgroup-uniform, before any barrier)
  const uint32_t lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE, nw = blockDim.x / WAVE;
  const uint32_t lo = lane * NI;
  float z[NI];
  vload<NI>(z, Z + (size_t)slot * hp.Kp + lo);
  for (uint32_t item = wid; item < hp.num_items; item += nw) {
    float d[NI];
    vload<NI>(d, D + (size_t)item * hp.Kp + lo);
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < NI; ++i) dot = fmaf(d[i], z[i], dot);
    const float y = wave_sum(dot) + bp[item];
    if (lane == 0) score[item] = y;
  }
  __syncthreads();
  {
    const int64_t a = row_ptr[row];
    const uint32_t n = (uint32_t)(row_ptr[row + 1] - a);
    for (uint32_t p = threadIdx.x; p < n; p += blockDim.x) score[col[a + p]] = -INFINITY;   // cdae.hpp:177-179
  }
  __syncthreads();
  for (int64_t p = ta + wid; p < tb; p += nw) {                     // (wave-uniform)
    const uint32_t tid = tcol[p];
    const float ts = score[tid];
    uint32_t before = 0;
    for (uint32_t item = lane; item < hp.num_items; item += WAVE) {
      const float v = score[item];
      before += (v > ts || (v == ts && item < tid)) ? 1u : 0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off, WAVE);
    if (lane == 0) { ranks[p - p0] = before; tscore[p - p0] = ts; }
  }
}

// ---- filtered top-k (cdae_hip_recommend_rows_filtered): an item allow list for the call, per-row exclusions that are no inputs --------
// The top-k kernels take the exclusion as data and do not care where a decoder row sits in memory: the score of (row, item) is a
// function of z, D[item] and b'[item] only.  So a filter is served exactly.  filter_bits_kernel is the ONE place where the filter is
// interpreted: it writes the chunk's exclusion table in the index space the sweep runs in, and recommend_mfma_kernel and
// recommend_kernel<NI, true> both mask from that table.  With an allow list the sweep runs over a packed copy of the allowed decoder
// rows (pack_decoder_kernel, once per call) with num_items := n_allow: ascending places in the pack are ascending item ids, so the tie
// rule survives, and remap_ids_kernel turns the places of the lists back into item ids.
//
// filter_bits_kernel: bits[(r - r0) * words + x / 32] |= 1 << (x % 32) for every item of row r of up to two CSRs (the rated rows when
// the call excludes them, the excl rows when it has any; a null row_ptr leaves a CSR out), x = the item, or pos[item] when there is an
// allow list (0xFFFFFFFF: the item is not allowed, so it is no candidate anyway and is skipped).  rated_bits_kernel's two forms and
// its reasons: one wavefront per row, no memset launch in front, the row of words built in LDS and written once when it fits, else
// cleared in global memory by its own wavefront, which waits for its own stores (s_waitcnt: same-wave order is all that is needed; no
// agent-scope fence, which would write back the L2 under whatever the other streams run) before its atomics.
// one wavefront: the items of row `row` of up to two CSRs, mapped through pos, ORed into the row of words w (LDS or global memory:
// inlined into either form, so each keeps the atomics of its own address space)
__device__ __forceinline__ void filter_mark(const int64_t* __restrict__ rated_ptr, const uint32_t* __restrict__ rated_col,
                                            const int64_t* __restrict__ excl_ptr, const uint32_t* __restrict__ excl_col,
                                            const uint32_t* __restrict__ pos, uint64_t row, uint32_t lane, uint32_t* w) {
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int64_t* ptr = c ? excl_ptr : rated_ptr;
    const uint32_t* col = c ? excl_col : rated_col;
    if (!ptr) continue;                                            // (uniform over the launch)
    const int64_t a = ptr[row], b = ptr[row + 1];
    for (int64_t p = a + lane; p < b; p += WAVE) {
      uint32_t x = col[p];
      if (pos) x = pos[x];
      if (x != 0xFFFFFFFFu) atomicOr(&w[x >> 5], 1u << (x & 31u));
    }
  }
}
__global__ void __launch_bounds__(256)
filter_bits_kernel(const int64_t* __restrict__ rated_ptr, const uint32_t* __restrict__ rated_col, const int64_t* __restrict__ excl_ptr,
                   const uint32_t* __restrict__ excl_col, const uint32_t* __restrict__ pos, uint64_t r0, uint32_t nu, uint32_t words,
                   uint32_t* __restrict__ bits) {
  __shared__ uint32_t lrow[4][RATED_LDS_WORDS];
  const uint32_t wid = threadIdx.x / WAVE;
  const uint32_t slot = blockIdx.x * (blockDim.x / WAVE) + wid;
  const uint32_t lane = threadIdx.x % WAVE;
  if (slot >= nu) return;                                          // (no workgroup barrier in this kernel)
  uint32_t* out = bits + (size_t)slot * words;
  if (words <= RATED_LDS_WORDS) {
    uint32_t* w = lrow[wid];
    for (uint32_t i = lane; i < words; i += WAVE) w[i] = 0u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    filter_mark(rated_ptr, rated_col, excl_ptr, excl_col, pos, r0 + slot, lane, w);          // LDS
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (uint32_t i = lane; i < words; i += WAVE) out[i] = w[i];
    return;
  }
  {                                                                // 16-byte stores over the aligned middle of the row, words at its ends
    const uint32_t head = min(words, (uint32_t)((16u - ((uintptr_t)out & 15u)) & 15u) / 4u), quads = (words - head) / 4u;
    for (uint32_t i = lane; i < head; i += WAVE) out[i] = 0u;
    uint4* o4 = reinterpret_cast<uint4*>(out + head);
    for (uint32_t i = lane; i < quads; i += WAVE) o4[i] = make_uint4(0u, 0u, 0u, 0u);
    for (uint32_t i = head + 4u * quads + lane; i < words; i += WAVE) out[i] = 0u;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  filter_mark(rated_ptr, rated_col, excl_ptr, excl_col, pos, r0 + slot, lane, out);
}

// pos[allow[p]] = p over a 0xFF fill of pos[num_items] (hipMemsetAsync in front): item -> place in the allow list
__global__ void __launch_bounds__(256)
allow_pos_kernel(const uint32_t* __restrict__ allow, uint32_t n_allow, uint32_t* __restrict__ pos) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n_allow) pos[allow[p]] = p;
}

// Dp[p] = D[allow[p]] (whole rows of Kp floats, pad elements included: a wave load and a wave store per row, a wavefront per row,
// PACK_WAVES rows to a workgroup, no LDS and no barrier) and bpp[p] = b'[allow[p]].
constexpr int PACK_WAVES = 4;
template <int NI>
__global__ void __launch_bounds__(PACK_WAVES * WAVE)
pack_decoder_kernel(const uint32_t* __restrict__ allow, uint32_t n_allow, uint32_t Kp, const float* __restrict__ D,
                    const float* __restrict__ bp, float* __restrict__ Dp, float* __restrict__ bpp) {
  const uint32_t wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const uint32_t p = blockIdx.x * PACK_WAVES + wid;
  if (p >= n_allow) return;
  const uint32_t item = allow[p];
  float v[NI];
  vload<NI>(v, D + (size_t)item * Kp + lane * NI);
  vstore<NI>(Dp + (size_t)p * Kp + lane * NI, v);
  if (lane == 0) bpp[p] = bp[item];
}

// ---- similar items (cdae_hip_similar_items): top-k item neighbours by dot or cosine ---------------------------------------------------
// The sweeps above take the table, the hidden rows and the mask as data, so "the items nearest to item q" is a sweep whose hidden row is
// a row of the item table itself: z := T[q] (DOT) or T[q] / |T[q]| (COSINE) over the rows T[i] or T[i] / |T[i]|, a bias of +0.0.
// gather_rows_kernel makes both operands and is the only arithmetic the entry point adds:
//   out[p] = T[ids[p]] (ids == nullptr: T[p]), whole rows of Kp floats, a wavefront per row as in pack_decoder_kernel; under COSINE the
//   row divided by its norm, in the one order include/cdae_hip.h states: lane l adds the squares of its NI elements in ascending order
//   in fp64, the 64 partials are added by six __shfl_xor steps of distance 1, 2, 4, 8, 16, 32 (fp64 addition commutes, so every lane
//   holds the bits of the balanced tree over neighbouring lanes), n = (float)sqrt(ss) and x / n are correctly rounded, and a row with
//   ss == 0 becomes +0.0 everywhere.  (The square of an fp32 value is exact in fp64, so a contraction of the multiply and the add into
//   one fma changes no bit.)  A row's image depends on that row alone: a query's row and its place in the table image are the same bits.
template <int NI, bool COSINE>
__global__ void __launch_bounds__(PACK_WAVES * WAVE)
gather_rows_kernel(const uint32_t* __restrict__ ids, uint32_t n, uint32_t Kp, const float* __restrict__ T, float* __restrict__ out) {
  const uint32_t wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const uint32_t p = blockIdx.x * PACK_WAVES + wid;
  if (p >= n) return;                                              // (wavefront-uniform, no barrier in this kernel)
  const uint32_t row = ids ? ids[p] : p;
  float v[NI];
  vload<NI>(v, T + (size_t)row * Kp + lane * NI);
  if constexpr (COSINE) {
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < NI; ++i) ss = ss + (double)v[i] * (double)v[i];
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) ss = ss + __shfl_xor(ss, off, WAVE);
    const float norm = (float)__dsqrt_rn(ss);
#pragma unroll
    for (int i = 0; i < NI; ++i) v[i] = ss == 0.0 ? 0.f : __fdiv_rn(v[i], norm);
  }
  vstore<NI>(out + (size_t)p * Kp + lane * NI, v);
}

// ptr[i] = i over [n]: with the queries as its columns, the CSR whose row r holds query r alone (exclude_self through filter_bits_kernel)
__global__ void __launch_bounds__(256)
iota_ptr_kernel(size_t n, int64_t* __restrict__ ptr) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) ptr[i] = (int64_t)i;
}

// ids[i] = allow[ids[i]] over the [n] places of a chunk's lists; the sentinel stays the sentinel
__global__ void __launch_bounds__(256)
remap_ids_kernel(const uint32_t* __restrict__ allow, size_t n, uint32_t* __restrict__ ids) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = ids[i];
  if (p != 0xFFFFFFFFu) ids[i] = allow[p];
}

}  // namespace cdae
