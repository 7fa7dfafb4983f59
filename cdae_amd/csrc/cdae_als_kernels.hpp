// cdae_als_kernels.hpp — WRMF fitted by alternating least squares (cdae_hip_create_als).
//
// One half-step solves, for every row u with a non-empty interaction row R_u and the other side's table Y frozen,
//     A_u x_u = b_u,   A_u = G + alpha * sum_{i in R_u} y_i y_i^T + lambda * I,   G = Y^T Y,   b_u = (1 + alpha) * sum_{i in R_u} y_i
// by `steps` iterations of conjugate gradients from the current x_u.  A_u is never formed: A_u p = G p + alpha sum_i y_i (y_i . p)
// + lambda p.  Two kernels (+ a fold):
//   als_gram_kernel / als_gram_fold_kernel   G from the table, on v_mfma_f32_32x32x2_f32, the same bits on every call
//   als_solve_kernel<NI>                     32 rows per workgroup: the sparse part per row on the VALU, G p for the block's 32
//                                            vectors at once on the matrix cores — G is read once per block and product
#pragma once
#include "cdae_kernels.hpp"
#include "cdae_recommend_kernels.hpp"      // floatx16

namespace cdae {

// ---- G = T^T T -------------------------------------------------------------------------------------------------------------------
// T is [rows x Kp] with zero pad columns, so G's pad rows and columns come out zero without a mask.  The rows are cut into
// als_gram_slices(rows) slices of als_gram_slice_rows(rows) rows — both functions of the row count alone.  One wavefront owns one
// 32 x 32 tile of one slice's partial Gram: output (i, j) of tile (a, b) is sum_r T[r][32 a + i] * T[r][32 b + j], the A operand's
// lane (i, k) and the B operand's lane (k, j) are both plain coalesced loads of row r0 + k, and the chain over r ascends.  No atomics:
// the partials are added in slice order by als_gram_fold_kernel.  G[i][j] and G[j][i] see the same products in the same order, so G is
// symmetric to the bit.
constexpr uint32_t ALS_GRAM_SLICES_MAX = 32;
constexpr uint32_t ALS_GRAM_SLICE_MIN_ROWS = 256;
__host__ __device__ inline uint32_t als_gram_slices(uint64_t rows) {
  const uint64_t s = (rows + ALS_GRAM_SLICE_MIN_ROWS - 1) / ALS_GRAM_SLICE_MIN_ROWS;
  return (uint32_t)(s < 1 ? 1 : (s > ALS_GRAM_SLICES_MAX ? ALS_GRAM_SLICES_MAX : s));
}
__host__ __device__ inline uint64_t als_gram_slice_rows(uint64_t rows) {
  const uint64_t per = (rows + als_gram_slices(rows) - 1) / als_gram_slices(rows);
  return (per + 1) & ~(uint64_t)1;             // two rows per MFMA
}

__global__ void __launch_bounds__(64)
als_gram_kernel(const float* __restrict__ T, uint64_t rows, uint32_t Kp, float* __restrict__ part /* [slices][Kp x Kp] */) {
  const uint32_t tiles = Kp / 32u;
  const uint32_t a = blockIdx.x / tiles, b = blockIdx.x % tiles, slice = blockIdx.y;
  const uint32_t lane = threadIdx.x, col = lane & 31u, half = lane >> 5;
  const uint64_t per = als_gram_slice_rows(rows);
  const uint64_t r_begin = (uint64_t)slice * per;
  const uint64_t r_end = r_begin + per < rows ? r_begin + per : rows;
  floatx16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const float* Ta = T + 32u * a + col;
  const float* Tb = T + 32u * b + col;
  for (uint64_t r0 = r_begin; r0 < r_end; r0 += 2) {
    const uint64_t r = r0 + half;
    const bool in = r < r_end;                 // (an odd tail: the second row of the pair is a zero row)
    const float va = in ? Ta[r * Kp] : 0.f;
    const float vb = in ? Tb[r * Kp] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(va, vb, acc, 0, 0, 0);
  }
  // C[i][j]: lane holds i = 8 q + 4 half + e of column j = lane & 31
  float* out = part + (size_t)slice * Kp * Kp;
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      out[(size_t)(32u * a + 8u * q + 4u * half + e) * Kp + 32u * b + col] = acc[4 * q + e];
}

__global__ void __launch_bounds__(256)
als_gram_fold_kernel(const float* __restrict__ part, uint32_t slices, uint32_t n /* Kp x Kp */, float* __restrict__ G) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  float s = part[i];
  for (uint32_t k = 1; k < slices; ++k) s += part[(size_t)k * n + i];
  G[i] = s;
}

// ---- the block solve -------------------------------------------------------------------------------------------------------------
// A workgroup owns ALS_BLOCK_ROWS = 32 consecutive rows: 32 right-hand sides are one MFMA tile's width.  It has WAVES wavefronts
// (4; 8 at Kp = 512) and each serves 32 / WAVES rows in turn, keeping their x, r and p in registers in the lane-owns-
// [l NI, (l + 1) NI) layout: 3 * (32 / WAVES) * NI registers (96 at Kp = 256 and at Kp = 512).
//
// One product A p of the whole block:
//   1. every wavefront writes the p of its rows to the LDS tile P[32][Kp + 4] (a zero row for an absent row of a last block)
//   2. Q = G P on the matrix cores: output tile t (rows 32 t .. 32 t + 31 of Q) belongs to wavefront t % WAVES; its A operand is
//      read from G in global memory (once per block and product: Kp^2 floats, L2-resident), its B operand from the LDS tile, and the
//      chain over k ascends.  Column j of the product depends on column j of P alone, so a row's result does not depend on its
//      neighbours in the block.  The accumulators stay in registers until every wavefront has read P, then overwrite it: one tile,
//      not two.
//   3. every wavefront reads Q back row by row and adds, per row, alpha * sum_i y_i (y_i . p) — a wavefront dot product (wave_sum)
//      and an axpy per interaction, items in CSR order — and lambda * p.
// LDS: 32 * (Kp + 4) floats = 33 280 B at Kp = 256 (the kernel is held to 256 registers per lane, so a CU takes two workgroups by
// registers and four by LDS), 66 048 B at Kp = 512: 32 rows still fit there, so the block is 32 rows at every Kp and the
// K = 512 form only takes eight wavefronts instead of four to keep the per-lane state at 96 registers.
// Results leave through ordinary vector stores; an absent row and (in place) an empty row write nothing.
constexpr uint32_t ALS_BLOCK_ROWS = 32;
constexpr float ALS_RS_STOP = 1e-20f;
template <int NI> constexpr int als_waves() { return NI == 8 ? 8 : 4; }
template <int NI> constexpr size_t als_solve_lds_bytes() { return (size_t)ALS_BLOCK_ROWS * (64 * NI + 4) * sizeof(float); }

template <int NI>
__device__ __forceinline__ void als_load_row(const float* __restrict__ p, uint32_t lane, float (&v)[NI]) {
  if constexpr (NI % 4 == 0) {
#pragma unroll
    for (int e = 0; e < NI; e += 4) {
      const float4 t = *reinterpret_cast<const float4*>(p + lane * NI + e);
      v[e] = t.x; v[e + 1] = t.y; v[e + 2] = t.z; v[e + 3] = t.w;
    }
  } else if constexpr (NI == 2) {
    const float2 t = *reinterpret_cast<const float2*>(p + lane * 2);
    v[0] = t.x; v[1] = t.y;
  } else {
    v[0] = p[lane];
  }
}
template <int NI>
__device__ __forceinline__ void als_store_row(float* __restrict__ p, uint32_t lane, const float (&v)[NI]) {
  if constexpr (NI % 4 == 0) {
#pragma unroll
    for (int e = 0; e < NI; e += 4) *reinterpret_cast<float4*>(p + lane * NI + e) = make_float4(v[e], v[e + 1], v[e + 2], v[e + 3]);
  } else if constexpr (NI == 2) {
    *reinterpret_cast<float2*>(p + lane * 2) = make_float2(v[0], v[1]);
  } else {
    p[lane] = v[0];
  }
}
template <int NI>
__device__ __forceinline__ float als_dot(const float (&a)[NI], const float (&b)[NI]) {
  float s = a[0] * b[0];
#pragma unroll
  for (int e = 1; e < NI; ++e) s = fmaf(a[e], b[e], s);
  return wave_sum(s);
}

// x0 == nullptr: every row starts from zero.  dst may be x0 (the half-step: in place; an empty row is then left as it is) or another
// table (cdae_hip_als_solve_rows: an empty row receives its start vector).  row_ptr / col: the CSR of the n_rows rows, items < rows of Y.
// WEIGHTED (cdae_hip_als_set_confidence, cdae_hip_als_solve_rows_weighted): w holds one confidence weight per entry of col, the pair's
// confidence is 1 + alpha * w.  Per interaction the weight is read beside the item id (wavefront-uniform), the dot product y . p is
// scaled by it before the axpy into sp, and b is accumulated as fmaf(fmaf(alpha, w, 1), y, sb) in CSR order, so the residual is sb - ap.
// The binary form (WEIGHTED = false: a handle without weights) never reads w: b = (1 + alpha) * sum y.
template <int NI, bool WEIGHTED = false>
__global__ void __launch_bounds__(als_waves<NI>() * 64, 2)      // two wavefronts per SIMD: at most 256 registers per lane
als_solve_kernel(const int64_t* __restrict__ row_ptr, const uint32_t* __restrict__ col, uint64_t n_rows,
                 const float* __restrict__ Y, const float* __restrict__ G, const float* x0, float* dst,
                 float alpha, float lambda, uint32_t steps, const float* __restrict__ w) {
  constexpr int WAVES = als_waves<NI>();
  constexpr int RPW = (int)ALS_BLOCK_ROWS / WAVES;           // rows per wavefront
  constexpr int Kp = 64 * NI;
  constexpr int ROW = Kp + 4;                                // LDS row stride in floats
  constexpr int TILES = Kp / 32;
  constexpr int TPW = (TILES + WAVES - 1) / WAVES;           // output tiles per wavefront
  extern __shared__ __attribute__((aligned(16))) char als_smem[];
  float* P = reinterpret_cast<float*>(als_smem);             // [32][ROW]: the block's p vectors, then Q = G P in the same place
  const uint32_t lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
  const uint32_t col_u = lane & 31u, half = lane >> 5;
  const uint64_t row0 = (uint64_t)blockIdx.x * ALS_BLOCK_ROWS + (uint64_t)wave * RPW;
  const bool in_place = dst == x0;

  float x[RPW][NI], r[RPW][NI], p[RPW][NI], rs[RPW];
  bool live[RPW];                                            // the row exists, has interactions and has not stopped
#pragma unroll
  for (int t = 0; t < RPW; ++t) {
    const uint64_t row = row0 + t;
    const bool valid = row < n_rows;
    live[t] = valid && row_ptr[row + 1] > row_ptr[row];
    if (valid && x0) als_load_row<NI>(x0 + row * Kp, lane, x[t]);
    else {
#pragma unroll
      for (int e = 0; e < NI; ++e) x[t][e] = 0.f;
    }
#pragma unroll
    for (int e = 0; e < NI; ++e) { p[t][e] = live[t] ? x[t][e] : 0.f; r[t][e] = 0.f; }     // the first product is A x
    rs[t] = 0.f;
  }

  for (uint32_t it = 0; it <= steps; ++it) {                 // product 0 gives the residual, products 1 .. steps are the CG iterations
    // 1. stage the block's p
#pragma unroll
    for (int t = 0; t < RPW; ++t) {
      float z[NI];
#pragma unroll
      for (int e = 0; e < NI; ++e) z[e] = live[t] ? p[t][e] : 0.f;
      als_store_row<NI>(P + (wave * RPW + t) * ROW, lane, z);
    }
    __syncthreads();
    // 2. Q = G P
    floatx16 acc[TPW];
#pragma unroll
    for (int q = 0; q < TPW; ++q)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[q][e] = 0.f;
    if (wave < (uint32_t)TILES) {
      const float* brow = P + col_u * ROW + 4 * half;
#pragma unroll 2
      for (int c = 0; c < Kp / 8; ++c) {
        const float4 b4 = *reinterpret_cast<const float4*>(brow + 8 * c);
#pragma unroll
        for (int q = 0; q < TPW; ++q) {
          const uint32_t tile = wave + (uint32_t)(WAVES * q);
          if (tile < (uint32_t)TILES) {
            const float4 a4 = *reinterpret_cast<const float4*>(G + (size_t)(32u * tile + col_u) * Kp + 8 * c + 4 * half);
            acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc[q], 0, 0, 0);
            acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc[q], 0, 0, 0);
            acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc[q], 0, 0, 0);
            acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc[q], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();                                         // every wavefront has read P
    if (wave < (uint32_t)TILES) {
#pragma unroll
      for (int q = 0; q < TPW; ++q) {
        const uint32_t tile = wave + (uint32_t)(WAVES * q);
        if (tile < (uint32_t)TILES) {
          // C[k][j]: lane holds k = 32 tile + 8 g + 4 half + e of column (block row) j = lane & 31
#pragma unroll
          for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4*>(P + col_u * ROW + 32u * tile + 8u * g + 4u * half) =
                make_float4(acc[q][4 * g], acc[q][4 * g + 1], acc[q][4 * g + 2], acc[q][4 * g + 3]);
        }
      }
    }
    __syncthreads();
    // 3. per row: the sparse part, then the step
#pragma unroll
    for (int t = 0; t < RPW; ++t) {
      if (live[t]) {                                         // (wavefront-uniform)
        float ap[NI], sp[NI], sb[NI];
        als_load_row<NI>(P + (wave * RPW + t) * ROW, lane, ap);
#pragma unroll
        for (int e = 0; e < NI; ++e) { sp[e] = 0.f; sb[e] = 0.f; }
        // four interactions at a time: their item rows are loaded and their dot products reduced side by side (the loads of one item
        // do not wait for the reduction of the one before), the axpys stay in CSR order — the same sums as one item at a time
        const int64_t q1 = row_ptr[row0 + t + 1];            // (wavefront-uniform: read again rather than kept per row)
        int64_t q = row_ptr[row0 + t];
        for (; q + 4 <= q1; q += 4) {
          float y[4][NI], d[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) als_load_row<NI>(Y + (size_t)col[q + j] * Kp, lane, y[j]);
#pragma unroll
          for (int j = 0; j < 4; ++j) d[j] = als_dot<NI>(y[j], p[t]);
          float wq[4];
          if constexpr (WEIGHTED) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { wq[j] = w[q + j]; d[j] *= wq[j]; }
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int e = 0; e < NI; ++e) sp[e] = fmaf(y[j][e], d[j], sp[e]);
            if (it == 0) {
              if constexpr (WEIGHTED) {
                const float c = fmaf(alpha, wq[j], 1.f);
#pragma unroll
                for (int e = 0; e < NI; ++e) sb[e] = fmaf(c, y[j][e], sb[e]);
              } else {
#pragma unroll
                for (int e = 0; e < NI; ++e) sb[e] += y[j][e];
              }
            }
          }
        }
        for (; q < q1; ++q) {
          float y[NI];
          als_load_row<NI>(Y + (size_t)col[q] * Kp, lane, y);
          const float wq = WEIGHTED ? w[q] : 1.f;
          const float d = WEIGHTED ? als_dot<NI>(y, p[t]) * wq : als_dot<NI>(y, p[t]);
#pragma unroll
          for (int e = 0; e < NI; ++e) sp[e] = fmaf(y[e], d, sp[e]);
          if (it == 0) {
            if constexpr (WEIGHTED) {
              const float c = fmaf(alpha, wq, 1.f);
#pragma unroll
              for (int e = 0; e < NI; ++e) sb[e] = fmaf(c, y[e], sb[e]);
            } else {
#pragma unroll
              for (int e = 0; e < NI; ++e) sb[e] += y[e];
            }
          }
        }
#pragma unroll
        for (int e = 0; e < NI; ++e) ap[e] = ap[e] + alpha * sp[e] + lambda * p[t][e];
        if (it == 0) {
#pragma unroll
          for (int e = 0; e < NI; ++e) { r[t][e] = (WEIGHTED ? sb[e] : (1.f + alpha) * sb[e]) - ap[e]; p[t][e] = r[t][e]; }
          rs[t] = als_dot<NI>(r[t], r[t]);
        } else {
          const float a = rs[t] / als_dot<NI>(p[t], ap);
#pragma unroll
          for (int e = 0; e < NI; ++e) { x[t][e] = fmaf(a, p[t][e], x[t][e]); r[t][e] = fmaf(-a, ap[e], r[t][e]); }
          const float rs_new = als_dot<NI>(r[t], r[t]);
          const float beta = rs_new / rs[t];
#pragma unroll
          for (int e = 0; e < NI; ++e) p[t][e] = fmaf(beta, p[t][e], r[t][e]);
          rs[t] = rs_new;
        }
        if (rs[t] < ALS_RS_STOP) live[t] = false;            // converged: the row keeps the x it has
      }
    }
    __syncthreads();                                         // Q has been read: the tile is the next product's P
  }

#pragma unroll
  for (int t = 0; t < RPW; ++t) {
    const uint64_t row = row0 + t;
    if (row < n_rows && (!in_place || row_ptr[row + 1] > row_ptr[row])) als_store_row<NI>(dst + row * Kp, lane, x[t]);
  }
}

// ---- the objective ---------------------------------------------------------------------------------------------------------------
// L = sum_{all u,i} c_ui (p_ui - s_ui)^2 + lambda (|X|^2 + |Y|^2), s = x_u . y_i, is never formed densely:
//   sum over all pairs of s^2 = <X^T X, Y^T Y>_F;   a stored pair adds c (1 - s)^2 - s^2;   the penalty is lambda (tr X^T X + tr Y^T Y).
// als_objective_kernel: one wavefront per user row; s from the solve's lane layout and wave_sum in fp32, the pair's term accumulated
// in fp64 in CSR order -> rows[u] (0 for an empty row).  The host adds rows[] in row order.  w == nullptr: every weight is 1.
// als_objective_gram_kernel: ONE workgroup; the Frobenius product of the two Grams and their traces in fp64, every thread a strided
// chain in ascending order and a fixed tree over the 256 threads: the same bits on every call.  No atomics anywhere.
template <int NI>
__global__ void __launch_bounds__(256)
als_objective_kernel(const int64_t* __restrict__ row_ptr, const uint32_t* __restrict__ col, const float* __restrict__ w, uint64_t n_rows,
                     const float* __restrict__ X, const float* __restrict__ Y, float alpha, double* __restrict__ rows) {
  constexpr int Kp = 64 * NI;
  const uint32_t lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
  const uint64_t row = (uint64_t)blockIdx.x * 4u + wave;
  if (row >= n_rows) return;                                 // (wavefront-uniform)
  float x[NI];
  als_load_row<NI>(X + row * Kp, lane, x);
  double acc = 0.0;
  const int64_t q1 = row_ptr[row + 1];
  for (int64_t q = row_ptr[row]; q < q1; ++q) {
    float y[NI];
    als_load_row<NI>(Y + (size_t)col[q] * Kp, lane, y);
    const double s = (double)als_dot<NI>(y, x);
    const double c = 1.0 + (double)alpha * (double)(w ? w[q] : 1.f);
    acc += c * (1.0 - s) * (1.0 - s) - s * s;
  }
  if (lane == 0) rows[row] = acc;
}

__global__ void __launch_bounds__(256)
als_objective_gram_kernel(const float* __restrict__ Gx, const float* __restrict__ Gy, uint32_t Kp, double* __restrict__ out3) {
  __shared__ double red[3][256];
  const uint32_t t = threadIdx.x;
  double f = 0.0, tx = 0.0, ty = 0.0;
  for (uint32_t i = t; i < Kp * Kp; i += 256u) f += (double)Gx[i] * (double)Gy[i];
  for (uint32_t i = t; i < Kp; i += 256u) { tx += (double)Gx[(size_t)i * Kp + i]; ty += (double)Gy[(size_t)i * Kp + i]; }
  red[0][t] = f; red[1][t] = tx; red[2][t] = ty;
  __syncthreads();
  for (uint32_t step = 128u; step >= 1u; step >>= 1) {
    if (t < step) {
#pragma unroll
      for (int k = 0; k < 3; ++k) red[k][t] += red[k][t + step];
    }
    __syncthreads();
  }
  if (t < 3u) out3[t] = red[t][0];
}

}  // namespace cdae
