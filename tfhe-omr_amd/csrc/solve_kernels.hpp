// Solve mod 257 on the device (include/omr_gpu.h, "Solve mod 257"): a blocked form of
// solve_matrix_mod_257 (matrix.rs:164-247) that makes the same pivot choices as the CPU statement
// (retriever.hip, solve_mod257) and therefore returns the same bits, singular column included.
//
// The augmented matrix W = [matrix | rhs] lives in the auditor's scratch as u16 [rows][ld], values < 257,
// ld = cols + width rounded up to 8 words so that every row starts on a 16-byte boundary. Per panel of
// SOLVE_PANEL columns starting at i0 (pc of them in the last panel):
//   solve_panel_kernel   one workgroup factorises the columns [i0, i0 + pc) over the rows [i0, rows): first
//                        non-zero pivot, swap, scale, eliminate, inside the panel only. It leaves the
//                        multipliers where the eliminated entries were, the pivot's inverse on the diagonal
//                        and the unit upper factor above it, and records the pivot rows.
//   solve_swap_kernel    one thread per column right of the panel: applies the panel's row swaps to it and
//                        forms the panel's pivot rows there (forward substitution through the panel's
//                        lower factor, scaled by the inverses).
//   solve_update_kernel  W22 -= L21 * U12 mod 257 over a grid of SOLVE_TILE_ROWS x SOLVE_TILE_WIDTH tiles,
//                        both factors staged in LDS, products summed unreduced in u32.
// Back substitution is blocked the same way, from the last block of SOLVE_PANEL rows up: solve_back_kernel
// solves the block's unit upper triangle per rhs column, solve_update_kernel subtracts its contribution
// from the rhs of every row above. solve_store_kernel copies rows 0 .. cols - 1 of the rhs out.
// A panel that finds no pivot writes 1 + column to *status; every kernel reads that word first and does
// nothing once it is set. Launches are stream-ordered; nothing here waits on another workgroup.
#pragma once

#include "common.hpp"
#include "weights.hpp"

namespace omr {

constexpr int SOLVE_PANEL = 32;        // columns per panel step, rows per back-substitution block
constexpr int SOLVE_PANEL_T = 1024;    // threads of the panel workgroup
constexpr int SOLVE_TILE_ROWS = 64;    // trailing-update tile
constexpr int SOLVE_TILE_WIDTH = 64;
constexpr int SOLVE_UPDATE_T = 256;    // 16 x 16 threads, 4 x 4 entries each
constexpr int SOLVE_COL_T = 256;       // threads of the per-column kernels
constexpr uint32_t SOLVE_NO_PIVOT = 0xFFFFFFFFu;
constexpr uint32_t P32 = (uint32_t)P;

__device__ __forceinline__ uint32_t inv257(uint32_t v) {  // v^(p-2) mod p, v in [1, 256]
  uint32_t r = 1, b = v;
#pragma unroll
  for (int e = 0; e < 8; ++e) {  // p - 2 = 255 = 0b11111111
    r = r * b % P32;
    b = b * b % P32;
  }
  return r;
}

// [matrix | rhs] reduced mod 257 into W (pad columns zero); one thread per word of W.
__global__ void __launch_bounds__(SOLVE_COL_T)
solve_load_kernel(const uint16_t *__restrict__ matrix, const uint16_t *__restrict__ rhs, uint32_t rows, uint32_t cols,
                  uint32_t width, uint32_t ld, uint16_t *__restrict__ W) {
  const size_t idx = (size_t)blockIdx.x * SOLVE_COL_T + threadIdx.x;
  if (idx >= (size_t)rows * ld) return;
  const uint32_t j = (uint32_t)(idx / ld), k = (uint32_t)(idx % ld);
  uint32_t v = 0;
  if (k < cols) v = matrix[(size_t)j * cols + k];
  else if (k < cols + width) v = rhs[(size_t)j * width + (k - cols)];
  W[idx] = (uint16_t)(v % P32);
}

// The panel step. One workgroup; thread t owns the rows i + 1 + t, i + 1 + t + 1024, .. of each column step.
__global__ void __launch_bounds__(SOLVE_PANEL_T)
solve_panel_kernel(uint16_t *__restrict__ W, uint32_t rows, uint32_t ld, uint32_t i0, uint32_t pc,
                   uint32_t *__restrict__ pivots, uint32_t *__restrict__ status) {
  if (*status) return;
  __shared__ uint32_t s_piv[2];
  __shared__ uint32_t s_row[SOLVE_PANEL];
  const uint32_t tid = threadIdx.x;
  if (tid < 2) s_piv[tid] = SOLVE_NO_PIVOT;
  __syncthreads();
  // the first pivot: the smallest row j >= i0 with a non-zero entry in column i0
  for (uint32_t j = i0 + tid; j < rows; j += SOLVE_PANEL_T)
    if (W[(size_t)j * ld + i0] != 0) {
      atomicMin(&s_piv[0], j);
      break;
    }
  __syncthreads();
  for (uint32_t t = 0; t < pc; ++t) {
    const uint32_t i = i0 + t, piv = s_piv[t & 1];
    if (piv == SOLVE_NO_PIVOT) {  // uniform: every thread read the same word
      if (tid == 0) *status = 1 + i;
      return;
    }
    if (tid < 64) {  // one wave: swap the panel's part of rows i and piv, scale the new row i
      const uint32_t c = tid < pc ? tid : 0;
      const uint32_t a = W[(size_t)i * ld + i0 + c], b = W[(size_t)piv * ld + i0 + c];
      const uint32_t iv = inv257((uint32_t)__shfl((int)b, (int)t));  // b of lane t: the pivot
      if (tid < pc) {
        // left of t: the multipliers move with their rows; at t: the inverse; right of t: the scaled row
        const uint32_t nb = c < t ? b : (c == t ? iv : b * iv % P32);
        if (piv != i) W[(size_t)piv * ld + i0 + c] = (uint16_t)a;
        W[(size_t)i * ld + i0 + c] = (uint16_t)nb;
        s_row[c] = nb;
      }
      if (tid == 0) {
        pivots[i] = piv;
        s_piv[(t + 1) & 1] = SOLVE_NO_PIVOT;
      }
    }
    __syncthreads();
    // rows below i: subtract entry(j, i) times row i right of column i inside the panel; the entry stays
    // as the row's multiplier. The rows of a thread increase, so its first hit is its smallest.
    uint32_t mine = SOLVE_NO_PIVOT;
    if (pc == SOLVE_PANEL) {
      // a full panel: i0 is a multiple of 32 and ld of 8, so a row's panel part is four aligned 16-byte
      // words. Registers are indexed by constants only: the column step enters through srm, row i with its
      // entries up to column i zeroed (a zero coefficient leaves an entry as it is), and through two
      // 2-byte loads of the row's entries in columns i and i + 1.
      uint32_t srm[SOLVE_PANEL];
#pragma unroll
      for (int cc = 0; cc < SOLVE_PANEL; ++cc) srm[cc] = (uint32_t)cc > t ? s_row[cc] : 0u;
      const uint32_t tn = t + 1 < (uint32_t)SOLVE_PANEL ? t + 1 : t, sr_next = t + 1 < (uint32_t)SOLVE_PANEL ? s_row[tn] : 0u;
      for (uint32_t j = i + 1 + tid; j < rows; j += SOLVE_PANEL_T) {
        uint16_t *row16 = W + (size_t)j * ld + i0;
        uint4 *row = reinterpret_cast<uint4 *>(row16);
        uint4 q[SOLVE_PANEL / 8];
#pragma unroll
        for (int x = 0; x < SOLVE_PANEL / 8; ++x) q[x] = row[x];
        const uint32_t c = row16[t];
        // the row's entry in column i + 1 after this step (0 in the panel's last step)
        const uint32_t next = t + 1 < (uint32_t)SOLVE_PANEL ? (row16[tn] + P32 * P32 - c * sr_next) % P32 : 0u;
        if (c) {
          uint32_t v[SOLVE_PANEL];
#pragma unroll
          for (int x = 0; x < SOLVE_PANEL / 8; ++x) {
            const uint32_t w4[4] = {q[x].x, q[x].y, q[x].z, q[x].w};
#pragma unroll
            for (int y = 0; y < 4; ++y) {
              v[8 * x + 2 * y] = w4[y] & 0xFFFFu;
              v[8 * x + 2 * y + 1] = w4[y] >> 16;
            }
          }
#pragma unroll
          for (int cc = 1; cc < SOLVE_PANEL; ++cc) v[cc] = (v[cc] + P32 * P32 - c * srm[cc]) % P32;
#pragma unroll
          for (int x = 0; x < SOLVE_PANEL / 8; ++x)
            row[x] = make_uint4(v[8 * x] | v[8 * x + 1] << 16, v[8 * x + 2] | v[8 * x + 3] << 16,
                                v[8 * x + 4] | v[8 * x + 5] << 16, v[8 * x + 6] | v[8 * x + 7] << 16);
        }
        if (next != 0 && mine == SOLVE_NO_PIVOT) mine = j;
      }
    } else {
      for (uint32_t j = i + 1 + tid; j < rows; j += SOLVE_PANEL_T) {
        uint16_t *row = W + (size_t)j * ld + i0;
        const uint32_t c = row[t];
        uint32_t next = 0;  // the row's entry in column i + 1 after this step
        if (c) {
          for (uint32_t cc = t + 1; cc < pc; ++cc) {
            const uint32_t v = (row[cc] + P32 * P32 - c * s_row[cc]) % P32;
            row[cc] = (uint16_t)v;
            if (cc == t + 1) next = v;
          }
        } else if (t + 1 < pc) {
          next = row[t + 1];
        }
        if (next != 0 && mine == SOLVE_NO_PIVOT) mine = j;
      }
    }
    if (mine != SOLVE_NO_PIVOT) atomicMin(&s_piv[(t + 1) & 1], mine);
    __syncthreads();
  }
}

// Row swaps and pivot rows right of the panel: one thread per column k in [k0, ld).
__global__ void __launch_bounds__(SOLVE_COL_T)
solve_swap_kernel(uint16_t *__restrict__ W, uint32_t ld, uint32_t i0, uint32_t pc, uint32_t k0,
                  const uint32_t *__restrict__ pivots, const uint32_t *__restrict__ status) {
  if (*status) return;
  __shared__ uint16_t s_l[SOLVE_PANEL][SOLVE_PANEL + 2];
  __shared__ uint32_t s_piv[SOLVE_PANEL];
  for (uint32_t e = threadIdx.x; e < pc * pc; e += SOLVE_COL_T) s_l[e / pc][e % pc] = W[(size_t)(i0 + e / pc) * ld + i0 + e % pc];
  if (threadIdx.x < pc) s_piv[threadIdx.x] = pivots[i0 + threadIdx.x];
  __syncthreads();
  const uint32_t k = k0 + blockIdx.x * SOLVE_COL_T + threadIdx.x;
  if (k >= ld) return;
  for (uint32_t t = 0; t < pc; ++t) {  // in the order the panel made them
    const uint32_t piv = s_piv[t];
    if (piv == i0 + t) continue;
    const uint16_t a = W[(size_t)(i0 + t) * ld + k];
    W[(size_t)(i0 + t) * ld + k] = W[(size_t)piv * ld + k];
    W[(size_t)piv * ld + k] = a;
  }
  // u_t = inv_t (a_t - sum_{s < t} l_ts u_s): at most 31 products of at most 256^2 per sum
  uint32_t u[SOLVE_PANEL];
#pragma unroll
  for (int t = 0; t < SOLVE_PANEL; ++t) {
    if ((uint32_t)t < pc) {
      uint32_t acc = 0;
#pragma unroll
      for (int s = 0; s < t; ++s) acc += (uint32_t)s_l[t][s] * u[s];
      const uint32_t a = W[(size_t)(i0 + t) * ld + k];
      u[t] = (a + P32 - acc % P32) % P32 * s_l[t][t] % P32;
      W[(size_t)(i0 + t) * ld + k] = (uint16_t)u[t];
    } else {
      u[t] = 0;
    }
  }
}

// W[j][k] -= sum_{t < depth} W[j][lc + t] * W[ur + t][k] mod 257 for j in [r0, r1), k in [c0, c1); the two
// factors do not overlap the updated block. BACK only names the back substitution's instance.
template <bool BACK>
__global__ void __launch_bounds__(SOLVE_UPDATE_T)
solve_update_kernel(uint16_t *__restrict__ W, uint32_t ld, uint32_t r0, uint32_t r1, uint32_t c0, uint32_t c1,
                    uint32_t lc, uint32_t ur, uint32_t depth, const uint32_t *__restrict__ status) {
  if (*status) return;
  __shared__ uint16_t s_a[SOLVE_TILE_ROWS][SOLVE_PANEL + 2];
  __shared__ uint16_t s_b[SOLVE_PANEL][SOLVE_TILE_WIDTH];
  const uint32_t tid = threadIdx.x, tr = r0 + blockIdx.y * SOLVE_TILE_ROWS, tc = c0 + blockIdx.x * SOLVE_TILE_WIDTH;
  for (uint32_t e = tid; e < SOLVE_TILE_ROWS * SOLVE_PANEL; e += SOLVE_UPDATE_T) {
    const uint32_t r = e / SOLVE_PANEL, t = e % SOLVE_PANEL;
    s_a[r][t] = (tr + r < r1 && t < depth) ? W[(size_t)(tr + r) * ld + lc + t] : (uint16_t)0;
  }
  for (uint32_t e = tid; e < SOLVE_PANEL * SOLVE_TILE_WIDTH; e += SOLVE_UPDATE_T) {
    const uint32_t t = e / SOLVE_TILE_WIDTH, c = e % SOLVE_TILE_WIDTH;
    s_b[t][c] = (tc + c < c1 && t < depth) ? W[(size_t)(ur + t) * ld + tc + c] : (uint16_t)0;
  }
  __syncthreads();
  // thread (ty, tx): rows 4 ty .. 4 ty + 3, columns tx, tx + 16, tx + 32, tx + 48
  const uint32_t ty = tid / 16, tx = tid % 16;
  uint32_t acc[4][4] = {};
#pragma unroll 8
  for (int t = 0; t < SOLVE_PANEL; ++t) {  // 32 products of at most 256^2: below 2^21
    uint32_t a[4], b[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] = s_a[4 * ty + r][t];
#pragma unroll
    for (int c = 0; c < 4; ++c) b[c] = s_b[t][tx + 16 * c];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[r][c] += a[r] * b[c];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint32_t j = tr + 4 * ty + r;
    if (j >= r1) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const uint32_t k = tc + tx + 16 * c;
      if (k >= c1) continue;
      uint16_t *w = W + (size_t)j * ld + k;
      *w = (uint16_t)((*w + P32 - acc[r][c] % P32) % P32);
    }
  }
}

// Back substitution inside the block of rows [b0, b0 + pb): x_t = y_t - sum_{s > t} U[b0 + t][b0 + s] x_s per
// rhs column k in [k0, ld), one thread per column, from the block's last row up.
__global__ void __launch_bounds__(SOLVE_COL_T)
solve_back_kernel(uint16_t *__restrict__ W, uint32_t ld, uint32_t b0, uint32_t pb, uint32_t k0,
                  const uint32_t *__restrict__ status) {
  if (*status) return;
  __shared__ uint16_t s_u[SOLVE_PANEL][SOLVE_PANEL + 2];
  for (uint32_t e = threadIdx.x; e < pb * pb; e += SOLVE_COL_T) s_u[e / pb][e % pb] = W[(size_t)(b0 + e / pb) * ld + b0 + e % pb];
  __syncthreads();
  const uint32_t k = k0 + blockIdx.x * SOLVE_COL_T + threadIdx.x;
  if (k >= ld) return;
  uint32_t x[SOLVE_PANEL];
#pragma unroll
  for (int t = SOLVE_PANEL - 1; t >= 0; --t) {
    if ((uint32_t)t < pb) {
      uint32_t acc = 0;
#pragma unroll
      for (int s = t + 1; s < SOLVE_PANEL; ++s) acc += (uint32_t)s_u[t][s] * x[s];  // x[s] = 0 for s >= pb
      const uint32_t y = W[(size_t)(b0 + t) * ld + k];
      x[t] = (y + P32 - acc % P32) % P32;
      W[(size_t)(b0 + t) * ld + k] = (uint16_t)x[t];
    } else {
      x[t] = 0;
    }
  }
}

// solution[k][b] = W[k][cols + b], unless the solve failed
__global__ void __launch_bounds__(SOLVE_COL_T)
solve_store_kernel(const uint16_t *__restrict__ W, uint32_t ld, uint32_t cols, uint32_t width,
                   uint16_t *__restrict__ solution, const uint32_t *__restrict__ status) {
  if (*status) return;
  const size_t idx = (size_t)blockIdx.x * SOLVE_COL_T + threadIdx.x;
  if (idx >= (size_t)cols * width) return;
  solution[idx] = W[(idx / width) * ld + cols + idx % width];
}

// The indexed matrix of a retrieval: m[j][k] = w(j, indices[k]) (weights.hpp, indexed_weight_block); one
// thread per (combination, index). Every row is a real combination of the board.
__global__ void __launch_bounds__(SOLVE_COL_T)
retrieve_matrix_kernel(WeightKey key, const uint64_t *__restrict__ indices, uint32_t rows, uint32_t cols,
                       uint16_t *__restrict__ m) {
  const size_t idx = (size_t)blockIdx.x * SOLVE_COL_T + threadIdx.x;
  if (idx >= (size_t)rows * cols) return;
  const uint64_t g = indices[idx % cols];
  uint16_t w[16];
  indexed_weight_block(key, (uint32_t)(idx / cols), g >> 4, w);
  uint16_t v = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) v = (g & 15) == (uint64_t)i ? w[i] : v;  // no runtime-indexed local array
  m[idx] = v;
}

// The same matrix in the reference's convention (weights.hpp, "Reference payload weights by seek"):
// m[j][k] = w(j * all + indices[k]), the word at raw position pos(n) of the reference stream.
__global__ void __launch_bounds__(SOLVE_COL_T)
retrieve_matrix_seek_kernel(WeightKey key, omr_weight_seek seek, uint64_t all, const uint64_t *__restrict__ indices,
                            uint32_t rows, uint32_t cols, uint16_t *__restrict__ m) {
  const size_t idx = (size_t)blockIdx.x * SOLVE_COL_T + threadIdx.x;
  if (idx >= (size_t)rows * cols) return;
  const uint64_t p = seek_pos(seek, (uint64_t)(idx / cols) * all + indices[idx % cols]);
  uint32_t w[16];
  chacha_block(12, key.k, p >> 4, 0, w);
  uint32_t v = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) v = (p & 15) == (uint64_t)i ? w[i] : v;  // no runtime-indexed local array
  m[idx] = weight_of_word(v);
}

// The right-hand side of a retrieval from decoded payload ciphertexts u16 [n_ct][2048]: combination j is in
// ciphertext j / per, slots (j % per) * 612 onward.
__global__ void __launch_bounds__(SOLVE_COL_T)
retrieve_rhs_kernel(const uint16_t *__restrict__ decoded, uint32_t rows, uint32_t per, uint16_t *__restrict__ rhs) {
  const size_t idx = (size_t)blockIdx.x * SOLVE_COL_T + threadIdx.x;
  if (idx >= (size_t)rows * PAYLOAD_LEN) return;
  const uint32_t j = (uint32_t)(idx / PAYLOAD_LEN), b = (uint32_t)(idx % PAYLOAD_LEN);
  rhs[idx] = decoded[(size_t)(j / per) * N2 + (j % per) * PAYLOAD_LEN + b];
}

// The same for a layout with a payload length of its own (weights.hpp, payload_word_at): combination j's L
// words gathered across the `stripes` ciphertexts of its group; rhs [rows][L].
__global__ void __launch_bounds__(SOLVE_COL_T)
retrieve_rhs_len_kernel(const uint16_t *__restrict__ decoded, uint32_t rows, uint32_t per, uint32_t L, uint32_t stripes,
                        uint16_t *__restrict__ rhs) {
  const size_t idx = (size_t)blockIdx.x * SOLVE_COL_T + threadIdx.x;
  if (idx >= (size_t)rows * L) return;
  rhs[idx] = decoded[payload_word_at((uint32_t)(idx / L), (uint32_t)(idx % L), L, per, stripes)];
}

}  // namespace omr
