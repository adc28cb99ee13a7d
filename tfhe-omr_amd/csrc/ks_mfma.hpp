// LWE key switch on the matrix cores (NonPowOf2LweKeySwitchingKey::key_switch, detector.rs:560-563,
// with the modulus switch :571-575 and offset :577-594).
//
// The key switch is a binary-by-integer matrix product:
//   acc[m][col] = sum_i sum_j bit_j(x[m][i]) * KSK[i][j][col]      (i < 1024, j < 27, col <= 670)
// so it runs as an int8 GEMM: A[m][32 i + j] = bit_j(x[m][i]) (0/1, j < 27, zero for j >= 27),
// B_l[32 i + j][col] = the l-th 7-bit limb of KSK[i][j][col] (l = 0..3, 28 bits >= 27), one
// v_mfma_i32_32x32x32_i8 per (32 messages x 32 columns x 32 digits x limb). Per limb the int32
// sums stay below 27648 * 127 < 2^22; acc = sum_l C_l 2^(7 l) < 2^43 is exact in int64 and then
// reduced mod q1 like the oracle's u64 sum, so the output is bit-identical.
// The geometry (KSM_COLS, KSM_LIMBS, KSKB_WORDS, KS_SPLIT) is in kernels.hpp, the KSK's conversion to
// the int8 limbs (ksk_to_i8_kernel) in key_convert.hpp.
#pragma once

#include "kernels.hpp"

namespace omr {

typedef int omr_v4i __attribute__((ext_vector_type(4)));
typedef int omr_v16i __attribute__((ext_vector_type(16)));

// Output column `col` of one message from the exact key-switch sum (detector.rs:560-594):
// b' = b - sum (columns < 670: -sum), modulus switch q1 -> 4096 (round half up), and the
// offset b += 7 * 128 on the body.
__device__ __forceinline__ uint32_t ks_epilogue(uint64_t sum, uint64_t bq, int col) {
  const uint64_t s = sum % Q1;
  uint64_t v = col < NI ? (Q1 - s) % Q1 : (bq + Q1 - s) % Q1;
  v = ((2ull * QI * v + Q1) / (2ull * Q1)) % QI;
  if (col == NI) v = (v + CLUES * (QI / TI)) % QI;
  return (uint32_t)v;
}

// 0/1 bytes of the 16 bits of x starting at bit `base` (A fragment: 16 int8 per lane): each
// nibble n spreads to four bytes as (n * 0x204081) & 0x01010101 (shifted copies 0, 7, 14, 21
// never overlap).
__device__ __forceinline__ omr_v4i bit_bytes16(uint32_t x, int base) {
  omr_v4i a;
#pragma unroll
  for (int v = 0; v < 4; ++v) a[v] = (int)((((x >> (base + 4 * v)) & 15u) * 0x204081u) & 0x01010101u);
  return a;
}

// grid (ceil(B / 64), 21), 64 threads: one wave computes messages m0 .. m0 + 63 (two 32-row
// tiles) x columns c0 .. c0 + 31 for the 4 limbs. Operand maps of v_mfma_i32_32x32x32_i8 (as the
// bf16 32x32x16 form, 16 elements per lane): lane l (r = l & 31, h = l >> 5) holds A[row r][k = 16 h
// + e] and B[k = 16 h + e][col r]; D: col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 h.
__global__ __launch_bounds__(64, 2) void ks_mfma_kernel(const uint32_t *__restrict__ lwe1t,
                                                     const uint32_t *__restrict__ kskb,
                                                     uint32_t *__restrict__ lwe_int, int B) {
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int m0 = blockIdx.x * 64, c0 = blockIdx.y * 32;
  omr_v16i acc[2][KSM_LIMBS];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int l = 0; l < KSM_LIMBS; ++l) acc[t][l] = omr_v16i{};
  const bool live0 = m0 + r < B, live1 = m0 + 32 + r < B;
  const omr_v4i *bbase = reinterpret_cast<const omr_v4i *>(kskb) + (size_t)(c0 + r) * 2 + h;
#pragma unroll 1
  for (int i = 0; i < N1; ++i) {
    const uint32_t x0 = live0 ? lwe1t[(size_t)i * B + m0 + r] : 0u;
    const uint32_t x1 = live1 ? lwe1t[(size_t)i * B + m0 + 32 + r] : 0u;
    const omr_v4i a0 = bit_bytes16(x0, 16 * h), a1 = bit_bytes16(x1, 16 * h);
#pragma unroll
    for (int l = 0; l < KSM_LIMBS; ++l) {
      const omr_v4i b = bbase[((size_t)i * KSM_LIMBS + l) * KSM_COLS * 2];
      acc[0][l] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b, acc[0][l], 0, 0, 0);
      acc[1][l] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b, acc[1][l], 0, 0, 0);
    }
  }
  const int col = c0 + r;
  if (col > NI) return;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int m = m0 + 32 * t + (reg & 3) + 8 * (reg >> 2) + 4 * h;
      if (m >= B) continue;
      const uint64_t sum = (uint64_t)acc[t][0][reg] + ((uint64_t)acc[t][1][reg] << 7) +
                           ((uint64_t)acc[t][2][reg] << 14) + ((uint64_t)acc[t][3][reg] << 21);
      lwe_int[(size_t)m * (NI + 1) + col] = ks_epilogue(sum, lwe1t[(size_t)N1 * B + m], col);
    }
}

// Sum of the 7 extracted LWEs mod q1 (detector.rs:556), transposed to [N1+1][B] for the key
// switch (lanes = messages).
__global__ void sum7_kernel(const uint32_t *__restrict__ ext, uint32_t *__restrict__ lwe1t,
                            int B) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)B * (N1 + 1)) return;
  const size_t m = idx % B, i = idx / B;
  uint32_t s = 0;
#pragma unroll
  for (int c = 0; c < CLUES; ++c) s += ext[(m * CLUES + c) * (N1 + 1) + i];
  lwe1t[i * B + m] = s % (uint32_t)Q1;
}

// ---- key switch, split over the input coefficients (the latency path: a lone message otherwise
// gets 21 waves for 88 MB of KSK) ------------------------------------------------------------------

// grid (ceil(B / 64), 21, KS_SPLIT): ks_mfma_kernel's tile over input coefficients
// [z * 1024 / KS_SPLIT, (z + 1) * 1024 / KS_SPLIT); int32 limb sums to part[z][m][col][limb].
__global__ __launch_bounds__(64, 2) void ks_mfma_split_kernel(const uint32_t *__restrict__ lwe1t,
                                                           const uint32_t *__restrict__ kskb,
                                                           int *__restrict__ part, int B, int Bpad) {
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int m0 = blockIdx.x * 64, c0 = blockIdx.y * 32, z = blockIdx.z;
  omr_v16i acc[2][KSM_LIMBS];
#pragma unroll
  for (int tt = 0; tt < 2; ++tt)
#pragma unroll
    for (int l = 0; l < KSM_LIMBS; ++l) acc[tt][l] = omr_v16i{};
  const bool live0 = m0 + r < B, live1 = m0 + 32 + r < B;
  const omr_v4i *bbase = reinterpret_cast<const omr_v4i *>(kskb) + (size_t)(c0 + r) * 2 + h;
  constexpr int SL = N1 / KS_SPLIT;
#pragma unroll 1
  for (int i = z * SL; i < (z + 1) * SL; ++i) {
    const uint32_t x0 = live0 ? lwe1t[(size_t)i * B + m0 + r] : 0u;
    const uint32_t x1 = live1 ? lwe1t[(size_t)i * B + m0 + 32 + r] : 0u;
    const omr_v4i a0 = bit_bytes16(x0, 16 * h), a1 = bit_bytes16(x1, 16 * h);
#pragma unroll
    for (int l = 0; l < KSM_LIMBS; ++l) {
      const omr_v4i bv = bbase[((size_t)i * KSM_LIMBS + l) * KSM_COLS * 2];
      acc[0][l] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, bv, acc[0][l], 0, 0, 0);
      acc[1][l] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, bv, acc[1][l], 0, 0, 0);
    }
  }
  const int col = c0 + r;
#pragma unroll
  for (int tt = 0; tt < 2; ++tt)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int m = m0 + 32 * tt + (reg & 3) + 8 * (reg >> 2) + 4 * h;
      int *p = part + (((size_t)z * Bpad + m) * KSM_COLS + col) * KSM_LIMBS;
#pragma unroll
      for (int l = 0; l < KSM_LIMBS; ++l) p[l] = acc[tt][l][reg];
    }
}

// Sum of the slices and ks_mfma_kernel's epilogue: one thread per (message, output column).
__global__ void ks_combine_kernel(const int *__restrict__ part, const uint32_t *__restrict__ lwe1t,
                                  uint32_t *__restrict__ lwe_int, int B, int Bpad) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * (NI + 1)) return;
  const int m = idx / (NI + 1), col = idx % (NI + 1);
  int64_t limb[KSM_LIMBS] = {0, 0, 0, 0};
  for (int z = 0; z < KS_SPLIT; ++z) {
    const int *p = part + (((size_t)z * Bpad + m) * KSM_COLS + col) * KSM_LIMBS;
#pragma unroll
    for (int l = 0; l < KSM_LIMBS; ++l) limb[l] += p[l];
  }
  const uint64_t sum = (uint64_t)limb[0] + ((uint64_t)limb[1] << 7) + ((uint64_t)limb[2] << 14) +
                       ((uint64_t)limb[3] << 21);
  lwe_int[(size_t)m * (NI + 1) + col] = ks_epilogue(sum, lwe1t[(size_t)N1 * B + m], col);
}

}  // namespace omr
