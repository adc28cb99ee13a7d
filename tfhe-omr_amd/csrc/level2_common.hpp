// What every level-2 kernel family shares (br2_ntt.hpp: the modular NTT; br2_fft.hpp: the exact
// FFT): the gadget and trace digit words, rotated LDS reads, a GGSW key row, the initial
// accumulator and the trace's N^-1.
#pragma once

#include "kernels.hpp"

namespace omr {

constexpr double NINV2 = -549755813880.0;  // 2048^-1 mod q2 = 1125350151012361, centred (secret.rs:167-168)

// Coefficient c of the initial body accumulator X^{-b} * LUT2 (the mask starts at 0), canonical.
__device__ __forceinline__ double acc2_init(const double *lut2, int b, int c) {
  const int rr = (2 * N2 - (b % (2 * N2))) % (2 * N2);
  return canon_small<Mod<2>>(rot_read<N2>(lut2, c, rr));
}

// Level-2 gadget digits (logB 7, d 6, drop 8) in closed form: y = floor((v + 2^7) / 2^8) has
// balanced base-128 digits d_k in [-64, 63] (k < 5) and a top digit d_5 in [-64, 64]; with the
// bias 64 (1 + 128 + ... + 128^5), y' = y + bias is exact in FP64 (0 <= y' < 2^43) and splits
// exactly into lo = y' mod 2^21 (fields 0-2) and hi = floor(y' / 2^21) (fields 3-5). Field k holds
// d_k + 64: 7 bits at 7 (k mod 3) in word k / 3, the top field 8 bits (bit 21 of lo is zero, so
// the (offset, width) of field j of either word is (7 j, j == 2 ? 8 : 7)). Same digits as the
// recursive NonPowOf2ApproxSignedBasis decomposition of the oracle (gadget convention in
// include/omr_gpu.h; tests/test_digit_forms.py checks every boundary).
struct Digits2 {
  static constexpr int DW = 2;
  static_assert(LOGB2 == 7 && D2 == 6 && DROP2 == 8, "closed form written for the level-2 basis");
  __device__ static __forceinline__ void pack(double v, uint32_t (&pk)[DW]) {
    const double y = floor(__fma_rn(v, 1.0 / 256.0, 0.5)) + 2216338399296.0;  // + 17315143744 + 64 * 2^35
    const double hi = floor(y * (1.0 / 2097152.0));
    const double lo = __fma_rn(-hi, 2097152.0, y);
    pk[0] = (uint32_t)(int)lo;
    pk[1] = (uint32_t)(int)hi;
  }
  // d_{j + 3 h} + 64 (the word is chosen at compile time, the offset may be a run-time uniform)
  template <int H>
  __device__ static __forceinline__ int field(const uint32_t (&pk)[DW], int j) {
    return (int)__builtin_amdgcn_ubfe(pk[H], 7 * j, j == 2 ? 8 : 7);
  }
  __device__ static __forceinline__ int get_int(const uint32_t (&pk)[DW], int k) {
    return (k < 3 ? field<0>(pk, k) : field<1>(pk, k - 3)) - 64;
  }
};
// Trace basis (q2, 2, None): 25 balanced base-4 digits (24 in [-2, 1], the top one in [-2, 3]).
struct DigitsTrace {
  static constexpr int DW = 2;
  static_assert(DT == 25, "closed form written for the trace basis");
  // Closed form of the recursive balanced base-4 decomposition (d = y - 4 floor(y / 4 + 1/2), 24
  // times, then the rest; round 5): y' = v + 2 (1 + 4 + ... + 4^23) has field k (bits 2k, 2k + 1)
  // = d_k + 2 for k < 24 and y' >> 48 = d_24. Y = y' + 1.5 * 2^52 is exact (|v| < 2^49) and the low
  // 51 bits of its mantissa are y' in two's complement, so the words are Y's two dwords, each field
  // XORed with 2 (a two's-complement 2-bit digit: one v_bfe_i32): 1 FP64 add and 2 XORs per
  // coefficient instead of 24 floor / fma / conversion rounds (tests/test_lvl1_offset_model.py).
  __device__ static __forceinline__ void pack(double v, uint32_t (&pk)[DW]) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v + (187649984473770.0 + 6755399441055744.0));
    pk[0] = (uint32_t)b ^ 0xAAAAAAAAu;      // digits 0..15
    pk[1] = (uint32_t)(b >> 32) ^ 0xAAAAu;  // digits 16..23 in bits 0..15, d_24 in bits 16..18
  }
  __device__ static __forceinline__ int get_int(const uint32_t (&pk)[DW], int k) {
    const uint32_t w = k < 16 ? pk[0] : pk[1];
    return (int)__builtin_amdgcn_sbfe(w, k < 16 ? 2 * k : 2 * (k - 16), k == DT - 1 ? 3 : 2);
  }
  __device__ static __forceinline__ double get(const uint32_t (&pk)[DW], int k) { return (double)get_int(pk, k); }
};

// (X^r * p)[j] for p in LDS as t = (j - r) mod 2N: p[t] for t < N, -p[t - N] above (the sign
// flipped by one xor of bit 63 instead of compare/select pairs and a multiply).
template <int N>
__device__ __forceinline__ double rot_read_lds(const double *p, int j, int r) {
  static_assert((N & (N - 1)) == 0 && N <= (1 << 20), "power-of-two ring degree");
  const uint32_t t = (uint32_t)(j - r) & (2 * N - 1);
  const double v = p[t & (N - 1)];
  const uint32_t hi = (uint32_t)(__builtin_bit_cast(uint64_t, v) >> 32) ^ ((t & N) << (31 - ilog2(N)));
  return __builtin_bit_cast(double, (__builtin_bit_cast(uint64_t, v) & 0xffffffffull) | ((uint64_t)hi << 32));
}

// One key row of the level-2 GGSW (NTT domain, [2][N]: A and B components), E residues per thread.
template <typename KeyT, int E>
struct KeyRow {
  KeyT a[E], b[E];
  __device__ __forceinline__ void load(const KeyT *__restrict__ row, int N, int off) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      a[e] = row[off + e];
      b[e] = row[N + off + e];
    }
  }
};

}  // namespace omr
