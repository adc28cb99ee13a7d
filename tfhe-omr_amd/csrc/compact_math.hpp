// Compact ciphertexts (include/omr_gpu.h, "Compact ciphertexts"): the per-value arithmetic and the bit
// stream, in exact integers. Shared by the CPU statement (compact.hip, omr_compact_cts_cpu /
// omr_compact_expand_cpu), the device kernels (compact_kernels.hpp) and the stand-alone host test
// (tests/host/compact_test.cpp). Needs nothing but <cstdint>: no HIP header, so that the host test builds
// with a plain C++ compiler.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define OMR_CHD __host__ __device__ inline __attribute__((always_inline))
#else
#define OMR_CHD inline
#endif

namespace omr {

constexpr int COMPACT_MIN_BITS = 16, COMPACT_MAX_BITS = 32;
constexpr uint64_t COMPACT_Q2 = 1125899906826241ull;  // OMR_Q2
constexpr int COMPACT_N = 2048;                       // OMR_N2
// the same figure as the device's Mod<2>::Q, for the quotient estimate
constexpr double COMPACT_Q2_F = 1125899906826241.0;

OMR_CHD bool compact_bits_ok(int bits) { return bits >= COMPACT_MIN_BITS && bits <= COMPACT_MAX_BITS; }
// bytes of one compact ciphertext: 2 polynomials x 2048 values x bits / 8
OMR_CHD size_t compact_ct_bytes(int bits) { return (size_t)512 * (size_t)bits; }
// 32-bit words of one packed polynomial
OMR_CHD int compact_poly_words(int bits) { return 64 * bits; }

// y = floor((2 x Q + q2) / (2 q2)) mod Q for x in [0, q2), Q = 2^bits, without a division.
// The FP64 estimate e = floor(x (1 / q2) Q + 1/2) is within one of y: x is an exact double, the rounded
// reciprocal and the product err by 2^-53 relative each, scaling by Q is exact (a power of two), so the
// estimate is off by under 2^-20 for a quotient below 2^32, and adding 1/2 rounds once more by as
// little. The difference
//   d = 2 x Q + q2 - 2 q2 e
// then lies in (-2 q2, 4 q2), far inside 64 signed bits, so computing it in wrapping 64-bit arithmetic
// gives it exactly although 2 x Q alone may need 83 bits; y is the e with 0 <= d < 2 q2.
OMR_CHD uint32_t compact_rescale(uint64_t x, int bits) {
  const double qf = (double)((uint64_t)1 << bits);
  uint64_t e = (uint64_t)((double)x * (1.0 / COMPACT_Q2_F) * qf + 0.5);
  int64_t d = (int64_t)((x << (bits + 1)) + COMPACT_Q2 - 2 * COMPACT_Q2 * e);
  if (d < 0) {
    --e;
    d += (int64_t)(2 * COMPACT_Q2);
  }
  if (d >= (int64_t)(2 * COMPACT_Q2)) ++e;
  return (uint32_t)(e & (((uint64_t)1 << bits) - 1));  // x close to q2 rounds to Q and wraps to 0
}

// The definition itself, with a 128-bit quotient (host only): the CPU statement uses this one.
inline uint32_t compact_rescale_wide(uint64_t x, int bits) {
  typedef unsigned __int128 wide;
  const wide y = ((((wide)x << 1) << bits) + COMPACT_Q2) / ((wide)2 * COMPACT_Q2);
  return (uint32_t)((uint64_t)y & (((uint64_t)1 << bits) - 1));
}

// x' = (y q2 + Q / 2) >> bits for y in [0, Q): the 82-bit product in two halves of q2. With
// q2 = qh 2^32 + ql the product is (y qh) 2^32 + y ql, y ql < 2^64 and y qh < 2^50; the high part is a
// multiple of 2^bits (bits <= 32), so the shift applies to the halves separately. x' < q2.
OMR_CHD uint64_t compact_unscale(uint32_t y, int bits) {
  const uint64_t ql = COMPACT_Q2 & 0xFFFFFFFFull, qh = COMPACT_Q2 >> 32;
  uint64_t hi = (uint64_t)y * qh;
  const uint64_t lo = (uint64_t)y * ql, lo2 = lo + ((uint64_t)1 << (bits - 1));
  if (lo2 < lo) hi += (uint64_t)1 << 32;  // the carry out of the low half is worth 2^64
  return (hi << (32 - bits)) + (lo2 >> bits);
}

// 32-bit word w of the stream of values v[0..2048): stream bits [32 w, 32 w + 32), value i at stream
// bits [i bits, (i + 1) bits). With 16 <= bits <= 32 a word meets at most three values. `v` is any
// indexable holder of values below 2^bits (an array on the host, LDS on the device).
// Positions are divided by `bits` with a multiply-high: for M = floor(2^32 / bits) + 1 (compact_magic,
// computed once on the host), k M / 2^32 exceeds k / bits by less than k / 2^32, which cannot reach the
// next multiple of 1 / bits while k < 2^27; stream positions are below 2^17.
OMR_CHD uint32_t compact_magic(int bits) { return (uint32_t)(((uint64_t)1 << 32) / (uint32_t)bits) + 1; }
OMR_CHD int compact_div(int k, uint32_t magic) { return (int)(((uint64_t)(uint32_t)k * magic) >> 32); }
template <class V>
OMR_CHD uint32_t compact_stream_word(const V &v, int w, int bits, uint32_t magic) {
  const int lo = 32 * w, first = compact_div(lo, magic), last = compact_div(lo + 31, magic);
  uint32_t word = 0;
  for (int i = first; i <= last; ++i) {
    const int s = i * bits - lo;  // in (-32, 32)
    const uint32_t val = v[i];
    word |= s >= 0 ? val << s : val >> -s;
  }
  return word;
}

// value i of a stream of 32-bit words (the inverse of compact_stream_word); a value that ends at a word
// boundary does not touch the next word, so the last value reads nothing beyond the stream
template <class W>
OMR_CHD uint32_t compact_stream_value(const W &words, int i, int bits) {
  const int k = i * bits, w = k >> 5, s = k & 31;
  uint64_t two = words[w];
  if (s + bits > 32) two |= (uint64_t)words[w + 1] << 32;
  return (uint32_t)((two >> s) & (((uint64_t)1 << bits) - 1));
}

// Host bit stream of one polynomial, byte by byte as the header states it (stream bit k is bit k mod 8 of
// byte k / 8): written without reference to the word form above, which the host test checks against it.
inline void compact_pack_bytes(const uint32_t *v, int bits, uint8_t *out) {
  const size_t nbytes = (size_t)COMPACT_N * bits / 8;
  for (size_t k = 0; k < nbytes; ++k) out[k] = 0;
  for (int i = 0; i < COMPACT_N; ++i)
    for (int b = 0; b < bits; ++b) {
      const size_t k = (size_t)i * bits + b;
      out[k >> 3] |= (uint8_t)(((v[i] >> b) & 1u) << (k & 7));
    }
}
inline void compact_unpack_bytes(const uint8_t *in, int bits, uint32_t *v) {
  for (int i = 0; i < COMPACT_N; ++i) {
    uint32_t val = 0;
    for (int b = 0; b < bits; ++b) {
      const size_t k = (size_t)i * bits + b;
      val |= (uint32_t)((in[k >> 3] >> (k & 7)) & 1u) << b;
    }
    v[i] = val;
  }
}

}  // namespace omr
