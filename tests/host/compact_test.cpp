// Stand-alone host test of csrc/compact_math.hpp (include/omr_gpu.h, "Compact ciphertexts"), meant for a
// build under the address and undefined-behaviour sanitizers (make build/compact_test; plain C++, no GPU):
// the FP64-estimate rescale the kernel uses against the 128-bit definition, the two-halves unscale
// against a 128-bit product, and the word form of the bit stream against the byte form, for every width,
// with exactly sized buffers so that an overrun of any of them is the sanitizer's to find.
#include <cstdio>
#include <cstring>
#include <vector>

#include "compact_math.hpp"

using namespace omr;

namespace {

typedef unsigned __int128 u128;
int fails = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++fails;                                                        \
    }                                                                 \
  } while (0)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t next() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the smallest x that rounds to y: ceil((2 q2 y - q2) / (2 Q)), for y >= 1
uint64_t step_at(uint64_t y, int bits) {
  const u128 num = (u128)2 * COMPACT_Q2 * y - COMPACT_Q2, den = (u128)2 << bits;
  return (uint64_t)((num + den - 1) / den);
}

void check_rescale(uint64_t x, int bits) {
  if (x >= COMPACT_Q2) return;
  const uint32_t want = compact_rescale_wide(x, bits), got = compact_rescale(x, bits);
  if (want != got) std::fprintf(stderr, "rescale x=%llu bits=%d: %u != %u\n", (unsigned long long)x, bits, got, want);
  EXPECT(want == got);
}

}  // namespace

int main() {
  for (int bits = COMPACT_MIN_BITS; bits <= COMPACT_MAX_BITS; ++bits) {
    const uint64_t Q = (uint64_t)1 << bits;
    EXPECT(compact_bits_ok(bits) && compact_ct_bytes(bits) == 2 * (size_t)compact_poly_words(bits) * 4);
    // rescale: the ends, every rounding step near the ends and the middle, random steps, random values
    EXPECT(compact_rescale(0, bits) == 0 && compact_rescale(COMPACT_Q2 - 1, bits) == 0);
    for (uint64_t x : {(uint64_t)0, (uint64_t)1, COMPACT_Q2 / 2, COMPACT_Q2 / 2 + 1, COMPACT_Q2 - 2, COMPACT_Q2 - 1})
      check_rescale(x, bits);
    std::vector<uint64_t> ys = {1, 2, 3, Q / 2 - 1, Q / 2, Q / 2 + 1, Q - 2, Q - 1, Q};
    for (int k = 0; k < 2000; ++k) ys.push_back(1 + next() % Q);
    for (uint64_t y : ys) {
      const uint64_t x = step_at(y, bits);
      for (int d = -2; d <= 2; ++d) check_rescale(x + (uint64_t)(int64_t)d, bits);
      if (x < COMPACT_Q2) EXPECT(compact_rescale_wide(x, bits) == (y & (Q - 1)) && compact_rescale_wide(x - 1, bits) == y - 1);
    }
    for (int k = 0; k < 20000; ++k) check_rescale(next() % COMPACT_Q2, bits);
    // unscale: against the 128-bit product, in range, and a fixed point of rescale
    std::vector<uint64_t> vs = {0, 1, Q / 2, Q - 1};
    for (int k = 0; k < 5000; ++k) vs.push_back(next() % Q);
    for (uint64_t y : vs) {
      const uint64_t want = (uint64_t)(((u128)y * COMPACT_Q2 + Q / 2) >> bits), got = compact_unscale((uint32_t)y, bits);
      EXPECT(want == got && got < COMPACT_Q2);
      EXPECT(compact_rescale(got, bits) == y);
    }
    // the multiply-high division over every stream position
    for (int k = 0; k < 32 * compact_poly_words(bits) + 32; ++k) EXPECT(compact_div(k, compact_magic(bits)) == k / bits);
    // the stream: words against bytes, both directions, on exactly sized buffers
    std::vector<uint32_t> v(COMPACT_N), back(COMPACT_N), words(compact_poly_words(bits));
    std::vector<uint8_t> bytes((size_t)compact_poly_words(bits) * 4);
    for (int pattern = 0; pattern < 3; ++pattern) {
      for (int i = 0; i < COMPACT_N; ++i)
        v[i] = pattern == 0 ? (uint32_t)(Q - 1) : pattern == 1 ? (uint32_t)(i & 1 ? Q - 1 : 0) : (uint32_t)(next() % Q);
      compact_pack_bytes(v.data(), bits, bytes.data());
      for (int w = 0; w < compact_poly_words(bits); ++w) words[w] = compact_stream_word(v, w, bits, compact_magic(bits));
      for (size_t k = 0; k < bytes.size(); ++k) EXPECT(bytes[k] == (uint8_t)(words[k / 4] >> (8 * (k % 4))));
      compact_unpack_bytes(bytes.data(), bits, back.data());
      EXPECT(back == v);
      for (int i = 0; i < COMPACT_N; ++i) EXPECT(compact_stream_value(words, i, bits) == v[i]);
    }
  }
  EXPECT(!compact_bits_ok(15) && !compact_bits_ok(33) && !compact_bits_ok(0) && !compact_bits_ok(-1));
  std::printf(fails ? "FAILED (%d)\n" : "compact_test: ok\n", fails);
  return fails ? 1 : 0;
}
