// Stand-alone host test of the payload length as a board parameter (include/omr_gpu.h): omr_get_payload_layout
// (csrc/weights.hip) and the host gather of a retrieval's right-hand side (csrc/retrieve_system.hpp,
// gather_rhs_host over weights.hpp's payload_word_at), meant for a build with csrc/weights.hip and csrc/keygen.hip
// under the address and undefined-behaviour sanitizers (make build/payload_len_test; no GPU is touched). The
// decoded ciphertexts and the right-hand side live in exactly sized heap buffers, so a read one word past the
// last ciphertext or a write one word past the last row is an error under the sanitizer. The expectation walks
// the layout the other way round, from (ciphertext, slot) to (combination, word), in the header's words.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "omr_gpu.h"
#include "retrieve_system.hpp"

namespace {

int fails = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++fails;                                                        \
    }                                                                 \
  } while (0)

const uint32_t LENGTHS[] = {1, 2, 127, 128, 129, 612, 682, 683, 1024, 1025, 2048, 2049, 4096, 4097, 16384};

void check_layout(uint32_t L, size_t pertinent) {
  omr_payload_layout ly{};
  EXPECT(omr_get_payload_layout(pertinent, L, &ly) == OMR_OK);
  const uint32_t stripes = (L + 2047) / 2048;
  uint32_t per = 1;
  if (L <= 2048) per = 2048 / L < 16 ? 2048 / L : 16;
  const uint32_t cc = (uint32_t)pertinent + 5, groups = (cc + per - 1) / per;
  EXPECT(ly.payload_len == L && ly.combination_count == cc && ly.cmb_count_per_cipher == per);
  EXPECT(ly.stripes == stripes && ly.payload_ct == groups * stripes && stripes <= 8);
}

// rows combinations of L words at `per` per group: every (ciphertext, slot) that holds a word is read exactly once.
void check_gather(uint32_t L, uint32_t per, uint32_t rows) {
  const uint32_t stripes = (L + 2047) / 2048, groups = (rows + per - 1) / per, n_ct = groups * stripes;
  std::vector<uint16_t> dec((size_t)n_ct * 2048);
  for (size_t i = 0; i < dec.size(); ++i) dec[i] = (uint16_t)((i * 40503u + 12345u) >> 3);
  omr::PayloadSystem sys;
  sys.rows = rows, sys.cols = 1, sys.per = per, sys.len = L, sys.stripes = stripes;
  std::vector<uint16_t> rhs((size_t)rows * L, 0xABCD);
  omr::gather_rhs_host(dec.data(), sys, rhs.data());
  size_t seen = 0;
  bool ok = true;
  for (uint32_t c = 0; c < n_ct; ++c) {
    const uint32_t s = c % stripes, group = c / stripes;
    for (uint32_t i = 0; i < 2048; ++i) {
      uint32_t j, l;
      if (stripes == 1) {
        if (i / L >= per) continue;
        j = group * per + i / L, l = i % L;
      } else {
        j = group, l = 2048 * s + i;
        if (l >= L) continue;
      }
      if (j >= rows) continue;  // a padding combination
      ok = ok && rhs[(size_t)j * L + l] == dec[(size_t)c * 2048 + i];
      ++seen;
    }
  }
  EXPECT(ok);
  EXPECT(seen == (size_t)rows * L);
}

}  // namespace

int main() {
  for (uint32_t L : LENGTHS)
    for (size_t pertinent : {(size_t)0, (size_t)3, (size_t)50, (size_t)8187}) check_layout(L, pertinent);
  omr_payload_layout ly{};
  EXPECT(omr_get_payload_layout(3, 0, &ly) == OMR_ERR_INVALID_ARGUMENT);
  EXPECT(omr_get_payload_layout(3, OMR_PAYLOAD_LEN_MAX + 1, &ly) == OMR_ERR_INVALID_ARGUMENT);
  EXPECT(omr_get_payload_layout(3, 612, nullptr) == OMR_ERR_INVALID_ARGUMENT);
  EXPECT(omr_get_payload_layout((size_t)UINT32_MAX - 4, 612, &ly) == OMR_ERR_INVALID_ARGUMENT);
  EXPECT(omr_get_payload_layout((size_t)UINT32_MAX - 5, 16384, &ly) == OMR_ERR_INVALID_ARGUMENT);  // 2^35 ciphertexts
  EXPECT(omr_get_payload_layout((size_t)UINT32_MAX - 5, 1, &ly) == OMR_OK && ly.payload_ct == 1u << 28);
  for (uint32_t L : LENGTHS) {
    const uint32_t per = omr::payload_per_max(L);
    for (uint32_t rows : {1u, 8u, 17u}) {
      check_gather(L, per, rows);
      if (per > 1) check_gather(L, 1, rows), check_gather(L, per - 1, rows);
    }
  }
  if (fails) {
    std::fprintf(stderr, "%d failures\n", fails);
    return 1;
  }
  std::puts("payload length host test OK");
  return 0;
}
