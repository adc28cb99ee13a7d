// The payload-weight statement shared by the host weight functions (weights.hip), the encode kernels
// (encode_kernels.hpp), the auditor's matrix kernels (solve_kernels.hpp) and PayloadWeights (ctx.hpp):
// indexed weights, the reference's weights by seek, and the one rule by which a consumer takes or builds a
// seek. Only the units that use weights include this.
#pragma once

#include <functional>
#include <string>

#include "common.hpp"

namespace omr {

// Indexed payload weights (include/omr_gpu.h, "Indexed payload weights": none in the reference): weight
// (j, g) is word g & 15 of the ChaCha12 block with counter g >> 4 and stream id "payw" << 32 | j, scaled
// to [0, 256] without a rejection step, so that any party evaluates any weight on its own. The key is
// the 32-byte weight seed as eight little-endian words, passed to kernels by value.
struct WeightKey {
  uint32_t k[8];
};
inline WeightKey weight_key(const uint8_t seed[32]) {
  WeightKey key;
  for (int i = 0; i < 8; ++i)
    key.k[i] = (uint32_t)seed[4 * i] | ((uint32_t)seed[4 * i + 1] << 8) | ((uint32_t)seed[4 * i + 2] << 16) |
               ((uint32_t)seed[4 * i + 3] << 24);
  return key;
}
constexpr uint64_t PAYW_STREAM = 0x70617977ull << 32;
// The 16 weights of combination j for the messages 16 block .. 16 block + 15.
OMR_HD void indexed_weight_block(const WeightKey &key, uint32_t j, uint64_t block, uint16_t out[16]) {
  uint32_t w[16];
  chacha_block(12, key.k, block, PAYW_STREAM | j, w);
#pragma unroll
  for (int i = 0; i < 16; ++i) out[i] = (uint16_t)(((uint64_t)w[i] * (uint64_t)P) >> 32);
}

// Payload length as a board parameter (include/omr_gpu.h): a payload of L words, 1 <= L <= OMR_PAYLOAD_LEN_MAX,
// takes payload_stripes(L) ciphertexts per group of at most payload_per_max(L) combinations. The layout
// function, the encode entry, the session and both retrievals share these.
inline bool payload_len_ok(size_t L) { return L >= 1 && L <= OMR_PAYLOAD_LEN_MAX; }
OMR_HD uint32_t payload_stripes(uint32_t L) { return (L + N2 - 1) / N2; }
OMR_HD uint32_t payload_per_max(uint32_t L) {
  if (L > (uint32_t)N2) return 1;
  const uint32_t fit = (uint32_t)N2 / L;
  return fit < OMR_PAYLOAD_PER_CT_MAX ? fit : OMR_PAYLOAD_PER_CT_MAX;
}
// Where word l < L of combination j lies among the decoded payload ciphertexts u16 [n_ct][N2]: group j / per,
// stripe l / N2; within a one-stripe ciphertext combination j % per starts at slot (j % per) * L (several
// stripes have per = 1, so that term is 0).
OMR_HD size_t payload_word_at(uint32_t j, uint32_t l, uint32_t L, uint32_t per, uint32_t stripes) {
  return ((size_t)(j / per) * stripes + l / (uint32_t)N2) * N2 + (size_t)(j % per) * L + l % (uint32_t)N2;
}

// Reference payload weights by seek (include/omr_gpu.h, "Reference payload weights by seek"): the
// statement that the builders, omr_payload_weights_at, the seek encode kernel and the auditor's matrix
// kernel share. The stream is omr_payload_weights': ChaCha12, stream id 0, raw position r = word r & 15
// of block r >> 4; Uniform<u16>(0, 257) rejects a word when the low half of word * 257 exceeds the zone.
OMR_HD bool weight_rejected(uint32_t word, uint32_t zone) { return (uint32_t)(word * (uint32_t)P) > zone; }
OMR_HD uint16_t weight_of_word(uint32_t word) { return (uint16_t)(((uint64_t)word * (uint64_t)P) >> 32); }
// pos(n): the raw position of accepted draw n < seek.draws.
OMR_HD uint64_t seek_pos(const omr_weight_seek &seek, uint64_t n) {
  uint64_t p = n;
  for (uint32_t k = 0; k < seek.n; ++k) p += seek.at[k] <= n ? 1 : 0;
  return p;
}
// The inverse: raw position r holds accepted draw *draw (true), or is a listed rejection (false). Raw
// positions beyond pos(seek.draws - 1) map to draws >= seek.draws, whatever lies there.
OMR_HD bool seek_draw_at(const omr_weight_seek &seek, uint64_t r, uint64_t *draw) {
  uint64_t below = 0;
  bool listed = false;
  for (uint32_t k = 0; k < seek.n; ++k) {
    const uint64_t rk = seek.at[k] + k;
    below += rk < r ? 1 : 0;
    listed = listed || rk == r;
  }
  *draw = r - below;
  return !listed;
}
// What every consumer checks before it uses a caller's seek for a board of combos x all weights.
inline bool seek_covers(const omr_weight_seek *seek, uint64_t combos, uint64_t all) {
  return seek && seek->n <= OMR_WEIGHT_SEEK_MAX && (all == 0 || combos <= seek->draws / all);
}
// Rejections a builder keeps: among the raw words [0, draws + OMR_WEIGHT_SEEK_MAX], T rejections r_0 < ..
// < r_(T-1) have r_k <= draws + 32 - (T - 1 - k), so at[k] <= draws + 33 - T. With T >= 34 every one of
// them matters (at[k] < draws) and the stream is over the cap; up to 33 the list holds them all.
constexpr uint32_t SEEK_LIST = OMR_WEIGHT_SEEK_MAX + 1;
constexpr uint64_t SEEK_MAX_DRAWS = 1ull << 62;
// The builders' common end: the smallest min(total, SEEK_LIST) rejected raw positions, in any order, to *out.
inline omr_status seek_from_hits(uint64_t *hits, uint64_t total, uint64_t draws, uint32_t zone, omr_weight_seek *out,
                                 const char *who) {
  const std::string over = std::string(who) + ": more than 32 rejections: use the table";
  if (total > SEEK_LIST) return set_error(OMR_ERR_INVALID_ARGUMENT, over);
  for (uint64_t i = 1; i < total; ++i)  // at most 33 entries: insertion sort
    for (uint64_t k = i; k > 0 && hits[k - 1] > hits[k]; --k) {
      const uint64_t t = hits[k];
      hits[k] = hits[k - 1];
      hits[k - 1] = t;
    }
  omr_weight_seek s{};
  s.draws = draws;
  s.zone = zone;
  for (uint64_t k = 0; k < total; ++k) {
    const uint64_t at = hits[k] - k;
    if (at >= draws) break;  // at[] is nondecreasing: the rejections that matter are a prefix
    if (s.n == OMR_WEIGHT_SEEK_MAX) return set_error(OMR_ERR_INVALID_ARGUMENT, over);
    s.at[s.n++] = at;
  }
  *out = s;
  return OMR_OK;
}

// weights.hip. The seek of a board of rows x all reference weights, for every consumer that accepts a NULL
// seek: the caller's if it covers the board, else one from `build` (the CPU or the device builder, given the
// seed and the draws) unless the board is too large for any seek.
using SeekBuilder = std::function<omr_status(const uint8_t seed[32], uint64_t draws, omr_weight_seek *out)>;
omr_status resolve_seek(const uint8_t seed[32], const omr_weight_seek *seek, uint64_t rows, uint64_t all,
                        const std::string &who, const SeekBuilder &build, omr_weight_seek *out);

}  // namespace omr
