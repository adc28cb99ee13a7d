// Shared constants and small host/device helpers for libomr_gpu.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/omr_gpu.h"

#define OMR_HD __host__ __device__ __forceinline__

namespace omr {

// Parameter set (omr_core/src/parameters/mod.rs:39-105).
constexpr int N0 = OMR_N0;           // clue LWE dimension
constexpr int Q0 = OMR_Q0;           // clue modulus
constexpr int CLUES = OMR_CLUE_COUNT;
constexpr uint64_t Q1 = OMR_Q1;      // FirstLevelField
constexpr int N1 = OMR_N1;
constexpr int LOGB1 = 5, D1 = 4, DROP1 = 7;
constexpr int KS_DIGITS = OMR_KS_DIGITS;
constexpr int NI = OMR_NI;
constexpr int QI = OMR_QI, TI = 32;
constexpr uint64_t Q2 = OMR_Q2;      // SecondLevelField
constexpr int N2 = OMR_N2;
constexpr int LOGB2 = 7, D2 = 6, DROP2 = 8;
constexpr int LOGBT = 2, DT = OMR_TRACE_DIGITS, TRACE_STEPS = OMR_TRACE_STEPS;
constexpr int P = OMR_P;
constexpr int PAYLOAD_LEN = OMR_PAYLOAD_LEN;
constexpr int BUCKETS = 130;         // key_gen/secret.rs:189-209
constexpr int SEGMENTS = 25;

// Noise standard deviations (parameters/mod.rs).
constexpr double SIGMA_CLUE = 0.8293;
constexpr double SIGMA_BR1 = 3.1859;
constexpr double SIGMA_KS = 2.0329 * 1024.0;
constexpr double SIGMA_BR2 = 0.3908;
constexpr double SIGMA_TRACE = 0.3908;

// Key sizes (elements) in the boundary layout of include/omr_gpu.h.
constexpr size_t BSK1_ELEMS = (size_t)N0 * 2 * D1 * 2 * N1;
constexpr size_t KSK_ELEMS = (size_t)N1 * KS_DIGITS * (NI + 1);
constexpr size_t BSK2_ELEMS = (size_t)NI * 2 * D2 * 2 * N2;
constexpr size_t TK_ELEMS = (size_t)TRACE_STEPS * DT * 2 * N2;

// ChaCha block (djb layout: 64-bit counter in words 12-13, 64-bit stream id in 14-15).
OMR_HD uint32_t rotl32(uint32_t v, int n) { return (v << n) | (v >> (32 - n)); }
OMR_HD void chacha_block(int rounds, const uint32_t key[8], uint64_t counter, uint64_t stream,
                         uint32_t out[16]) {
  uint32_t in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1],
                     key[2],      key[3],      key[4],      key[5],      key[6], key[7],
                     (uint32_t)counter, (uint32_t)(counter >> 32), (uint32_t)stream,
                     (uint32_t)(stream >> 32)};
  uint32_t x[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = in[i];
#define OMR_QR(a, b, c, d)                                                                   \
  x[a] += x[b]; x[d] = rotl32(x[d] ^ x[a], 16); x[c] += x[d]; x[b] = rotl32(x[b] ^ x[c], 12); \
  x[a] += x[b]; x[d] = rotl32(x[d] ^ x[a], 8);  x[c] += x[d]; x[b] = rotl32(x[b] ^ x[c], 7);
  for (int r = 0; r < rounds; r += 2) {
    OMR_QR(0, 4, 8, 12) OMR_QR(1, 5, 9, 13) OMR_QR(2, 6, 10, 14) OMR_QR(3, 7, 11, 15)
    OMR_QR(0, 5, 10, 15) OMR_QR(1, 6, 11, 12) OMR_QR(2, 7, 8, 13) OMR_QR(3, 4, 9, 14)
  }
#undef OMR_QR
#pragma unroll
  for (int i = 0; i < 16; ++i) out[i] = x[i] + in[i];
}

// Bucket choice for encode_pertinent_indices: ChaCha12 keyed by (seed, ct), block counter = the
// global message index, word s = segment. Replaces thread_rng + Uniform(0,130) (detector.rs:262,278)
// with a stream every shard can evaluate independently.
OMR_HD void bucket_words(uint64_t seed, uint32_t ct, uint64_t gi, uint32_t out[16]) {
  const uint32_t key[8] = {(uint32_t)seed, (uint32_t)(seed >> 32), 0x6f6d7262u, ct, 0, 0, 0, 0};
  chacha_block(12, key, gi, 0x62756b74u, out);
}
OMR_HD uint32_t bucket_of(uint32_t word) { return (uint32_t)(((uint64_t)word * BUCKETS) >> 32); }

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

// Error reporting (thread-local message behind omr_last_error()).
omr_status set_error(omr_status st, const std::string &msg);

// The messages [offset, offset + D) lie on a board of `all`: no sum that could wrap.
inline bool range_on_board(size_t offset, size_t D, size_t all) { return offset <= all && D <= all - offset; }

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

}  // namespace omr
