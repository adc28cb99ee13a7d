// Payload weights and the digest layout on the host (CPU; no HIP runtime call): the retrieval parameters,
// the seeded weight stream of Detector::encode_pertinent_payloads (detector.rs:376-387) as a table, the
// indexed weights and the reference's weights by seek (weights.hpp's statement, which the kernels share), the
// CPU seek builder, and the one rule by which a consumer takes or builds a seek.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "host_ring.hpp"
#include "weights.hpp"

using namespace omr;

extern "C" omr_status omr_get_retrieval_params(size_t all, size_t pertinent,
                                               omr_retrieval_params *rp) {
  if (!rp || all == 0) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_get_retrieval_params");
  uint32_t pw = 0;
  uint64_t acc = 1;
  // acc * p <= all without the product: 257^7 * 257 wraps to 257^8 - 2^64 = 5.8e17, and a board of that size or
  // more counted a ninth digit and on (for the largest size_t the loop never ended)
  while (acc <= all / (uint64_t)P) {
    acc *= (uint64_t)P;
    ++pw;
  }
  if (acc < all) ++pw;
  if (pw == 0) pw = 1;
  rp->index_slots_per_bucket = pw;
  rp->slots_per_bucket = pw + 1;
  rp->slots_per_segment = rp->slots_per_bucket * BUCKETS;
  rp->segment_per_cipher = N2 / rp->slots_per_segment;
  rp->max_encode_indices_cipher_count = SEGMENTS / rp->segment_per_cipher;
  rp->combination_count = (uint32_t)pertinent + 5;  // non-power-of-two p (retrieval_params.rs:85-89)
  rp->cmb_count_per_cipher = 2;
  rp->cmb_cipher_count = (rp->combination_count + 1) / 2;
  return OMR_OK;
}

extern "C" omr_status omr_get_payload_layout(size_t pertinent, size_t payload_len, omr_payload_layout *ly) {
  if (!ly || !payload_len_ok(payload_len) || pertinent > (size_t)UINT32_MAX - 5)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_get_payload_layout: NULL, or a length or count out of range");
  const uint32_t L = (uint32_t)payload_len;
  ly->payload_len = L;
  ly->combination_count = (uint32_t)pertinent + 5;  // as omr_get_retrieval_params
  ly->cmb_count_per_cipher = payload_per_max(L);
  ly->stripes = payload_stripes(L);
  const uint64_t groups = ((uint64_t)ly->combination_count + ly->cmb_count_per_cipher - 1) / ly->cmb_count_per_cipher;
  if (groups * ly->stripes > UINT32_MAX)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_get_payload_layout: more than 2^32 payload ciphertexts");
  ly->payload_ct = (uint32_t)(groups * ly->stripes);
  return OMR_OK;
}

extern "C" omr_status omr_payload_weights(const uint8_t seed[32], size_t all, uint32_t combos,
                                          uint32_t n_ct, uint32_t per_ct, uint16_t *out) {
  if (!seed || !out || (size_t)n_ct * per_ct < combos)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_payload_weights");
  const WeightKey key = weight_key(seed);
  const size_t count = (size_t)combos * all;
  uint32_t buf[16];
  uint64_t block = 0;
  int pos = 16;
  size_t n = 0;
  while (n < count) {
    if (pos == 16) {
      chacha_block(12, key.k, block++, 0, buf);
      pos = 0;
    }
    const uint32_t word = buf[pos++];
    if (weight_rejected(word, OMR_WEIGHT_ZONE)) continue;  // UniformInt<u16> rejection zone
    out[n++] = weight_of_word(word);
  }
  memset(out + count, 0, ((size_t)n_ct * per_ct * all - count) * sizeof(uint16_t));
  return OMR_OK;
}

namespace {

// The row loop of the two *_weights_at entries: out[r][k] = the weight at raw position at(j, k) of combination
// j = first_combo + r's stream, zero for a padding combination (j >= combos). One ChaCha block is kept, so
// sorted indices share blocks.
template <typename At>
void weight_rows(const WeightKey &key, bool stream_per_combo, uint32_t combos, uint32_t first_combo, uint32_t n_combos,
                 size_t n_indices, uint16_t *out, int nthreads, At at) {
  parallel_for(n_combos, nthreads, [&](size_t r) {
    uint16_t *o = out + r * n_indices;
    const uint64_t j = (uint64_t)first_combo + r;
    if (j >= combos) {  // a padding combination
      std::fill(o, o + n_indices, (uint16_t)0);
      return;
    }
    uint32_t w[16];
    uint64_t have = 0;  // the block in w, valid once k > 0
    for (size_t k = 0; k < n_indices; ++k) {
      const uint64_t p = at(j, k);
      if (k == 0 || (p >> 4) != have) chacha_block(12, key.k, have = p >> 4, stream_per_combo ? PAYW_STREAM | j : 0, w);
      o[k] = weight_of_word(w[p & 15]);
    }
  });
}

}  // namespace

// Indexed payload weights (include/omr_gpu.h, none in the reference), host side: weights.hpp's
// indexed_weight_block, the statement the encode kernel shares.
extern "C" omr_status omr_indexed_weights_at(const uint8_t seed[32], uint32_t combos, uint32_t first_combo,
                                             uint32_t n_combos, const size_t *indices, size_t n_indices,
                                             uint16_t *out, int nthreads) {
  if (!seed || (n_indices && !indices) || (n_combos && n_indices && !out))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_indexed_weights_at: NULL argument");
  if ((uint64_t)first_combo + n_combos > (uint64_t)UINT32_MAX + 1)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_indexed_weights_at: combination beyond 2^32");
  // weight (j, g) is word g & 15 of block g >> 4 of combination j's own stream
  weight_rows(weight_key(seed), true, combos, first_combo, n_combos, n_indices, out, nthreads,
              [&](uint64_t, size_t k) { return (uint64_t)indices[k]; });
  return OMR_OK;
}

extern "C" omr_status omr_indexed_weights_table(const uint8_t seed[32], size_t all, uint32_t combos, uint32_t n_ct,
                                                uint32_t per_ct, uint16_t *out, int nthreads) {
  const uint64_t rows = (uint64_t)n_ct * per_ct;
  if (!seed || !out || all == 0 || rows == 0 || rows < combos)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_indexed_weights_table: bad argument");
  const WeightKey key = weight_key(seed);
  constexpr size_t PIECE = 4096;  // 16-message blocks per work item
  const size_t nblk = (all + 15) / 16, pieces = (nblk + PIECE - 1) / PIECE;
  parallel_for((size_t)rows * pieces, nthreads, [&](size_t it) {
    const size_t j = it / pieces, b0 = (it % pieces) * PIECE, b1 = std::min(nblk, b0 + PIECE);
    uint16_t *o = out + j * all;
    if (j >= combos) {
      std::fill(o + b0 * 16, o + std::min(all, b1 * 16), (uint16_t)0);
      return;
    }
    uint16_t w[16];
    for (size_t b = b0; b < b1; ++b) {
      indexed_weight_block(key, (uint32_t)j, b, w);
      for (size_t i = 0; i < 16 && b * 16 + i < all; ++i) o[b * 16 + i] = w[i];
    }
  });
  return OMR_OK;
}

// Reference payload weights by seek (include/omr_gpu.h), host side: the scan that finds the stream's
// rejections and the recipient's matrix, over weights.hpp's statement.
extern "C" omr_status omr_weight_seek_build_zone_cpu(const uint8_t seed[32], uint64_t draws, uint32_t zone,
                                                     int nthreads, omr_weight_seek *out) {
  const char *who = "omr_weight_seek_build_cpu";
  if (!seed || !out) return set_error(OMR_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL argument");
  if (draws >= SEEK_MAX_DRAWS) return set_error(OMR_ERR_INVALID_ARGUMENT, std::string(who) + ": draws beyond 2^62");
  const WeightKey key = weight_key(seed);
  const uint64_t last = draws + OMR_WEIGHT_SEEK_MAX;  // the last raw word scanned
  constexpr uint64_t PIECE = 4096;                    // ChaCha blocks per work item
  const uint64_t nblk = (last >> 4) + 1, pieces = (nblk + PIECE - 1) / PIECE;
  std::vector<uint64_t> hits;  // every piece's first SEEK_LIST rejections: the stream's first SEEK_LIST are among them
  std::mutex mu;
  parallel_for((size_t)pieces, nthreads, [&](size_t it) {
    uint64_t mine[SEEK_LIST];
    uint32_t n = 0;
    const uint64_t b1 = std::min(nblk, ((uint64_t)it + 1) * PIECE);
    for (uint64_t b = (uint64_t)it * PIECE; b < b1 && n < SEEK_LIST; ++b) {
      uint32_t w[16];
      chacha_block(12, key.k, b, 0, w);
      for (int i = 0; i < 16 && n < SEEK_LIST; ++i)
        if (weight_rejected(w[i], zone) && b * 16 + i <= last) mine[n++] = b * 16 + i;
    }
    if (n) {
      std::lock_guard<std::mutex> lk(mu);
      hits.insert(hits.end(), mine, mine + n);
    }
  });
  std::sort(hits.begin(), hits.end());
  // more than SEEK_LIST found: the smallest SEEK_LIST + 1 decide, and seek_from_hits reports the overflow
  return seek_from_hits(hits.data(), std::min<uint64_t>(hits.size(), SEEK_LIST + 1), draws, zone, out, who);
}

extern "C" omr_status omr_weight_seek_build_cpu(const uint8_t seed[32], uint64_t draws, int nthreads,
                                                omr_weight_seek *out) {
  return omr_weight_seek_build_zone_cpu(seed, draws, OMR_WEIGHT_ZONE, nthreads, out);
}

extern "C" omr_status omr_payload_weights_at(const uint8_t seed[32], size_t all, uint32_t combos,
                                             const omr_weight_seek *seek, uint32_t first_combo, uint32_t n_combos,
                                             const size_t *indices, size_t n_indices, uint16_t *out, int nthreads) {
  if (!seed || !seek || (n_indices && !indices) || (n_combos && n_indices && !out))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_payload_weights_at: NULL argument");
  if (!seek_covers(seek, combos, all))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_payload_weights_at: the seek does not cover combination_count * all draws");
  for (size_t k = 0; k < n_indices; ++k)
    if (indices[k] >= all) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_payload_weights_at: index out of range");
  // weight (j, g) is accepted draw j * all + g of the one stream, found through the seek
  weight_rows(weight_key(seed), false, combos, first_combo, n_combos, n_indices, out, nthreads,
              [&](uint64_t j, size_t k) { return seek_pos(*seek, j * (uint64_t)all + indices[k]); });
  return OMR_OK;
}

omr_status omr::resolve_seek(const uint8_t seed[32], const omr_weight_seek *seek, uint64_t rows, uint64_t all,
                             const std::string &who, const SeekBuilder &build, omr_weight_seek *out) {
  if (seek) {
    if (!seek_covers(seek, rows, all))
      return set_error(OMR_ERR_INVALID_ARGUMENT, who + ": the seek does not cover combination_count * all draws");
    *out = *seek;
    return OMR_OK;
  }
  if (all > SEEK_MAX_DRAWS / (rows + 1)) return set_error(OMR_ERR_INVALID_ARGUMENT, who + ": board too large");
  return build(seed, rows * all, out);
}
