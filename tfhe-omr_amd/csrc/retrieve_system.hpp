// What the host retrieval (retriever.hip) and the auditor's (retrieve_device.hip) share, host code only: the
// reader of the index buckets, the checks on a payload system, where its matrix comes from with the host
// gather, and the NULL test of the payload entry points. Each is written here once; the two callers differ in
// where the decoded values and the solve live.
#pragma once

#include <set>
#include <string>

#include "hip_util.hpp"
#include "weights.hpp"

namespace omr {

// decode_pertinent_indices (retriever.rs:63-130) on one decoded index ciphertext: every bucket whose marker
// slot holds 1 adds its index to `set`. The caller loops over the ciphertexts and stops at the first one
// after which every pertinent index is known.
template <typename T>
void read_index_buckets(const T *dec, const omr_retrieval_params &rp, std::set<size_t> &set) {
  const size_t spb = rp.slots_per_bucket, sps = rp.slots_per_segment;
  for (size_t s0 = 0; s0 + sps <= (size_t)N2; s0 += sps)
    for (size_t b0 = s0; b0 + spb <= s0 + sps; b0 += spb) {
      if (dec[b0 + spb - 1] != 1) continue;  // bucket marker
      size_t v = 0;
      for (size_t k = spb - 1; k-- > 0;) v = v * P + dec[b0 + k];  // base-257 digits, LSD first
      set.insert(v);
    }
}
inline void write_indices(const std::set<size_t> &set, size_t *indices, size_t cap, size_t *found) {
  *found = set.size();
  size_t i = 0;
  for (size_t v : set) {
    if (i >= cap) break;
    indices[i++] = v;
  }
}

// The system of a payload retrieval: rows combinations in cols unknowns of `len` words each, `per` combinations
// per group of `stripes` ciphertexts (612 words and one stripe unless the entry takes a layout).
struct PayloadSystem {
  size_t rows = 0, cols = 0, per = 0, len = PAYLOAD_LEN, stripes = 1;
};
// The checks of every payload entry after its NULL test. cols = 0 (no index) is no error: nothing to solve.
// `ly` is the layout of an *_indexed_len entry (its combination_count, then, is the system's), NULL otherwise.
inline omr_status payload_system(size_t all, uint32_t combination_count, uint32_t n_ct, const size_t *indices,
                                 size_t n_indices, const std::string &who, PayloadSystem *sys,
                                 const omr_payload_layout *ly = nullptr) {
  omr_retrieval_params rp;
  OMR_TRY(omr_get_retrieval_params(all, n_indices, &rp));
  sys->rows = combination_count ? combination_count : rp.combination_count;
  sys->cols = n_indices;
  sys->per = rp.cmb_count_per_cipher;
  if (ly) {
    if (!payload_len_ok(ly->payload_len) || ly->cmb_count_per_cipher == 0 ||
        ly->cmb_count_per_cipher > payload_per_max(ly->payload_len))
      return set_error(OMR_ERR_INVALID_ARGUMENT, who + ": a payload length or combinations per ciphertext out of range");
    sys->rows = ly->combination_count;
    sys->per = ly->cmb_count_per_cipher;
    sys->len = ly->payload_len;
    sys->stripes = payload_stripes(ly->payload_len);
  }
  if (n_indices == 0) return OMR_OK;
  if ((size_t)n_ct / sys->stripes * sys->per < sys->rows)  // whole groups only
    return set_error(OMR_ERR_INVALID_ARGUMENT, who + ": too few payload ciphertexts");
  if (sys->rows < sys->cols)  // matrix.rs:171 asserts num_rows >= num_cols
    return set_error(OMR_ERR_INVALID_ARGUMENT, who + ": fewer combinations than indices");
  for (size_t i = 0; i < n_indices; ++i)
    if (indices[i] >= all) return set_error(OMR_ERR_INVALID_ARGUMENT, who + ": index out of range");
  return OMR_OK;
}

// Where the system's matrix comes from: the table's entries, the indexed weights of a seed, or the
// reference's weights of a seed through a seek (seek NULL: built inside the call, weights.hpp's resolve_seek).
struct MatrixSource {
  const uint16_t *weights = nullptr;
  const uint8_t *weight_seed = nullptr;
  bool by_seek = false;
  const omr_weight_seek *seek = nullptr;
};
// m[j][k] = the weight of combination j for the k-th index (retriever.rs:220-238), on the host. Every row is
// a real combination of the board. `seek` is the resolved seek of a by_seek source, unused otherwise.
inline omr_status fill_matrix_host(const MatrixSource &src, const omr_weight_seek &seek, const PayloadSystem &sys,
                                   size_t all, const size_t *indices, uint16_t *m) {
  const uint32_t rows = (uint32_t)sys.rows;
  if (src.by_seek) return omr_payload_weights_at(src.weight_seed, all, rows, &seek, 0, rows, indices, sys.cols, m, 0);
  if (!src.weights) return omr_indexed_weights_at(src.weight_seed, rows, 0, rows, indices, sys.cols, m, 0);
  for (size_t j = 0; j < sys.rows; ++j)
    for (size_t k = 0; k < sys.cols; ++k) m[j * sys.cols + k] = src.weights[j * all + indices[k]];
  return OMR_OK;
}

// The system's right-hand side from the decoded payload ciphertexts [n_ct][N2] (decode_combined_payloads,
// retriever.rs:318-362, for any layout): rhs[j][l] = word l of combination j (weights.hpp, payload_word_at).
template <typename T>
void gather_rhs_host(const T *dec, const PayloadSystem &sys, uint16_t *rhs) {
  for (size_t j = 0; j < sys.rows; ++j)
    for (size_t l = 0; l < sys.len; ++l)
      rhs[j * sys.len + l] = (uint16_t)dec[payload_word_at((uint32_t)j, (uint32_t)l, (uint32_t)sys.len, (uint32_t)sys.per,
                                                           (uint32_t)sys.stripes)];
}

// The NULL test of the payload entries: `owner` is the secret key pack or the auditor.
inline bool retrieve_args_ok(const void *owner, const void *pay_cts, const MatrixSource &src, const size_t *indices,
                             size_t n_indices, const uint16_t *payloads) {
  return owner && pay_cts && (src.weights || src.weight_seed) && (!n_indices || (indices && payloads));
}

}  // namespace omr
