// Client-side digest decoding (host, CPU): Retriever::decode_digest (retriever.rs:188-260) with
// decode_pertinent_indices (:63-130), decode_combined_payloads (:318-362) and
// solve_matrix_mod_257 (matrix.rs:164-247), and the bitmap digest's decoding (include/omr_gpu.h, "Bitmap
// digest": none in the reference). Used by clients of the detector, by bench.py's
// end-to-end check and by the multi-GPU driver; needs only the secret key pack.
#include <algorithm>
#include <mutex>
#include <new>
#include <set>
#include <string>
#include <vector>

#include "audit_decode.hpp"
#include "host_ring.hpp"
#include "retrieve_system.hpp"

using namespace omr;

namespace {

// The phase of one ciphertext: N2^-1 INTT(b - a * NTT(s2)), canonical in [0, q2) (retriever.rs:84-96).
// ct: u64 [2][N2] (a, b), NTT domain, any u64 words (reduced mod q2 first).
void phase_one(const omr_secret_key_pack *sk, const uint64_t *ct, uint64_t *ph) {
  const HostNtt &T = ntt2();
  const uint64_t *a = ct, *b = ct + N2;
  for (int j = 0; j < N2; ++j) {
    const uint64_t as = T.mul(a[j] % Q2, sk->s2_ntt[j], sk->s2_ntts[j]);
    const uint64_t bj = b[j] % Q2;
    ph[j] = bj >= as ? bj - as : bj + Q2 - as;
  }
  T.inv(ph);
}

// round(c * p / q2) half up, mod p, of the phase (retriever.rs:84-96).
void decrypt_decode_one(const omr_secret_key_pack *sk, const uint64_t *ct, uint32_t p, uint32_t *out) {
  std::vector<uint64_t> ph(N2);
  phase_one(sk, ct, ph.data());
  for (int j = 0; j < N2; ++j) {
    uint64_t t = (uint64_t)(((u128)ph[j] * (2 * p) + Q2) / ((u128)2 * Q2));
    out[j] = (uint32_t)(t >= p ? t - p : t);
  }
}

// The auditor's results for one ciphertext (include/omr_gpu.h, "Auditor"): its record, optionally its
// decoded values, and its tallies added into `sum`.
omr_ct_audit audit_one(const omr_secret_key_pack *sk, const uint64_t *ct, uint16_t *decoded, omr_audit_summary &sum) {
  std::vector<uint64_t> ph(N2);
  phase_one(sk, ct, ph.data());
  omr_ct_audit rec{0, 0, 0};
  for (int j = 0; j < N2; ++j) {
    const DecodedCoeff d = decode_coeff(ph[j]);
    if (decoded) decoded[j] = (uint16_t)d.t;
    if (j == 0) rec.first = d.t;
    rec.nonzero += d.t != 0;
    rec.max_abs_residual = std::max(rec.max_abs_residual, d.abs_r);
    ++sum.residual_bits[bit_length(d.abs_r)];
  }
  const bool zero = rec.nonzero == 0, one_hot = rec.nonzero == 1 && rec.first == 1;
  ++sum.ciphertexts;
  sum.zero += zero;
  sum.one_hot += one_hot;
  sum.other += !zero && !one_hot;
  sum.max_abs_residual = std::max(sum.max_abs_residual, rec.max_abs_residual);
  return rec;
}

}  // namespace

extern "C" omr_status omr_decrypt_decode(const omr_secret_key_pack *sk, const uint64_t *ct, size_t n,
                                         uint32_t *out) {
  if (!sk || (n && (!ct || !out)))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_decrypt_decode: NULL argument");
  parallel_for(n, 0, [&](size_t m) { decrypt_decode_one(sk, ct + m * 2 * N2, P, out + m * N2); });
  return OMR_OK;
}

extern "C" omr_status omr_audit_cpu(const omr_secret_key_pack *sk, const uint64_t *cts, size_t n,
                                    omr_ct_audit *records, uint16_t *decoded, omr_audit_summary *summary,
                                    int nthreads) {
  if (!sk) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_audit_cpu: NULL secret key pack");
  if (!records && !decoded && !summary) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_audit_cpu: no output requested");
  if (n == 0) return OMR_OK;
  if (!cts) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_audit_cpu: NULL ciphertexts");
  std::mutex mu;  // guards *summary: integer tallies, so the order of the merges does not matter
  parallel_for(n, nthreads, [&](size_t m) {
    omr_audit_summary one{};
    const omr_ct_audit rec = audit_one(sk, cts + m * 2 * N2, decoded ? decoded + m * N2 : nullptr, one);
    if (records) records[m] = rec;
    if (summary) {
      std::lock_guard<std::mutex> lk(mu);
      merge_summary(*summary, one);
    }
  });
  return OMR_OK;
}

extern "C" omr_status omr_retrieve_indices(const omr_secret_key_pack *sk, const uint64_t *idx_cts,
                                           uint32_t n_ct, size_t all_payloads_count,
                                           size_t pertinent_count, size_t *indices, size_t cap,
                                           size_t *found) {
  if (!sk || !found || (n_ct && !idx_cts) || (cap && !indices))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_retrieve_indices: NULL argument");
  omr_retrieval_params rp;
  OMR_TRY(omr_get_retrieval_params(all_payloads_count, pertinent_count, &rp));
  std::set<size_t> set;
  std::vector<uint32_t> dec(N2);
  // decode_digest stops at the first ciphertext after which every pertinent index is known
  for (uint32_t c = 0; c < n_ct; ++c) {
    decrypt_decode_one(sk, idx_cts + (size_t)c * 2 * N2, P, dec.data());
    read_index_buckets(dec.data(), rp, set);
    if (set.size() == pertinent_count) break;
  }
  write_indices(set, indices, cap, found);
  return OMR_OK;
}

namespace {

// Solve mod 257 (include/omr_gpu.h, "Solve mod 257"; solve_matrix_mod_257, matrix.rs:164-247) on the
// augmented system [matrix | rhs], any number of rows: forward elimination with the first non-zero pivot,
// then back substitution. nthreads > 1 splits the rows below the pivot once there is enough of them.
omr_status solve_mod257(const uint16_t *matrix, const uint16_t *rhs, size_t rows, size_t cols, size_t width,
                        uint16_t *solution, size_t *singular_col, int nthreads) {
  const size_t ld = cols + width;
  std::vector<uint16_t> w(rows * ld);  // values < 257
  for (size_t j = 0; j < rows; ++j) {
    for (size_t k = 0; k < cols; ++k) w[j * ld + k] = matrix[j * cols + k] % P;
    for (size_t b = 0; b < width; ++b) w[j * ld + cols + b] = rhs[j * width + b] % P;
  }
  uint16_t inv[P] = {0};  // v^(p-2) mod p
  for (uint32_t v = 1; v < (uint32_t)P; ++v) {
    uint32_t r = 1, b = v;
    for (uint32_t e = P - 2; e; e >>= 1, b = b * b % P)
      if (e & 1) r = r * b % P;
    inv[v] = (uint16_t)r;
  }
  // row j -= c * row i over the columns [k0, ld)
  auto reduce = [&](size_t j, size_t i, size_t col, size_t k0) {
    const uint32_t c = w[j * ld + col];
    if (!c) return;
    uint16_t *rj = &w[j * ld];
    const uint16_t *ri = &w[i * ld];
    for (size_t k = k0; k < ld; ++k) rj[k] = (uint16_t)((rj[k] + (uint32_t)P * P - c * ri[k]) % P);
  };
  for (size_t i = 0; i < cols; ++i) {
    size_t piv = rows;
    for (size_t j = i; j < rows; ++j)
      if (w[j * ld + i] != 0) {
        piv = j;
        break;
      }
    if (piv == rows) {
      if (singular_col) *singular_col = i;
      return set_error(OMR_ERR_NOT_INVERTIBLE, "Matrix is not invertible");
    }
    if (piv != i) std::swap_ranges(&w[i * ld], &w[i * ld] + ld, &w[piv * ld]);
    if (w[i * ld + i] != 1) {
      const uint32_t iv = inv[w[i * ld + i]];
      for (size_t k = i; k < ld; ++k) w[i * ld + k] = (uint16_t)(w[i * ld + k] * iv % P);
    }
    const size_t below = rows - i - 1;
    if (nthreads == 1 || below * (ld - i) < ((size_t)1 << 18)) {
      for (size_t j = i + 1; j < rows; ++j) reduce(j, i, i, i);
    } else {
      parallel_for(below, nthreads, [&](size_t r) { reduce(i + 1 + r, i, i, i); });
    }
  }
  for (size_t i = cols; i-- > 1;)
    for (size_t j = 0; j < i; ++j) reduce(j, i, i, cols);  // the matrix part above the diagonal is not read again
  for (size_t k = 0; k < cols; ++k)
    for (size_t b = 0; b < width; ++b) solution[k * width + b] = w[k * ld + cols + b];
  return OMR_OK;
}

// The body of the three omr_retrieve_payloads* entries after their NULL test: they differ in where the
// system's matrix comes from (retrieve_system.hpp). No row cap: the solve is this file's, on this thread.
omr_status retrieve_payloads_body(const omr_secret_key_pack *sk, const uint64_t *pay_cts, uint32_t n_ct, size_t all,
                                  uint32_t combination_count, const MatrixSource &src, const size_t *indices,
                                  size_t n_indices, uint16_t *payloads, const std::string &who,
                                  const omr_payload_layout *ly = nullptr) {
  if (!retrieve_args_ok(sk, pay_cts, src, indices, n_indices, payloads))
    return set_error(OMR_ERR_INVALID_ARGUMENT, who + ": NULL argument");
  PayloadSystem sys;
  OMR_TRY(payload_system(all, combination_count, n_ct, indices, n_indices, who, &sys, ly));
  if (sys.cols == 0) return OMR_OK;
  omr_weight_seek seek{};
  if (src.by_seek)
    OMR_TRY(resolve_seek(src.weight_seed, src.seek, sys.rows, all, who,
                         [](const uint8_t *seed, uint64_t draws, omr_weight_seek *out) {
                           return omr_weight_seek_build_cpu(seed, draws, 0, out);
                         },
                         &seek));
  // decode_combined_payloads: combination j lives in ciphertext j / per, slots (j % per) * 612.. (a layout
  // with a length of its own: retrieve_system.hpp, gather_rhs_host)
  std::vector<uint16_t> rhs(sys.rows * sys.len);
  std::vector<uint32_t> dec((size_t)n_ct * N2);
  parallel_for(n_ct, 0, [&](size_t c) { decrypt_decode_one(sk, pay_cts + c * 2 * N2, P, &dec[c * N2]); });
  gather_rhs_host(dec.data(), sys, rhs.data());
  std::vector<uint16_t> m(sys.rows * sys.cols);
  OMR_TRY(fill_matrix_host(src, seek, sys, all, indices, m.data()));
  // forward elimination with the first non-zero pivot, then back substitution (matrix.rs), on this thread
  return solve_mod257(m.data(), rhs.data(), sys.rows, sys.cols, sys.len, payloads, nullptr, 1);
}

}  // namespace

extern "C" omr_status omr_retrieve_payloads(const omr_secret_key_pack *sk, const uint64_t *pay_cts,
                                            uint32_t n_ct, size_t all_payloads_count,
                                            uint32_t combination_count, const uint16_t *weights,
                                            const size_t *indices,
                                            size_t n_indices, uint16_t *payloads) {
  return retrieve_payloads_body(sk, pay_cts, n_ct, all_payloads_count, combination_count, MatrixSource{weights}, indices,
                                n_indices, payloads, "omr_retrieve_payloads");
}

extern "C" omr_status omr_retrieve_payloads_indexed(const omr_secret_key_pack *sk, const uint64_t *pay_cts,
                                                    uint32_t n_ct, size_t all_payloads_count,
                                                    uint32_t combination_count, const uint8_t weight_seed[32],
                                                    const size_t *indices, size_t n_indices, uint16_t *payloads) {
  return retrieve_payloads_body(sk, pay_cts, n_ct, all_payloads_count, combination_count,
                                MatrixSource{nullptr, weight_seed}, indices, n_indices, payloads,
                                "omr_retrieve_payloads_indexed");
}

extern "C" omr_status omr_retrieve_payloads_indexed_len(const omr_secret_key_pack *sk, const uint64_t *pay_cts,
                                                        uint32_t n_ct, size_t all_payloads_count,
                                                        const omr_payload_layout *layout, const uint8_t weight_seed[32],
                                                        const size_t *indices, size_t n_indices, uint16_t *payloads) {
  const char *who = "omr_retrieve_payloads_indexed_len";
  if (!layout) return set_error(OMR_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL argument");
  return retrieve_payloads_body(sk, pay_cts, n_ct, all_payloads_count, layout->combination_count,
                                MatrixSource{nullptr, weight_seed}, indices, n_indices, payloads, who, layout);
}

extern "C" omr_status omr_retrieve_payloads_seek(const omr_secret_key_pack *sk, const uint64_t *pay_cts, uint32_t n_ct,
                                                 size_t all_payloads_count, uint32_t combination_count,
                                                 const uint8_t weight_seed[32], const omr_weight_seek *seek,
                                                 const size_t *indices, size_t n_indices, uint16_t *payloads) {
  return retrieve_payloads_body(sk, pay_cts, n_ct, all_payloads_count, combination_count,
                                MatrixSource{nullptr, weight_seed, true, seek}, indices, n_indices, payloads,
                                "omr_retrieve_payloads_seek");
}

extern "C" omr_status omr_solve_mod257_cpu(const uint16_t *matrix, const uint16_t *rhs, size_t rows, size_t cols,
                                           size_t width, uint16_t *solution, size_t *singular_col, int nthreads) {
  if (!matrix || !rhs || !solution) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_solve_mod257_cpu: NULL argument");
  if (cols < 1 || rows < cols || width < 1)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_solve_mod257_cpu: needs cols >= 1, rows >= cols, width >= 1");
  if (rows > OMR_SOLVE_MAX_ROWS)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_solve_mod257_cpu: more than OMR_SOLVE_MAX_ROWS (8192) rows");
  try {
    return solve_mod257(matrix, rhs, rows, cols, width, solution, singular_col, nthreads);
  } catch (const std::bad_alloc &) {
    return set_error(OMR_ERR_OUT_OF_MEMORY, "omr_solve_mod257_cpu: host allocation failed");
  }
}

extern "C" omr_status omr_bitmap_ct_count(size_t all, uint32_t *n_ct) {
  if (!n_ct) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_bitmap_ct_count: NULL argument");
  const size_t n = all / OMR_BITMAP_MESSAGES_PER_CT + (all % OMR_BITMAP_MESSAGES_PER_CT != 0);
  if (all == 0 || n > UINT32_MAX) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_bitmap_ct_count: bad board size");
  *n_ct = (uint32_t)n;
  return OMR_OK;
}

extern "C" omr_status omr_bitmap_indices(const uint16_t *decoded, uint32_t n_ct, size_t all, size_t *indices,
                                         size_t cap, size_t *found) {
  if (!decoded || !found || (cap && !indices))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_bitmap_indices: NULL argument");
  uint32_t want;
  const omr_status st = omr_bitmap_ct_count(all, &want);
  if (st != OMR_OK) return st;
  const char *bad = "omr_bitmap_indices: not a bitmap digest of this board";
  if (n_ct != want) return set_error(OMR_ERR_INVALID_ARGUMENT, bad);
  size_t n = 0;
  // increasing g = 16384 c + 2048 t + j: ciphertext, then bit plane, then coefficient
  for (uint32_t c = 0; c < n_ct; ++c) {
    const uint16_t *d = decoded + (size_t)c * N2;
    for (int j = 0; j < N2; ++j)
      if (d[j] >> OMR_BITMAP_BITS) return set_error(OMR_ERR_INVALID_ARGUMENT, bad);
    for (int t = 0; t < OMR_BITMAP_BITS; ++t)
      for (int j = 0; j < N2; ++j) {
        if (!((d[j] >> t) & 1)) continue;
        const size_t g = (size_t)c * OMR_BITMAP_MESSAGES_PER_CT + (size_t)t * N2 + j;
        if (g >= all) return set_error(OMR_ERR_INVALID_ARGUMENT, bad);
        if (n < cap) indices[n] = g;
        ++n;
      }
  }
  *found = n;
  return OMR_OK;
}

extern "C" omr_status omr_retrieve_bitmap(const omr_secret_key_pack *sk, const uint64_t *bitmap_cts, uint32_t n_ct,
                                          size_t all, size_t *indices, size_t cap, size_t *found) {
  if (!sk || !bitmap_cts || !found || (cap && !indices))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_retrieve_bitmap: NULL argument");
  uint32_t want;
  const omr_status st = omr_bitmap_ct_count(all, &want);
  if (st != OMR_OK) return st;
  if (n_ct != want) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_retrieve_bitmap: not a bitmap digest of this board");
  std::vector<uint32_t> dec((size_t)n_ct * N2);
  parallel_for(n_ct, 0, [&](size_t c) { decrypt_decode_one(sk, bitmap_cts + c * 2 * N2, P, &dec[c * N2]); });
  const std::vector<uint16_t> d16(dec.begin(), dec.end());  // decoded values are < 257
  return omr_bitmap_indices(d16.data(), n_ct, all, indices, cap, found);
}
